// Body of qs_compact_kernel and qs_compact_signals_kernel (scoring.hip), included after each kernel's prologue: the candidate lists
// of one series -- the whole input, or the segment the workgroup took from blockIdx.y.
// Expects from the enclosing scope: in, n (the series), ws (its QsWs), nsel, h and cur (the kernel's LDS arrays), wave, lane, PER,
// base (the workgroup's first element) and x (declared, double[PER]).
// Shared as text, not as a function: see the note at unroll_median_signals_kernel.
#pragma unroll
  for (int u = 0; u < PER; ++u) { const int64_t i = base + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  if (wave < nsel) {
    const QsState st = qs_descend(ws.hist + ((size_t)(QS_PRE - 1) * QS_SEL + wave) * QS_BINS, QS_PRE - 1, ws.state[(QS_PRE - 1) * QS_SEL + wave], h[wave]);
    if (lane == 0) { cur[wave] = st; if (blockIdx.x == 0) ws.state[QS_PRE * QS_SEL + wave] = st; }
  }
  __syncthreads();
  const int hi_sh = qs_shift(QS_PRE - 1);                 // the 33 bits fixed so far sit above it
  unsigned long long pre[QS_SEL];
  for (int s2 = 0; s2 < QS_SEL; ++s2) pre[s2] = s2 < nsel ? cur[s2].prefix : 0;
  for (; base < n; base += (int64_t)gridDim.x * (256 * PER)) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      if (base + u * 256 + threadIdx.x >= n) continue;
      const unsigned long long k = qs_key(x[u]);
#pragma unroll
      for (int s2 = 0; s2 < QS_SEL; ++s2)
        if (s2 < nsel && ((k ^ pre[s2]) >> hi_sh) == 0) {
          const unsigned int pos = atomicAdd(ws.cand_count + s2, 1u);
          if (pos < (unsigned int)QS_CAND) ws.cand[(size_t)s2 * QS_CAND + pos] = k;
          atomicMax(ws.kmax + s2, k);
          atomicMax(ws.kinv + s2, ~k);
        }
    }
    const int64_t nb = base + (int64_t)gridDim.x * (256 * PER);
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int64_t i = nb + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  }
