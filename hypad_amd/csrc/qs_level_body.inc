// Body of qs_level_kernel and qs_level_signals_kernel (scoring.hip), included once the level's state is in `cur`: the histogram of
// the level's digit over one series -- the whole input, or the segment the workgroup took from blockIdx.y.
// Expects from the enclosing scope: in, n (the series), ws (its QsWs), level, nsel, h and cur (the kernel's LDS arrays), PER, base
// (the workgroup's first element) and x (its first round of values, already requested).
// Shared as text, not as a function: see the note at unroll_median_signals_kernel.
  __syncthreads();                                                                  // (h doubled as the scan's staging rows)
  for (int i = threadIdx.x; i < QS_SEL * QS_BINS; i += 256) (&h[0][0])[i] = 0u;
  __syncthreads();
  const int sh = qs_shift(level), bins = qs_bins(level);
  const int hi_sh = sh + (level == QS_LEVELS - 1 ? 64 - QS_BITS * (QS_LEVELS - 1) : QS_BITS);     // bits above the digit
  unsigned long long pre[QS_SEL];
  for (int s2 = 0; s2 < QS_SEL; ++s2) pre[s2] = s2 < nsel ? cur[s2].prefix : 0;
  unsigned int nans = 0;
  for (; base < n; base += (int64_t)gridDim.x * (256 * PER)) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      if (base + u * 256 + threadIdx.x >= n) continue;
      if (level == 0 && x[u] != x[u]) ++nans;
      const unsigned long long k = qs_key(x[u]);
      const unsigned int digit = (unsigned int)(k >> sh) & (unsigned int)(bins - 1);
#pragma unroll
      for (int s2 = 0; s2 < QS_SEL; ++s2)
        if (s2 < nsel && (hi_sh >= 64 || ((k ^ pre[s2]) >> hi_sh) == 0)) atomicAdd(&h[s2][digit], 1u);
    }
    const int64_t nb = base + (int64_t)gridDim.x * (256 * PER);
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int64_t i = nb + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  }
  if (level == 0 && nans) atomicAdd(ws.nan_count, nans);
  __syncthreads();
  unsigned int* g = ws.hist + (size_t)level * QS_SEL * QS_BINS;
  for (int i = threadIdx.x; i < nsel * QS_BINS; i += 256) {
    const unsigned int c = (&h[0][0])[i];
    if (c) atomicAdd(g + i, c);
  }
