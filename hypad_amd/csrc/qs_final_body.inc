// Body of qs_final_kernel and qs_final_signals_kernel (scoring.hip), included after each kernel's prologue: the last three radix
// levels over every rank's candidate list; leaves the ranks' keys in `keys`, behind a barrier -- the interpolation is the kernel's own.
// Expects from the enclosing scope: in, n (the series -- the whole input, or the segment of blockIdx.x), ws (its QsWs), nsel, and the
// kernel's LDS arrays keys, stage and cur.
// Shared as text, not as a function: see the note at unroll_median_signals_kernel.
  const int grp = threadIdx.x >> 8, tg = threadIdx.x & 255, lane = threadIdx.x & 63;
  const bool live = grp < nsel;
  QsState st = ws.state[QS_PRE * QS_SEL + (live ? grp : 0)];
  const unsigned int c = live ? ws.cand_count[grp] : 0u;
  const unsigned long long kmx = live ? ws.kmax[grp] : 0ull, kmn = live ? ~ws.kinv[grp] : 0ull;
  const bool decided = !live || kmx == kmn;                // (group-uniform) every candidate is the same key
  const bool listed = c <= (unsigned int)QS_CAND;
  const unsigned long long* cand = ws.cand + (size_t)(live ? grp : 0) * QS_CAND;
  const int64_t m = decided ? 0 : (listed ? (int64_t)c : n);
  unsigned int* hst = stage[live ? grp : 0];
  for (int level = QS_PRE; level < QS_LEVELS; ++level) {   // (block-uniform trip count; a decided group only keeps the barriers)
    const int bins = qs_bins(level), sh = qs_shift(level);
    const int hi_sh = sh + (level == QS_LEVELS - 1 ? 64 - QS_BITS * (QS_LEVELS - 1) : QS_BITS);     // bits above the digit (<= 31)
    for (int i = tg; i < bins; i += 256) hst[i] = 0u;
    __syncthreads();
    for (int64_t i0 = 0; i0 < m; i0 += 4 * 256) {          // four loads in flight per thread
      unsigned long long k[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + u * 256 + tg;
        k[u] = i < m ? (listed ? cand[i] : qs_key(in[i])) : ~st.prefix;      // (~prefix never matches)
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (((k[u] ^ st.prefix) >> hi_sh) == 0) atomicAdd(hst + ((unsigned int)(k[u] >> sh) & (unsigned int)(bins - 1)), 1u);
    }
    __syncthreads();
    if (tg < 64 && !decided) {                             // the group's first wave scans its histogram
      const QsState nx = qs_descend_staged(hst, level, st);
      if (lane == 0) cur[grp] = nx;
    }
    __syncthreads();
    if (!decided) st = cur[grp];
  }
  if (live && tg == 0) keys[grp] = decided ? kmx : st.prefix;
  __syncthreads();
