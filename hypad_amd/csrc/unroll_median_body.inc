// Body of unroll_median_kernel<EPL, FILTER, UT> and unroll_median_signals_kernel<EPL, UT> (scoring.hip), included after each kernel's
// prologue: the tile loop over one series -- the whole series, or the segment the workgroup took from blockIdx.y.
// Expects from the enclosing scope: y_hat (the series' windows), median (its output), n (its windows), W (the window), EPL, UT,
// FILTER, summary (null: medians only) and stamps (the development library's clock stamps and counters, null: none); the segmented
// kernel fixes the last three to true, null and null.  USTAMP / UCOUNT are defined in front of unroll_median_kernel.
// Shared as text, not as a function: see the note at unroll_median_signals_kernel.
  constexpr int THREADS = UT * 4;                           // (shadows the file's 256: this kernel's block size follows its tile)
  constexpr int RUN = UT / 64;                               // elements per lane of one source row's run
  extern __shared__ __attribute__((aligned(16))) float usm[];
  const int WS = (W + 3) & ~3;                              // tile row stride (floats)
  float* tile = usm;                                        // [UT][WS]
  float* sorted = usm + UT * WS;                            // [waves][MAX_WINDOW]   (summary / candidates)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  constexpr int NWV = THREADS / 64;
  const int64_t T = n + W - 1;
  float* s = sorted + wave_s * MAX_WINDOW;
  const float INF = __int_as_float(0x7f800000);
#if HYPAD_DIAG
  const bool ucount = stamps && stamps[14] != 0;             // (counting costs one contended atomic per timestep: a run of its own)
#endif
  for (int64_t t0 = (int64_t)blockIdx.x * UT; t0 < T; t0 += (int64_t)gridDim.x * UT) {
    USTAMP(0);
    // ---- stage: rows r in [t0 - (W - 1), t0 + UT) (clipped to the matrix), their runs of this tile's timesteps
    constexpr int RB = 8 / RUN;                              // rows in flight per wave (8 loads per lane either way)
    if (t0 >= W - 1 && t0 + UT <= n) {
      // interior tile (all but the first and last two of a long series): no clipping, j0 == 0, 32-bit indices relative to the
      // tile's first row, the row number a scalar -- ~9 vector instructions per row and lane instead of ~30 of 64-bit arithmetic
      const float* base = y_hat + (t0 - (W - 1)) * W;
      const int nrows = W + UT - 1;
      for (int kb = wave_s * RB; kb < nrows; kb += NWV * RB) {
        float val[RB][RUN];
        int dst[RB][RUN];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
          const int k = kb + u;                              // (scalar) row of the tile's parallelogram
          const int jb = W - 1 - k > 0 ? W - 1 - k : 0;
#pragma unroll
          for (int h = 0; h < RUN; ++h) {
            const int j = jb + lane + 64 * h, tt = k - (W - 1) + j;
            const bool ok = k < nrows && j < W && tt < UT;
            dst[u][h] = ok ? tt * WS + j : -1;
            val[u][h] = ok ? base[k * W + j] : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < RB; ++u)
#pragma unroll
          for (int h = 0; h < RUN; ++h)
            if (dst[u][h] >= 0) tile[dst[u][h]] = val[u][h];
      }
    } else {
      const int64_t r_lo = t0 - (W - 1) > 0 ? t0 - (W - 1) : 0;
      const int64_t r_hi = t0 + UT < n ? t0 + UT : n;         // exclusive
      for (int64_t rb = r_lo + wave * RB; rb < r_hi; rb += NWV * RB) {
        float val[RB][RUN];
        int dst[RB][RUN];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
          const int64_t r = rb + u;
          const int jb = (int)(t0 - r > 0 ? t0 - r : 0);       // first column of row r inside the tile
#pragma unroll
          for (int h = 0; h < RUN; ++h) {
            const int j = jb + lane + 64 * h;                  // (a run is at most UT columns: RUN elements per lane)
            const int64_t t = r + j;
            dst[u][h] = -1; val[u][h] = 0.f;
            if (r < r_hi && j < W && t < t0 + UT && t < T) {
              const int j0 = (int)(t - n + 1 > 0 ? t - n + 1 : 0);
              dst[u][h] = (int)(t - t0) * WS + (j - j0);
              val[u][h] = y_hat[r * W + j];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < RB; ++u)
#pragma unroll
          for (int h = 0; h < RUN; ++h)
            if (dst[u][h] >= 0) tile[dst[u][h]] = val[u][h];
      }
    }
    USTAMP(1);
    __syncthreads();
    USTAMP(2);
    // (round 6: the timestep a wave works on is a scalar -- as a vector value every count, address and "wave-uniform" branch below was
    // vector arithmetic and exec-mask code)
    for (int tt = wave_s; tt < UT; tt += NWV) {
      const int64_t t = t0 + tt;
      if (t >= T) break;
      const int j0 = (int)(t - n + 1 > 0 ? t - n + 1 : 0);
      const int j1 = (int)(t + 1 < W ? t + 1 : W);
      const int cnt = j1 - j0;
      float* v = tile + tt * WS;
      // pad the row to a multiple of 4 with +inf (never below or equal to a finite value)
      if (lane < 4 && cnt + lane < ((cnt + 3) & ~3)) v[cnt + lane] = INF;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): LDS writes of this wave landed
      float mine[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) { const int i = lane + 64 * e; mine[e] = i < cnt ? v[i] : INF; }
      // A NaN on the anti-diagonal: np.median, np.percentile, np.min and np.max of it are NaN.  It compares false with everything, so
      // the counts below would give it rank 0 beside the minimum and leave the top slot of `s` unwritten -- a finite median of the
      // other values and a stale maximum.  One ballot per timestep; the wave writes the NaNs and skips the ranking.
      bool isnan_mine = false;                               // (an unordered compare takes two slots at once: one instruction at EPL 1 and 2)
#pragma unroll
      for (int e = 0; e < EPL; e += 2) isnan_mine |= __builtin_isunordered(mine[e], mine[e + 1 < EPL ? e + 1 : e]);
      if (__ballot(isnan_mine)) {                            // wave-uniform
        if (lane == 0) {
          const float QNAN = __int_as_float(0x7fc00000);
          median[t] = QNAN;
          if (summary)
            for (int q = 0; q < 5; ++q) summary[t * 5 + q] = (double)QNAN;
        }
        continue;
      }
      const int m1 = (cnt - 1) >> 1, m2 = cnt >> 1;
      float lo_med = 0.f, hi_med = 0.f;
      bool done = false;
      if (FILTER && !summary && cnt >= 64) {                 // wave-uniform
        // ranks inside the sample v[0 .. 31] (lanes >= 32 idle along)
        const float sv = v[lane & 31];
        int less = 0;
#pragma unroll
        for (int k0 = 0; k0 < 32; k0 += 4) {
          const float4 q = *reinterpret_cast<const float4*>(v + k0);
          less += (q.x < sv ? 1 : 0) + (q.y < sv ? 1 : 0) + (q.z < sv ? 1 : 0) + (q.w < sv ? 1 : 0);
        }
        float plo = less <= 10 ? sv : -INF, phi = less >= 21 ? sv : INF;     // 11th smallest (largest with <= 10 below), 22nd smallest
        plo = hypad::wave_max(plo); phi = hypad::wave_min(phi);                // (DPP butterflies: no LDS round trips on this chain)
        int c_lt = 0, c_le = 0;
        unsigned long long cm[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const bool in = lane + 64 * e < cnt;
          c_lt += __builtin_popcountll(__ballot(in && mine[e] < plo));
          c_le += __builtin_popcountll(__ballot(in && mine[e] <= phi));
          cm[e] = __ballot(in && mine[e] >= plo && mine[e] <= phi);
        }
        const int nc = c_le - c_lt;
        if (c_lt <= m1 && m2 < c_le && nc <= 64 && nc > 0) {
          // compact the candidates into the wave's slab, rank them against each other
          int base = 0;
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(cm[e] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)cm[e], 0u));
            if ((cm[e] >> lane) & 1ull) s[pos] = mine[e];
            base += __builtin_popcountll(cm[e]);
          }
          if (lane < 4 && nc + lane < ((nc + 3) & ~3)) s[nc + lane] = INF;
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_s_waitcnt(0xc07f);
          const float c = lane < nc ? s[lane] : INF;
          int rk = 0;
          for (int k0 = 0; k0 < nc; k0 += 4) {
            const float4 q = *reinterpret_cast<const float4*>(s + k0);
            rk += (q.x < c ? 1 : 0) + (q.y < c ? 1 : 0) + (q.z < c ? 1 : 0) + (q.w < c ? 1 : 0);
          }
          // without ties the "less" counts are a permutation of 0 .. nc - 1 (their sum tells): then the lanes holding local ranks
          // m1 - c_lt and m2 - c_lt hold the two middle values
          const float rsum = hypad::wave_sum(lane < nc ? (float)rk : 0.f);
          if (rsum == 0.5f * (float)nc * (float)(nc - 1)) {
            const unsigned long long k1 = __ballot(lane < nc && rk == m1 - c_lt), k2 = __ballot(lane < nc && rk == m2 - c_lt);
            lo_med = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), (int)__builtin_ctzll(k1)));
            hi_med = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), (int)__builtin_ctzll(k2)));
            done = true;
            UCOUNT(8);
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
      if (!done) {
        UCOUNT(9);
        // rank = #{k : v[k] < mine} + #{k < i : v[k] == mine}.  Fast pass: count "less" only (one compare + add-carry per value).
        // Without ties those counts are a permutation of 0 .. cnt-1, with ties two values share a count and the counts' sum falls
        // short of cnt (cnt - 1) / 2: only then is the ordered tie count needed.  (The sum is exact in fp32: < 2^15 at window 256.)
        int rank[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) rank[e] = 0;
        for (int k0 = 0; k0 < cnt; k0 += 4) {
          const float4 q = *reinterpret_cast<const float4*>(v + k0);
          const float vk[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < EPL; ++e) rank[e] += vk[u] < mine[e] ? 1 : 0;
        }
        float rsum = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) rsum += lane + 64 * e < cnt ? (float)rank[e] : 0.f;
        const bool ties = hypad::wave_sum(rsum) != 0.5f * (float)cnt * (float)(cnt - 1);
        if (ties) {                                      // wave-uniform
#pragma unroll
          for (int e = 0; e < EPL; ++e) rank[e] = 0;
          for (int k = 0; k < cnt; ++k) {
            const float vk = v[k];
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
              const int i = lane + 64 * e;
              rank[e] += (vk < mine[e]) || (vk == mine[e] && k < i);
            }
          }
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e)
          if (lane + 64 * e < cnt) s[rank[e]] = mine[e];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        lo_med = s[m1]; hi_med = s[m2];
      }
      if (lane == 0) {
        // np.median of float32 stays float32.  It is numpy's MEAN of the middle value(s), a sum that starts from +0.0: a median that
        // is a zero is +0.0 there even when the middle values are -0.0 -- hence the + 0.f, which changes nothing else
        median[t] = ((cnt & 1) ? lo_med : (lo_med + hi_med) * 0.5f) + 0.f;
        if (summary) {
          double* o = summary + t * 5;
          o[0] = (double)s[0];
          const double qs[3] = {0.25, 0.5, 0.75};
          for (int qi = 0; qi < 3; ++qi) {
            double pos = qs[qi] * (double)(cnt - 1);
            int a = (int)floor(pos);
            int b = a + 1 < cnt ? a + 1 : cnt - 1;
            o[1 + qi] = (double)np_lerp(s[a], s[b], (float)(pos - (double)a));
          }
          o[4] = (double)s[cnt - 1];
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    USTAMP(3);
    __syncthreads();
  }
