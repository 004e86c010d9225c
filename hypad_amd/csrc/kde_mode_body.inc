// Body of kde_mode_kernel<KPL> and kde_mode_signals_kernel<KPL> (scoring.hip), included after each kernel's prologue: the
// timestep loop of one series -- the whole series, or the segment the workgroup took from blockIdx.y.
// Expects from the enclosing scope: critic (the series' critic values), modes (its output), n (its windows), W (the window), KPL.
// Shared as text, not as a function: see the note at unroll_median_signals_kernel.
  constexpr int WMAX = 64 * KPL;                            // the window class: 9 KB of LDS per workgroup and slot, 18 KB at window 100
  __shared__ double vals[THREADS / 64][WMAX];
  __shared__ __attribute__((aligned(16))) float vals32[THREADS / 64][WMAX + 4];      // + the padding the fp32 pass reads past the end
  __shared__ __attribute__((aligned(16))) float nsq32[THREADS / 64][WMAX + 4];       // -(value^2) for the factored form of the fp32 pass
  __shared__ double terms[THREADS / 64][KDE_CB * WMAX];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t T = n + W - 1;
  double* v = vals[wave];
  float* vf = vals32[wave];
  float* nf = nsq32[wave];
  // per-thread constants of the timestep loop, held in SCALAR registers (they are wave-uniform; as vector values the compiler kept them
  // in scratch memory across the loop: 20 bytes of private segment per lane and two scratch loads per timestep)
  auto uniform = [](double x) __attribute__((always_inline)) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
  };
  // Scott's factor n^(-2/5) for every sample count 1 .. W, one power per thread, once (the 2 (W - 1) edge timesteps have fewer than W
  // samples; a double-precision pow inside the loop -- ~200 instructions, its 40 polynomial constants hoisted into vector registers
  // across the loop -- was what this kernel spilled around)
  __shared__ double scott[WMAX];
  for (int c = threadIdx.x; c < W && c < WMAX; c += THREADS) scott[c] = pow((double)(c + 1), -0.4);
  __syncthreads();
  const double rW1 = uniform(W > 1 ? 1.0 / (double)(W - 1) : 0.0);
  for (int64_t t = (int64_t)blockIdx.x * (THREADS / 64) + wave; t < T; t += (int64_t)gridDim.x * (THREADS / 64)) {
    const int j0 = (int)(t - n + 1 > 0 ? t - n + 1 : 0);
    const int j1 = (int)(t + 1 < W ? t + 1 : W);
    const int cnt = __builtin_amdgcn_readfirstlane(j1 - j0);      // (wave-uniform: the pair loops below run on scalar counters)
    double s = 0.0;
    for (int k = lane; k < cnt; k += 64) {
      const float xf = critic[t - (j0 + k)];
      v[k] = (double)xf;
      vf[k] = xf;
      s += (double)xf;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    const double mean = wave_sum(s) / (double)cnt;
    double q = 0.0;
    for (int k = lane; k < cnt; k += 64) { const double d = v[k] - mean; q += d * d; }
    const double var = cnt > 1 ? wave_sum(q) * (cnt == W ? rW1 : 1.0 / (double)(cnt - 1)) : 0.0;      // np.cov: ddof = 1, `c *= 1 / fact`
    // Scott: factor = n^(-1/5), squared.  (All but the 2 (W - 1) edge timesteps have cnt == W: that power is taken once per
    // thread, not once per timestep -- a double-precision pow is ~200 instructions.)
    const double cov = var * uniform(scott[cnt - 1]);
    double out;
    if (cnt > 1 && cov > 0.0 && cov == cov) {
      // pass 1: fp32 densities of this lane's samples.  exp(-d^2 inv) = exp2(-(c d)^2) with c = sqrt(inv log2 e): the samples are
      // centred and rescaled once (pass 2 reads the fp64 copies), so a pair costs a subtract, a multiply, an exp2 and an add; the
      // slab is padded with +inf to a multiple of four (a padded pair contributes exp2(-inf) = 0) and read four values at a
      // time, every value once for all of the lane's samples.
      // The samples are CENTRED first, in fp64 (densities depend on differences only): rescaling the raw values would leave the
      // fp32 copies with an absolute error of |value| 2^-24 c, which at |mean| / bandwidth beyond ~1e4 exceeds the screen's margin.
      // The scale itself only has to be good to fp32 (an error in it is a slightly different bandwidth for every sample alike: 2e-7
      // relative in the densities): one v_rsq_f32 instead of an fp64 division and square root per timestep; the fp64 1 / (2 cov) that
      // pass 2 uses is taken only when pass 2 runs.  (A covariance outside the fp32 range makes the screen all-NaN or all-equal: pass 2
      // then sees every sample, as before.)
      const double c64 = (double)__builtin_amdgcn_rsqf((float)cov * 1.3862943611198906f);     // sqrt(log2 e / (2 cov))
      float amax = 0.f;
      for (int k = lane; k < cnt; k += 64) {
        const float y = (float)((v[k] - mean) * c64);
        vf[k] = y; nf[k] = -(y * y);
        amax = fmaxf(amax, fabsf(y));
      }
      amax = wave_max(amax);
      // (Measured and dropped in round 3, twice: using the kernel matrix's symmetry -- each unordered pair evaluated once.  With the
      // partner's share delivered by ds_add_f32: 3.28 ms against 0.42 ms for 125 000 windows (LDS float atomics).  With the values
      // parked in a small LDS matrix in chunks of eight steps and collected by the partners after a wave barrier (no atomics,
      // conflict-free strides, immediate offsets): 0.69 ms -- three per-lane LDS operations per pair cost more issue time than the
      // quarter-rate exponential they save; the broadcast form below reads each value once for all 64 lanes.)
      const bool factored = amax <= 8.f;                   // (wave-uniform; NaN -> the direct form)
      if (lane < 4 && cnt + lane < ((cnt + 3) & ~3)) {      // padding to a multiple of four: a pair that contributes exp2(-inf) = 0 in either form
        vf[cnt + lane] = factored ? 0.f : __int_as_float(0x7f800000);
        nf[cnt + lane] = __int_as_float(0xff800000);
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xc07f);
      // (Measured and dropped in round 3: giving the cnt % 64 samples of the last slot 64 / b lanes each -- groups of b = 32, 16, ..
      // samples by the binary digits of the remainder, each lane a share of the values, shares added by xor shuffles: 25 + 13 + 2 steps
      // of four values per lane at window 100 instead of 25 + 25, 20 % fewer exponentials by counter, and no faster: 0.292 against
      // 0.287 ms.  Per-lane LDS addresses and the shuffles cost what the idle lanes did.)
      float d32[KPL], xs[KPL];
      float acc[KPL][4];                                   // one accumulator per position in the group of four: <= ceil(cnt / 4) terms each
#pragma unroll
      for (int u = 0; u < KPL; ++u) {
        const int k = lane + 64 * u;
        xs[u] = vf[k < cnt ? k : 0];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[u][c] = 0.f;
      }
      const int nu = (cnt + 63) >> 6;                                             // sample slots in use (wave-uniform)
      if (factored) {
        // exp2(-(x - v)^2) = exp2(-x^2) exp2(2 x v - v^2): the pair costs a fused multiply-add (2 x in a register, v and -v^2 from
        // LDS), an exp2 and an add -- three issue slots instead of four -- and exp2(-x^2) multiplies the finished sum once.
        // |x|, |v| <= 8 keeps 2 x v - v^2 <= x^2 <= 64 inside the fp32 exponent range and its rounding (the product's and
        // -v^2's: 2^-24 x 64 each at the very worst) inside the budget written out at the threshold below.
        float x2[KPL];
#pragma unroll
        for (int u = 0; u < KPL; ++u) x2[u] = 2.f * xs[u];
        for (int m = 0; m < cnt; m += 4) {
          const float4 q4 = *reinterpret_cast<const float4*>(vf + m);
          const float4 n4 = *reinterpret_cast<const float4*>(nf + m);
          const float vm[4] = {q4.x, q4.y, q4.z, q4.w}, nm[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            if (u >= nu) continue;
            // (two fused multiply-adds per instruction: v_pk_fma_f32 -- the same roundings)
            typedef float v2f __attribute__((ext_vector_type(2)));
            const v2f xx = {x2[u], x2[u]};
            const v2f a01 = __builtin_elementwise_fma(xx, v2f{vm[0], vm[1]}, v2f{nm[0], nm[1]});
            const v2f a23 = __builtin_elementwise_fma(xx, v2f{vm[2], vm[3]}, v2f{nm[2], nm[3]});
            acc[u][0] += __builtin_amdgcn_exp2f(a01.x); acc[u][1] += __builtin_amdgcn_exp2f(a01.y);
            acc[u][2] += __builtin_amdgcn_exp2f(a23.x); acc[u][3] += __builtin_amdgcn_exp2f(a23.y);
          }
        }
#pragma unroll
        for (int u = 0; u < KPL; ++u) d32[u] = ((acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3])) * __builtin_amdgcn_exp2f(-(xs[u] * xs[u]));
      } else {
        for (int m = 0; m < cnt; m += 4) {
          const float4 q4 = *reinterpret_cast<const float4*>(vf + m);
          const float vm[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            if (u >= nu) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) { const float d = xs[u] - vm[c]; acc[u][c] += __builtin_amdgcn_exp2f(-(d * d)); }
          }
        }
#pragma unroll
        for (int u = 0; u < KPL; ++u) d32[u] = (acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3]);
      }
      float mx = -1.f;
#pragma unroll
      for (int u = 0; u < KPL; ++u) {
        if (lane + 64 * u >= cnt) d32[u] = -1.f;
        mx = fmaxf(mx, d32[u]);
      }
      mx = wave_max(mx);
      // Relative error of an fp32 density D~ against the exact D, all terms positive.  Direct form, exp2(-(x - v)^2):
      //  * arguments: a centred, rescaled sample y carries 2^-24 |y| <= 1e-6 (|y| < 32 for every pair that contributes: two of <= 256
      //    samples within a few units of each other lie at most 2.6 sqrt(255 / 2) = 29 units from the mean; a lone outlier beyond that
      //    sees only its own term, exactly 1), a difference d twice that, d^2 an absolute 2 |d| 2e-6 (+ 2^-24 d^2 from the product);
      //    a term's relative error is ln 2 times that, and weighted by the terms themselves (|d| 2^(-d^2) <= 0.52, the self term is 1)
      //    the sum's is <= 3e-6;
      //  * v_exp_f32: 1 ulp = 1.2e-7;
      //  * accumulation: four partial sums of <= 64 terms, each add 2^-24 of a partial sum that never exceeds the result: 3.8e-6, + 1.2e-7
      //    for the two combining adds
      // -> eps <= 7.1e-6 at window 256 (4.8e-6 at 100).  Factored form (all |y| <= 8), exp2(-x^2) exp2(2 x v - v^2):
      //  * the samples' own rounding (|y| <= 8: 2^-24 x 8): 0.7e-6 by the same weighting;
      //  * the argument 2 x v - v^2 (|.| <= 64): -v^2 rounded once, the fused multiply-add once, 2^-24 x 64 = 3.8e-6 absolute together
      //    at the very worst -> ln 2 x 3.8e-6 = 2.6e-6;  exp2(-x^2): x^2 rounded (1.9e-6 absolute -> 1.3e-6) + 1 ulp;
      //  * v_exp_f32 1.2e-7, accumulation 3.9e-6 as above, the closing product 6e-8
      // -> eps <= 8.8e-6.  If k* is the true arg-max, D~[k*] >= (1 - eps) D[k*] >= (1 - eps) D[j] >= (1 - eps) / (1 + eps) D~[j] for
      // every j: the screen keeps k* as long as its margin exceeds 2 eps = 1.8e-5.  Margin 4e-5 (rounds 2-3 used 2e-4 with one
      // accumulator per sample: 1.7 fp64 evaluations per timestep on random-normal values, 0.6 now).
      const float thr = mx * (1.f - 4e-5f);
      // pass 2: fp64 densities of the candidates, in ascending sample order (the first maximum is kept); of every sample if
      // pass 1 produced no candidate (a bandwidth so small that its reciprocal leaves the fp32 range makes the screen NaN).
      // A wave pays for a sequential sum as if all 64 lanes ran it, so a candidate's sum is NOT given to one lane with its
      // exponentials: the lanes compute a candidate's cnt exponentials side by side into LDS (two per lane at window 100), four
      // candidates per batch, then lane c adds candidate c's terms in index order -- the same additions in the same order as
      // the one-lane loop, hence the same bits, at 1/20 of its cycles.
      double best = -1.0;
      int besti = 0x7fffffff;
      double* tm = terms[wave];
      {
        // one candidate only: the screen has decided (its margin is far above the fp32 pass's error), no fp64 sum is needed
        int ncand = 0, first = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < KPL; ++u) {
          const unsigned long long mk = __ballot(lane + 64 * u < cnt && d32[u] >= thr);
          ncand += __builtin_popcountll(mk);
          if (mk && first == 0x7fffffff) first = __builtin_ctzll(mk) + 64 * u;
        }
        if (ncand == 1) besti = first;
      }
      double inv = 0.0;
      if (__builtin_amdgcn_readfirstlane(besti) == 0x7fffffff) inv = 0.5 / cov;          // (only the fp64 pass needs it)
      for (int round = 0; round < 2 && besti == 0x7fffffff; ++round) {
        // First the candidates' fp64 densities as TREE sums (a lane's own terms, then the wave's butterfly: no LDS, no sequential add):
        // either order of adding <= 256 positive terms is within 3e-14 of the exact sum, so a candidate more than 1e-12 below the
        // largest tree sum cannot be the arg-max of the ordered sums either.  One survivor (the usual case): it is the arg-max, and
        // the ordered sums -- a lane adding 100 terms one after the other: half of this pass's time -- are not taken at all; several
        // (equal samples, true near-ties): only those go through the ordered sums below, which decide as before.
        bool keep[KPL];
        {
          double dq[KPL];
#pragma unroll
          for (int u = 0; u < KPL; ++u) dq[u] = -1.0;
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            unsigned long long mask = __ballot(lane + 64 * u < cnt && (round == 1 || d32[u] >= thr));
            while (mask) {                                                        // wave-uniform
              const int k = __builtin_ctzll(mask) + 64 * u;
              mask &= mask - 1;
              const double xk = v[k];
              double loc = 0.0;
              for (int m = lane; m < cnt; m += 64) { const double d = xk - v[m]; loc += exp(-d * d * inv); }
              const double dp = wave_sum(loc);
              if (lane == (k & 63)) dq[u] = dp;
            }
          }
          double mx2 = -1.0;
#pragma unroll
          for (int u = 0; u < KPL; ++u) mx2 = fmax(mx2, dq[u]);
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) mx2 = fmax(mx2, __shfl_xor(mx2, off, WAVE));
          const double thr2 = mx2 * (1.0 - 1e-12);
          int nkeep = 0, first = 0x7fffffff;
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            keep[u] = dq[u] >= thr2 && dq[u] > 0.0;
            const unsigned long long mk = __ballot(keep[u]);
            nkeep += __builtin_popcountll(mk);
            if (mk && first == 0x7fffffff) first = __builtin_ctzll(mk) + 64 * u;
          }
          if (nkeep == 1) { besti = first; break; }
        }
#pragma unroll
        for (int u = 0; u < KPL; ++u) {
          unsigned long long mask = __ballot(keep[u]);
          while (mask) {                                                          // wave-uniform
            int kc[KDE_CB];
            int nb = 0;
#pragma unroll
            for (int c = 0; c < KDE_CB; ++c) {
              kc[c] = -1;
              if (mask) { kc[c] = __builtin_ctzll(mask) + 64 * u; mask &= mask - 1; nb = c + 1; }
            }
#pragma unroll
            for (int c = 0; c < KDE_CB; ++c) {
              if (kc[c] < 0) continue;
              const double xk = v[kc[c]];
              for (int m = lane; m < cnt; m += 64) { const double d = xk - v[m]; tm[c * WMAX + m] = exp(-d * d * inv); }
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);
            double dens = -1.0;
            if (lane < nb) {
              dens = 0.0;
              const double* tp = tm + lane * WMAX;
              int m = 0;
              for (; m + 8 <= cnt; m += 8) {                 // (the terms of eight steps requested together; added in index order)
                double t8[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) t8[x] = tp[m + x];
#pragma unroll
                for (int x = 0; x < 8; ++x) dens += t8[x];
              }
              for (; m < cnt; ++m) dens += tp[m];
            }
#pragma unroll
            for (int c = 0; c < KDE_CB; ++c) {
              const double dc = __shfl(dens, c, WAVE);
              if (c < nb && dc > best) { best = dc; besti = kc[c]; }
            }
            __builtin_amdgcn_wave_barrier();
          }
        }
      }
      out = v[besti < cnt ? besti : 0];                    // (all densities NaN -- a covariance whose reciprocal overflows: scipy's arg-max of NaNs is 0)
    } else {
      // median by rank counting (cnt <= 256)
      double lo = 0.0, hi = 0.0;
      for (int k = lane; k < cnt; k += 64) {
        const double xk = v[k];
        int rank = 0;
        for (int m = 0; m < cnt; ++m) rank += (v[m] < xk) || (v[m] == xk && m < k);
        if (rank == (cnt - 1) / 2) lo = xk;
        if (rank == cnt / 2) hi = xk;
      }
      out = 0.5 * (wave_sum(lo) + wave_sum(hi));
    }
    if (lane == 0) modes[t] = out;
    __builtin_amdgcn_wave_barrier();
  }
