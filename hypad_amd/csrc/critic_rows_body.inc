// Body of critic_rows_kernel<SC, LC> and critic_rows_signals_kernel<SC, LC> (score_forward.hip), included after each kernel's
// prologue: the workgroup stages the padded critic_x image, then its waves walk the 16-row tiles of one signal.
// Expects from the enclosing scope: smem (the dynamic LDS), cxpad (the signal's padded image), x, x_ld (its windows), out (its output),
// rows (its windows' count), S, L and SC.
// Shared as text, not as a function: see the note in front of the signal-group kernels of score_forward.hip.
  const CriticPad cp = critic_pad(S, L, 4);
  const int ldin = cp.ldin, LQ = cp.LQ, nh = 4;
  const int lane = threadIdx.x & 63, wave = wave_id();
  float* in = smem + cp.total + wave * (16 * ldin + 2 * 16 * LQ);
  float* act = in + 16 * ldin;
  stage_params(smem, cxpad, cp.total);
  // the tile's constant part: the ones column behind the window (the layer's bias sits in that column of the image), zero padding
  for (int i = lane; i < 16 * ldin; i += 64) { const int c = i % ldin; in[i] = c == S ? 1.f : 0.f; }
  for (int i = lane; i < 2 * 16 * LQ; i += 64) act[i] = 0.f;
  __syncthreads();
  const float* w0 = smem + cp.w0; const float* wh = smem + cp.wh; const float* wl = smem + cp.wl;
  const int nwaves = blockDim.x >> 6;
  const int64_t tiles = (rows + 15) >> 4, stride = (int64_t)gridDim.x * nwaves;
  constexpr int NV = SC ? (16 * SC + 63) / 64 : 1;     // floats of a tile per lane (compiled-in window; any other streams its rows)
  float xr[NV];
  auto fetch = [&](int64_t t) __attribute__((always_inline)) {
    const int64_t r0 = t * 16;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i = lane + 64 * u, r = i / S, c = i - r * S;
      const int64_t row = r0 + r < rows ? r0 + r : rows - 1;
      xr[u] = i < 16 * S ? x[row * x_ld + c] : 0.f;
    }
  };
  int64_t t = (int64_t)blockIdx.x * nwaves + wave;
  if constexpr (SC != 0) { if (t < tiles) fetch(t); }
  for (; t < tiles; t += stride) {
    if constexpr (SC != 0) {
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int i = lane + 64 * u, r = i / S, c = i - r * S;
        if (i < 16 * S) in[r * ldin + c] = xr[u];
      }
    } else {
      for (int i = lane; i < 16 * S; i += 64) {
        const int r = i / S, c = i - r * S;
        const int64_t row = t * 16 + r < rows ? t * 16 + r : rows - 1;
        in[r * ldin + c] = x[row * x_ld + c];
      }
    }
    wave_lds_fence();
    if constexpr (SC != 0) { if (t + stride < tiles) fetch(t + stride); }          // the next tile's rows arrive under this tile's layers
    for (int li = 0; li < nh; ++li) {
      const float* A = li == 0 ? in : act + ((li - 1) & 1) * 16 * LQ;
      const float* Wl = li == 0 ? w0 : wh + (li - 1) * L * LQ;
      float* ao = act + (li & 1) * 16 * LQ;
      wave_gemm_nt(A, li == 0 ? ldin : LQ, Wl, li == 0 ? ldin : LQ, L, L + 1, li == 0 ? cp.Kin : cp.Lp, lane, [&](int r, int c, float pre) {
        if (c < L) ao[r * LQ + c] = pre * leaky_slope(pre);
        else if (c == L) ao[r * LQ + c] = 1.f;
      });
      wave_lds_fence();
    }
    if (lane < 16) {
      const float* xa = act + ((nh - 1) & 1) * 16 * LQ + lane * LQ;
      float o = 0.f;
      for (int c = 0; c <= L; ++c) o += xa[c] * wl[c];
      if (t * 16 + lane < rows) out[t * 16 + lane] = o;
    }
    wave_lds_fence();
  }
