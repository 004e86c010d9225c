// What lstm_fwd_lds2_kernel<K, H, NW> and lstm_fwd_lds3_kernel<K, H, NW> (lstm_t1_lds.hip) have in common up to their tile loops,
// included at the top of each kernel behind its column map:
//  * staging: this workgroup's direction, its W_ih as column tiles smem[ct][16][ld] in the order the kernel's map gives, the summed
//    biases bias_s[3][H] behind them, one barrier;
//  * the row-tile machinery: the lane coordinates, a wave's first tile with its x rows in registers (a[], at[]: load_group,
//    load_tail) and `pass`, one run of some column tiles through the whole K with the software prefetch of the next tile.
// Expects from the enclosing scope: the kernel's arguments, K, H, NW, NFB, REM and the macro HYPAD_LSTM_COLUMN(ct, n, gate, unit):
// statements that set gate (0 / 1 / 2 = i / g / o; 3: none) and unit of column n of tile ct.  Leaves smem, ld, NT, dir, bias_s, lane,
// wave, j, q, nt_ok, tile, tstep, ntiles, load_group, load_tail and pass for the kernel's tile loop.
// Shared as text, not as a function: see the note at unroll_median_signals_kernel (scoring.hip).  The column map too: as a lambda
// (either by reference or by value) it changed the bytes of all five instantiations (docs/history/lstm_t1_split.md).
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int KG = (K + 15) / 16;
  constexpr int NT = 3 * NFB + (REM ? 1 : 0), ld = KG * 16 + 4;
  static_assert(REM <= 5, "the remainder tile holds 3 x (H % 16) columns");
  static_assert(NFB >= 1 && NFB <= 4, "hidden <= 64");
  const int dir = blockIdx.x & 1, slice = blockIdx.x >> 1, nslices = gridDim.x >> 1;
  const float* __restrict__ w = dir ? wr : wf;
  const float* __restrict__ b1 = dir ? bir : bif;
  const float* __restrict__ b2 = dir ? bhr : bhf;
  float* bias_s = smem + lstm_lds2_floats(K, H) - 3 * H;     // [3][H]: b_ih + b_hh of gates i, g, o
  for (int idx = threadIdx.x; idx < NT * 16 * ld; idx += 64 * NW) {
    const int ct = idx / (16 * ld), rem = idx - ct * 16 * ld, n = rem / ld, k = rem - n * ld;
    int gate, unit;
    HYPAD_LSTM_COLUMN(ct, n, gate, unit)
    smem[idx] = (gate < 3 && unit < H && k < K) ? w[(int64_t)((gate == 0 ? 0 : gate + 1) * H + unit) * K + k] : 0.f;      // i, f, g, o -> i, g, o
  }
  for (int idx = threadIdx.x; idx < 3 * H; idx += 64 * NW) {
    const int gate = idx / H, unit = idx - gate * H, pg = (gate == 0 ? 0 : gate + 1) * H + unit;
    bias_s[idx] = b1[pg] + b2[pg];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = wave_id(), j = lane & 15, q = lane >> 4;
  const int64_t ntiles = (rows + 15) >> 4;
  constexpr int gfull = K >> 4;                               // full k-groups; the rest (K & 15) in `tq` quads
  constexpr int tq = ((K & 15) + 3) >> 2;
  const bool vec = (K & 3) == 0 && ((uintptr_t)x & 15) == 0;
  const bool nt_ok = (H & 15) == 0 && gates_save && ((uintptr_t)gates_save & 63) == 0;
  float4 a[gfull > 0 ? gfull : 1];                            // full groups: x[row][16 g + 4 q ..+ 3]
  float at[3] = {0.f, 0.f, 0.f};                              // tail: x[row][16 gfull + 4 c + q]
  auto load_group = [&](int64_t tile, int g) __attribute__((always_inline)) {
    const int64_t r0 = tile << 4;
    const int64_t row = r0 + j < rows ? r0 + j : rows - 1;
    const float* xr = x + row * K;
    const int k0 = 16 * g + 4 * q;
    if (vec) a[g] = *reinterpret_cast<const float4*>(xr + k0);
    else a[g] = make_float4(xr[k0], xr[k0 + 1], xr[k0 + 2], xr[k0 + 3]);
  };
  auto load_tail = [&](int64_t tile) __attribute__((always_inline)) {
    const int64_t r0 = tile << 4;
    const int64_t row = r0 + j < rows ? r0 + j : rows - 1;
    const float* xr = x + row * K;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int k = 16 * gfull + 4 * c + q;
      at[c] = (c < tq && k < K) ? xr[k] : 0.f;
    }
  };
  const int64_t tstep = (int64_t)nslices * NW;
  int64_t tile = (int64_t)slice * NW + wave;
  if (tile < ntiles) {
#pragma unroll
    for (int g = 0; g < gfull; ++g) load_group(tile, g);
    load_tail(tile);
  }
  // one pass: NTP column tiles starting at ct0 through the whole K; FETCH: the next tile's rows replace a[g] as soon as group g is
  // done (`next` is always a valid tile: the last one repeats itself -- no branch inside the loop)
  auto pass = [&](auto ntp_tag, auto fetch_tag, int ct0, f32x4* acc, int64_t next) __attribute__((always_inline)) {
    constexpr int NTP = decltype(ntp_tag)::value;
    constexpr bool fetch_next = decltype(fetch_tag)::value;
#pragma unroll
    for (int t = 0; t < NTP; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wb = smem + (ct0 * 16 + j) * ld + 4 * q;
#pragma unroll
    for (int g = 0; g < gfull; ++g) {
      {
        float4 b[NTP];
#pragma unroll
        for (int t = 0; t < NTP; ++t) b[t] = *reinterpret_cast<const float4*>(wb + t * 16 * ld + 16 * g);
#pragma unroll
        for (int t = 0; t < NTP; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].x, b[t].x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NTP; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].y, b[t].y, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NTP; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].z, b[t].z, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NTP; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].w, b[t].w, acc[t], 0, 0, 0);
        if constexpr (fetch_next) load_group(next, g);
      }
    }
    // the partial group: lane (n, q) of B holds W[n][16 gfull + 4 c + q]
    const float* wt = smem + (ct0 * 16 + j) * ld + 16 * gfull + q;
#pragma unroll
    for (int c = 0; c < tq; ++c) {
      float bt[NTP];
#pragma unroll
      for (int t = 0; t < NTP; ++t) bt[t] = wt[t * 16 * ld + 4 * c];
#pragma unroll
      for (int t = 0; t < NTP; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[c], bt[t], acc[t], 0, 0, 0);
    }
    if constexpr (fetch_next) load_tail(next);
  };
