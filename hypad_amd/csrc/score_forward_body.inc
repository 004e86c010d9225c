// Body of score_forward_packed_kernel<SC, LC, MT> and score_forward_signals_kernel<SC, LC, MT> (score_forward.hip), included after each
// kernel's prologue: encoder -> decoder -> head and row distances of one tile of 16 MT windows.
// Expects from the enclosing scope: a (the ScoreArgs of the tile's signal), r0 (the tile's first row within that signal), S, L, MT,
// ROWS, ldS, gp (the GenPack) and the LDS tiles xs, zs, bufA, bufB.
// Shared as text, not as a function: see the note in front of the signal-group kernels of score_forward.hip.
  const int valid = (int)(a.rows - r0 < ROWS ? a.rows - r0 : ROWS);
  const int lane = threadIdx.x & 63, wave = wave_id();
  tile_load_b(xs, ldS, a.x + r0 * a.x_ld, (int)a.x_ld, ROWS, S, valid);
  __syncthreads();
  encoder_fwd_tile_packed<false, false, MT>(xs, ldS, S, L, a.pk, gp, bufA, ENC_LDG, bufB, ENC_LDH, zs, nullptr, nullptr, valid);
  DecSave none{16, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  decoder_trunk_fwd_tile_packed<MT>(zs, L, S, a.pk, gp, bufA, bufB, ldS, no_drop(), [](int r) { return r; }, none, valid);
  if (a.eucl) tile_store_b(a.eucl + r0 * S, S, bufA, ldS, ROWS, S, valid);
  if (a.hyperbolic) {
    // the head on the reconstruction AND on the real windows (anomaly_detection.py:84-90): u rows of both, then the ball rows
    float* urec; float* ureal;
    if constexpr (MT == 1) {
      for (int i = threadIdx.x; i < 16 * ldS; i += blockDim.x) bufA[16 * ldS + i] = xs[i];      // rows 16-31: the real windows
      __syncthreads();
      gemm_nt_packed<2>(bufA, ldS, S, S, a.pk + gp.head, nullptr, bufB, ldS, 0);
      __syncthreads();
      head_rows_tile(bufB, ldS, 32, S, a.head_b);
      urec = bufB; ureal = bufB + 16 * ldS;
    } else {
      gemm_nt_packed<MT>(bufA, ldS, S, S, a.pk + gp.head, nullptr, bufB, ldS, 0);
      __syncthreads();                                       // (e has been read -- by the product and by the store above)
      gemm_nt_packed<MT>(xs, ldS, S, S, a.pk + gp.head, nullptr, bufA, ldS, 0);
      __syncthreads();
      head_rows_tile(bufB, ldS, ROWS, S, a.head_b);
      head_rows_tile(bufA, ldS, ROWS, S, a.head_b);
      urec = bufB; ureal = bufA;
    }
    __syncthreads();
    if (a.hyper) tile_store_b(a.hyper + r0 * S, S, urec, ldS, ROWS, S, valid);
    if (a.hyper_real) tile_store_b(a.hyper_real + r0 * S, S, ureal, ldS, ROWS, S, valid);
    if (a.rowdist && wave < 4 * MT) {
      // (pred = real window on the ball, true = reconstruction): anomaly_detection_utils.py:58-65; four rows per wave
      epl16_dispatch(S, [&](auto tag) {
        using R16 = RowT<16, decltype(tag)::value>;
        const int r = wave * 4 + (lane >> 4);
        const float d = rowdist_row(row_load<R16>(ureal + r * ldS, S, lane), row_load<R16>(urec + r * ldS, S, lane));
        if ((lane & 15) == 0 && r < valid) a.rowdist[r0 + r] = d;
      });
    }
  }
