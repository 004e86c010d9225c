// One weight item of the dW + Adam launches: a 16 x 16 tile of dW = left^T right on MFMA over the item's reduction rows, Adam on the
// lane's four elements in registers, the arena and (generator) the packed copies written back.  Text shared by dw_adam_items_body and
// dw_adam_critic_body (dw_adam.hip), included as the body of their `d.kind == DW_WEIGHT` branch.  Expects in scope:
//   d             the item, with DwItem's field names (n0, k0, nrows, ncols, p_off, p_ld, left_off, left_ld, right_off, right_ld,
//                 red_rows, and the packed positions fwd, fwd_kg, nbase, bwd, bwd_ng, mbase, gate_H: fwd = bwd = -1 without copies)
//   P, M, V       the model's parameter / first-moment / second-moment arena of the item's network
//   ws            the model's workspace (operand rows at ws + d.left_off / d.right_off; packed copies at ws + a.pk_off)
//   co            AdamCoef of this step;  a: the launch's IterArgs
//   lane, j, q    lane of the wave, lane & 15, lane >> 4
//   KS            compile-time: k-steps (groups of four reduction rows) kept in flight
//   DW_CRITIC_LOAD_ORDER (optional macro): the optimiser state is requested in front of the operand rows instead of behind their first batch
      const int n0 = d.n0, k0 = d.k0;
      // out-of-range columns are clamped (their results are dropped below); rows past red_rows contribute zeros
      const int nj = n0 + j < d.nrows ? n0 + j : d.nrows - 1, kj = k0 + j < d.ncols ? k0 + j : d.ncols - 1;
      // Operands through buffer loads: one per-lane byte offset (row q, column nj / kj) plus a scalar row offset per load,
      // so the ~100 loads of an item cost no vector address arithmetic (with flat addressing that arithmetic took longer
      // than the memory round trip).  Row offsets are clamped on the scalar side; masked rows contribute zeros below.
      const __amdgpu_buffer_rsrc_t lrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ws + d.left_off), 0, 0x7fffffff, 0x00020000);
      const __amdgpu_buffer_rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ws + d.right_off), 0, 0x7fffffff, 0x00020000);
      // red_rows is a multiple of 16 (whole batches of B = 16 m rows): the reduction runs in groups of four k-steps, each
      // entirely in range, so nothing is clamped or masked.
      const int lvo = (q * d.left_ld + nj) * 4, rvo = (q * d.right_ld + kj) * 4;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      // the optimiser state of this lane's four elements travels with the operand loads (one round trip, not two)
      int po[4]; float pp[4], pm[4], pvv[4];
      float* Pb = P + d.p_off; float* Mb = M + d.p_off; float* Vb = V + d.p_off;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 4 * q + r, k = k0 + j;
        const bool ok = n < d.nrows && k < d.ncols;
        po[r] = ok ? n * d.p_ld + k : -1;
      }
      // (requested BEHIND the first batch of operand rows -- loads return in order, and the products need only the rows.  With
      // DW_CRITIC_LOAD_ORDER defined in front of the #include it is requested before them, as the critic launches always did)
      auto load_state = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t oc = po[r] >= 0 ? (uint32_t)po[r] : 0u;
          pp[r] = Pb[oc]; pm[r] = Mb[oc]; pvv[r] = Vb[oc];
        }
      };
#ifdef DW_CRITIC_LOAD_ORDER
      load_state();
#else
      if (d.red_rows <= 0) load_state();
#endif
      for (int rc = 0; rc < d.red_rows; rc += 4 * KS) {    // up to KS k-steps in flight
        float la[KS], rb[KS];
#pragma unroll
        for (int c = 0; c < KS / 4; ++c)
          if (rc + 16 * c < d.red_rows) {                  // wave-uniform
#pragma unroll
            for (int u = 4 * c; u < 4 * c + 4; ++u) {
              la[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(lrs, lvo, (rc + 4 * u) * d.left_ld * 4, 0));
              rb[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrs, rvo, (rc + 4 * u) * d.right_ld * 4, 0));
            }
          }
#ifndef DW_CRITIC_LOAD_ORDER
        if (rc == 0) load_state();
#endif
#pragma unroll
        for (int c = 0; c < KS / 4; ++c)
          if (rc + 16 * c < d.red_rows) {
#pragma unroll
            for (int u = 4 * c; u < 4 * c + 4; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(la[u], rb[u], acc, 0, 0, 0);
          }
      }
      float* pk = ws + a.pk_off;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = pp[r], m = pm[r], v = pvv[r];
        adam_update(p, m, v, acc[r], co);
        if (po[r] >= 0) {
          const uint32_t o = (uint32_t)po[r];
          Pb[o] = p; Mb[o] = m; Vb[o] = v;
          const int nc = d.nbase + n0 + 4 * q + r, k = k0 + j;             // compact row, column
          if (d.fwd >= 0) {
            int nf = nc;                                                     // forward copy row: gates padded to 16-row blocks
            if (d.gate_H > 0) nf += ((nc >= d.gate_H) + (nc >= 2 * d.gate_H)) * (((d.gate_H + 15) & ~15) - d.gate_H);   // nc < 3H
            pk[d.fwd + (((nf >> 4) * d.fwd_kg + (k >> 4)) * 64 + (nf & 15) + 16 * ((k & 15) >> 2)) * 4 + (k & 3)] = p;
          }
          if (d.bwd >= 0) {
            const int mm = d.mbase + nc;                                      // reduction index of the transposed copy
            pk[d.bwd + (((k >> 4) * d.bwd_ng + (mm >> 4)) * 64 + (k & 15) + 16 * ((mm & 15) >> 2)) * 4 + (mm & 3)] = p;
          }
        }
      }
