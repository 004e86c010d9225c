// One bias item of the dW + Adam launches: the column sums of 16 columns of `left` over the item's reduction rows, Adam on them, and the
// same gradient applied to a second destination (b_hh) where the item names one.  Text shared by dw_adam_items_body and
// dw_adam_critic_body (dw_adam.hip), included as the body of their `d.kind == DW_BIAS` branch.  Expects in scope:
//   d             the item, with DwItem's field names (n0, nrows, p_off, p_off2, left_off, left_ld, red_rows, and the packed position
//                 of the summed bias bsum, nbase, gate_H: bsum = -1 without copies)
//   P, M, V       the model's parameter / first-moment / second-moment arena of the item's network
//   ws            the model's workspace (rows at ws + d.left_off; packed copies at ws + a.pk_off)
//   co            AdamCoef of this step;  a: the launch's IterArgs
//   j, q          lane & 15, lane >> 4
//   KS            compile-time: rows per lane kept in flight
//   DW_CRITIC_LOAD_ORDER (optional macro): the optimiser state is requested behind the sums instead of with the rows
      // 16 columns per item; lane (j, q) sums rows r = q (mod 4), then the four row classes are folded by shuffles
      const int n = d.n0 + j;
      const bool nv = n < d.nrows;
      const float* left = ws + d.left_off + (nv ? n : d.nrows - 1);
      const int rlast = d.red_rows - 1;
      // the optimiser state with the rows (one round trip: as a second one behind the sums it made the bias items the launch's long pole)
      const bool own = nv && q == 0;
      const int64_t o1 = d.p_off + (own ? n : 0), o2 = (d.p_off2 >= 0 ? d.p_off2 : d.p_off) + (own ? n : 0);
#ifndef DW_CRITIC_LOAD_ORDER
      const float p1_ = P[o1], m1_ = M[o1], v1_ = V[o1], p2_ = P[o2], m2_ = M[o2], v2_ = V[o2];
#endif
      float g = 0.f;
      for (int rc = 0; rc < d.red_rows; rc += 4 * KS) {    // KS rows per lane in flight
        float t[KS];
#pragma unroll
        for (int u = 0; u < KS; ++u) {
          const int r = rc + 4 * u + q;
          t[u] = left[(int64_t)(r < rlast ? r : rlast) * d.left_ld];
        }
#pragma unroll
        for (int u = 0; u < KS; ++u) g += rc + 4 * u + q < d.red_rows ? t[u] : 0.f;
      }
      g += __shfl_xor(g, 16, WAVE);
      g += __shfl_xor(g, 32, WAVE);
      if (own) {
#ifdef DW_CRITIC_LOAD_ORDER
        // (behind the sums, where the critic launches always requested it: requested with the rows the compiler contracts the two
        // updates below the other way round -- fma(b1, m, (1 - b1) g) for fma(1 - b1, g, b1 m) -- and the critics' bias moments leave
        // the bits they had)
        const float p1_ = P[o1], m1_ = M[o1], v1_ = V[o1], p2_ = P[o2], m2_ = M[o2], v2_ = V[o2];
#endif
        float p = p1_, m = m1_, v = v1_;
        adam_update(p, m, v, g, co);
        P[o1] = p; M[o1] = m; V[o1] = v;
        float bs = p;
        if (d.p_off2 >= 0) {
          p = p2_; m = m2_; v = v2_;
          adam_update(p, m, v, g, co);
          P[o2] = p; M[o2] = m; V[o2] = v;
          bs += p;
        }
        if (d.bsum >= 0) {
          int nf = d.nbase + n;
          if (d.gate_H > 0) { const int x = nf / d.gate_H; nf = x * ((d.gate_H + 15) & ~15) + nf - x * d.gate_H; }
          ws[a.pk_off + d.bsum + nf] = bs;
        }
      }
