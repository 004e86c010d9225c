// The three WGAN-GP minibatch steps of train.py (critic_x_iteration :18-104, critic_z_iteration :107-186,
// decoder_iteration :189-249) with the optimizer step fused in.
//
// Launch structure (every kernel: one model per blockIdx.y):
//   hypad_critic_{x,z}_iteration (per-iteration entry points; also hypad_train_epoch's fallback for shapes that
//   critic_fused.hip cannot take):
//                          pass kernel  (row tiles: frozen generator forward, 3 critic passes, first GP backward, partial norms)
//                          gp kernel    (row tiles: whole-batch norm -> second-order chain)
//                          dw_adam      (16x16 weight tiles: dW = left^T right on MFMA, Adam in registers)
//   hypad_decoder_iteration:
//                          pack kernel  (MFMA-native copies of the generator weights into the workspace; inside an epoch the
//                                        dW kernel keeps them current instead)
//                          gen kernel   (one workgroup per (row tile, chain): G = z -> decoder -> critic_x and back,
//                                        R = x -> encoder -> critic_z, decoder, reconstruction loss and back; every
//                                        (delta, activation) pair written for dw_adam)
//                          dw_adam      (Adam or Riemannian Adam; writes arena + packed copies)
//   hypad_train_epoch:     pack once -> critic phase (critic_fused.hip: precompute + one launch per critic_x || critic_z
//                          iteration) -> n_batches x (gen, dw_adam)
// The dw_adam launches -- kernels, descriptor tables, launch code -- are dw_adam.hip, reached through the launch_dw_* functions of
// train_common.h; this file holds the row-tile kernels that write their operand rows, the pack launch and the entry points.
// Training only: the scoring forward pass (score_forward.hip) borrows the pack launch through launch_pack_generator, and the
// stand-alone optimiser steps are in ops_dense.hip.
// No gradient buffer exists: a weight's gradient tile lives in MFMA accumulators and is consumed by the update.
// Formulas: oracle/manual.py (CPU derivation sheet, validated against autograd and the reference fixtures).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include <vector>

#include "../../include/hypad.h"
#include "critic_mfma.h"
#include "train_common.h"

using namespace hypad;
using namespace hypad::train;

namespace {

// ------------------------------------------------------------------------------------------------ critic passes
// The three passes of a WGAN-GP critic update on one 16-row tile -- real (dout -1/B), fake (+1/B), interpolated
// (dout 1: the first backward of the gradient penalty, train.py:72-81) -- carried together as 48 rows on the VALU path
// (critic_valu.h).  Writes every (left, right) pair the dW kernel needs, the interpolated pass's masks for the
// gradient-penalty kernel, g = d(prob)/d(interpolated) and the tile's partial sums.
// real / fake: LDS tiles (in_dim columns).  inter: LDS [16][ldi] scratch; gbuf: LDS [16][ldgb] for g (may alias `real`:
// it is written after the last read of `real`).  P: the critic's weights (staged in LDS when they fit).
__device__ __forceinline__ void critic_three_passes(const IterArgs& a, int sig, int tile, uint32_t tick, const float* real, int ldr,
                                                    const float* fake, int ldf, float* inter, int ldi, float* gbuf, int ldgb,
                                                    const float* P, const CriticLayout& cl, const CriticBatchLds& cb, float* ws,
                                                    const CritWs& cw, int mask_real, int mask_fake, int mask_inter, float* red) {
  const int L = a.L, B = a.B, nh = cl.nh, in_dim = cl.in_dim, LQ = cb.LQ;
  const int g0 = tile * 16;
  const float* mbase = a.masks ? a.masks + sig * a.mask_sig_stride : nullptr;
  const int64_t mblk = (int64_t)nh * B * L;
  const int midx[3] = {mask_real, mask_fake, mask_inter};
  DropSrc ds[3];
#pragma unroll
  for (int p = 0; p < 3; ++p)
    ds[p] = drop_src(a, sig, mbase ? mbase + midx[p] * mblk : nullptr, RS_DROP_CRITIC + 8 * midx[p], tick, cl.p_drop);
  // interpolation (train.py:64-69 / 149-154)
  const float* ainj = a.alpha ? a.alpha + ((int64_t)sig * B + g0) * in_dim : nullptr;
  tile_for(16, in_dim, [&](int r, int c) {
    float al = ainj ? ainj[r * in_dim + c] : rng_uniform(a.seed, tick, RS_ALPHA, (uint32_t)(sig + a.rng_sig0), (uint32_t)((g0 + r) * in_dim + c));
    inter[r * ldi + c] = al * real[r * ldr + c] + (1.f - al) * fake[r * ldf + c];
  });
  __syncthreads();
  critic_batch_fwd([&](int r) { return r < 16 ? real + r * ldr : r < 32 ? fake + (r - 16) * ldf : inter + (r - 32) * ldi; },
                   P, cl, L, cb,
                   [&](int li, int r, int c) {
                     const int p = r >> 4;
                     return p == 0 ? ds[0].get(li, g0 + (r & 15), c, L) : p == 1 ? ds[1].get(li, g0 + (r & 15), c, L)
                                                                                   : ds[2].get(li, g0 + (r & 15), c, L);
                   });
  // what dW needs from the forward: layer inputs of the real / fake passes, masks of the interpolated pass
  tile_store(ws + cw.in_right + (int64_t)g0 * in_dim, in_dim, real, ldr, 16, in_dim, 16);
  tile_store(ws + cw.in_right + ((int64_t)B + g0) * in_dim, in_dim, fake, ldf, 16, in_dim, 16);
  for (int li = 0; li < nh; ++li) {
    tile_store_p(ws + cw.act[li] + (int64_t)g0 * L, L, B, cb.act + li * cb.R * LQ, LQ, 32, L, 32);
    tile_store(ws + cw.dm[li] + (int64_t)g0 * L, L, cb.dm + (li * cb.R + 32) * LQ, LQ, 16, L, 16);
  }
  float* sums = red + 32;
  if (threadIdx.x < 2) {
    float s = 0.f;
    for (int r = 0; r < 16; ++r) s += cb.out[threadIdx.x * 16 + r];
    sums[threadIdx.x] = s;
  }
  if (threadIdx.x < 48) {
    const int p = threadIdx.x >> 4;
    ws[cw.left[nh] + (int64_t)p * B + g0 + (threadIdx.x & 15)] = p == 0 ? -1.f / B : p == 1 ? 1.f / B : 1.f;
  }
  const float invB = 1.f / B;
  const float* d0 = critic_batch_bwd([&](int r) { return r < 16 ? -invB : r < 32 ? invB : 1.f; }, P, cl, L, cb,
                                     [&](int li, const float* delta) { tile_store_p(ws + cw.left[li] + (int64_t)g0 * L, L, B, delta, LQ, 48, L, 48); });
  // g = delta_0 W_0 for the interpolated rows (train.py:75-81)
  dense_rows_valu_t(d0 + 32 * LQ, LQ, L, P + cl.wof(0), in_dim, 16, [&](int r, int c, float v) { gbuf[r * ldgb + c] = v; });
  __syncthreads();
  tile_store(ws + cw.in_right + ((int64_t)2 * B + g0) * in_dim, in_dim, gbuf, ldgb, 16, in_dim, 16);
  float sq = 0.f;
  tile_for(16, in_dim, [&](int r, int c) { float v = gbuf[r * ldgb + c]; sq += v * v; });
  sq = block_sum(sq, red);
  if (threadIdx.x == 0) {
    float* part = ws + cw.partial + tile * 4;
    part[0] = sq; part[1] = sums[0]; part[2] = sums[1]; part[3] = 0.f;
  }
}

__device__ __forceinline__ void load_z(const IterArgs& a, int sig, int tile, uint32_t tick, float* zs /* [16][LP] */) {
  const float* zinj = a.z ? a.z + ((int64_t)sig * a.B + tile * 16) * a.L : nullptr;
  const int L = a.L;
  if (zinj || (L & 1)) {
    tile_for(16, L, [&](int r, int c) {
      zs[r * LP + c] = zinj ? zinj[r * L + c] : rng_normal(a.seed, tick, RS_Z, (uint32_t)(sig + a.rng_sig0), (uint32_t)((tile * 16 + r) * L + c));
    });
  } else {                                  // two normals per Philox evaluation: the same numbers as rng_normal per element
    for (int i = threadIdx.x; i < 16 * (L >> 1); i += blockDim.x) {
      const int r = i / (L >> 1), c = 2 * (i - r * (L >> 1));
      const uint32_t idx = (uint32_t)((tile * 16 + r) * L + c);
      Philox ph(a.seed);
      const uint4 rr = ph(idx >> 1, RS_Z, tick, (uint32_t)(sig + a.rng_sig0));
      zs[r * LP + c] = sqrtf(-2.0f * __logf(u32_to_unit_open(rr.x))) * __cosf(6.28318530717958647692f * u32_to_unit(rr.y));
      zs[r * LP + c + 1] = sqrtf(-2.0f * __logf(u32_to_unit_open(rr.z))) * __cosf(6.28318530717958647692f * u32_to_unit(rr.w));
    }
  }
}

// ---- critic_x pass (train.py:18-81)
__device__ __forceinline__ void cx_pass_body(const IterArgs& a, float* smem) {
  const int sig = blockIdx.y, tile = blockIdx.x, S = a.S, L = a.L, B = a.B;
  const CriticLayout cl = cx_layout(S, L);
  const LdsPlan lp = lds_plan(S, 16, 16, cl.total, critic_batch_lds_floats(48, L));
  const DecLayout dl = dec_layout(S, L, a.hyperbolic);
  const CritWs cw = crit_ws(B, S, L, 4);
  const float* PD = a.P.dec + (int64_t)sig * a.pd;
  const float* PC = a.P.cx + (int64_t)sig * a.pcx;
  float* ws = a.ws + sig * a.ws_sig_stride;
  float* xs = smem + lp.xs; float* zs = smem + lp.zs; float* bufA = smem + lp.bufA; float* bufB = smem + lp.bufB;
  float* red = smem + lp.small + 3 * 16 * LP;
  const CriticBatchLds cs = critic_batch_lds(smem + lp.crit, 48, L);
  const uint32_t tick = (uint32_t)a.counters[3];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.counters[a.opt] += 1;
  if (lp.stage) { stage_params(smem + lp.cparams, PC, cl.total); PC = smem + lp.cparams; }

  tile_load_rows(xs, lp.ldS, a.x + sig * a.x_sig_stride, a.x_ld, a.row_index ? a.row_index + (int64_t)sig * a.ri_sig_stride : nullptr, tile * 16, 16, S, 16);
  load_z(a, sig, tile, tick, zs);
  __syncthreads();
  // decoder (frozen, train-mode dropout): x_ = decoder(z)
  const float* mbase = a.masks ? a.masks + sig * a.mask_sig_stride : nullptr;
  DropSrc ddrop = drop_src(a, sig, mbase ? mbase + (int64_t)12 * B * L : nullptr, RS_DROP_DEC0, tick, 0.2f);
  DecSave none{16, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const int grow0 = tile * 16;
  float* wst = smem + lp.wst;
  decoder_trunk_fwd_tile<1>(zs, L, S, PD, dl, bufA, bufB, lp.ldS, ddrop, [grow0](int r) { return grow0 + r; }, none, 16, wst);
  float* gen = bufA; float* other = bufB;
  if (a.hyperbolic) {
    gemm_nt<1>(bufA, lp.ldS, PD + dl.head_w, S, S, S, identity_map(), nullptr, nullptr, bufB, lp.ldS, 0, wst);
    __syncthreads();
    head_rows_tile(bufB, lp.ldS, 16, S, PD + dl.head_b);
    __syncthreads();
    gen = bufB; other = bufA;
  }
  // `other` receives the interpolation; g reuses the x tile (dead once the interpolation exists)
  critic_three_passes(a, sig, tile, tick, xs, lp.ldS, gen, lp.ldS, other, lp.ldS, xs, lp.ldS, PC, cl, cs, ws, cw, 0, 1, 2, red);
}

// ---- critic_z pass (train.py:107-166)
__device__ __forceinline__ void cz_pass_body(const IterArgs& a, float* smem) {
  const int sig = blockIdx.y, tile = blockIdx.x, S = a.S, L = a.L, B = a.B;
  const CriticLayout cl = cz_layout(L);
  const LdsPlan lp = lds_plan(S, 16, 16, cl.total, critic_batch_lds_floats(48, L));
  const EncLayout el = enc_layout(S, L);
  const CritWs cw = crit_ws(B, L, L, 2);
  const float* PE = a.P.enc + (int64_t)sig * a.pe;
  const float* PC = a.P.cz + (int64_t)sig * a.pcz;
  float* ws = a.ws + sig * a.ws_sig_stride;
  float* xs = smem + lp.xs; float* zs = smem + lp.zs; float* bufA = smem + lp.bufA; float* bufB = smem + lp.bufB;
  float* small = smem + lp.small;
  float* red = small + 3 * 16 * LP;
  const CriticBatchLds cs = critic_batch_lds(smem + lp.crit, 48, L);
  const uint32_t tick = (uint32_t)a.counters[3];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) a.counters[a.opt] += 1;
  if (lp.stage) { stage_params(smem + lp.cparams, PC, cl.total); PC = smem + lp.cparams; }

  tile_load_rows(xs, lp.ldS, a.x + sig * a.x_sig_stride, a.x_ld, a.row_index ? a.row_index + (int64_t)sig * a.ri_sig_stride : nullptr, tile * 16, 16, S, 16);
  load_z(a, sig, tile, tick, zs);                       // real = z ~ N(0,1)
  __syncthreads();
  float* zenc = zs + 16 * LP;                           // fake = encoder(x)
  encoder_fwd_tile(xs, lp.ldS, S, L, PE, el, bufA, ENC_LDG, bufB, ENC_LDH, zenc, nullptr, nullptr, 16, smem + lp.wst);
  // injected mask order (hypad.h): fake | valid | interpolated
  critic_three_passes(a, sig, tile, tick, zs, LP, zenc, LP, small, LP, small + 16 * LP, LP, PC, cl, cs, ws, cw, 1, 0, 2, red);
}

// ---- gradient-penalty body: whole-batch norm and the second-order chain (oracle/manual.py
// critic_gp_pairs): GP rows of every `right` matrix.
template <bool IS_X>
__device__ __forceinline__ void gp_body(const IterArgs& a, float* smem) {
  const int sig = blockIdx.y, tile = blockIdx.x, L = a.L, B = a.B;
  const int in_dim = IS_X ? a.S : a.L;
  const int nh = IS_X ? 4 : 2;
  const CriticLayout cl = IS_X ? cx_layout(a.S, L) : cz_layout(L);
  const CritWs cw = crit_ws(B, in_dim, L, nh);
  const float* PC = IS_X ? a.P.cx + (int64_t)sig * a.pcx : a.P.cz + (int64_t)sig * a.pcz;
  float* ws = a.ws + sig * a.ws_sig_stride;
  const int ldu = pad4(in_dim) + 4;
  float* us = smem;                         // [16][ldu]
  float* e0 = us + 16 * ldu;                // [16][LP]
  float* e1 = e0 + 16 * LP;                 // [16][LP]
  float* pc = e1 + 16 * LP;                 // staged critic weights
  stage_params(pc, PC, cl.total);
  PC = pc;
  const int ntiles = B / 16;
  float gsum = 0.f, sreal = 0.f, sfake = 0.f;
  for (int t = 0; t < ntiles; ++t) {        // fixed order: deterministic
    const float* part = ws + cw.partial + t * 4;
    gsum += part[0]; sreal += part[1]; sfake += part[2];
  }
  const float nrm = sqrtf(gsum + 1e-12f);                       // train.py:90
  const float gp = (nrm - 1.f) * (nrm - 1.f);
  const float coef = 10.f * 2.f * (nrm - 1.f) / nrm;            // d(10 gp)/d g = coef * g
  if (tile == 0 && threadIdx.x == 0) {
    float* lo = a.losses + sig * a.loss_sig_stride;
    lo[0] = sfake / B - sreal / B + 10.f * gp;                  // train.py:98-99
    lo[1] = gp; lo[2] = sreal / B; lo[3] = sfake / B;
  }
  float* grow = ws + cw.in_right + ((int64_t)2 * B + tile * 16) * in_dim;
  tile_for(16, in_dim, [&](int r, int c) {
    const float u = coef * grow[r * in_dim + c];
    grow[r * in_dim + c] = u;                // right of layer 0 (GP rows) = ugrad
    us[r * ldu + c] = u;
  });
  __syncthreads();
  dense_rows_valu(us, ldu, in_dim, PC + cl.wof(0), nullptr, 16, L, [&](int r, int c, float v) { e0[r * LP + c] = v; });
  __syncthreads();
  float* cur = e0; float* nxt = e1;
  for (int li = 1; li <= nh; ++li) {
    // ep_{li-1} = e_{li-1} * dm_{li-1}: right of layer li (GP rows)
    const float* dm = ws + cw.dm[li - 1] + (int64_t)tile * 16 * L;
    float* dst = ws + cw.act[li - 1] + ((int64_t)2 * B + tile * 16) * L;
    tile_for(16, L, [&](int r, int c) {
      const float v = cur[r * LP + c] * dm[r * L + c];
      cur[r * LP + c] = v;
      dst[r * L + c] = v;
    });
    __syncthreads();
    if (li < nh) {
      dense_rows_valu(cur, LP, L, PC + cl.wof(li), nullptr, 16, L, [&](int r, int c, float v) { nxt[r * LP + c] = v; });
      __syncthreads();
      float* t = cur; cur = nxt; nxt = t;
    }
  }
}
HD int gp_lds_floats(int in_dim, int critic_floats) { return 16 * (pad4(in_dim) + 4) + 2 * 16 * LP + critic_floats; }

// ------------------------------------------------------------------------------------------------ generator body
// decoder_iteration (train.py:189-249).  Its three chains are independent until the weight gradients are summed:
//   role 0 (G):  z ~ N(0,1) -> decoder -> critic_x -> -mean(fake_x)                      and back through the decoder;
//   role 1 (R):  x -> encoder -> decoder -> reconstruction loss against x (hyperbolic: Poincare distance between the
//                Moebius heads of x_rec and of x) and back through decoder and encoder;
//   role 2 (Z):  x -> encoder -> critic_z -> -mean(fake_z) and back through the encoder (gen_role_z).  The encoder's
//                backward is linear in the gradient of its output, so the two contributions (through the decoder, chain R;
//                through critic_z, chain Z) are propagated separately and meet in the weight-gradient reduction, which runs
//                over both chains' operand rows (train_common.h GenWs).  Chain Z repeats the encoder forward of its 16 rows
//                -- 13 k cycles on its own CU -- and takes critic_z (7 k cycles, five barrier-separated 20-wide stages) off
//                chain R, the longest of the three.
// One workgroup per (16-row tile, role): blockIdx.z = role.  Operand rows in the workspace are pass-major as before:
// pass 0 = decoder(z), pass 1 = decoder(encoder(x)), pass 2 (hyperbolic only) = hyperbolic_linear(x).
struct GenLds {
  int hb, xs, zs, bufA, bufB, small, cw, ct, total, ldS;
};
HD GenLds gen_lds(int S, int L, int hyper, int role) {
  GenLds p;
  p.ldS = lds_stride(S);
  const CriticPad cp = role == 0 ? critic_pad(S, L, 4) : critic_pad(L, L, 2);      // (chain R stages no critic; same plan as Z)
  const int rows_head = (role == 1 && hyper) ? 32 : 16;
  const int a = 16 * (6 * DEC_H + 4), b = rows_head * p.ldS;
  const int bufFloats = a > b ? a : b;
  int o = 0;
  p.hb = o; o += (role == 1 && hyper) ? 16 * p.ldS : 0;   // chain R, hyperbolic: the head's 32 input rows = [tanh output | real windows],
  p.xs = o; o += role >= 1 ? 16 * p.ldS : 0;              // contiguous: the windows are gathered straight into the second half
  p.zs = o; o += 32 * LP;
  p.bufA = o; o += bufFloats;
  p.bufB = o; o += bufFloats;
  p.small = o; o += 3 * 16 * LP + 64;             // dzc | dzs | spare, then 64 reduction slots
  p.cw = o; o += cp.total;                        // the role's frozen critic, padded image (critic_mfma.h)
  p.ct = o; o += critic_tile_floats(cp, role == 0 ? 4 : 2);
  p.total = o;
  return p;
}

// Chain Z of the generator step (see above): encoder forward of the tile's windows, critic_z forward / backward, encoder
// backward of that gradient; operand rows into the second halves of xg / enc_h / dzenc / dgenc.
template <int SC, int LC, int BC, bool WSC1 = false>
__device__ __forceinline__ void gen_role_z(const IterArgs& a, float* smem) {
  const int S = SC ? SC : a.S, L = LC ? LC : a.L, B = BC ? BC : a.B;
  const int sig = blockIdx.y + a.sig0, tile = blockIdx.x >> 3;
  const GenLds lp = gen_lds(S, L, a.hyperbolic, 2);
  const int ldS = lp.ldS;
  const GenWs gw = gen_ws(B, S, L);
  float* ws = a.ws + sig * a.ws_sig_stride;
  const float* pk = ws + a.pk_off;
  const GenPack gp = gen_pack(S, L, a.hyperbolic);
  float* xs = smem + lp.xs; float* zs = smem + lp.zs; float* bufA = smem + lp.bufA; float* bufB = smem + lp.bufB;
  float* dzc = smem + lp.small;             // [16][LP] gradient of -mean(critic_z) w.r.t. the encoder output
  float* cw = smem + lp.cw; float* ct = smem + lp.ct;
  const uint32_t tick = (uint32_t)a.counters[3] + (uint32_t)(a.step_add > 0 ? a.step_add : 0);
  const int g0 = tile * 16;
  const float* mbase = a.masks ? a.masks + sig * a.mask_sig_stride : nullptr;
  const CriticLayout clz = cz_layout(L);
  const CriticPad cpz = critic_pad(L, L, 2);
  // (the gather first: loads return in order, and the weight prefetch -- cold lines, rewritten by the previous launch -- would
  // hold its two dependent round trips back)
  tile_load_rows(xs, ldS, a.x + sig * a.x_sig_stride, a.x_ld, a.row_index ? a.row_index + (int64_t)sig * a.ri_sig_stride : nullptr, g0, 16, S, 16);
  const LstmPre pre_enc = lstm_layer_prefetch<WSC1>(pk + gp.enc_g[0], pk + gp.enc_g[1], ENC_H, S);
  stage_critic_padded(cw, a.P.cz + (int64_t)sig * a.pcz, clz, L, cpz);
  __syncthreads();
  tile_store(ws + gw.xg + (int64_t)(B + g0) * S, S, xs, ldS, 16, S, 16);
  float* zin = zs + 16 * LP;
  float* gates = ws + gw.enc_g2 + (int64_t)g0 * 8 * ENC_H;
  encoder_fwd_tile_packed<true, WSC1>(xs, ldS, S, L, pk, gp, bufA, ENC_LDG, bufB, ENC_LDH, zin, gates,
                                ws + gw.enc_h + (int64_t)(B + g0) * 2 * ENC_H, 16, pre_enc);
  const PackedPre pre_edt = gemm_nt_prefetch<WSC1>(pk + gp.enc_d_t, L, 2 * ENC_H);
  // critic_z(encoder(x)) and its input gradient (frozen critic; -mean(fake_z), train.py:215-217)
  const DropSrc dz = drop_src(a, sig, mbase, RS_DROP_CRITIC + 8 * 0, tick, clz.p_drop);
  const float sum_crit = critic_tile_fwd_bwd(zin, LP, cw, clz, L, cpz, ct, -1.f / B, [&](int li, int r, int c) { return dz.get4(li, g0 + r, c, L); },
                                             [&](int li, int r, int c) { return dz.get(li, g0 + r, c, L); }, dzc, LP);
  tile_store(ws + gw.dzenc + (int64_t)(B + g0) * L, L, dzc, LP, 16, L, 16);
  // encoder backward of that gradient
  float* dP = bufA;
  {
    LstmCellBwdEpi epi{gates, ENC_H, dP, ENC_LDG, 16, 16, nullptr, 0, ws + gw.dgenc + (int64_t)(B + g0) * 6 * ENC_H, {}, {}, {}, {}, {}};
    gemm_nt_packed_epi<1, true, decltype(epi), WSC1>(dzc, LP, L, 2 * ENC_H, pk + gp.enc_d_t, nullptr, 0, pre_edt, epi);      // dH, cell backward in the epilogue
  }
  float* part_out = ws + gw.partial + tile * 4;
  if (threadIdx.x == 0) part_out[2] = sum_crit;
  if (tile == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    // optimizer step number and its bias corrections (double-precision powers): once per launch, for the dW + Adam launch --
    // here, on the chain with slack; they go to the workspace of the launch's first model (IterArgs.sig0)
    const int step = a.counters[a.opt] + 1 + (a.step_add > 0 ? a.step_add : 0);
    if (a.step_add < 0) a.counters[a.opt] = step;
    const AdamCoef c0 = adam_coef(a.lr, a.b1, a.b2, a.eps, a.wd, a.riemannian, a.stabilize, step);
    float* ac = a.ws + (int64_t)a.sig0 * a.ws_sig_stride + gw.adamc;
    ac[0] = c0.bc1; ac[1] = c0.bc2; ac[2] = c0.sqrt_bc2;
  }
}

// SC / LC / BC: window length, latent width, batch as compile-time constants (0 = from the arguments); see
// critic_fused.hip: every layer of the chain runs once per launch, so index arithmetic is never amortised.
static_assert(TB == 512, "gen_body deals rows over 8 waves");
template <bool HYPER, int SC, int LC, int BC, bool WSC1 = false>
__device__ __forceinline__ void gen_body(const IterArgs& a, float* smem) {
  const int S = SC ? SC : a.S, L = LC ? LC : a.L, B = BC ? BC : a.B;
  const int sig = blockIdx.y + a.sig0, tile = blockIdx.x >> 3, role = blockIdx.z;
  __builtin_amdgcn_s_setprio(2);            // (tile_gemm.h mfma_prio_*: the MFMA loops run below everything else)
  if (role == 2) { gen_role_z<SC, LC, BC, WSC1>(a, smem); return; }
  const GenLds lp = gen_lds(S, L, HYPER ? 1 : 0, role);
  const int ldS = lp.ldS;
  const EncLayout el = enc_layout(S, L);
  const DecLayout dl = dec_layout(S, L, HYPER ? 1 : 0);
  const GenWs gw = gen_ws(B, S, L);
  const float* PE = a.P.enc + (int64_t)sig * a.pe;
  const float* PD = a.P.dec + (int64_t)sig * a.pd;
  float* ws = a.ws + sig * a.ws_sig_stride;
  const float* pk = ws + a.pk_off;          // MFMA-native copies of the generator weights (pack_generator_kernel / dW kernel)
  const GenPack gp = gen_pack(S, L, HYPER ? 1 : 0);
  float* xs = smem + lp.xs; float* zs = smem + lp.zs; float* bufA = smem + lp.bufA; float* bufB = smem + lp.bufB;
  float* small = smem + lp.small;
  float* red = small + 3 * 16 * LP;
  float* cw = smem + lp.cw; float* ct = smem + lp.ct;
  float* Ein = (HYPER && role == 1) ? smem + lp.hb : bufA;      // the Moebius head's input rows
  const uint32_t tick = (uint32_t)a.counters[3] + (uint32_t)(a.step_add > 0 ? a.step_add : 0);
  // (the optimizer step number and its bias corrections -- two double-precision powers on one lane, ~2 k cycles -- are taken by
  // chain Z's first workgroup, which ends at 40 k of the kernel's 88 k cycles: gen_role_z)
  const int g0 = tile * 16;                 // first batch row of this tile
  const int pass = role;                    // decoder pass carried by this workgroup
  const int64_t prow0 = (int64_t)pass * B + g0;          // its first operand row in the pass-major workspace arrays
  const float* mbase = a.masks ? a.masks + sig * a.mask_sig_stride : nullptr;
  const int64_t BL = (int64_t)B * L;
  const int lane = threadIdx.x & 63, wave = wave_id(), nw = blockDim.x >> 6;
  float sum_crit = 0.f, sum_aux = 0.f;
  constexpr int ldH = 2 * DEC_H + 4, ldG = 6 * DEC_H + 4, ldA0 = 52;
  GEN_STAMP(0);
  // (Rounds 1-4 started with an "L2 warm-up": the workgroups of chains G and R together touched every 128-byte line of the packed
  // weights once, so that the layers would find them in this XCD's L2.  Since the weights come through prefetched sc1 buffer loads a
  // stage ahead it only stood in front of the chains' first loads -- loads return in order: the window gather and the first layer's
  // weights waited behind ~0.4 MB of cold lines.  Without it: 2.749 against 2.766 ms per epoch, 36.0 against 36.15 us per launch.)
  float* zin;                               // decoder input rows [16][LP]
  PackedPre pre_d1;                         // first weights of the decoder's first layer, requested a stage ahead
  if (role == 0) {
    pre_d1 = gemm_nt_prefetch<WSC1>(pk + gp.d1, L, DEC_D1);
    const CriticLayout clx = cx_layout(S, L);
    stage_critic_padded(cw, a.P.cx + (int64_t)sig * a.pcx, clx, L, critic_pad(S, L, 4));
    load_z(a, sig, tile, tick, zs);
    zin = zs;
    __syncthreads();
  } else {
    // ---- encoder(x)  (critic_z(encoder(x)) and its way back through the encoder: chain Z)
    // the window gather is two dependent memory round trips (row index, then the row)
    GEN_STAMP(14);
    tile_load_rows(xs, ldS, a.x + sig * a.x_sig_stride, a.x_ld, a.row_index ? a.row_index + (int64_t)sig * a.ri_sig_stride : nullptr, g0, 16, S, 16);
    const LstmPre pre_enc = lstm_layer_prefetch<WSC1>(pk + gp.enc_g[0], pk + gp.enc_g[1], ENC_H, S);      // behind the gather (loads return in order)
    GEN_STAMP(15);
    GEN_STAMP(12);
    __syncthreads();
    GEN_STAMP(13);
    tile_store(ws + gw.xg + (int64_t)g0 * S, S, xs, ldS, 16, S, 16);
    if (HYPER) tile_store(ws + gw.ecat + (int64_t)(2 * B + g0) * S, S, xs, ldS, 16, S, 16);      // the head's second row block (pass 2)
    zin = zs + 16 * LP;
    encoder_fwd_tile_packed<true, WSC1>(xs, ldS, S, L, pk, gp, bufA, ENC_LDG, bufB, ENC_LDH, zin,
                                  ws + gw.enc_g + (int64_t)g0 * 8 * ENC_H, ws + gw.enc_h + (int64_t)g0 * 2 * ENC_H, 16, pre_enc);
    GEN_STAMP(1);
    pre_d1 = gemm_nt_prefetch<WSC1>(pk + gp.d1, L, DEC_D1);
  }
  GEN_STAMP(2);
  // ---- decoder trunk on this role's pass
  tile_store(ws + gw.zcat + prow0 * L, L, zin, LP, 16, L, 16);
  DecSave sv;
  sv.ps = 16;
  sv.a0 = ws + gw.a0 + prow0 * DEC_D1;
  sv.g0 = ws + gw.g0 + prow0 * 8 * DEC_H;
  sv.h0d = ws + gw.h0d + prow0 * 2 * DEC_H;
  sv.mask = ws + gw.mask + prow0 * 2 * DEC_H;
  sv.g1 = ws + gw.g1 + prow0 * 8 * DEC_H;
  sv.h1 = ws + gw.h1 + prow0 * 2 * DEC_H;
  sv.e = ws + gw.ecat + prow0 * S;
  sv.stamps = (a.stamps && blockIdx.x == 0 && blockIdx.y == 0) ? a.stamps + (int64_t)blockIdx.z * 48 * 8 : nullptr;
  // injected layout: critic_z 2x(B,L) | critic_x 4x(B,L) | decoder(z) (B,128) | decoder(enc(x)) (B,128): as a
  // (layer, batch, 128) array with "layer" = pass, the two decoder masks are rows [0,B) and [B,2B) of one block.
  const DropSrc dd = drop_src(a, sig, mbase ? mbase + 6 * BL : nullptr, RS_DROP_DEC0, tick, 0.2f);
  const int growp = pass * B + g0;
  const PackedPre pre_head = decoder_trunk_fwd_tile_packed<1, true, WSC1>(zin, L, S, pk, gp, bufA, bufB, ldS, dd, [growp](int r) { return growp + r; }, sv, 16,
                                                                    pre_d1, HYPER ? pk + gp.head : nullptr, S, S, Ein);
  GEN_STAMP(3);
  // E = tanh output in Ein[0..15]
  const int hrows = (HYPER && role == 1) ? 32 : 16;       // rows through the Moebius head: role R adds pass 2 = the real window
  float u_keep[16], hb_keep[16];            // this wave's head rows: pre-activations and bias (lane's elements), forward -> backward
  if (HYPER) {
    GEN_STAMP(20);
    if (role == 1) gemm_nt_packed<2, true, ActIdentity, WSC1>(Ein, ldS, S, S, pk + gp.head, nullptr, bufB, ldS, 0, 0, pre_head);
    else gemm_nt_packed<1, true, ActIdentity, WSC1>(Ein, ldS, S, S, pk + gp.head, nullptr, bufB, ldS, 0, 0, pre_head);
    __syncthreads();
    GEN_STAMP(21);
    GEN_STAMP(22);
    // the Moebius head, row-wise in place (head_rows_tile's row dealing: four rows per wave, one per 16-lane DPP row).  The wave
    // that carries a row forward carries it backward as well: u (the head's pre-activations) and the bias stay in its registers
    // until then -- the backward used to re-read u from the workspace, a memory round trip in the middle of the chain.
    epl16_dispatch(S, [&](auto tag) {
      constexpr int EPL = decltype(tag)::value;
      using R16 = RowT<16, EPL>;
      const R16 hb = row_load<R16>(PD + dl.head_b, S, lane);
      const int r = wave * 4 + (lane >> 4);
      if (wave * 4 < hrows) {
        const R16 u = row_load<R16>(bufB + r * ldS, S, lane);
#pragma unroll
        for (int e = 0; e < EPL; ++e) { u_keep[e] = u.v[e]; hb_keep[e] = hb.v[e]; }
        row_store(bufB + r * ldS, head_row(u, hb), S, lane);
      }
    });
    __syncthreads();
  }
  float* R = HYPER ? bufB : bufA;           // decoder outputs (rows 0-15: this pass [, rows 16-31: hyper_x])
  float* dR = HYPER ? bufA : bufB;          // their gradients
  GEN_STAMP(4);
  if (role == 0) {
    // ---- critic_x(x_gen) and its input gradient (loss term -mean(fake_x), train.py:205-207)
    const CriticLayout clx = cx_layout(S, L);
    const DropSrc dx = drop_src(a, sig, mbase ? mbase + 2 * BL : nullptr, RS_DROP_CRITIC + 8 * 1, tick, clx.p_drop);
    sum_crit = critic_tile_fwd_bwd(R, ldS, cw, clx, L, critic_pad(S, L, 4), ct, -1.f / B,
                                   [&](int li, int r, int c) { return dx.get4(li, g0 + r, c, L); },
                                   [&](int li, int r, int c) { return dx.get(li, g0 + r, c, L); }, dR, ldS);
  }
  GEN_STAMP(5);
  if (HYPER) {
    if (role == 1) {
      // ---- hyperbolic reconstruction loss 10 * sum(dist)/B (train.py:226-234) and its gradients
      float part = 0.f;
      if (wave < 4) {                                 // 16 row pairs: four per wave, one per 16-lane DPP row
        epl16_dispatch(S, [&](auto tag) {
          using R16 = RowT<16, decltype(tag)::value>;
          const int r = wave * 4 + (lane >> 4);
          R16 du, dv;
          const float d = rowdist_row_bwd(row_load<R16>(R + r * ldS, S, lane), row_load<R16>(R + (16 + r) * ldS, S, lane), 10.f / B, du, dv);
          row_store(dR + r * ldS, du, S, lane);
          row_store(dR + (16 + r) * ldS, dv, S, lane);
          const float d0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 0)), d1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 16));
          const float d2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 32)), d3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 48));
          part = (d0 + d1) + (d2 + d3);
        });
      }
      if (lane == 0) red[16 + wave] = part;
      __syncthreads();
      for (int w = 0; w < nw; ++w) sum_aux += red[16 + w];
    }
    GEN_STAMP(23);
    const PackedPre pre_ht = gemm_nt_prefetch<WSC1>(pk + gp.head_t, S, S);        // the backward products' weights, each a stage ahead
    // ---- Moebius head backward, row-wise: dR -> dU (in place); this wave's share of the bias gradient in registers
    // (four rows per wave, one per 16-lane DPP row; the row's bias gradient goes to its own row of R: the head outputs are dead)
    epl16_dispatch(S, [&](auto tag) {
      constexpr int EPL = decltype(tag)::value;
      using R16 = RowT<16, EPL>;
      const int r = wave * 4 + (lane >> 4);
      if (wave * 4 < hrows) {
        R16 du, db, u, hb;
#pragma unroll
        for (int e = 0; e < EPL; ++e) { u.v[e] = u_keep[e]; hb.v[e] = hb_keep[e]; }
        head_row_bwd(u, hb, row_load<R16>(dR + r * ldS, S, lane), du, db);
        row_store(dR + r * ldS, du, S, lane);
        row_store(ws + gw.du + (prow0 + prow(r, B)) * S, du, S, lane);       // the dW kernel's operand rows, straight from here
        // the wave's four bias-gradient rows are summed across its four 16-lane groups before they leave the registers: the
        // column sums below then add one row per wave instead of four
#pragma unroll
        for (int e = 0; e < R16::EPL; ++e) {
          float v = db.v[e];
          v += __shfl_xor(v, 16, 64);
          v += __shfl_xor(v, 32, 64);
          db.v[e] = v;
        }
        if (lane < 16) row_store(R + wave * ldS, db, S, lane);                // row `wave` of R: this wave's partial
      }
    });
    __syncthreads();
    GEN_STAMP(24);
    for (int c = threadIdx.x; c < S; c += blockDim.x) {
      float s = 0.f;
      for (int w = 0; w < hrows / 4; ++w) s += R[w * ldS + c];
      ws[gw.ballpart + ((int64_t)role * (B / 16) + tile) * S + c] = s;
    }
    __syncthreads();
    GEN_STAMP(25);
    // dE = dU W_h for the decoder pass, and d(pre-tanh) = dE * (1 - E^2) in its epilogue (E re-read from the workspace,
    // requested before the reduction)
    {
      struct TanhBwdEpi {
        float* Ys; int ldy; const float* E; int ldE; float* gout; float e[4]; int vo;
        __device__ __forceinline__ void prefetch(int n, int q, bool ok) {
          vo = (4 * q * ldE + (ok ? n : 0)) * 4;                          // (buffer addressing: tile_gemm.h GBuf)
          const GBuf eb(E);
#pragma unroll
          for (int r = 0; r < 4; ++r) e[r] = ok ? eb.ld(vo, r * ldE * 4) : 0.f;
        }
        __device__ __forceinline__ void emit(int, int r, int row, int n, float v) {
          const float o = v * (1.f - e[r] * e[r]);
          Ys[row * ldy + n] = o; GBuf(gout).st(o, vo, r * ldE * 4);      // LDS tile + the dW kernel's operand rows
        }
      } epi{R, ldS, ws + gw.ecat + prow0 * S, S, ws + gw.dpre2 + prow0 * S, {}, 0};
      gemm_nt_packed_epi<1, true, decltype(epi), WSC1>(dR, ldS, S, S, pk + gp.head_t, nullptr, 0, pre_ht, epi);
    }
    __syncthreads();
    GEN_STAMP(26);
  } else {
    if (role == 1) {
      // ---- 10 * MSE(x, x_rec) (train.py:241-242): E in bufA (= R), gradients into bufB (= dR)
      float part = 0.f;
      tile_for(16, S, [&](int r, int c) {
        const float diff = R[r * ldS + c] - xs[r * ldS + c];
        part += diff * diff;
        dR[r * ldS + c] = 20.f * diff / ((float)B * (float)S);
      });
      sum_aux = block_sum(part, red);
      __syncthreads();
    }
    tile_for(16, S, [&](int r, int c) {
      const float e = R[r * ldS + c];
      dR[r * ldS + c] *= 1.f - e * e;
    });
    __syncthreads();
  }
  // The backward half ping-pongs between the two big LDS tiles X (holds d(pre-tanh)) and Y; every LSTM cell backward runs in
  // the epilogue of the product that makes its dH (LstmCellBwdEpi), so a layer is one stage: product -> gate deltas.
  float* X = HYPER ? R : dR;                // d(pre-tanh) [16][ldS]
  float* Y = HYPER ? dR : R;
  GEN_STAMP(6);
  const PackedPre pre_d2t = gemm_nt_prefetch<WSC1>(pk + gp.d2_t, S, 2 * DEC_H);
  if (!HYPER) tile_store(ws + gw.dpre2 + prow0 * S, S, X, ldS, 16, S, 16);        // (hyperbolic: written by the epilogue above)
  const PackedPre pre_l1t = gemm_nt_prefetch<WSC1>(pk + gp.l_t[1], 6 * DEC_H, 2 * DEC_H);
  // dH1 = dpre W2, layer 1 cell backward -> dG1 in Y
  {
    LstmCellBwdEpi epi{ws + gw.g1 + prow0 * 8 * DEC_H, DEC_H, Y, ldG, 16, 16, nullptr, 0, ws + gw.dg1 + prow0 * 6 * DEC_H, {}, {}, {}, {}, {}};
    gemm_nt_packed_epi<1, true, decltype(epi), WSC1>(X, ldS, S, 2 * DEC_H, pk + gp.d2_t, nullptr, 0, pre_d2t, epi);
  }
  GEN_STAMP(32);
  __syncthreads();
  GEN_STAMP(7);
  GEN_STAMP(33);
  const PackedPre pre_l0t = gemm_nt_prefetch<WSC1>(pk + gp.l_t[0], 6 * DEC_H, DEC_D1);
  GEN_STAMP(34);
  // dH0d = dG1 W_ih(l1) (both directions: one stacked reduction), x the inter-layer dropout mask, layer 0 cell backward -> dG0 in X
  {
    LstmCellBwdEpi epi{ws + gw.g0 + prow0 * 8 * DEC_H, DEC_H, X, ldG, 16, 16,
                       a.drop_mode != 0 ? ws + gw.mask + prow0 * 2 * DEC_H : nullptr, 2 * DEC_H, ws + gw.dg0 + prow0 * 6 * DEC_H, {}, {}, {}, {}, {}};
    gemm_nt_packed_epi<1, true, decltype(epi), WSC1>(Y, ldG, 6 * DEC_H, 2 * DEC_H, pk + gp.l_t[1], nullptr, 0, pre_l1t, epi);
  }
  GEN_STAMP(35);
  __syncthreads();
  GEN_STAMP(36);
  GEN_STAMP(8);
  GEN_STAMP(37);
  PackedPre pre_d1t{};
  if (role == 1) pre_d1t = gemm_nt_prefetch<WSC1>(pk + gp.d1_t, DEC_D1, L);
  GEN_STAMP(38);
  gemm_nt_packed<1, true, ActIdentity, WSC1>(X, ldG, 6 * DEC_H, DEC_D1, pk + gp.l_t[0], nullptr, Y, ldA0, 0, 0, pre_l0t, ActIdentity{}, nullptr, 0,
                          ws + gw.da0 + prow0 * DEC_D1, DEC_D1);                  // (+ the dW kernel's operand rows)
  GEN_STAMP(39);
  __syncthreads();
  GEN_STAMP(9);
  float* part_out = ws + gw.partial + tile * 4;
  if (role == 0) {
    if (threadIdx.x == 0) part_out[1] = sum_crit;
    GEN_STAMP(11);
    return;
  }
  // dZ = dA0 W1: the gradient reaching the encoder's output
  const PackedPre pre_edt = gemm_nt_prefetch<WSC1>(pk + gp.enc_d_t, L, 2 * ENC_H);
  gemm_nt_packed<1, true, ActIdentity, WSC1>(Y, ldA0, DEC_D1, L, pk + gp.d1_t, nullptr, X, LP, 0, 0, pre_d1t, ActIdentity{}, nullptr, 0,
                          ws + gw.dzenc + (int64_t)g0 * L, L);                     // (the critic_z part of dZ: chain Z)
  __syncthreads();
  GEN_STAMP(10);
  // ---- encoder backward: dH = dZ W_dense, cell backward -> dG in Y
  {
    LstmCellBwdEpi epi{ws + gw.enc_g + (int64_t)g0 * 8 * ENC_H, ENC_H, Y, ENC_LDG, 16, 16, nullptr, 0,
                       ws + gw.dgenc + (int64_t)g0 * 6 * ENC_H, {}, {}, {}, {}, {}};
    gemm_nt_packed_epi<1, true, decltype(epi), WSC1>(X, LP, L, 2 * ENC_H, pk + gp.enc_d_t, nullptr, 0, pre_edt, epi);
  }
  if (threadIdx.x == 0) part_out[0] = sum_aux;
  GEN_STAMP(11);
}

// ---- kernels: single iterations, and the critic_x || critic_z pair (blockIdx.z picks the critic)
__global__ __launch_bounds__(TB) void cx_pass_kernel(IterArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cx_pass_body(a, smem);
}
__global__ __launch_bounds__(TB) void cz_pass_kernel(IterArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  cz_pass_body(a, smem);
}
__global__ __launch_bounds__(TB) void critic_pass_pair_kernel(IterArgs ax, IterArgs az) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (blockIdx.z == 0) cx_pass_body(ax, smem); else cz_pass_body(az, smem);
}
template <bool IS_X>
__global__ __launch_bounds__(TB) void critic_gp_kernel(IterArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  gp_body<IS_X>(a, smem);
}
__global__ __launch_bounds__(TB) void critic_gp_pair_kernel(IterArgs ax, IterArgs az) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (blockIdx.z == 0) gp_body<true>(ax, smem); else gp_body<false>(az, smem);
}
// Workgroups are dealt round-robin over the 8 XCDs (MI355X_MICROARCH.md, dispatch): blockIdx.x is stretched by 8 and
// only the blocks that land on XCD (signal mod 8) work, so the 2 * B/16 workgroups of one model share an L2 -- each
// generator weight is fetched from HBM once per launch instead of once per workgroup.  Placement is a speed matter
// only: results do not depend on it.
// (Measured and dropped in round 3: four extra workgroups per XCD that read the packed weights once, in the chains' order, to leave
// them in that XCD's L2 ahead of the chains' sc1 loads -- the weights were rewritten a launch ago on other XCDs.  No change:
// 40.14 vs 40.17 us per launch.  The chains' weight fetches are already hidden behind the previous stage; what a chain's 88 k
// cycles consist of is MFMA issue plus the epilogues' vector instructions, which do not overlap on one SIMD: DESIGN.md §4.)
template <bool HYPER, int SC, int LC, int BC>
__global__ __launch_bounds__(TB) void gen_kernel(IterArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (a.guard && a.counters[4] != 0) return;         // fail-stop behind a resident critic launch that gave up (hypad_epoch_status)
  // chain Z (blockIdx.z == 2) goes to the neighbouring XCD: it reads only the encoder's weights and must not queue behind
  // chains G and R for the 32 CUs of theirs (batch 256: 16 tiles x 2 chains fill an XCD)
  if ((blockIdx.x & 7) != ((blockIdx.y + a.sig0 + (blockIdx.z == 2 ? 1 : 0)) & 7)) return;
  gen_body<HYPER, SC, LC, BC, true>(a, smem);        // (weights through sc1 buffer loads: tile_gemm.h WeightBlocks)
}

// ------------------------------------------------------------------------------------------------ host: launches
// LDS of the stand-alone critic launches (cx_pass / cz_pass and their pair form, critic_gp), which every training path falls back
// on: the window tile, the critic's weights and the 48-row activation tiles.  Latent 29..32 with windows above 240 need more than
// the 160 KiB of a CU (256 x 32: 164 544 bytes): refused by check_dims, before any launch, instead of by a failed hipFuncSetAttribute.
bool critic_launches_fit(int S, int L) {
  const int cxf = cx_layout(S, L).total, czf = cz_layout(L).total, scratch = critic_batch_lds_floats(48, L);
  const int f[4] = {lds_plan(S, 16, 16, cxf, scratch).total, lds_plan(S, 16, 16, czf, scratch).total, gp_lds_floats(S, cxf),
                    gp_lds_floats(L, czf)};
  for (int v : f)
    if ((size_t)v * sizeof(float) > 160 * 1024) return false;
  return true;
}

int check_dims(const hypad_dims* d) {
  if (!d || d->signal_shape <= 0 || d->latent_dim <= 0 || d->batch <= 0 || d->n_signals <= 0 || d->first_signal < 0) return HYPAD_EINVAL;
  if (d->batch % 16 != 0) return HYPAD_EINVAL;
  if (d->signal_shape > MAX_S || d->latent_dim > MAX_L) return HYPAD_EUNSUPPORTED;
  if (!critic_launches_fit(d->signal_shape, d->latent_dim)) return HYPAD_EUNSUPPORTED;
  if (!dw_tables_fit(*d)) return HYPAD_EUNSUPPORTED;       // cannot happen within MAX_S / MAX_L
  // the closed forms device code uses for a critic's tensor offsets (layout.h CriticLayout::wof / bof) ARE the layout's table
  const CriticLayout cls[2] = {cx_layout(d->signal_shape, d->latent_dim), cz_layout(d->latent_dim)};
  for (const CriticLayout& cl : cls)
    for (int li = 0; li <= cl.nh; ++li)
      if (cl.wof(li) != cl.w[li] || cl.bof(li) != cl.b[li]) return HYPAD_EUNSUPPORTED;
  return HYPAD_OK;
}

// ------------------------------------------------------------------------------------------------ packed generator weights
// Builds the MFMA-native copies (layout.h GenPack) from the parameter arenas: one thread per float4 of a packed block.
struct PackDesc {
  int kind;            // 0 W, 1 W with LSTM gate rows compacted, 2 W^T, 3 [W_fwd; W_rev]^T with compacted gate rows, 4 summed biases, 5 critic_x padded image,
                       // 6 snapshot of the critics' parameters, moments and the counters (hypad_epoch_restore)
  int net;             // HYPAD_NET_ENCODER / HYPAD_NET_DECODER
  int dst, nout, kred; // packed matrix: nout output rows, kred reduction columns
  int src0, src1, ld, H;
};
struct PackTable { int n; int max_units; PackDesc d[32]; };
// Layout of the epoch snapshot (hypad_epoch_restore): per signal [P.cx | M.cx | V.cx | P.cz | M.cz | V.cz], then counters[0..3]
HD int64_t snapshot_floats(int pcx, int pcz, int n_signals) { return (int64_t)n_signals * 3 * (pcx + pcz) + 4; }
// one float4 of one signal's snapshot: to the snapshot (restore = false) or back to the arenas
__device__ __forceinline__ void snapshot_move(const IterArgs& a, float* snap, int sig, int u, bool restore) {
  const int qx = a.pcx / 4, qz = a.pcz / 4;
  if (u >= 3 * (qx + qz)) return;
  float4* sn = reinterpret_cast<float4*>(snap + (int64_t)sig * 3 * (a.pcx + a.pcz)) + u;
  const bool is_x = u < 3 * qx;
  const int v = is_x ? u : u - 3 * qx, q = is_x ? qx : qz;
  const int which = v / q, e = v - which * q;
  const hypad_nets& N = which == 0 ? a.P : (which == 1 ? a.M : a.V);
  float4* ar = reinterpret_cast<float4*>(is_x ? N.cx + (int64_t)sig * a.pcx : N.cz + (int64_t)sig * a.pcz) + e;
  if (restore) *ar = *sn; else *sn = *ar;
}
__global__ __launch_bounds__(256) void epoch_restore_kernel(IterArgs a, float* snap, int n_signals) {
  snapshot_move(a, snap, blockIdx.y, blockIdx.x * 256 + threadIdx.x, true);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 8) {
    const int32_t* saved = reinterpret_cast<const int32_t*>(snap + (int64_t)n_signals * 3 * (a.pcx + a.pcz));
    a.counters[threadIdx.x] = threadIdx.x < 4 ? saved[threadIdx.x] : 0;
  }
}
__global__ __launch_bounds__(256) void pack_generator_kernel(IterArgs a, PackTable tab, unsigned* zero_ptr, int zero_words, float* snap) {
  if (a.guard && a.counters[4] != 0) return;   // fail-stop: in particular the snapshot of the state the failed epoch began from stays
  if (a.guard && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) a.counters[5] = 0;      // (placement census of the resident launch)
  if (zero_words) {                            // (launch_pack: one word per thread of the grid)
    const int64_t flat = (((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    if (flat < zero_words) zero_ptr[flat] = 0u;
  }
  const PackDesc d = tab.d[blockIdx.y];
  const int sig = blockIdx.z;
  float* pk = a.ws + sig * a.ws_sig_stride + a.pk_off + d.dst;
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (d.kind == 6) {
    snapshot_move(a, snap, sig, u, false);
    if (u < 4 && sig == 0) reinterpret_cast<int32_t*>(snap + (int64_t)gridDim.z * 3 * (a.pcx + a.pcz))[u] = a.counters[u];
    return;
  }
  if (d.kind == 5) {                           // critic_x as the padded image of critic_mfma.h (stage_critic_padded's arithmetic, once)
    const CriticLayout cl = cx_layout(a.S, a.L);
    const CriticPad cp = critic_pad(a.S, a.L, 4);
    if (u < cp.total) {
      const float* C = a.P.cx + (int64_t)sig * a.pcx;
      const int L = a.L, in_dim = cl.in_dim;
      float v;
      if (u < cp.wh) { const int n = u / cp.ldin, k = u - n * cp.ldin; v = k < in_dim ? C[cl.wof(0) + n * in_dim + k] : (k == in_dim ? C[cl.bof(0) + n] : 0.f); }
      else if (u < cp.wl) {
        const int i = u - cp.wh, li = 1 + i / (L * cp.LQ), rem = i - (li - 1) * L * cp.LQ, n = rem / cp.LQ, k = rem - n * cp.LQ;
        v = k < L ? C[cl.wof(li) + n * L + k] : (k == L ? C[cl.bof(li) + n] : 0.f);
      } else { const int k = u - cp.wl; v = k < L ? C[cl.wof(cl.nh) + k] : (k == L ? C[cl.bof(cl.nh)] : 0.f); }
      pk[u] = v;
    }
    return;
  }
  const float* P = d.net == HYPAD_NET_ENCODER ? a.P.enc + (int64_t)sig * a.pe : a.P.dec + (int64_t)sig * a.pd;
  auto gate_row = [&](int n) { return n < d.H ? n : n + d.H; };           // compact [i|g|o] -> PyTorch [i,f,g,o] row
  const int Hp = (d.H + 15) & ~15;
  // forward gate matrices: packed row x * Hp + u (gate x of unit u; layout.h gate_rows) -> PyTorch row, or -1 for padding
  auto padded_gate_row = [&](int n) { const int x = n / Hp, u = n - x * Hp; return u < d.H ? (x == 0 ? 0 : x == 1 ? 2 * d.H : 3 * d.H) + u : -1; };
  if (d.kind == 4) {
    if (u < ((d.nout + 15) & ~15)) {
      float v = 0.f;
      if (u < d.nout) {
        const int r = d.H > 0 ? padded_gate_row(u) : u;
        if (r >= 0) v = P[d.src0 + r] + (d.src1 >= 0 ? P[d.src1 + r] : 0.f);
      }
      pk[u] = v;
    }
    return;
  }
  const int kg = (d.kred + 15) >> 4, units = ((d.nout + 15) >> 4) * kg * 64;
  if (u >= units) return;
  const int blk = u >> 6, lane = u & 63, tn = blk / kg, g = blk - tn * kg;
  const int n = 16 * tn + (lane & 15), k0 = 16 * g + 4 * (lane >> 4);
  float v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = k0 + c;
    float x = 0.f;
    if (n < d.nout && k < d.kred) {
      if (d.kind == 0) x = P[d.src0 + n * d.ld + k];
      else if (d.kind == 1) { const int r = padded_gate_row(n); x = r >= 0 ? P[d.src0 + r * d.ld + k] : 0.f; }
      else if (d.kind == 2) x = P[d.src0 + k * d.ld + n];
      else { const int dir = k >= 3 * d.H ? 1 : 0, kc = k - dir * 3 * d.H; x = P[(dir ? d.src1 : d.src0) + gate_row(kc) * d.ld + n]; }
    }
    v[c] = x;
  }
  reinterpret_cast<float4*>(pk)[u] = make_float4(v[0], v[1], v[2], v[3]);
}
// nets: bit 0 the encoder's copies, bit 1 the decoder's; forward_only: without the transposed copies of the backward products
PackTable pack_table(const hypad_dims& dm, bool with_critic = false, bool with_snapshot = false, int nets = 3, bool forward_only = false) {
  const int S = dm.signal_shape, L = dm.latent_dim;
  const EncLayout el = enc_layout(S, L);
  const DecLayout dl = dec_layout(S, L, dm.hyperbolic);
  const GenPack gp = gen_pack(S, L, dm.hyperbolic);
  PackTable t; t.n = 0; t.max_units = 0;
  auto push = [&](int kind, int net, int dst, int nout, int kred, int src0, int src1, int ld, int H) {
    if (!(nets & (net == HYPAD_NET_ENCODER ? 1 : 2)) || (forward_only && (kind == 2 || kind == 3))) return;
    PackDesc d{kind, net, dst, nout, kred, src0, src1, ld, H};
    t.d[t.n++] = d;
    const int units = kind == 4 ? ((nout + 15) & ~15) : ((nout + 15) >> 4) * ((kred + 15) >> 4) * 64;
    if (units > t.max_units) t.max_units = units;
  };
  const int E = HYPAD_NET_ENCODER, D = HYPAD_NET_DECODER;
  for (int d = 0; d < 2; ++d) {
    push(1, E, gp.enc_g[d], gate_rows(ENC_H), S, el.dir[d].w_ih, -1, S, ENC_H);
    push(4, E, gp.enc_gb[d], gate_rows(ENC_H), 0, el.dir[d].b_ih, el.dir[d].b_hh, 0, ENC_H);
  }
  push(0, E, gp.enc_d, L, 2 * ENC_H, el.dense_w, -1, 2 * ENC_H, 0);
  push(4, E, gp.enc_db, L, 0, el.dense_b, -1, 0, 0);
  push(0, D, gp.d1, DEC_D1, L, dl.d1_w, -1, L, 0);
  push(4, D, gp.d1b, DEC_D1, 0, dl.d1_b, -1, 0, 0);
  for (int l = 0; l < 2; ++l) {
    const int in = l == 0 ? DEC_D1 : 2 * DEC_H;
    for (int d = 0; d < 2; ++d) {
      push(1, D, gp.l_g[l][d], gate_rows(DEC_H), in, dl.l[l][d].w_ih, -1, in, DEC_H);
      push(4, D, gp.l_gb[l][d], gate_rows(DEC_H), 0, dl.l[l][d].b_ih, dl.l[l][d].b_hh, 0, DEC_H);
    }
    push(3, D, gp.l_t[l], in, 6 * DEC_H, dl.l[l][0].w_ih, dl.l[l][1].w_ih, in, DEC_H);
  }
  push(0, D, gp.d2, S, 2 * DEC_H, dl.d2_w, -1, 2 * DEC_H, 0);
  push(4, D, gp.d2b, S, 0, dl.d2_b, -1, 0, 0);
  if (dm.hyperbolic) {
    push(0, D, gp.head, S, S, dl.head_w, -1, S, 0);
    push(2, D, gp.head_t, S, S, dl.head_w, -1, S, 0);
  }
  push(2, E, gp.enc_d_t, 2 * ENC_H, L, el.dense_w, -1, 2 * ENC_H, 0);
  push(2, D, gp.d2_t, 2 * DEC_H, S, dl.d2_w, -1, 2 * DEC_H, 0);
  push(2, D, gp.d1_t, L, DEC_D1, dl.d1_w, -1, L, 0);
  if (with_critic) {                           // behind the generator's copies (the scoring workspace reserves it: score_forward.hip)
    const int units = critic_pad(S, L, 4).total;
    PackDesc d{5, HYPAD_NET_CRITIC_X, score_critic_offset(S, L, dm.hyperbolic), units, 0, 0, -1, 0, 0};
    t.d[t.n++] = d;
    if (units > t.max_units) t.max_units = units;
  }
  if (with_snapshot) {
    const int units = 3 * (cx_layout(S, L).total + cz_layout(L).total) / 4;
    PackDesc d{6, HYPAD_NET_CRITIC_X, 0, units, 0, 0, -1, 0, 0};
    t.d[t.n++] = d;
    if (units > t.max_units) t.max_units = units;
  }
  return t;
}
// zero_ptr / zero_words: a block the next launches need zeroed (the critic phase's epoch words and flags), one word per thread
// snap: where to snapshot the critics' state for hypad_epoch_restore, or null
int launch_pack(const IterArgs& a, const hypad_dims& dm, hipStream_t s, unsigned* zero_ptr = nullptr, int zero_words = 0, bool* zeroed = nullptr,
                bool with_critic = false, float* snap = nullptr, int nets = 3, bool forward_only = false) {
  const PackTable t = pack_table(dm, with_critic, snap != nullptr, nets, forward_only);
  const dim3 grid((t.max_units + 255) / 256, t.n, dm.n_signals);
  const bool z = zero_ptr && zero_words > 0 && (int64_t)zero_words <= (int64_t)grid.x * grid.y * grid.z * 256;
  if (zeroed) *zeroed = z;
  hipLaunchKernelGGL(pack_generator_kernel, grid, dim3(256), 0, s, a, t, z ? zero_ptr : nullptr, z ? zero_words : 0, snap);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

#if HYPAD_DIAG
long long* g_gen_stamps = nullptr;     // development builds only (libhypad_hip_dev.so)
#endif

struct IterCall {
  const float* x; int64_t x_sig_stride; int64_t x_row_stride; const int32_t* row_index; int64_t ri_sig_stride = 0;
  const float* z; const float* alpha;
  int train_mode; const float* masks; uint64_t seed;
  float* losses; int64_t loss_sig_stride;
  void* workspace; size_t workspace_bytes;
  int guard = 0;
  int flags = 0;                         // hypad_epoch_io.flags (HYPAD_EPOCH_DW_* select the dW + Adam launch's placement)
};

// opt: 0 critic_x, 1 critic_z, 2 generator
int fill_args(IterArgs& a, const hypad_dims* d, const hypad_train_state* st, const IterCall& io, int opt) {
  int rc = check_dims(d);
  if (rc) return rc;
  if (!st || !st->params.enc || !st->params.dec || !st->params.cx || !st->params.cz || !st->counters) return HYPAD_EINVAL;
  if (!io.x || !io.losses) return HYPAD_EINVAL;
  const int64_t per = ws_floats_per_signal(*d);
  if (!io.workspace || io.workspace_bytes < (size_t)per * d->n_signals * sizeof(float)) return HYPAD_EWORKSPACE;
  a.S = d->signal_shape; a.L = d->latent_dim; a.B = d->batch; a.hyperbolic = d->hyperbolic;
  a.P = st->params; a.M = st->exp_avg; a.V = st->exp_avg_sq;
  a.pe = enc_layout(a.S, a.L).total; a.pd = dec_layout(a.S, a.L, a.hyperbolic).total;
  a.pcx = cx_layout(a.S, a.L).total; a.pcz = cz_layout(a.L).total;
  a.counters = st->counters;
  a.x = io.x; a.x_sig_stride = io.x_sig_stride; a.x_ld = io.x_row_stride > 0 ? io.x_row_stride : d->signal_shape; a.row_index = io.row_index;
  a.z = io.z; a.alpha = io.alpha;
  a.drop_mode = io.train_mode ? (io.masks ? 1 : 2) : 0;
  a.masks = io.masks; a.seed = io.seed;
  a.losses = io.losses; a.loss_sig_stride = io.loss_sig_stride;
  a.ws = (float*)io.workspace + (opt == 1 ? ws_cz_offset(*d) : 0);
  a.ws_sig_stride = per;
  a.pk_off = ws_pack_offset(*d) - (opt == 1 ? ws_cz_offset(*d) : 0);       // a.ws is shifted for critic_z
  a.lr = st->lr; a.b1 = st->beta1; a.b2 = st->beta2; a.eps = st->eps; a.wd = 0.f; a.stabilize = 0; a.riemannian = 0;
  a.opt = opt; a.tick_owner = 1; a.stamps = nullptr; a.guard = io.guard; a.sig0 = 0; a.step_add = -1;
  a.rng_sig0 = d->first_signal; a.ri_sig_stride = io.ri_sig_stride;
#if HYPAD_DIAG
  a.stamps = g_gen_stamps;
#endif
  if (opt == 0) {
    if (!st->exp_avg.cx || !st->exp_avg_sq.cx) return HYPAD_EINVAL;
    a.mask_sig_stride = (int64_t)12 * a.B * a.L + (int64_t)a.B * 2 * DEC_H;
  } else if (opt == 1) {
    if (!st->exp_avg.cz || !st->exp_avg_sq.cz) return HYPAD_EINVAL;
    a.mask_sig_stride = (int64_t)6 * a.B * a.L;
  } else {
    if (!st->exp_avg.enc || !st->exp_avg_sq.enc || !st->exp_avg.dec || !st->exp_avg_sq.dec) return HYPAD_EINVAL;
    a.mask_sig_stride = (int64_t)6 * a.B * a.L + (int64_t)2 * a.B * 2 * DEC_H;
    if (a.hyperbolic) { a.riemannian = 1; a.wd = st->gen_weight_decay; a.stabilize = st->gen_stabilize; }
  }
  return HYPAD_OK;
}

// Optional profiling marks: ev[k] is recorded on the stream after the k-th kernel of an iteration (ev[0] before the first).
#define HYPAD_MARK(ev, k, s) do { if (ev) (void)hipEventRecord((ev)[k], s); } while (0)

inline size_t cx_pass_lds(const IterArgs& a) {
  return (size_t)lds_plan(a.S, 16, 16, cx_layout(a.S, a.L).total, critic_batch_lds_floats(48, a.L)).total * sizeof(float);
}
inline size_t cz_pass_lds(const IterArgs& a) {
  return (size_t)lds_plan(a.S, 16, 16, cz_layout(a.L).total, critic_batch_lds_floats(48, a.L)).total * sizeof(float);
}
inline size_t gp_x_lds(const IterArgs& a) { return (size_t)gp_lds_floats(a.S, cx_layout(a.S, a.L).total) * sizeof(float); }
inline size_t gp_z_lds(const IterArgs& a) { return (size_t)gp_lds_floats(a.L, cz_layout(a.L).total) * sizeof(float); }

int run_cx(const hypad_dims* d, const hypad_train_state* st, const IterCall& io, hipStream_t s, hipEvent_t* ev = nullptr) {
  IterArgs a;
  int rc = fill_args(a, d, st, io, 0);
  if (rc) return rc;
  const size_t lds = cx_pass_lds(a), lds2 = gp_x_lds(a);
  hipError_t e = allow_lds((const void*)cx_pass_kernel, lds);
  if (e == hipSuccess) e = allow_lds((const void*)critic_gp_kernel<true>, lds2);
  if (e != hipSuccess) return (int)e;
  dim3 grid(a.B / 16, d->n_signals);
  HYPAD_MARK(ev, 0, s);
  hipLaunchKernelGGL(cx_pass_kernel, grid, dim3(TB), lds, s, a);
  HYPAD_CHECK_LAUNCH();
  HYPAD_MARK(ev, 1, s);
  hipLaunchKernelGGL(critic_gp_kernel<true>, grid, dim3(TB), lds2, s, a);
  HYPAD_CHECK_LAUNCH();
  HYPAD_MARK(ev, 2, s);
  rc = launch_dw_critic(a, d->n_signals, s);
  if (rc) return rc;
  HYPAD_MARK(ev, 3, s);
  return HYPAD_OK;
}

int run_cz(const hypad_dims* d, const hypad_train_state* st, const IterCall& io, hipStream_t s, hipEvent_t* ev = nullptr) {
  IterArgs a;
  int rc = fill_args(a, d, st, io, 1);
  if (rc) return rc;
  const size_t lds = cz_pass_lds(a), lds2 = gp_z_lds(a);
  hipError_t e = allow_lds((const void*)cz_pass_kernel, lds);
  if (e == hipSuccess) e = allow_lds((const void*)critic_gp_kernel<false>, lds2);
  if (e != hipSuccess) return (int)e;
  dim3 grid(a.B / 16, d->n_signals);
  HYPAD_MARK(ev, 0, s);
  hipLaunchKernelGGL(cz_pass_kernel, grid, dim3(TB), lds, s, a);
  HYPAD_CHECK_LAUNCH();
  HYPAD_MARK(ev, 1, s);
  hipLaunchKernelGGL(critic_gp_kernel<false>, grid, dim3(TB), lds2, s, a);
  HYPAD_CHECK_LAUNCH();
  HYPAD_MARK(ev, 2, s);
  rc = launch_dw_critic(a, d->n_signals, s);
  if (rc) return rc;
  HYPAD_MARK(ev, 3, s);
  return HYPAD_OK;
}

// critic_x_iteration and critic_z_iteration of one minibatch side by side (train.py:320-327: disjoint weights, frozen
// generator): three launches with blockIdx.z selecting the critic.  losses_x / losses_z: where each writes its 4 floats.
// io_z: critic_z's own call description when the two iterations take different injected planes (null: io for both).
int run_critic_pair(const hypad_dims* d, const hypad_train_state* st, const IterCall& io, float* losses_x, float* losses_z,
                    hipStream_t s, hipEvent_t* ev = nullptr, const IterCall* io_z = nullptr) {
  IterArgs ax, az;
  IterCall cx = io, cz = io_z ? *io_z : io;
  cx.losses = losses_x; cz.losses = losses_z;
  int rc = fill_args(ax, d, st, cx, 0);
  if (rc) return rc;
  rc = fill_args(az, d, st, cz, 1);
  if (rc) return rc;
  az.tick_owner = 0;                       // one rng tick per launch group; the two critics use distinct Philox streams
  az.seed = ax.seed ^ CRITIC_Z_SEED_XOR;
  size_t lds = cx_pass_lds(ax), l2 = cz_pass_lds(az);
  if (l2 > lds) lds = l2;
  size_t ldsg = gp_x_lds(ax), g2 = gp_z_lds(az);
  if (g2 > ldsg) ldsg = g2;
  hipError_t e = allow_lds((const void*)critic_pass_pair_kernel, lds);
  if (e == hipSuccess) e = allow_lds((const void*)critic_gp_pair_kernel, ldsg);
  if (e != hipSuccess) return (int)e;
  dim3 grid(ax.B / 16, d->n_signals, 2);
  HYPAD_MARK(ev, 0, s);
  hipLaunchKernelGGL(critic_pass_pair_kernel, grid, dim3(TB), lds, s, ax, az);
  HYPAD_CHECK_LAUNCH();
  HYPAD_MARK(ev, 1, s);
  hipLaunchKernelGGL(critic_gp_pair_kernel, grid, dim3(TB), ldsg, s, ax, az);
  HYPAD_CHECK_LAUNCH();
  HYPAD_MARK(ev, 2, s);
  rc = launch_dw_critic_pair(ax, az, d->n_signals, s);
  if (rc) return rc;
  HYPAD_MARK(ev, 3, s);
  return HYPAD_OK;
}

// with_decay = false: the decay-only parameters are left alone (the caller advances them with run_decay_steps)
// sig0 / nsig / step_add: the models [sig0, sig0 + nsig) only, as generator iteration `step_add` of an epoch (IterArgs.step_add);
// defaults: all models, counters read and advanced by the launches themselves.
// reps > 1 (hypad_profile_iteration kind 5): each of the two kernels launched `reps` times back to back between its events -- an
// event pair around ONE short launch measures the event path too (10 - 20 % on a 9 us kernel)
int run_gen(const hypad_dims* d, const hypad_train_state* st, const IterCall& io, hipStream_t s, hipEvent_t* ev = nullptr, bool pack = true,
            bool with_decay = true, int sig0 = 0, int nsig = -1, int step_add = -1, int reps = 1) {
  IterArgs a;
  int rc = fill_args(a, d, st, io, 2);
  if (rc) return rc;
  if (nsig < 0) nsig = d->n_signals;
  a.sig0 = sig0; a.step_add = step_add;
  dim3 grid(8 * (a.B / 16), nsig, 3);                    // blockIdx.x >> 3: tile (see gen_kernel); blockIdx.z: role G / R / Z
  const int l0 = gen_lds(a.S, a.L, a.hyperbolic, 0).total, l1 = gen_lds(a.S, a.L, a.hyperbolic, 1).total;
  const size_t lds = (size_t)(l0 > l1 ? l0 : l1) * sizeof(float);
  if (lds > 160 * 1024) return HYPAD_EUNSUPPORTED;
  if (pack) {                             // the workspace is scratch between calls: rebuild the packed weights
    rc = launch_pack(a, *d, s);           // (inside an epoch the dW + Adam kernel keeps them current)
    if (!rc) rc = launch_dw_items(a, *d, with_decay, s);
    if (rc) return rc;
  }
  HYPAD_MARK(ev, 0, s);
  const bool ref_cfg = a.S == 100 && a.L == 20 && a.B == 64;          // BASELINE.json configs[0..2]
  const bool mv_cfg = a.S == 150 && a.L == 20 && a.B == 256;          // configs[3]: 5 channels x 30, batch 256
#define HYPAD_LAUNCH_GEN(...)                                                     \
  do {                                                                           \
    hipError_t e = allow_lds((const void*)gen_kernel<__VA_ARGS__>, lds);         \
    if (e != hipSuccess) return (int)e;                                          \
    for (int r = 0; r < reps; ++r) hipLaunchKernelGGL((gen_kernel<__VA_ARGS__>), grid, dim3(TB), lds, s, a);    \
  } while (0)
  const bool wadi_cfg = a.S == 123 && a.L == 20 && a.B == 64;         // the reference's configs/multivariate.yaml:5-7 as shipped (WADI)
  const bool swat_cfg = a.S == 51 && a.L == 20 && a.B == 64;          // ... and its SWAT alternative
  if (a.hyperbolic) {
    if (ref_cfg) HYPAD_LAUNCH_GEN(true, 100, 20, 64); else if (mv_cfg) HYPAD_LAUNCH_GEN(true, 150, 20, 256);
    else if (wadi_cfg) HYPAD_LAUNCH_GEN(true, 123, 20, 64); else if (swat_cfg) HYPAD_LAUNCH_GEN(true, 51, 20, 64); else HYPAD_LAUNCH_GEN(true, 0, 0, 0);
  }
  else { if (ref_cfg) HYPAD_LAUNCH_GEN(false, 100, 20, 64); else HYPAD_LAUNCH_GEN(false, 0, 0, 0); }
#undef HYPAD_LAUNCH_GEN
  HYPAD_CHECK_LAUNCH();
  HYPAD_MARK(ev, 1, s);
  rc = launch_dw_gen(a, *d, with_decay, nsig, io.flags, reps, s);      // (from the records written behind the pack launch)
  if (rc) return rc;
  HYPAD_MARK(ev, 2, s);
  return HYPAD_OK;
}

int run_decay_steps(const hypad_dims* d, const hypad_train_state* st, const IterCall& io, int nsteps, hipStream_t s) {
  if (!d->hyperbolic || nsteps <= 0) return HYPAD_OK;          // torch.optim.Adam (Euclidean generator) has no weight decay: nothing moves
  IterArgs a;
  int rc = fill_args(a, d, st, io, 2);
  if (rc) return rc;
  return launch_decay_steps(a, *d, nsteps, s);
}

IterCall from_io(const hypad_iter_io* io) {
  IterCall c;
  c.x = io->x; c.x_sig_stride = io->x_signal_stride; c.x_row_stride = io->x_row_stride; c.row_index = io->row_index; c.z = io->z; c.alpha = io->alpha;
  c.train_mode = io->drop.train_mode; c.masks = io->drop.masks; c.seed = io->drop.seed;
  c.losses = io->losses; c.loss_sig_stride = 4; c.workspace = io->workspace; c.workspace_bytes = io->workspace_bytes;
  return c;
}

}  // namespace

int hypad::train::launch_pack_generator(const IterArgs& a, const hypad_dims& d, hipStream_t s, bool with_critic) {
  return launch_pack(a, d, s, nullptr, 0, nullptr, with_critic);
}

// development aid (not declared in hypad.h): device buffer of 64 int64 stamped by the generator kernel, or null
#if HYPAD_DIAG
extern "C" __attribute__((visibility("default"))) void hypad_diag_set_gen_stamps(long long* p) { g_gen_stamps = p; }
#endif

extern "C" {

// Floats in front of the hoisted critic phase's area in an epoch workspace: the per-signal iteration workspaces, then the snapshot
// of the critics' state (hypad_epoch_restore), 64-byte aligned
static size_t epoch_base_floats(const hypad_dims& d) {
  const size_t snap = (size_t)snapshot_floats(cx_layout(d.signal_shape, d.latent_dim).total, cz_layout(d.latent_dim).total, d.n_signals);
  return (size_t)ws_floats_per_signal(d) * d.n_signals + ((snap + 15) & ~(size_t)15);
}
static float* epoch_snapshot_ptr(const hypad_dims& d, void* workspace) { return (float*)workspace + (size_t)ws_floats_per_signal(d) * d.n_signals; }

size_t hypad_train_workspace_bytes(const hypad_dims* d) {
  if (check_dims(d)) return 0;
  return (size_t)ws_floats_per_signal(*d) * d->n_signals * sizeof(float);
}

int hypad_pack_generator(const hypad_dims* d, const hypad_train_state* st, void* workspace, size_t workspace_bytes, hypad_stream_t s) {
  int rc = check_dims(d);
  if (rc) return rc;
  if (!st || !st->params.enc || !st->params.dec || !workspace) return HYPAD_EINVAL;
  const int64_t per = ws_floats_per_signal(*d);
  if (workspace_bytes < (size_t)per * d->n_signals * sizeof(float)) return HYPAD_EWORKSPACE;
  IterArgs a{};
  a.S = d->signal_shape; a.L = d->latent_dim; a.B = d->batch; a.hyperbolic = d->hyperbolic;
  a.P = st->params;
  a.pe = enc_layout(a.S, a.L).total; a.pd = dec_layout(a.S, a.L, a.hyperbolic).total;
  a.ws = (float*)workspace; a.ws_sig_stride = per; a.pk_off = ws_pack_offset(*d);
  return launch_pack(a, *d, (hipStream_t)s);
}
int hypad_packed_region(const hypad_dims* d, int64_t* offset_floats, int64_t* signal_stride_floats, int64_t* count_floats) {
  int rc = check_dims(d);
  if (rc) return rc;
  if (offset_floats) *offset_floats = ws_pack_offset(*d);
  if (signal_stride_floats) *signal_stride_floats = ws_floats_per_signal(*d);
  if (count_floats) *count_floats = gen_pack(d->signal_shape, d->latent_dim, d->hyperbolic).total;
  return HYPAD_OK;
}
// One critic's iteration as a ONE-ITERATION PHASE of the hoisted form (critic_fused.hip): pack the frozen generator half the critic
// looks at (forward copies only), record precompute (decoder(z) or encoder(x), noise / interpolation / dropout -> record), the
// iteration launch (register-resident MFMA chains -> gradient slabs) and its finalising launch (slab reduction, whole-batch norm,
// Adam, weights and moments back to the arenas, loss row) -- ~40 us of GPU time against 76 (critic_x) / 47 (critic_z) for the
// stand-alone pass / gradient-penalty / dW launches below, whose critic passes run on the vector ALU.  Taken when the caller's
// workspace has room for it (hypad_epoch_workspace_bytes(dims, 1, 1)) and the shape fits the iteration kernel; HYPAD_ITER_PHASE=0
// keeps the stand-alone launches.  Same arithmetic per row as the epoch's critic phase; against the stand-alone launches only the
// floating-point summation order (and the device dropout streams) differ.
static int run_critic_single(const hypad_dims* d, const hypad_train_state* st, const hypad_iter_io* io, int critic, hipStream_t s, bool* taken) {
  *taken = false;
  static const int enabled = HYPAD_TUNE_INT("HYPAD_ITER_PHASE", 1);
  if (!enabled || check_dims(d) || !critic_phase_supported(*d)) return HYPAD_OK;
  const size_t base = epoch_base_floats(*d);
  const size_t have = io->workspace_bytes / sizeof(float);
  if (!io->workspace || have < base + critic_phase_fixed_floats(*d) + critic_phase_floats_per_iter(*d)) return HYPAD_OK;
  IterCall c = from_io(io);
  IterArgs ax, az;
  int rc = fill_args(ax, d, st, c, 0);
  if (!rc) rc = fill_args(az, d, st, c, 1);
  if (rc) return rc;
  *taken = true;
  rc = launch_pack(critic == 0 ? ax : az, *d, s, nullptr, 0, nullptr, false, nullptr, critic == 0 ? 2 : 1, true);
  if (rc) return rc;
  hypad_epoch_noise nz{};
  const bool inj = io->drop.train_mode && io->drop.masks;
  if (critic == 0) { nz.z_cx = io->z; nz.alpha_cx = io->alpha; nz.masks_cx = inj ? io->drop.masks : nullptr; }
  else { nz.z_cz = io->z; nz.alpha_cz = io->alpha; nz.masks_cz = inj ? io->drop.masks : nullptr; }
  // (the phase files critic_x's loss row at row 0 and critic_z's at row 1 of an iteration: the caller's row is row `critic`)
  return run_critic_phase(ax, az, io->row_index, 1, io->losses - 4 * critic, (float*)io->workspace + base, have - base, d->n_signals, s, nullptr,
                          &nz, nullptr, nullptr, HYPAD_EPOCH_PER_ITERATION, critic);
}
int hypad_critic_x_iteration(const hypad_dims* d, const hypad_train_state* st, const hypad_iter_io* io, hypad_stream_t s) {
  if (!io) return HYPAD_EINVAL;
  bool taken = false;
  const int rc = run_critic_single(d, st, io, 0, (hipStream_t)s, &taken);
  if (taken || rc) return rc;
  return run_cx(d, st, from_io(io), (hipStream_t)s);
}
int hypad_critic_z_iteration(const hypad_dims* d, const hypad_train_state* st, const hypad_iter_io* io, hypad_stream_t s) {
  if (!io) return HYPAD_EINVAL;
  bool taken = false;
  const int rc = run_critic_single(d, st, io, 1, (hipStream_t)s, &taken);
  if (taken || rc) return rc;
  return run_cz(d, st, from_io(io), (hipStream_t)s);
}
int hypad_decoder_iteration(const hypad_dims* d, const hypad_train_state* st, const hypad_iter_io* io, hypad_stream_t s) {
  if (!io) return HYPAD_EINVAL;
  return run_gen(d, st, from_io(io), (hipStream_t)s);
}

// Profiling aid for bench.py: runs ONE iteration with HIP events between its kernels on `stream`, synchronises the
// stream and returns each kernel's duration in milliseconds (critic iterations: pass, gp, dw_adam; generator: gen,
// dw_adam).  Not capturable (creates events, synchronises).
int hypad_profile_iteration(int kind, const hypad_dims* d, const hypad_train_state* st, const hypad_iter_io* io, float* ms_out,
                            int n_out, hypad_stream_t s) {
  if (!io || !ms_out || kind < 0 || kind > 5) return HYPAD_EINVAL;
  const int nk = (kind == 2 || kind == 5) ? 2 : 3;
  constexpr int GEN_REPS = 64;
  if (n_out < nk) return HYPAD_EINVAL;
  if (kind >= 3 && !io->losses) return HYPAD_EINVAL;
  hipEvent_t ev[4];
  int kind4_div = 0;
  for (int i = 0; i <= nk; ++i) {
    hipError_t e = hipEventCreate(&ev[i]);
    if (e != hipSuccess) return (int)e;
  }
  int rc;
  if (kind == 0) rc = run_cx(d, st, from_io(io), (hipStream_t)s, ev);
  else if (kind == 1) rc = run_cz(d, st, from_io(io), (hipStream_t)s, ev);
  else if (kind == 2) rc = run_gen(d, st, from_io(io), (hipStream_t)s, ev);
  else if (kind == 5) rc = run_gen(d, st, from_io(io), (hipStream_t)s, ev, true, false, 0, -1, -1, GEN_REPS);      // (no decay-only tensors: the launch an epoch issues)
  else if (kind == 3) rc = run_critic_pair(d, st, from_io(io), io->losses, io->losses + 4 * (int64_t)d->n_signals, (hipStream_t)s, ev);
  else {
    IterArgs ax, az;
    IterCall c = from_io(io);
    constexpr int PROF_ITERS = 145;        // the critic phase of one configs[1] epoch (5 passes x 29 minibatches): ONE launch of 145
                                           // iterations in the persistent form -- the same launch hypad_train_epoch issues, so a
                                           // profiler's mean duration of that kernel is over like launches -- or one launch without
                                           // an Adam prologue + 144 steady-state launches
    c.loss_sig_stride = 2 * PROF_ITERS * 4;
    rc = fill_args(ax, d, st, c, 0);
    if (!rc) rc = fill_args(az, d, st, c, 1);
    const size_t base = epoch_base_floats(*d);
    if (!rc && !critic_phase_supported(*d)) rc = HYPAD_EUNSUPPORTED;
    if (!rc && io->workspace_bytes < (base + critic_phase_fixed_floats(*d) + PROF_ITERS * critic_phase_floats_per_iter(*d)) * sizeof(float)) rc = HYPAD_EWORKSPACE;
    if (!rc) rc = launch_pack(ax, *d, (hipStream_t)s);      // the precompute reads the packed generator weights
    int persistent = 0;
    if (!rc) rc = run_critic_phase(ax, az, nullptr, PROF_ITERS, io->losses, (float*)io->workspace + base,
                                   io->workspace_bytes / sizeof(float) - base, d->n_signals, (hipStream_t)s, ev, nullptr, &persistent);
    if (!rc) kind4_div = persistent ? PROF_ITERS : PROF_ITERS - 1;
  }
  if (rc == HYPAD_OK) {
    hipError_t e = hipStreamSynchronize((hipStream_t)s);
    if (e != hipSuccess) rc = (int)e;
  }
  for (int i = 0; i < nk && rc == HYPAD_OK; ++i) {
    hipError_t e = hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]);
    if (e != hipSuccess) rc = (int)e;
  }
  if (rc == HYPAD_OK && kind4_div > 0) ms_out[2] /= (float)kind4_div;      // mean of the steady-state launches
  if (rc == HYPAD_OK && kind == 5) { ms_out[0] /= (float)GEN_REPS; ms_out[1] /= (float)GEN_REPS; }
  for (int i = 0; i <= nk; ++i) (void)hipEventDestroy(ev[i]);
  return rc;
}

size_t hypad_epoch_workspace_bytes(const hypad_dims* d, int n_batches, int n_critics) {
  if (check_dims(d) || n_batches <= 0 || n_critics < 0) return 0;
  int64_t n = (int64_t)n_batches * n_critics;
  if (n > 512) n = 512;
  const size_t base = epoch_base_floats(*d);
  if (!critic_phase_supported(*d) || n == 0) return (size_t)ws_floats_per_signal(*d) * d->n_signals * sizeof(float);      // per-minibatch launch groups only
  return (base + critic_phase_fixed_floats(*d) + (size_t)n * critic_phase_floats_per_iter(*d)) * sizeof(float);
}

namespace {
// Fork / join events of the generator phase's model groups (hypad_epoch_io.aux_streams): created once per process on first use.
// (Event creation is not a stream operation: legal while a stream is being captured.  One epoch call at a time per process uses them.)
struct GenFork { hipEvent_t forked; hipEvent_t joined[7]; };
GenFork* gen_fork_events() {
  static GenFork f;
  static int state = 0;                    // 0 not tried, 1 ready, -1 failed
  if (state == 0) {
    bool ok = hipEventCreateWithFlags(&f.forked, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 7 && ok; ++i) ok = hipEventCreateWithFlags(&f.joined[i], hipEventDisableTiming) == hipSuccess;
    state = ok ? 1 : -1;
  }
  return state == 1 ? &f : nullptr;
}
__global__ void advance_counters_kernel(int32_t* counters, int opt, int n) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (counters[4] != 0) return;          // fail-stop (hypad_epoch_status): the launches before this one were no-ops
    counters[opt] += n; counters[3] += n;
  }
}
} // namespace
int hypad_train_epoch(const hypad_dims* d, const hypad_train_state* st, const hypad_epoch_io* io, hypad_stream_t s) {
  if (!io || !io->row_index || io->n_batches <= 0 || io->n_critics < 0) return HYPAD_EINVAL;
  int rc = check_dims(d);
  if (rc) return rc;
  const hypad_epoch_noise* nz = io->noise;
  const bool inj_masks = io->train_mode && nz && (nz->masks_cx || nz->masks_cz || nz->masks_gen);
  if (inj_masks && !(nz->masks_cx && nz->masks_cz && nz->masks_gen)) return HYPAD_EINVAL;      // all three planes or none
  IterCall c;
  c.x = io->x; c.x_sig_stride = io->x_signal_stride; c.x_row_stride = io->x_row_stride; c.z = nullptr; c.alpha = nullptr;
  c.ri_sig_stride = io->row_index_signal_stride;
  c.train_mode = io->train_mode; c.masks = nullptr; c.seed = io->seed;
  c.workspace = io->workspace; c.workspace_bytes = io->workspace_bytes;
  c.guard = 1;                                          // every launch of the epoch stops behind a resident critic launch that gave up
  c.flags = io->flags;
  const int iters = (2 * io->n_critics + 1) * io->n_batches;
  c.loss_sig_stride = (int64_t)iters * 4;
  int it = 0;
  const int64_t pass_rows = (int64_t)io->n_batches * d->batch;
  const size_t base = epoch_base_floats(*d);
  const size_t have = io->workspace_bytes / sizeof(float);
  const int64_t B = d->batch, L = d->latent_dim, S = d->signal_shape, ns = d->n_signals;
  const int64_t mk_cx = 12 * B * L + B * 2 * DEC_H, mk_cz = 6 * B * L, mk_gen = 6 * B * L + 2 * B * 2 * DEC_H;   // hypad_iter_io.drop layouts
  const bool hoisted = io->n_critics > 0 && critic_phase_supported(*d) &&
                       have >= base + critic_phase_fixed_floats(*d) + critic_phase_floats_per_iter(*d) && !(io->flags & HYPAD_EPOCH_PER_MINIBATCH);
  unsigned* zero_ptr = nullptr;                        // the resident critic launch's epoch words / flags: zeroed by the pack launch
  int zero_words = 0;
  bool zeroed = false;
  if (hoisted) critic_phase_zero_block(*d, (float*)io->workspace + base, have - base, io->n_critics * io->n_batches, &zero_ptr, &zero_words, io->flags);
  // the resident critic launch can give up (bounded waits): the state it began from is kept for hypad_epoch_restore
  float* snap = hoisted && critic_phase_persistent(*d, io->flags) ? epoch_snapshot_ptr(*d, io->workspace) : nullptr;
  {                                                    // packed generator weights: built once, then kept current by the dW kernel
    IterArgs ag;
    c.row_index = io->row_index; c.losses = io->losses;
    rc = fill_args(ag, d, st, c, 2);
    if (!rc) rc = launch_pack(ag, *d, (hipStream_t)s, zero_ptr, zero_words, &zeroed, false, snap);
    if (!rc) rc = launch_dw_items(ag, *d, false, (hipStream_t)s);      // (the epoch's generator steps leave the decay-only tensors to decay_steps_kernel)
    if (rc) return rc;
  }
  if (hoisted) {                                       // train.py:315-328, generator forwards hoisted (critic_fused.hip)
    IterArgs ax, az;
    c.row_index = io->row_index; c.losses = io->losses;
    c.masks = inj_masks ? nz->masks_cx : nullptr;      // (non-null selects the injected-mask mode; the planes travel in `nz`)
    rc = fill_args(ax, d, st, c, 0);
    c.masks = inj_masks ? nz->masks_cz : nullptr;
    if (!rc) rc = fill_args(az, d, st, c, 1);
    c.masks = nullptr;
    if (rc) return rc;
    const int n = io->n_critics * io->n_batches;
    if (io->enc_table && io->enc_table_rows <= 0) return HYPAD_EINVAL;
    rc = run_critic_phase(ax, az, io->row_index, n, io->losses, (float*)io->workspace + base, have - base, d->n_signals,
                          (hipStream_t)s, nullptr, nz, nullptr, zeroed ? zero_ptr : nullptr, io->flags, -1, io->enc_table, io->enc_table_rows);
    if (rc) return rc;
    it = 2 * n;
  } else {
    for (int k = 0; k < io->n_critics; ++k) {          // train.py:315-328, one launch group per minibatch
      for (int b = 0; b < io->n_batches; ++b) {
        const int64_t ci = (int64_t)k * io->n_batches + b;          // critic iteration index of the injected planes
        c.row_index = io->row_index + k * pass_rows + (int64_t)b * d->batch;
        c.losses = io->losses;             // (validated by fill_args; the pair writes to the two pointers below)
        IterCall cz = c;
        if (nz) {
          c.z = nz->z_cx ? nz->z_cx + ci * ns * B * L : nullptr; c.alpha = nz->alpha_cx ? nz->alpha_cx + ci * ns * B * S : nullptr;
          cz.z = nz->z_cz ? nz->z_cz + ci * ns * B * L : nullptr; cz.alpha = nz->alpha_cz ? nz->alpha_cz + ci * ns * B * L : nullptr;
          if (inj_masks) { c.masks = nz->masks_cx + ci * ns * mk_cx; cz.masks = nz->masks_cz + ci * ns * mk_cz; }
        }
        rc = run_critic_pair(d, st, c, io->losses + (int64_t)it * 4, io->losses + (int64_t)(it + 1) * 4, (hipStream_t)s, nullptr, &cz);
        it += 2;
        if (rc) return rc;
      }
    }
    c.z = nullptr; c.alpha = nullptr; c.masks = nullptr;
  }
  // train.py:347-352.  The models are independent of each other: with auxiliary streams they run in groups, one chain of
  // (generator launch, dW + Adam launch) x n_batches per group and stream, so a group's optimizer launch overlaps another group's
  // generator launch (a generator launch keeps 12 workgroups per model busy for ~37 us, the optimizer launch that follows is
  // latency- or bandwidth-bound: in lock step the chip idles through both).  Every launch then carries its own step number and
  // rng tick (IterArgs.step_add) and nobody advances the counters until the groups have joined.
  int groups = 1 + (io->aux_streams ? (io->n_aux_streams < 0 ? 0 : io->n_aux_streams > 7 ? 7 : io->n_aux_streams) : 0);
  if (groups > d->n_signals) groups = d->n_signals;
  if (io->n_batches < 1) groups = 1;
  GenFork* fork = nullptr;
  if (groups > 1) {
    fork = gen_fork_events();
    if (!fork) groups = 1;
  }
  if (groups > 1) {
    hipError_t e = hipEventRecord(fork->forked, (hipStream_t)s);
    for (int g = 1; g < groups && e == hipSuccess; ++g) e = hipStreamWaitEvent((hipStream_t)io->aux_streams[g - 1], fork->forked, 0);
    if (e != hipSuccess) return (int)e;
  }
  const int it_gen0 = it;
  for (int g = 0; g < groups; ++g) {
    const int s0 = (int)((int64_t)d->n_signals * g / groups), s1 = (int)((int64_t)d->n_signals * (g + 1) / groups);
    hipStream_t gs = g == 0 ? (hipStream_t)s : (hipStream_t)io->aux_streams[g - 1];
    for (int b = 0; b < io->n_batches; ++b) {
      c.row_index = io->row_index + io->n_critics * pass_rows + (int64_t)b * d->batch;
      c.losses = io->losses + (int64_t)(it_gen0 + b) * 4;
      if (nz) {
        c.z = nz->z_gen ? nz->z_gen + (int64_t)b * ns * B * L : nullptr;
        c.masks = inj_masks ? nz->masks_gen + (int64_t)b * ns * mk_gen : nullptr;
      }
      rc = run_gen(d, st, c, gs, nullptr, false, false, s0, s1 - s0, groups > 1 ? b : -1);
      if (rc) return rc;
    }
  }
  it = it_gen0 + io->n_batches;
  if (groups > 1) {
    hipError_t e = hipSuccess;
    for (int g = 1; g < groups && e == hipSuccess; ++g) {
      e = hipEventRecord(fork->joined[g - 1], (hipStream_t)io->aux_streams[g - 1]);
      if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)s, fork->joined[g - 1], 0);
    }
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(advance_counters_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, st->counters, 2, io->n_batches);      // generator steps (counters[2]) and rng ticks
    HYPAD_CHECK_LAUNCH();
  }
  // W_hh and the f-gate rows: all of the epoch's weight-decay steps at once (see decay_table)
  c.losses = io->losses;
  return run_decay_steps(d, st, c, io->n_batches, (hipStream_t)s);
}

int hypad_critic_phase_persistent(const hypad_dims* d) {
  if (check_dims(d) || !critic_phase_supported(*d)) return 0;
  return critic_phase_persistent(*d) ? 1 : 0;
}

int hypad_critic_phase_producers(const hypad_dims* d, int n_iters) {
  if (check_dims(d)) return 0;
  return critic_phase_producers(*d, n_iters) ? 1 : 0;
}

int hypad_epoch_record_info(const hypad_dims* d, int n_batches, int n_critics, int critic, hypad_record_info* out) {
  if (check_dims(d) || n_batches <= 0 || n_critics <= 0 || !out) return HYPAD_EINVAL;
  const int64_t n = (int64_t)n_batches * n_critics;
  if (n > 512) return HYPAD_EUNSUPPORTED;
  int rc = critic_phase_record_info(*d, (int)n, critic, out);
  if (rc) return rc;
  out->offset_floats += (int64_t)epoch_base_floats(*d);
  return HYPAD_OK;
}

int hypad_epoch_status(const hypad_train_state* st, int* status_host, hypad_stream_t s) {
  if (!st || !st->counters || !status_host) return HYPAD_EINVAL;
  int32_t v = 0;
  hipError_t e = hipMemcpyAsync(&v, st->counters + 4, sizeof(v), hipMemcpyDeviceToHost, (hipStream_t)s);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)s);
  if (e != hipSuccess) return (int)e;
  *status_host = (int)v;
  return HYPAD_OK;
}

int hypad_epoch_restore(const hypad_dims* d, const hypad_train_state* st, void* workspace, size_t workspace_bytes, hypad_stream_t s) {
  int rc = check_dims(d);
  if (rc) return rc;
  if (!st || !st->counters || !st->params.cx || !st->params.cz || !st->exp_avg.cx || !st->exp_avg.cz || !st->exp_avg_sq.cx || !st->exp_avg_sq.cz)
    return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < epoch_base_floats(*d) * sizeof(float)) return HYPAD_EWORKSPACE;
  IterArgs a{};
  a.P = st->params; a.M = st->exp_avg; a.V = st->exp_avg_sq; a.counters = st->counters;
  a.pcx = cx_layout(d->signal_shape, d->latent_dim).total; a.pcz = cz_layout(d->latent_dim).total;
  const int units = 3 * (a.pcx + a.pcz) / 4;
  hipLaunchKernelGGL(epoch_restore_kernel, dim3((units + 255) / 256, d->n_signals), dim3(256), 0, (hipStream_t)s, a, epoch_snapshot_ptr(*d, workspace),
                     d->n_signals);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

}  // extern "C"
