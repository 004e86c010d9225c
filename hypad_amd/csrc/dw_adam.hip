// The weight-gradient + Adam step that closes every training iteration of train_iters.hip: the operand rows its row-tile kernels left in
// the workspace -> dW = left^T right on MFMA -> Adam (critics, Euclidean generator) or Riemannian Adam (hyperbolic generator) in registers.
// No gradient buffer exists: a weight's gradient tile lives in MFMA accumulators and is consumed by the update.
//
//   descriptors (DwDesc / DwTableT)     what has a gradient: weight blocks, bias vectors, decay-only ranges, the ball-valued head bias;
//                                       critic_table / gen_table build them on the host, dw_item() cuts a descriptor into per-wave items
//   generator: dw_items_kernel          the items as prepared records (DwItem) behind every pack launch, then per step
//              dw_adam_kernel           one wave per record (dw_adam_items_body); keeps the packed weight copies current, writes the losses
//              decay_steps_kernel       the never-read decay-only tensors, all of an epoch's steps at once
//   critics:   dw_adam_small_kernel, dw_adam_pair_kernel   one critic / critic_x || critic_z, items derived from the table in registers
//                                       (dw_adam_critic_body) -- the stand-alone launches every training path falls back on
// One copy of each item: the weight tile and the bias column sum are text shared by the two bodies (dw_weight_item.inc,
// dw_bias_item.inc); as functions they changed the registers of every dw_adam_kernel instantiation (docs/history/dw_adam_split.md).
// train_iters.hip reaches this file through the launch functions at its end (declared in train_common.h).
// Formulas: oracle/manual.py (CPU derivation sheet, validated against autograd and the reference fixtures).
#include <hip/hip_runtime.h>

#include "../../include/hypad.h"
#include "train_common.h"

using namespace hypad;
using namespace hypad::train;

namespace {

// ------------------------------------------------------------------------------------------------ descriptors and items
enum DwKind : int { DW_WEIGHT = 0, DW_BIAS = 1, DW_DECAY = 2, DW_BALL = 3 };
struct DwDesc {
  int16_t kind, net;
  int32_t p_off, p_ld, nrows, ncols;          // destination block (weights: nrows x ncols at row stride p_ld)
  int32_t left_off, left_ld, right_off, right_ld;
  int32_t red_rows;
  int32_t p_off2;                             // second destination with the same gradient (b_hh), or -1
  int32_t begin;                              // first work item
};
template <int CAP, int BLK>
struct DwTableT {
  static constexpr int cap = CAP, blk = BLK;
  int n, total_items;                         // n < 0: the table did not fit (host check)
  // Work items are dealt four to a workgroup (one per wave) and every descriptor starts on a workgroup boundary, so a
  // workgroup finds its descriptor with one byte lookup instead of a search (byte b of word b / 4).
  uint32_t block_desc[BLK / 4];
  DwDesc d[CAP];
};
using DwTable = DwTableT<60, 512>;            // generator (S = MAX_S needs ~470 workgroups)
using DwTableS = DwTableT<12, 64>;            // one critic

// Where a generator weight block / bias vector lives in the packed copies (layout.h GenPack), found from its arena offset:
// the dW + Adam kernel keeps the copies current so that an epoch never re-packs.
struct ShadowRef {
  int fwd, fwd_kg;       // forward copy: blocks of (compact rows, K), or -1
  int nbase;             // compact row of the block's row 0 (LSTM: 0 for the i gate rows, H for the g|o rows)
  int bwd, bwd_ng;       // backward-data copy (W^T), or -1; ng = k-groups of its reduction
  int mbase;             // reduction index of compact row 0 in the backward copy (direction * 3H)
  int bsum;              // summed-bias vector, or -1 (bias items)
  int gate_H;            // LSTM gate matrices: hidden size (forward copy rows are x * up16(H) + u); 0 otherwise
};
__device__ __forceinline__ ShadowRef shadow_ref(int net, int p_off, int S, int L, int hyper) {
  ShadowRef r{-1, 0, 0, -1, 0, 0, -1, 0};
  const GenPack gp = gen_pack(S, L, hyper);
  if (net == HYPAD_NET_ENCODER) {
    const EncLayout el = enc_layout(S, L);
    for (int d = 0; d < 2; ++d) {
      const int w = el.dir[d].w_ih, wg = w + 2 * ENC_H * S;
      if (p_off == w || p_off == wg) { r.fwd = gp.enc_g[d]; r.fwd_kg = (S + 15) >> 4; r.nbase = p_off == w ? 0 : ENC_H; r.gate_H = ENC_H; }
      const int b = el.dir[d].b_ih;
      if (p_off == b || p_off == b + 2 * ENC_H) { r.bsum = gp.enc_gb[d]; r.nbase = p_off == b ? 0 : ENC_H; r.gate_H = ENC_H; }
    }
    if (p_off == el.dense_w) { r.fwd = gp.enc_d; r.fwd_kg = (2 * ENC_H + 15) >> 4; r.bwd = gp.enc_d_t; r.bwd_ng = (L + 15) >> 4; }
    if (p_off == el.dense_b) r.bsum = gp.enc_db;
  } else if (net == HYPAD_NET_DECODER) {
    const DecLayout dl = dec_layout(S, L, hyper);
    if (p_off == dl.d1_w) { r.fwd = gp.d1; r.fwd_kg = (L + 15) >> 4; r.bwd = gp.d1_t; r.bwd_ng = (DEC_D1 + 15) >> 4; }
    if (p_off == dl.d1_b) r.bsum = gp.d1b;
    for (int l = 0; l < 2; ++l) {
      const int in = l == 0 ? DEC_D1 : 2 * DEC_H;
      for (int d = 0; d < 2; ++d) {
        const int w = dl.l[l][d].w_ih, wg = w + 2 * DEC_H * in;
        if (p_off == w || p_off == wg) {
          r.fwd = gp.l_g[l][d]; r.fwd_kg = (in + 15) >> 4; r.nbase = p_off == w ? 0 : DEC_H; r.gate_H = DEC_H;
          r.bwd = gp.l_t[l]; r.bwd_ng = (6 * DEC_H) >> 4; r.mbase = d * 3 * DEC_H;
        }
        const int b = dl.l[l][d].b_ih;
        if (p_off == b || p_off == b + 2 * DEC_H) { r.bsum = gp.l_gb[l][d]; r.nbase = p_off == b ? 0 : DEC_H; r.gate_H = DEC_H; }
      }
    }
    if (p_off == dl.d2_w) { r.fwd = gp.d2; r.fwd_kg = (2 * DEC_H + 15) >> 4; r.bwd = gp.d2_t; r.bwd_ng = (S + 15) >> 4; }
    if (p_off == dl.d2_b) r.bsum = gp.d2b;
    if (hyper && p_off == dl.head_w) { r.fwd = gp.head; r.fwd_kg = (S + 15) >> 4; r.bwd = gp.head_t; r.bwd_ng = (S + 15) >> 4; }
  }
  return r;
}

// ---- the generator's dW + Adam launch from prepared work-item records.  A wave of that launch used to spend 2.2 of its 5.5 us before its
// first operand load left: the workgroup's descriptor byte and the 52-byte descriptor out of a 3 KB kernel-argument table (whose
// scalar registers the compiler spilled), the tile's (n0, k0) by integer division, clamps, and shadow_ref()'s search for the packed
// positions of the updated weights.  All of that depends on the dimensions only: dw_items_kernel writes it once per pack launch, 128
// bytes per item, and a wave fetches its record with two scalar loads.
struct DwItem {                                // 32 words (train_common.h DW_ITEM_WORDS)
  int32_t kind;                                // DwKind, or -1: nothing to do (padding behind a descriptor's last item)
  int32_t net;
  int32_t n0, k0;                              // weight tile origin; bias: n0 = first column; decay: n0 = first element
  int32_t nrows, ncols, p_off, p_ld, p_off2;
  int32_t left_off, left_ld, right_off, right_ld, red_rows;
  int32_t fwd, fwd_kg, nbase, bwd, bwd_ng, mbase, bsum, gate_H;      // ShadowRef
  int32_t table_sig;                           // dw_table_sig of the table the records were written from: a launch that expects another table refuses them
  int32_t pad[9];
};
// what the records of a workspace depend on: the table (item count, with / without the decay-only ranges) and the dimensions.  The launch
// that consumes them carries the signature it expects; records written for another table (a pack with other arguments, or a caller that
// used the workspace as scratch in between) poison the step's loss instead of silently applying the wrong item set.
__host__ __device__ inline int32_t dw_table_sig(int total_items, int S, int L, int hyper, int n_desc) {
  uint32_t h = 0x9E3779B9u * (uint32_t)(total_items + 1);
  h ^= (uint32_t)S << 20; h ^= (uint32_t)L << 10; h ^= (uint32_t)n_desc << 2; h ^= (uint32_t)(hyper ? 1 : 0);
  return (int32_t)(h | 0x40000000u);          // never 0 (a zeroed workspace is not a table)
}
static_assert(sizeof(DwItem) == 4 * DW_ITEM_WORDS, "DwItem is DW_ITEM_WORDS words");
// Work item `item` of a table: its descriptor's fields, the tile origin and (SHADOW) where the packed copies keep what it updates;
// kind -1 for an item past the table's end or in the padding behind a descriptor's last item.  The one derivation: dw_items_kernel
// stores it, the critic launches -- no packed copies -- take it in registers.
template <bool SHADOW, class Table>
__device__ __forceinline__ DwItem dw_item(const Table& tab, int item, int S, int L, int hyper) {
  DwItem it{};
  it.kind = -1;
  it.table_sig = dw_table_sig(tab.total_items, S, L, hyper, tab.n);
  if constexpr (!SHADOW) it.fwd = it.bwd = it.bsum = -1;
  if (item < tab.total_items) {
    const int bx = item >> 2;
    const int di = (tab.block_desc[bx >> 2] >> (8 * (bx & 3))) & 0xff;
    const DwDesc d = tab.d[di];
    const int local = item - d.begin;
    bool live = false;
    if (d.kind == DW_WEIGHT) {
      const int tk = (d.ncols + 15) >> 4;
      live = local < ((d.nrows + 15) >> 4) * tk;
      it.n0 = (local / tk) * 16; it.k0 = (local % tk) * 16;
    } else if (d.kind == DW_BIAS) { live = local * 16 < d.nrows; it.n0 = local * 16; }
    else if (d.kind == DW_DECAY) { live = local * 256 < d.nrows; it.n0 = local * 256; }
    else if (d.kind == DW_BALL) live = local == 0;
    if (live) {
      it.kind = d.kind; it.net = d.net; it.nrows = d.nrows; it.ncols = d.ncols; it.p_off = d.p_off; it.p_ld = d.p_ld; it.p_off2 = d.p_off2;
      it.left_off = d.left_off; it.left_ld = d.left_ld; it.right_off = d.right_off; it.right_ld = d.right_ld; it.red_rows = d.red_rows;
      if constexpr (SHADOW) {
        const ShadowRef sh = shadow_ref(d.net, d.p_off, S, L, hyper);
        it.fwd = sh.fwd; it.fwd_kg = sh.fwd_kg; it.nbase = sh.nbase; it.bwd = sh.bwd; it.bwd_ng = sh.bwd_ng; it.mbase = sh.mbase; it.bsum = sh.bsum; it.gate_H = sh.gate_H;
      }
    }
  }
  return it;
}
__global__ __launch_bounds__(256) void dw_items_kernel(DwTable tab, DwItem* __restrict__ out, int S, int L, int hyper) {
  const int item = blockIdx.x * 256 + threadIdx.x;
  if (item >= DW_ITEM_CAP) return;
  out[item] = dw_item<true>(tab, item, S, L, hyper);
}

// SC / LC / BC: compile-time dims of the reference configuration (0 = run-time), which fold the layout arithmetic of gen_ws() into
// constants.
// (Measured and dropped in round 3: 32 x 32 weight tiles -- four accumulators per wave, half the operand loads per MFMA and per
// parameter -- for the many-signal launches: 157 registers (2 waves per SIMD instead of 3) and three round trips per item made
// the launch SLOWER at 8 / 16 / 32 signals per GPU: 33 -> 42, 56 -> 64, 101 -> 110 us.  The operand re-reads of the 16 x 16 tiles
// are L2 hits once a model's tiles share an XCD (COLOC); what the launch waits for is its scattered 64-byte store segments.)
// What the launch's time consists of at 32 signals per GPU (round 3 what-if builds, 85.6 us): without the packed copies' stores
// 69 us, without the moments' stores 83, without the operand loads 62, without the optimiser-state loads 74 -- i.e. bytes, not
// instructions: writing the packed copies as 16-byte stores (transposed copy as is, forward copy after a DPP quad transpose)
// instead of eight scattered 4-byte stores per lane changed nothing (84.5 us; 11.5 at one signal) and was dropped.
// KS: k-steps (groups of four reduction rows) a weight item keeps in flight: 48 covers B <= 64 in one memory round trip.
// (16 halves the registers and doubles the waves per SIMD; measured with 8 and 32 signals per GPU it changes nothing --
// with many signals the launch moves ~9 MB per signal and sits at ~3.5 TB/s of HBM traffic.)
constexpr int DW_KS_MANY = 16;               // k-steps in flight in the many-signal (co-located) form of the dW + Adam launch: 61 registers, seven waves
                                             // per SIMD instead of three (126 registers at 48).  Round 3, same box, launch time at 8 / 16 / 32 signals
                                             // per GPU: 48 -> 30.5 / 49.0 / 86.4 us, 32 -> 29.4 / 45.2 / 77.7, 24 -> 27.2 / 41.7 / 70.3, 16 -> 26.7 / 41.1 /
                                             // 68.1 (same accumulation order: same bits).  The one-signal launch keeps 48: it is as long as its slowest
                                             // item, and an item with all its operand rows in flight makes ONE memory round trip
constexpr int DW_KS_ONE = 48;                // ... that launch (the spread form), and the critic launches: their 3 B reduction rows in one round trip up to B = 64

// chunk > 0 (the spread placement): the records are cut into eight contiguous chunks of `chunk` items and workgroup bx takes its four
// from chunk bx mod 8 -- the workgroups of one chunk land on one XCD (round-robin dispatch), a matrix's tiles are neighbours in the
// table, so its operand rows are fetched into one or two L2s instead of all eight.  Speed / traffic only: the items are independent.
template <int SC, int LC, int BC, int KS>
__device__ __forceinline__ void dw_adam_items_body(const IterArgs& a, const DwItem* __restrict__ items, int total_items, const int bx, const int32_t table_sig,
                                                   const int chunk = 0, const int model = (int)blockIdx.y) {      // model: index inside the launch (blockIdx.y, or the co-located form's own)
  const int S_ = SC ? SC : a.S, L_ = LC ? LC : a.L, B_ = BC ? BC : a.B;
  const int sig = model + a.sig0;
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int j = lane & 15, q = lane >> 4;
  float* ws = a.ws + sig * a.ws_sig_stride;
  int item = bx * (THREADS / 64) + wave;                // the launch covers total_items: one item per wave
  if (chunk > 0) {
    const int c = bx & 7, in_chunk = (bx >> 3) * (THREADS / 64) + wave;
    item = in_chunk < chunk ? c * chunk + in_chunk : total_items;
  }
  // the record (wave-uniform address: scalar loads from the constant address space -- nothing writes the table during this launch) ...
  using CWord = const __attribute__((address_space(4))) int32_t;
  DwItem d;
  {
    CWord* src = (CWord*)(items + (item < total_items ? item : 0));
    int32_t* dst = reinterpret_cast<int32_t*>(&d);
#pragma unroll
    for (int i = 0; i < 23; ++i) dst[i] = src[i];          // (the 23 words in use)
  }
  if (d.table_sig != table_sig) {                           // (wave-uniform) records of another table: refuse them loudly -- a NaN loss for this model
    if (threadIdx.x == 0 && a.losses) { float* lo = a.losses + sig * a.loss_sig_stride; lo[0] = lo[1] = __builtin_nanf(""); }
    return;
  }
  // ... and, in the same batch of scalar fetches, the step counter and the bias corrections the generator launch left behind
  const int step = a.counters[a.opt] + (a.step_add >= 0 ? a.step_add + 1 : 0);      // (step_add < 0: already incremented by the iteration's first kernel)
  const float* ac = a.ws + (int64_t)a.sig0 * a.ws_sig_stride + gen_ws(B_, S_, L_).adamc;
  AdamCoef co;
  co.lr = a.lr; co.b1 = a.b1; co.b2 = a.b2; co.eps = a.eps; co.wd = a.wd; co.riemannian = a.riemannian; co.stabilize = a.stabilize;
  co.step = step; co.bc1 = ac[0]; co.bc2 = ac[1]; co.sqrt_bc2 = ac[2];
  const int64_t arena = d.net == HYPAD_NET_ENCODER ? a.pe : a.pd;
  float* P = (d.net == HYPAD_NET_ENCODER ? a.P.enc : a.P.dec) + sig * arena;
  float* M = (d.net == HYPAD_NET_ENCODER ? a.M.enc : a.M.dec) + sig * arena;
  float* V = (d.net == HYPAD_NET_ENCODER ? a.V.enc : a.V.dec) + sig * arena;
  if (item < total_items && d.kind >= 0) {
    if (d.kind == DW_WEIGHT) {
#include "dw_weight_item.inc"
    } else if (d.kind == DW_BIAS) {
#include "dw_bias_item.inc"
    } else if (d.kind == DW_DECAY) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = d.n0 + e * 64 + lane;
        if (n < d.nrows) {
          const int64_t o = d.p_off + n;
          float p = P[o], m = M[o], v = V[o];
          adam_update(p, m, v, 0.f, co);
          P[o] = p; M[o] = m; V[o] = v;
        }
      }
    } else if (d.kind == DW_BALL) {                // hyperbolic_linear.bias; gradient = sum of the per-tile partial column sums
      const float* left = ws + d.left_off;
      // (the ball rows with the gradient's parts: one round trip -- this item is the longest of the launch)
      const RowVec Pr = row_load(P + d.p_off, d.nrows, lane), Mr = row_load(M + d.p_off, d.nrows, lane), Vr = row_load(V + d.p_off, d.nrows, lane);
      RowVec g;
#pragma unroll
      for (int e = 0; e < MAX_EPL; ++e) g.v[e] = 0.f;
      for (int r0 = 0; r0 < d.red_rows; r0 += 8) {           // eight partial rows in flight per round trip (fixed order)
        float t[8][MAX_EPL];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = r0 + u < d.red_rows ? r0 + u : d.red_rows - 1;
#pragma unroll
          for (int e = 0; e < MAX_EPL; ++e) {
            const int c = lane + 64 * e;
            t[u][e] = c < d.nrows ? left[(int64_t)r * d.left_ld + c] : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
          for (int e = 0; e < MAX_EPL; ++e) g.v[e] += r0 + u < d.red_rows ? t[u][e] : 0.f;
      }
      radam_ball_wave(P + d.p_off, M + d.p_off, V + d.p_off, Pr, Mr, Vr, g, d.nrows, lane, co);
    }
  }
#if HYPAD_DIAG
  if (a.stamps && model == 0 && lane == 0 && item < 1024) {      // (scripts/diag_dw_items.py)
    a.stamps[3 * 48 * 8 + 64 + 2 * item] = (long long)__builtin_amdgcn_s_memrealtime();
    a.stamps[3 * 48 * 8 + 64 + 2 * item + 1] = item < total_items && d.kind >= 0 ? d.kind * 1000 + d.net * 100 + (d.red_rows >> 4) : -1;
  }
#endif
  if (bx == 0 && threadIdx.x == 0) {               // generator losses (train.py:232-234, 243-244)
    const GenWs gw = gen_ws(B_, S_, L_);
    float aux = 0.f, fx = 0.f, fz = 0.f;
    for (int t = 0; t < B_ / 16; ++t) {
      const float* part = ws + gw.partial + t * 4;
      aux += part[0]; fx += part[1]; fz += part[2];
    }
    aux = a.hyperbolic ? aux / a.B : aux / ((float)a.B * (float)a.S);
    float* lo = a.losses + sig * a.loss_sig_stride;
    lo[0] = 10.f * aux - fx / a.B - fz / a.B;
    lo[1] = aux; lo[2] = fx / a.B; lo[3] = fz / a.B;
    if (model == 0 && a.tick_owner && a.step_add < 0) a.counters[3] += 1;     // rng tick: nobody reads it inside this kernel
  }
}
// COLOC: one model's weight tiles share an XCD's L2 -- its ~0.9 MB of operand rows are fetched from HBM once, not once per XCD.
// Workgroups are dealt round-robin over the 8 XCDs, so in a ONE-dimensional grid workgroup id lands on XCD id mod 8: the launch's
// models go in groups of eight, id mod 8 picks the model of the group and id / 8 its workgroup -- 8 x blocks x ceil(models / 8)
// workgroups, none of them empty while the model count is a multiple of eight.  (Rounds 2-4 stretched blockIdx.x by 8 under a
// (blocks, models) grid and let seven of eight workgroups leave at once: 10 500 workgroups at 8 models, 1.2 us of the launch's
// 18.8 for the dispatcher to deal them -- 3.212 -> 3.178 ms per epoch at 8 models.  What the launch takes at 8 models and more
// is its bytes: 6.4 MB per model in one burst of loads and one of stores through the model's XCD, ~3 TB/s over the chip.)  Used
// from 8 signals per GPU on.  Speed only: no result depends on it.
template <int SC, int LC, int BC, int KS, bool COLOC = false>
__global__ __launch_bounds__(THREADS) void dw_adam_kernel(IterArgs a, const DwItem* __restrict__ items, int total_items, int chunk, int32_t table_sig) {
  if (a.guard && a.counters[4] != 0) return;
  if constexpr (COLOC) {
    // chunk carries the launch's model count here
    const int blocks = (total_items + THREADS / 64 - 1) / (THREADS / 64);
    const int t = (int)(blockIdx.x >> 3), model = (t / blocks) * 8 + (int)(blockIdx.x & 7);
    if (model >= chunk) return;
    dw_adam_items_body<SC, LC, BC, KS>(a, items, total_items, t % blocks, table_sig, 0, model);
  } else {
    // (chunk > 0: the grid is 8 x chunk / 4 workgroups, chunk = ceil(total / 8) rounded up to a multiple of four)
    dw_adam_items_body<SC, LC, BC, KS>(a, items, total_items, (int)blockIdx.x, table_sig, chunk);
  }
}
// ---- a critic's dW + Adam launch: the table travels in the kernel arguments (a dozen descriptors), a wave derives its item in registers
// (no packed copies: dw_item<false>) and takes the step's bias corrections itself.  Weight and bias items only (critic_table).
__device__ __forceinline__ void dw_adam_critic_body(const IterArgs& a, const DwTableS& tab) {
  constexpr int KS = DW_KS_ONE;
  const int sig = blockIdx.y + a.sig0;
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int j = lane & 15, q = lane >> 4;
  float* ws = a.ws + sig * a.ws_sig_stride;
  // (the coefficients in front of the item: 61 / 118 spilled scalars in the two kernels, item first 89 / 158 and a scratch slot)
  const int step = a.counters[a.opt] + (a.step_add >= 0 ? a.step_add + 1 : 0);      // (step_add < 0: already incremented by the iteration's first kernel)
  const AdamCoef co = adam_coef(a.lr, a.b1, a.b2, a.eps, a.wd, a.riemannian, a.stabilize, step);
  const DwItem d = dw_item<false>(tab, (int)blockIdx.x * (THREADS / 64) + wave, a.S, a.L, a.hyperbolic);      // one item per wave
  const int64_t arena = d.net == HYPAD_NET_CRITIC_X ? a.pcx : a.pcz;
  float* P = (d.net == HYPAD_NET_CRITIC_X ? a.P.cx : a.P.cz) + sig * arena;
  float* M = (d.net == HYPAD_NET_CRITIC_X ? a.M.cx : a.M.cz) + sig * arena;
  float* V = (d.net == HYPAD_NET_CRITIC_X ? a.V.cx : a.V.cz) + sig * arena;
  // The items' text with the critic launches' own load order: a weight item's optimiser state in front of its operand rows (behind their
  // first batch, the generator's order, the two kernels take 140 / 144 registers; so 128) and a bias item's behind its sums (see there)
  if (d.kind == DW_WEIGHT) {
#define DW_CRITIC_LOAD_ORDER
#include "dw_weight_item.inc"
  } else if (d.kind == DW_BIAS) {
#include "dw_bias_item.inc"
#undef DW_CRITIC_LOAD_ORDER
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && blockIdx.y == 0 && a.tick_owner && a.step_add < 0) a.counters[3] += 1;     // rng tick: nobody reads it inside this kernel
}
__global__ __launch_bounds__(THREADS) void dw_adam_small_kernel(IterArgs a, DwTableS tab) { dw_adam_critic_body(a, tab); }
__global__ __launch_bounds__(THREADS) void dw_adam_pair_kernel(IterArgs ax, DwTableS tx, IterArgs az, DwTableS tz) {
  if (blockIdx.z == 0) dw_adam_critic_body(ax, tx); else dw_adam_critic_body(az, tz);
}

// ------------------------------------------------------------------------------------------------ host: tables
template <class Table>
struct TableBuilder {
  Table t;
  bool overflow = false;
  TableBuilder() { t.n = 0; t.total_items = 0; for (int i = 0; i < Table::blk / 4; ++i) t.block_desc[i] = 0; }
  void push(DwDesc d, int items) {
    if (items <= 0) return;
    const int start = (t.total_items + 3) & ~3;          // descriptors start on a workgroup boundary
    const int b0 = start / 4, b1 = (start + items + 3) / 4;
    if (t.n >= Table::cap || b1 > Table::blk) { overflow = true; return; }
    d.begin = start;
    for (int b = b0; b < b1; ++b) t.block_desc[b >> 2] |= (uint32_t)t.n << (8 * (b & 3));
    t.d[t.n++] = d;
    t.total_items = start + items;
  }
  Table done() { if (overflow) t.n = -1; return t; }
  void weight(int net, int p_off, int p_ld, int nrows, int ncols, int left_off, int left_ld, int right_off, int right_ld, int red) {
    DwDesc d{};
    d.kind = DW_WEIGHT; d.net = (int16_t)net; d.p_off = p_off; d.p_ld = p_ld; d.nrows = nrows; d.ncols = ncols;
    d.left_off = left_off; d.left_ld = left_ld; d.right_off = right_off; d.right_ld = right_ld; d.red_rows = red; d.p_off2 = -1;
    push(d, ((nrows + 15) / 16) * ((ncols + 15) / 16));
  }
  void bias(int net, int p_off, int p_off2, int n, int left_off, int left_ld, int red) {
    DwDesc d{};
    d.kind = DW_BIAS; d.net = (int16_t)net; d.p_off = p_off; d.p_off2 = p_off2; d.nrows = n; d.ncols = 1;
    d.left_off = left_off; d.left_ld = left_ld; d.red_rows = red;
    push(d, (n + 15) / 16);
  }
  bool skip_decay = false;                     // decay-only ranges are left to decay_steps_kernel (hypad_train_epoch)
  void decay(int net, int p_off, int n) {
    if (skip_decay) return;
    DwDesc d{};
    d.kind = DW_DECAY; d.net = (int16_t)net; d.p_off = p_off; d.nrows = n; d.p_off2 = -1;
    push(d, (n + 255) / 256);
  }
  void ball(int net, int p_off, int n, int left_off, int left_ld, int red) {
    DwDesc d{};
    d.kind = DW_BALL; d.net = (int16_t)net; d.p_off = p_off; d.nrows = n; d.left_off = left_off; d.left_ld = left_ld;
    d.red_rows = red; d.p_off2 = -1;
    push(d, 1);
  }
  // one LSTM direction: weight_ih rows [0,H) <- compact cols [c0, c0+H); rows [2H,4H) <- cols [c0+H, c0+3H)
  void lstm_dir(int net, const LstmDir& ld, int H, int K, int left_off, int left_ld, int c0, int right_off, int right_ld, int red,
                bool decay_too) {
    weight(net, ld.w_ih, K, H, K, left_off + c0, left_ld, right_off, right_ld, red);
    weight(net, ld.w_ih + 2 * H * K, K, 2 * H, K, left_off + c0 + H, left_ld, right_off, right_ld, red);
    bias(net, ld.b_ih, ld.b_hh, H, left_off + c0, left_ld, red);
    bias(net, ld.b_ih + 2 * H, ld.b_hh + 2 * H, 2 * H, left_off + c0 + H, left_ld, red);
    if (decay_too) {   // no data gradient: f-gate rows and W_hh still decay under RiemannianAdam
      decay(net, ld.w_ih + H * K, H * K);
      decay(net, ld.w_hh, 4 * H * H);
      decay(net, ld.b_ih + H, H);
      decay(net, ld.b_hh + H, H);
    }
  }
};

DwTableS critic_table(int net, const CriticLayout& cl, const CritWs& cw, int B, int L) {
  TableBuilder<DwTableS> tb;
  for (int li = 0; li <= cl.nh; ++li) {
    int k = li == 0 ? cl.in_dim : L, n = li == cl.nh ? 1 : L;
    int right = li == 0 ? cw.in_right : cw.act[li - 1];
    tb.weight(net, cl.w[li], k, n, k, cw.left[li], n, right, k, 3 * B);
    tb.bias(net, cl.b[li], -1, n, cw.left[li], n, 2 * B);      // the GP rows carry no bias gradient
  }
  return tb.done();
}

// Parameters that never receive a data gradient -- W_hh and the f-gate rows of W_ih / b_ih / b_hh of every LSTM direction (h0 =
// c0 = 0 at T = 1: SURVEY.md A.2) -- but still move under RiemannianAdam's weight decay (train.py:286): 119 k of the generator's
// 245 k floats at window 100, 45 % of the dW + Adam launch's optimiser traffic.  No kernel ever reads them, so inside an epoch
// they are advanced ONCE, after the last generator step, by all the epoch's steps at a time (decay_steps_kernel): the same
// arithmetic in the same order, element by element -- bit-identical -- with 1 / n_batches of the traffic.
struct DecayTable { int n, total; int net[24], off[24], len[24], begin[24]; };
DecayTable decay_table(const hypad_dims& dm) {
  DecayTable t{};
  const int S = dm.signal_shape, L = dm.latent_dim;
  const EncLayout el = enc_layout(S, L);
  const DecLayout dl = dec_layout(S, L, dm.hyperbolic);
  auto add = [&](int net, int off, int len) { t.net[t.n] = net; t.off[t.n] = off; t.len[t.n] = len; t.begin[t.n] = t.total; t.total += (len + 255) & ~255; ++t.n; };
  auto dir = [&](int net, const LstmDir& ld, int H, int K) { add(net, ld.w_ih + H * K, H * K); add(net, ld.w_hh, 4 * H * H); add(net, ld.b_ih + H, H); add(net, ld.b_hh + H, H); };
  for (int d = 0; d < 2; ++d) dir(HYPAD_NET_ENCODER, el.dir[d], ENC_H, S);
  for (int d = 0; d < 2; ++d) { dir(HYPAD_NET_DECODER, dl.l[0][d], DEC_H, DEC_D1); dir(HYPAD_NET_DECODER, dl.l[1][d], DEC_H, 2 * DEC_H); }
  return t;
}
// the last `nsteps` generator steps of the decay-only parameters; counters[opt] already holds the last step's number
__global__ __launch_bounds__(256) void decay_steps_kernel(IterArgs a, DecayTable tab, int nsteps) {
  __shared__ float bc[2 * 64];
  if (a.guard && a.counters[4] != 0) return;
  const int sig = blockIdx.y;
  const int last = a.counters[a.opt];
  const int e = blockIdx.x * 256 + threadIdx.x;
  int r = 0;
  for (int i = 1; i < tab.n; ++i) r = e >= tab.begin[i] ? i : r;          // (ranges start on 256-element boundaries: block-uniform)
  const int idx = e - tab.begin[r];
  const bool live = idx < tab.len[r];
  const int net = tab.net[r];
  const int64_t o = (int64_t)sig * (net == HYPAD_NET_ENCODER ? a.pe : a.pd) + tab.off[r] + (live ? idx : 0);
  float* P = (net == HYPAD_NET_ENCODER ? a.P.enc : a.P.dec) + o;
  float* M = (net == HYPAD_NET_ENCODER ? a.M.enc : a.M.dec) + o;
  float* V = (net == HYPAD_NET_ENCODER ? a.V.enc : a.V.dec) + o;
  float p = *P, m = *M, v = *V;
  AdamCoef co;
  co.lr = a.lr; co.b1 = a.b1; co.b2 = a.b2; co.eps = a.eps; co.wd = a.wd; co.riemannian = a.riemannian; co.stabilize = a.stabilize; co.step = 0;
  co.bc1 = 1.f; co.bc2 = 1.f; co.sqrt_bc2 = 1.f;
  for (int s0 = 0; s0 < nsteps; s0 += 64) {                               // bias corrections of 64 steps at a time (double-precision powers)
    __syncthreads();
    if (threadIdx.x < 64 && s0 + threadIdx.x < nsteps) {
      const AdamCoef c = adam_coef(a.lr, a.b1, a.b2, a.eps, a.wd, a.riemannian, a.stabilize, last - nsteps + 1 + s0 + threadIdx.x);
      bc[2 * threadIdx.x] = c.bc1; bc[2 * threadIdx.x + 1] = c.bc2;
    }
    __syncthreads();
    const int n = nsteps - s0 < 64 ? nsteps - s0 : 64;
    for (int k = 0; k < n; ++k) {
      co.bc1 = bc[2 * k]; co.bc2 = bc[2 * k + 1];
      adam_update(p, m, v, 0.f, co);
    }
  }
  if (live) { *P = p; *M = m; *V = v; }
}

DwTable gen_table(const hypad_dims& dm, bool with_decay = true) {
  const int B = dm.batch, S = dm.signal_shape, L = dm.latent_dim;
  const bool hyp = dm.hyperbolic != 0;
  const EncLayout el = enc_layout(S, L);
  const DecLayout dl = dec_layout(S, L, dm.hyperbolic);
  const GenWs gw = gen_ws(B, S, L);
  TableBuilder<DwTable> tb;
  tb.skip_decay = !with_decay;
  for (int d = 0; d < 2; ++d)
    tb.lstm_dir(HYPAD_NET_ENCODER, el.dir[d], ENC_H, S, gw.dgenc, 6 * ENC_H, d * 3 * ENC_H, gw.xg, S, 2 * B, hyp);     // chains R and Z
  tb.weight(HYPAD_NET_ENCODER, el.dense_w, 2 * ENC_H, L, 2 * ENC_H, gw.dzenc, L, gw.enc_h, 2 * ENC_H, 2 * B);
  tb.bias(HYPAD_NET_ENCODER, el.dense_b, -1, L, gw.dzenc, L, 2 * B);
  tb.weight(HYPAD_NET_DECODER, dl.d1_w, L, DEC_D1, L, gw.da0, DEC_D1, gw.zcat, L, 2 * B);
  tb.bias(HYPAD_NET_DECODER, dl.d1_b, -1, DEC_D1, gw.da0, DEC_D1, 2 * B);
  for (int d = 0; d < 2; ++d) {
    tb.lstm_dir(HYPAD_NET_DECODER, dl.l[0][d], DEC_H, DEC_D1, gw.dg0, 6 * DEC_H, d * 3 * DEC_H, gw.a0, DEC_D1, 2 * B, hyp);
    tb.lstm_dir(HYPAD_NET_DECODER, dl.l[1][d], DEC_H, 2 * DEC_H, gw.dg1, 6 * DEC_H, d * 3 * DEC_H, gw.h0d, 2 * DEC_H, 2 * B, hyp);
  }
  tb.weight(HYPAD_NET_DECODER, dl.d2_w, 2 * DEC_H, S, 2 * DEC_H, gw.dpre2, S, gw.h1, 2 * DEC_H, 2 * B);
  tb.bias(HYPAD_NET_DECODER, dl.d2_b, -1, S, gw.dpre2, S, 2 * B);
  if (hyp) {
    tb.weight(HYPAD_NET_DECODER, dl.head_w, S, S, S, gw.du, S, gw.ecat, S, 3 * B);
    tb.ball(HYPAD_NET_DECODER, dl.head_b, S, gw.ballpart, S, 2 * (B / 16));      // per (role, tile) partial column sums
  }
  return tb.done();
}

inline int dw_blocks(int items) { int b = (items + 3) / 4; return b < 1 ? 1 : b; }
// opt (IterArgs.opt): 0 critic_x, 1 critic_z
DwTableS critic_table_of(const IterArgs& a) {
  return a.opt == 0 ? critic_table(HYPAD_NET_CRITIC_X, cx_layout(a.S, a.L), crit_ws(a.B, a.S, a.L, 4), a.B, a.L)
                    : critic_table(HYPAD_NET_CRITIC_Z, cz_layout(a.L), crit_ws(a.B, a.L, a.L, 2), a.B, a.L);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ host: launches (train_common.h)
bool hypad::train::dw_tables_fit(const hypad_dims& d) { return gen_table(d).n >= 0; }      // (the critic tables are far smaller)

int hypad::train::launch_dw_critic(const IterArgs& a, int n_signals, hipStream_t s) {
  const DwTableS tab = critic_table_of(a);
  hipLaunchKernelGGL(dw_adam_small_kernel, dim3(dw_blocks(tab.total_items), n_signals), dim3(THREADS), 0, s, a, tab);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad::train::launch_dw_critic_pair(const IterArgs& ax, const IterArgs& az, int n_signals, hipStream_t s) {
  const DwTableS tx = critic_table_of(ax);
  const DwTableS tz = critic_table_of(az);
  const int items = tx.total_items > tz.total_items ? tx.total_items : tz.total_items;
  hipLaunchKernelGGL(dw_adam_pair_kernel, dim3(dw_blocks(items), n_signals, 2), dim3(THREADS), 0, s, ax, tx, az, tz);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

// the work-item records of the generator's dW + Adam launch (DwItem), into signal 0's workspace: behind every pack launch whose
// workspace generator steps will run in (run_gen with pack = true; hypad_train_epoch once per epoch)
int hypad::train::launch_dw_items(const IterArgs& a, const hypad_dims& d, bool with_decay, hipStream_t s) {
  const DwTable tab = gen_table(d, with_decay);
  if (tab.n < 0 || tab.total_items > DW_ITEM_CAP) return HYPAD_EUNSUPPORTED;
  DwItem* items = reinterpret_cast<DwItem*>(a.ws + ws_items_offset(d));
  hipLaunchKernelGGL(dw_items_kernel, dim3(DW_ITEM_CAP / 256), dim3(256), 0, s, tab, items, d.signal_shape, d.latent_dim, d.hyperbolic);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad::train::launch_dw_gen(const IterArgs& a, const hypad_dims& d, bool with_decay, int nsig, int flags, int reps, hipStream_t s) {
  const bool ref_cfg = a.S == 100 && a.L == 20 && a.B == 64;          // BASELINE.json configs[0..2]
  const bool mv_cfg = a.S == 150 && a.L == 20 && a.B == 256;          // configs[3]: 5 channels x 30, batch 256
  const bool wadi_cfg = a.S == 123 && a.L == 20 && a.B == 64;         // the reference's configs/multivariate.yaml:5-7 as shipped (WADI)
  const bool swat_cfg = a.S == 51 && a.L == 20 && a.B == 64;          // ... and its SWAT alternative
  const DwTable tab = gen_table(d, with_decay);            // (its item count; the records themselves were written behind the pack launch)
  const DwItem* items = reinterpret_cast<const DwItem*>(a.ws + ws_items_offset(d));
  const int total_items = tab.total_items;
  const int32_t tsig = dw_table_sig(tab.total_items, d.signal_shape, d.latent_dim, d.hyperbolic, tab.n);      // (the records carry the signature of the table they were written from)
  const bool coloc = (flags & HYPAD_EPOCH_DW_COLOC) ? true : (flags & HYPAD_EPOCH_DW_SPREAD) ? false : d.n_signals >= 8;      // (measured: -2 % of the epoch at 8-32 signals, +8 % at 1-2: few signals' tiles want all of the chip's CUs)
  const int dw_chunk = ((tab.total_items + 7) / 8 + 3) & ~3;          // spread placement: eight chunks of the records, one per XCD (dw_adam_items_body)
  const dim3 dgrid = coloc ? dim3(8 * dw_blocks(tab.total_items) * ((nsig + 7) / 8)) : dim3(8 * (dw_chunk / 4), nsig);
  for (int r = 0; r < reps; ++r) {
    if (coloc) {
      if (ref_cfg) hipLaunchKernelGGL((dw_adam_kernel<100, 20, 64, DW_KS_MANY, true>), dgrid, dim3(THREADS), 0, s, a, items, total_items, coloc ? nsig : dw_chunk, tsig);
      else if (mv_cfg) hipLaunchKernelGGL((dw_adam_kernel<150, 20, 256, DW_KS_MANY, true>), dgrid, dim3(THREADS), 0, s, a, items, total_items, coloc ? nsig : dw_chunk, tsig);
      else hipLaunchKernelGGL((dw_adam_kernel<0, 0, 0, DW_KS_MANY, true>), dgrid, dim3(THREADS), 0, s, a, items, total_items, coloc ? nsig : dw_chunk, tsig);
    } else if (ref_cfg) hipLaunchKernelGGL((dw_adam_kernel<100, 20, 64, DW_KS_ONE>), dgrid, dim3(THREADS), 0, s, a, items, total_items, coloc ? nsig : dw_chunk, tsig);
    else if (mv_cfg) hipLaunchKernelGGL((dw_adam_kernel<150, 20, 256, DW_KS_ONE>), dgrid, dim3(THREADS), 0, s, a, items, total_items, coloc ? nsig : dw_chunk, tsig);
    else if (wadi_cfg) hipLaunchKernelGGL((dw_adam_kernel<123, 20, 64, DW_KS_ONE>), dgrid, dim3(THREADS), 0, s, a, items, total_items, coloc ? nsig : dw_chunk, tsig);
    else if (swat_cfg) hipLaunchKernelGGL((dw_adam_kernel<51, 20, 64, DW_KS_ONE>), dgrid, dim3(THREADS), 0, s, a, items, total_items, coloc ? nsig : dw_chunk, tsig);
    else hipLaunchKernelGGL((dw_adam_kernel<0, 0, 0, DW_KS_ONE>), dgrid, dim3(THREADS), 0, s, a, items, total_items, coloc ? nsig : dw_chunk, tsig);
  }
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad::train::launch_decay_steps(const IterArgs& a, const hypad_dims& d, int nsteps, hipStream_t s) {
  const DecayTable tab = decay_table(d);
  hipLaunchKernelGGL(decay_steps_kernel, dim3(tab.total / 256, d.n_signals), dim3(256), 0, s, a, tab, nsteps);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
