// The scoring forward pass: the test-loop body of anomaly_detection.py:67-113 (eval mode) for one trained model
// (hypad_score_forward_packed) or a group of them (hypad_score_forward_signals), on the training kernels' building blocks
// (nets.h, critic_mfma.h).
//
// Launch structure:
//   pack kernel                      (train_iters.hip, through launch_pack_generator: MFMA-native copies of the generator's weights
//                                     and the padded critic_x image into the workspace)
//   critic_rows[_signals]_kernel     (critic_x of every window: the weight image LDS-resident, one 16-row tile per wave at a time)
//   score_forward_{packed,signals}_kernel  (16 or 32 windows per workgroup: encoder -> decoder -> head, row distances)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "../../include/hypad.h"
#include "critic_mfma.h"
#include "train_common.h"

using namespace hypad;
using namespace hypad::train;

namespace {

// ------------------------------------------------------------------------------------------------ scoring forward, packed
// The test-loop body (anomaly_detection.py:67-113, eval mode) on the training kernels' machinery: 512 threads per 16 rows,
// packed weights (no LDS re-shape), LSTM cells in the gate products' epilogues, the critic as LDS-resident MFMA layers, the
// row-wise ball math four rows per wave.  The critic value of the windows (anomaly_detection.py:96-101) comes from its own launch,
// critic_rows_kernel: inside this kernel it was six workgroup barriers and an 18 KB weight image per 16 windows for 1 % of the FLOPs
// (0.526 -> 0.479 ms per 125 000 windows without it; the launch below takes 0.02).
//
// critic_x over rows, eval mode: the padded weight image (critic_mfma.h CriticPad) goes into LDS once per workgroup, then every WAVE walks
// its own 16-row tiles -- rows into a wave-private LDS tile (the next tile's rows are requested into registers before the layers of
// the current one), four layers on wave_gemm_nt with nothing but wave-local fences between them, the last layer as 16 dot products.
// Same products in the same order as critic_tile_fwd: same bits.
constexpr int CR_WAVES = 8;                  // waves per workgroup (fewer where the wave-private tiles of a wide window would not fit the LDS)
HD int critic_rows_lds_floats(int S, int L, int waves) {
  const CriticPad cp = critic_pad(S, L, 4);
  return cp.total + waves * (16 * cp.ldin + 2 * 16 * cp.LQ);
}
template <int SC, int LC>
__global__ __launch_bounds__(64 * CR_WAVES) void critic_rows_kernel(const float* __restrict__ cxpad, const float* __restrict__ x, int64_t x_ld,
                                                                    float* __restrict__ out, int64_t rows, int S_, int L_) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = SC ? SC : S_, L = LC ? LC : L_;
#include "critic_rows_body.inc"
}
int launch_critic_rows(const float* cxpad, const float* x, int64_t x_ld, float* out, int64_t rows, int S, int L, hipStream_t s) {
  int waves = CR_WAVES;
  while (waves > 1 && (size_t)critic_rows_lds_floats(S, L, waves) * sizeof(float) > 160 * 1024) waves >>= 1;
  const size_t lds = (size_t)critic_rows_lds_floats(S, L, waves) * sizeof(float);
  if (lds > 160 * 1024) return HYPAD_EUNSUPPORTED;
  const int64_t tiles = (rows + 15) / 16;
  // (its LDS plan puts one workgroup on a CU: 256 of them cover an MI355X, the tiles go round)
  const unsigned grid = (unsigned)std::min<int64_t>((tiles + waves - 1) / waves, 256);
  if (S == 100 && L == 20) {
    hipError_t e = allow_lds((const void*)critic_rows_kernel<100, 20>, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((critic_rows_kernel<100, 20>), dim3(grid), dim3(64 * waves), lds, s, cxpad, x, x_ld, out, rows, S, L);
  } else {
    hipError_t e = allow_lds((const void*)critic_rows_kernel<0, 0>, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((critic_rows_kernel<0, 0>), dim3(grid), dim3(64 * waves), lds, s, cxpad, x, x_ld, out, rows, S, L);
  }
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
struct ScoreArgs {
  const float* pk; const float* head_b; const float* x; int64_t x_ld;
  float* hyper; float* eucl; float* hyper_real; float* rowdist;
  int64_t rows; int S, L, hyperbolic;
};
struct ScoreLds { int xs, zs, bufA, bufB, total, ldS; };
constexpr int SCORE_WPE = 4;
HD ScoreLds score_lds(int S, int L, int MT) {
  ScoreLds p; int o = 0;
  p.ldS = lds_stride(S);
  const int rows = 16 * MT;
  int buf = rows * (2 * DEC_H + 4) > rows * p.ldS ? rows * (2 * DEC_H + 4) : rows * p.ldS;       // h tiles / e and head tiles
  if (MT == 1 && buf < 32 * p.ldS) buf = 32 * p.ldS;                                             // (the 32-row head tile of the 16-window form)
  buf = (buf + 3) & ~3;
  p.xs = o; o += rows * p.ldS;
  p.zs = o; o += rows * LP;
  p.bufA = o; o += buf;
  p.bufB = o; o += buf;
  p.total = o;
  return p;
}
// MT = 1: 16 windows per workgroup (small calls: more workgroups).  MT = 2: 32 windows -- every weight block a wave fetches feeds two
// row tiles, the stages' barriers and per-tile set-up are paid once per 32 windows.  Same products in the same order per row: same bits.
template <int SC, int LC, int MT>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(SCORE_WPE, SCORE_WPE))) void score_forward_packed_kernel(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int ROWS = 16 * MT;
  const int S = SC ? SC : a.S, L = LC ? LC : a.L;
  const ScoreLds lp = score_lds(S, L, MT);
  const int ldS = lp.ldS;
  const GenPack gp = gen_pack(S, L, a.hyperbolic);
  float* xs = smem + lp.xs; float* zs = smem + lp.zs; float* bufA = smem + lp.bufA; float* bufB = smem + lp.bufB;
  const int64_t r0 = (int64_t)blockIdx.x * ROWS;
#include "score_forward_body.inc"
}


// ------------------------------------------------------------------------------------------------ scoring forward, signal groups
// hypad_score_forward_signals: n models (stacked arenas, packed by one launch into per-signal slots of the workspace), ragged window
// counts, outputs concatenated in row order.  The signal table travels in the kernel arguments, SIG_CHUNK signals per launch.  A
// workgroup's signal is a scalar -- readfirstlane of a search over the table, or blockIdx.y: as a vector value it makes every buffer
// descriptor divergent and the compiler wraps each buffer store in a waterfall loop (b117628).  A forward tile never straddles two
// signals.  The per-tile code is score_forward_packed_kernel's and critic_rows_kernel's own: score_forward_body.inc and
// critic_rows_body.inc, included by the single-signal kernel and by its twin below after their prologues.  Shared as text and not as
// inline functions, which changed the single-signal kernels' scalar register counts (score_forward_packed_kernel 74 -> 75,
// critic_rows_kernel 56 -> 54); an included text compiles to the bytes of the copies it replaced
// (docs/history/scoring_shared_bodies.md).  So every signal's rows are those of a hypad_score_forward_packed call on that signal
// alone, bit for bit (tests/test_gpu_score_signals.py).
constexpr int SIG_CHUNK = 64;
struct SigTable {
  int n, sig0;                    // signals in this launch; index of the first one in the group (its arenas and packed slot)
  int tile_off[SIG_CHUNK + 1];    // forward launch: first workgroup of each signal, tile_off[n] = the grid
  int64_t row_off[SIG_CHUNK];     // first output row of each signal
  int64_t rows[SIG_CHUNK];        // its windows (> 0)
  int64_t x_off[SIG_CHUNK];       // its first float in x
};
template <int SC, int LC, int MT>
__global__ __launch_bounds__(TB) __attribute__((amdgpu_waves_per_eu(SCORE_WPE, SCORE_WPE))) void score_forward_signals_kernel(ScoreArgs g, SigTable t,
                                                                                                                                  int64_t ws_stride, int pd) {
  int sl = 0;
  for (int k = 1; k < t.n; ++k) sl += (int)blockIdx.x >= t.tile_off[k];
  sl = __builtin_amdgcn_readfirstlane(sl);
  const int sg = t.sig0 + sl;
  const int S = SC ? SC : g.S, L = LC ? LC : g.L;
  const int64_t o = t.row_off[sl];
  ScoreArgs a = g;
  a.pk = g.pk + sg * ws_stride;
  a.head_b = g.head_b ? g.head_b + (int64_t)sg * pd : nullptr;
  a.x = g.x + t.x_off[sl];
  a.hyper = g.hyper ? g.hyper + o * S : nullptr;
  a.eucl = g.eucl ? g.eucl + o * S : nullptr;
  a.hyper_real = g.hyper_real ? g.hyper_real + o * S : nullptr;
  a.rowdist = g.rowdist ? g.rowdist + o : nullptr;
  a.rows = t.rows[sl];
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int ROWS = 16 * MT;
  const ScoreLds lp = score_lds(S, L, MT);
  const int ldS = lp.ldS;
  const GenPack gp = gen_pack(S, L, a.hyperbolic);
  float* xs = smem + lp.xs; float* zs = smem + lp.zs; float* bufA = smem + lp.bufA; float* bufB = smem + lp.bufB;
  const int64_t r0 = (int64_t)((int)blockIdx.x - t.tile_off[sl]) * ROWS;         // (row 0 of this tile within its signal)
#include "score_forward_body.inc"
}
// grid (workgroups per signal, signals of the launch): the workgroups of signal blockIdx.y walk its 16-row tiles as critic_rows_kernel's do
template <int SC, int LC>
__global__ __launch_bounds__(64 * CR_WAVES) void critic_rows_signals_kernel(const float* __restrict__ ws, int64_t ws_stride, int64_t cx_off,
                                                                            const float* __restrict__ x0, int64_t x_ld, float* __restrict__ out0,
                                                                            SigTable tab, int S_, int L_) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int S = SC ? SC : S_, L = LC ? LC : L_;
  const int sl = blockIdx.y;
  const int64_t rows = tab.rows[sl];
  if ((int64_t)blockIdx.x * (blockDim.x >> 6) * 16 >= rows) return;          // (no tile for this workgroup: the whole workgroup leaves)
  const float* __restrict__ cxpad = ws + (tab.sig0 + sl) * ws_stride + cx_off;
  const float* __restrict__ x = x0 + tab.x_off[sl];
  float* __restrict__ out = out0 + tab.row_off[sl];
#include "critic_rows_body.inc"
}

}  // namespace

extern "C" {

size_t hypad_score_workspace_bytes(int S, int L, int hyperbolic) {
  if (S < 1 || S > MAX_S || L < 1 || L > MAX_L) return 0;
  return (size_t)(score_critic_offset(S, L, hyperbolic) + critic_pad(S, L, 4).total) * sizeof(float);      // packed generator + padded critic_x
}
int hypad_score_forward_packed(const float* enc, const float* dec, const float* cx, const float* x, int64_t x_row_stride, float* hyper,
                               float* eucl, float* hyper_real, float* critic, float* rowdist, int64_t rows, int S, int L,
                               int hyperbolic, void* workspace, size_t workspace_bytes, hypad_stream_t s) {
  if (S < 1 || S > MAX_S || L < 1 || L > MAX_L) return HYPAD_EUNSUPPORTED;
  if (!enc || !dec || !x || rows < 0 || (critic && !cx)) return HYPAD_EINVAL;
  if (x_row_stride > (1 << 24)) return HYPAD_EUNSUPPORTED;       // (a tile's rows are addressed with 32-bit byte offsets)
  if (!workspace || workspace_bytes < hypad_score_workspace_bytes(S, L, hyperbolic)) return HYPAD_EWORKSPACE;
  if (rows == 0) return HYPAD_OK;
  hypad_dims d; d.signal_shape = S; d.latent_dim = L; d.batch = 16; d.hyperbolic = hyperbolic; d.n_signals = 1; d.first_signal = 0;
  IterArgs pa{};
  pa.S = S; pa.L = L; pa.B = 16; pa.hyperbolic = hyperbolic;
  pa.P.enc = const_cast<float*>(enc); pa.P.dec = const_cast<float*>(dec);
  pa.pe = enc_layout(S, L).total; pa.pd = dec_layout(S, L, hyperbolic).total;
  pa.ws = (float*)workspace; pa.ws_sig_stride = 0; pa.pk_off = 0;
  pa.P.cx = const_cast<float*>(cx); pa.pcx = cx_layout(S, L).total;
  int rc = launch_pack_generator(pa, d, (hipStream_t)s, cx != nullptr);
  if (rc) return rc;
  if (critic) {          // (the image the pack launch wrote: critic_mfma.h CriticPad)
    rc = launch_critic_rows((const float*)workspace + score_critic_offset(S, L, hyperbolic), x, x_row_stride > 0 ? x_row_stride : S, critic, rows, S, L, (hipStream_t)s);
    if (rc) return rc;
  }
  if (!hyper && !eucl && !hyper_real && !rowdist) return HYPAD_OK;      // (only the critic value was asked for)
  ScoreArgs a;
  a.pk = (const float*)workspace; a.head_b = hyperbolic ? dec + dec_layout(S, L, 1).head_b : nullptr;
  a.x = x; a.x_ld = x_row_stride > 0 ? x_row_stride : S;
  a.hyper = hyper; a.eucl = eucl; a.hyper_real = hyper_real; a.rowdist = rowdist;
  a.rows = rows; a.S = S; a.L = L; a.hyperbolic = hyperbolic;
  // 32 windows per workgroup once that still leaves every CU several workgroups (two are resident on a CU at a time)
  // (the reference window only: the run-time-shape build of the 32-window form and the one for window 150 do not fit 128 registers)
  const bool ref_shape = S == 100 && L == 20;
  const int mt = ref_shape && rows >= (int64_t)32 * 2048 ? 2 : 1;
  const size_t lds = (size_t)score_lds(S, L, mt).total * sizeof(float);
  if (lds > 160 * 1024) return HYPAD_EUNSUPPORTED;
  const int64_t tiles = (rows + 16 * mt - 1) / (16 * mt);
  if (tiles > 0x7fffffff) return HYPAD_EINVAL;
  const void* fn = ref_shape ? (mt == 2 ? (const void*)score_forward_packed_kernel<100, 20, 2> : (const void*)score_forward_packed_kernel<100, 20, 1>)
                   : (const void*)score_forward_packed_kernel<0, 0, 1>;
  hipError_t e = allow_lds(fn, lds);
  if (e != hipSuccess) return (int)e;
  void* kargs[] = {&a};
  e = hipLaunchKernel(fn, dim3((unsigned)tiles), dim3(TB), kargs, lds, (hipStream_t)s);
  if (e != hipSuccess) return (int)e;
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
// the plan of a group: offsets valid (row_off[0] = 0, every signal > 0 windows, x_off >= 0), tile form from the total
static int score_signals_check(int n_signals, const int64_t* row_off, const int64_t* x_off) {
  if (n_signals < 1 || !row_off || row_off[0] != 0) return HYPAD_EINVAL;
  for (int i = 0; i < n_signals; ++i)
    if (row_off[i + 1] <= row_off[i] || (x_off && x_off[i] < 0)) return HYPAD_EINVAL;
  return HYPAD_OK;
}
static int64_t score_signals_stride(int S, int L, int hyperbolic) {      // floats per signal's slot in the workspace (256-byte aligned)
  return ((int64_t)score_critic_offset(S, L, hyperbolic) + critic_pad(S, L, 4).total + 63) & ~(int64_t)63;
}
static int score_signals_mt(int S, int L, int64_t total_rows) {          // the tile form hypad_score_forward_packed would take for total_rows
  return S == 100 && L == 20 && total_rows >= (int64_t)32 * 2048 ? 2 : 1;
}
size_t hypad_score_signals_workspace_bytes(int S, int L, int hyperbolic, int n_signals) {
  if (S < 1 || S > MAX_S || L < 1 || L > MAX_L || n_signals < 1) return 0;
  return (size_t)score_signals_stride(S, L, hyperbolic) * n_signals * sizeof(float);
}
int hypad_score_signals_tiles(int S, int L, int n_signals, const int64_t* row_off, int* rows_per_tile, int64_t* tiles) {
  if (S < 1 || S > MAX_S || L < 1 || L > MAX_L) return HYPAD_EUNSUPPORTED;
  int rc = score_signals_check(n_signals, row_off, nullptr);
  if (rc) return rc;
  const int rows = 16 * score_signals_mt(S, L, row_off[n_signals]);
  int64_t t = 0;
  for (int i = 0; i < n_signals; ++i) t += (row_off[i + 1] - row_off[i] + rows - 1) / rows;
  if (rows_per_tile) *rows_per_tile = rows;
  if (tiles) *tiles = t;
  return HYPAD_OK;
}
int hypad_score_forward_signals(const float* enc, const float* dec, const float* cx, int n_signals, const int64_t* row_off, const int64_t* x_off,
                                const float* x, int64_t x_row_stride, float* hyper, float* eucl, float* hyper_real, float* critic, float* rowdist,
                                int S, int L, int hyperbolic, void* workspace, size_t workspace_bytes, hypad_stream_t s) {
  if (S < 1 || S > MAX_S || L < 1 || L > MAX_L) return HYPAD_EUNSUPPORTED;
  int rc = score_signals_check(n_signals, row_off, x_off);
  if (rc) return rc;
  if (!x_off || !enc || !dec || !x || x_row_stride < 0 || (critic && !cx)) return HYPAD_EINVAL;
  if (x_row_stride > (1 << 24)) return HYPAD_EUNSUPPORTED;       // (a tile's rows are addressed with 32-bit byte offsets)
  if (n_signals > 65535) return HYPAD_EUNSUPPORTED;              // (the pack launch's grid.z)
  if (!workspace || workspace_bytes < hypad_score_signals_workspace_bytes(S, L, hyperbolic, n_signals)) return HYPAD_EWORKSPACE;
  const int64_t stride = score_signals_stride(S, L, hyperbolic), x_ld = x_row_stride > 0 ? x_row_stride : S;
  const int mt = score_signals_mt(S, L, row_off[n_signals]);
  hypad_dims d; d.signal_shape = S; d.latent_dim = L; d.batch = 16; d.hyperbolic = hyperbolic; d.n_signals = n_signals; d.first_signal = 0;
  IterArgs pa{};
  pa.S = S; pa.L = L; pa.B = 16; pa.hyperbolic = hyperbolic;
  pa.P.enc = const_cast<float*>(enc); pa.P.dec = const_cast<float*>(dec);
  pa.pe = enc_layout(S, L).total; pa.pd = dec_layout(S, L, hyperbolic).total;
  pa.ws = (float*)workspace; pa.ws_sig_stride = stride; pa.pk_off = 0;
  pa.P.cx = const_cast<float*>(cx); pa.pcx = cx_layout(S, L).total;
  rc = launch_pack_generator(pa, d, (hipStream_t)s, cx != nullptr);          // all signals' copies: one launch
  if (rc) return rc;
  const bool ref_shape = S == 100 && L == 20;
  const bool fwd = hyper || eucl || hyper_real || rowdist;
  const size_t lds = (size_t)score_lds(S, L, mt).total * sizeof(float);
  if (fwd && lds > 160 * 1024) return HYPAD_EUNSUPPORTED;
  int waves = CR_WAVES;
  while (waves > 1 && (size_t)critic_rows_lds_floats(S, L, waves) * sizeof(float) > 160 * 1024) waves >>= 1;
  const size_t clds = (size_t)critic_rows_lds_floats(S, L, waves) * sizeof(float);
  if (critic && clds > 160 * 1024) return HYPAD_EUNSUPPORTED;
  const void* fn = ref_shape ? (mt == 2 ? (const void*)score_forward_signals_kernel<100, 20, 2> : (const void*)score_forward_signals_kernel<100, 20, 1>)
                   : (const void*)score_forward_signals_kernel<0, 0, 1>;
  const void* cfn = ref_shape ? (const void*)critic_rows_signals_kernel<100, 20> : (const void*)critic_rows_signals_kernel<0, 0>;
  if (fwd) { hipError_t e = allow_lds(fn, lds); if (e != hipSuccess) return (int)e; }
  if (critic) { hipError_t e = allow_lds(cfn, clds); if (e != hipSuccess) return (int)e; }
  ScoreArgs a;
  a.pk = (const float*)workspace; a.head_b = hyperbolic ? dec + dec_layout(S, L, 1).head_b : nullptr;
  a.x = x; a.x_ld = x_ld;
  a.hyper = hyper; a.eucl = eucl; a.hyper_real = hyper_real; a.rowdist = rowdist;
  a.rows = 0; a.S = S; a.L = L; a.hyperbolic = hyperbolic;
  int pd = pa.pd;
  int64_t cx_off = score_critic_offset(S, L, hyperbolic);
  const int rows_per_tile = 16 * mt;
  for (int c0 = 0; c0 < n_signals; c0 += SIG_CHUNK) {        // (SIG_CHUNK signals per launch: the table is a kernel argument)
    SigTable t{};
    t.n = std::min(SIG_CHUNK, n_signals - c0); t.sig0 = c0;
    int64_t tiles = 0, max_rows = 0;
    for (int i = 0; i < t.n; ++i) {
      t.tile_off[i] = (int)tiles;
      t.row_off[i] = row_off[c0 + i]; t.rows[i] = row_off[c0 + i + 1] - row_off[c0 + i]; t.x_off[i] = x_off[c0 + i];
      tiles += (t.rows[i] + rows_per_tile - 1) / rows_per_tile;
      if (t.rows[i] > max_rows) max_rows = t.rows[i];
      if (tiles > 0x7fffffff) return HYPAD_EINVAL;
    }
    t.tile_off[t.n] = (int)tiles;
    if (critic) {          // (the images the pack launch wrote: critic_mfma.h CriticPad, one per signal)
      const int64_t per_sig = ((max_rows + 15) / 16 + waves - 1) / waves;
      const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(per_sig, (256 + t.n - 1) / t.n));
      const float* wsf = (const float*)workspace;
      void* cargs[] = {&wsf, (void*)&stride, &cx_off, (void*)&x, (void*)&x_ld, &critic, &t, &S, &L};
      hipError_t e = hipLaunchKernel(cfn, dim3(gx, (unsigned)t.n), dim3(64 * waves), cargs, clds, (hipStream_t)s);
      if (e != hipSuccess) return (int)e;
      HYPAD_CHECK_LAUNCH();
    }
    if (fwd) {
      void* kargs[] = {&a, &t, (void*)&stride, &pd};
      hipError_t e = hipLaunchKernel(fn, dim3((unsigned)tiles), dim3(TB), kargs, lds, (hipStream_t)s);
      if (e != hipSuccess) return (int)e;
      HYPAD_CHECK_LAUNCH();
    }
  }
  return HYPAD_OK;
}

}  // extern "C"
