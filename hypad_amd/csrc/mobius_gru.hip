// The Moebius GRU (hyperspace/hyrnn_nets.py:61-151 at k = -1): cell and sequence loop, forward and back-propagation through time; and
// mobius_pointwise_mul (math_.py:1361-1371) on its own.  Shapes: x (steps, rows, I), h (rows, H), w_ih (3H, I), w_hh (3H, H), bias
// (3, H) on the ball; chunk order r, h, z.
//
//   T(mh, h, mx, x, b) = ((mh scaled by |h|) (+) (mx scaled by |x|)) (+) b         one_rnn_transform, with mh = h W_h^T, mx = x W_i^T
//   r = sigmoid(logmap0(T_r))   z = sigmoid(logmap0(T_z))   rh = r (.) h   h~ = [fn](T_h on rh)   out = h (+) (z (.) ((-h) (+) h~))
//
// Forward.  (1) x_t W_ih^T of ALL steps is one GEMM over steps * rows rows (hypad_linear_act_fwd) into the workspace.  (2) The
// recurrence is ONE launch: a workgroup per 16-row tile walks the steps with the h tile in LDS -- gemm_nt of h against [W_hr; W_hz],
// a row pass (a wave per row, fp64 registers: rowops.h) to rh, gemm_nt of rh against W_hh's h block, a row pass to out_t, which is
// stored and becomes the next h tile (z is computed in the second pass, from the first product).  Weights are streamed from
// L2 (tile_gemm.h).  Rows are independent: no grid-wide hand-off.  The cell is steps = 1.
// The training form saves the six products per (step, row): [mx_r | mx_h | mx_z | mh_r | mh_z | m_rh], 6H floats; everything else is
// recomputed.  |rh| is taken from the fp32 rh the product was formed from, |h| from the stored fp32 h.
//
// Backward: ONE persistent launch walks the steps in reverse with the carried dL/dh tile in LDS.  Per step: row pass A through out,
// delta, h~ and the z gate; g_rh = g_mrh W_hh^h (gemm_nn); row pass B through rh = r (.) h and the r gate; dL/dh_prev += [g_mh_r |
// g_mh_z] [W_hr; W_hz] (gemm_nn).  The product gradients, rh_t, h_{t-1}, the per-row bias gradients and dL/d|x_t| go to the workspace;
// the parameter and input gradients are then dense contractions over steps * rows rows (hypad_linear_act_bwd, hypad_column_sum,
// grad_x += dL/d|x| x / |x|).  No atomics: every sum has one owner and a fixed order.
//
// Dynamic LDS of one workgroup, ld(n) = pad4(n) + 4 floats:
//   forward    4 (16 (2 ld(H) + ld(3H)) + 2304) + 128 bytes -- h, rh, the products, the wave-private weight slabs, |x_t|; 92 032 at H = 256
//   backward   4 (16 (3 ld(H) + ld(2H))) + 128 bytes       -- h, dL/dh, g_rh, [g_mrh or g_mh_r | g_mh_z], dL/d|rh|;    83 072 at H = 256
// both are checked against gfx950's 160 KiB per workgroup before anything is launched.
#include <hip/hip_runtime.h>

#include "../../include/hypad.h"
#include "nets.h"

using namespace hypad;

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int RPW = 16 / WAVES;                         // rows of the tile per wave
constexpr int WST = WAVES * WSTAGE_FLOATS;
constexpr int MAX_DIM = 64 * MAX_EPL;
constexpr size_t LDS_LIMIT = 160 * 1024;                 // a gfx950 workgroup's LDS
using R = RowD<64, MAX_EPL>;                            // a row per wave: at most 4 fp64 elements per lane and row value

__host__ __device__ inline int ld_of(int n) { return pad4(n) + 4; }
inline size_t gru_fwd_lds(int H) { return (size_t)(16 * (2 * ld_of(H) + ld_of(3 * H)) + WST) * sizeof(float) + 16 * sizeof(double); }
inline size_t gru_bwd_lds(int H) { return (size_t)(16 * (3 * ld_of(H) + ld_of(2 * H))) * sizeof(float) + 16 * sizeof(double); }

__device__ __forceinline__ double rowd_norm(const R& a) { return sqrt(rowd_dot(a, a)); }
__device__ __forceinline__ double global_row_norm(const float* __restrict__ p, int n, int lane) {
  double s = 0.0;
  for (int c = lane; c < n; c += 64) { const double v = p[c]; s += v * v; }
  return sqrt(groupd_sum<64>(s));
}
__device__ __forceinline__ R apply_nonlin(const R& y, int nonlin) {
  if (nonlin == NONLIN_TANH) return mobius_fn_row<NONLIN_TANH>(y);
  if (nonlin == NONLIN_RELU) return mobius_fn_row<NONLIN_RELU>(y);
  return y;
}
__device__ __forceinline__ R apply_nonlin_bwd(const R& y, const R& go, int nonlin) {
  if (nonlin == NONLIN_TANH) return mobius_fn_row_bwd<NONLIN_TANH>(y, go);
  if (nonlin == NONLIN_RELU) return mobius_fn_row_bwd<NONLIN_RELU>(y, go);
  return go;
}
__device__ __forceinline__ R rowd_neg(const R& a) {
  R o;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) o.v[e] = -a.v[e];
  return o;
}
// the row the fp32 buffers hold of a value
__device__ __forceinline__ R rowd_as_stored(const R& a) {
  R o;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) o.v[e] = (double)(float)a.v[e];
  return o;
}

struct GruFwdArgs {
  const float* x; const float* h0; const float* w_hh; const float* bias;
  const float* pre;                                     // (steps * rows, 3H) = x W_ih^T
  float* out; float* saved;                             // (steps, rows, H); (steps, rows, 6H) or null
  int steps; int64_t rows; int I, H, nonlin;
};

__global__ __launch_bounds__(THREADS) void mobius_gru_fwd_kernel(GruFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = a.H, ldh = ld_of(H), ldy = ld_of(3 * H);
  float* hs = smem;                                     // [16][ldh]: h_{t-1}
  float* rs = hs + 16 * ldh;                            // [16][ldh]: rh
  float* ys = rs + 16 * ldh;                            // [16][ldy]: [mh_r | mh_z | m_rh]
  float* wst = ys + 16 * ldy;
  double* xn = reinterpret_cast<double*>(wst + WST);    // [16]: |x_t| of the rows
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, a.rows - r0);
  tile_load(hs, ldh, a.h0 + r0 * H, H, 16, H, valid);
  const R br = rowd_load<R>(a.bias, H, lane), bh = rowd_load<R>(a.bias + H, H, lane), bz = rowd_load<R>(a.bias + 2 * H, H, lane);
  __syncthreads();
  for (int t = 0; t < a.steps; ++t) {
    const int64_t tr0 = (int64_t)t * a.rows + r0;
    gemm_nt<1, true>(hs, ldh, a.w_hh, H, H, 2 * H, RowMap{H, H}, nullptr, nullptr, ys, ldy, 0, wst);
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < RPW; ++i) {
      const int r = wave * RPW + i;
      const bool ok = r < valid;
      const float* pre = a.pre + (tr0 + (ok ? r : 0)) * 3 * H;
      const R h = rowd_load<R>(hs + r * ldh, H, lane);
      const double xraw = ok ? global_row_norm(a.x + (tr0 + r) * a.I, a.I, lane) : 0.0;
      const R rg = sigmoid_logmap0_d(rnn_transform_row(rowd_load<R>(ys + r * ldy, H, lane), rowd_norm(h), rowd_load<R>(pre, ok ? H : 0, lane), xraw, br));
      rowd_store(rs + r * ldh, mobius_pointwise_mul_d(rg, h), H, lane);
      if (lane == 0) xn[r] = xraw;
      if (a.saved && ok) {
        float* sv = a.saved + (tr0 + r) * 6 * H;
        for (int c = lane; c < 3 * H; c += 64) sv[c] = pre[c];
        for (int c = lane; c < 2 * H; c += 64) sv[3 * H + c] = ys[r * ldy + c];
      }
    }
    __syncthreads();
    gemm_nt<1, true>(rs, ldh, a.w_hh + (size_t)H * H, H, H, H, identity_map(), nullptr, nullptr, ys, ldy, 2 * H, wst);
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < RPW; ++i) {
      const int r = wave * RPW + i;
      const bool ok = r < valid;
      const int hv = ok ? H : 0;
      const float* pre = a.pre + (tr0 + (ok ? r : 0)) * 3 * H;
      const R h = rowd_load<R>(hs + r * ldh, H, lane);
      const double xraw = xn[r], rhraw = rowd_norm(rowd_load<R>(rs + r * ldh, H, lane));
      const R z = sigmoid_logmap0_d(rnn_transform_row(rowd_load<R>(ys + r * ldy + H, H, lane), rowd_norm(h), rowd_load<R>(pre + 2 * H, hv, lane), xraw, bz));
      const R ht = apply_nonlin(rnn_transform_row(rowd_load<R>(ys + r * ldy + 2 * H, H, lane), rhraw, rowd_load<R>(pre + H, hv, lane), xraw, bh), a.nonlin);
      const R o = mobius_add_d(h, mobius_pointwise_mul_d(z, mobius_add_d(rowd_neg(h), ht)));
      rowd_store(hs + r * ldh, o, H, lane);             // (this wave's own row: nobody else reads it before the barrier)
      if (ok) {
        rowd_store(a.out + (tr0 + r) * H, o, H, lane);
        if (a.saved) {
          float* sv = a.saved + (tr0 + r) * 6 * H + 5 * H;
          for (int c = lane; c < H; c += 64) sv[c] = ys[r * ldy + 2 * H + c];
        }
      }
    }
    __syncthreads();
  }
}

struct GruBwdArgs {
  const float* x; const float* h0; const float* w_hh; const float* bias; const float* out; const float* saved;
  const float* gout; const float* ghl;                  // (steps, rows, H); (rows, H) or null
  float* gmx;                                           // (steps * rows, 3H): [g_mx_r | g_mx_h | g_mx_z]
  float* gmhr; float* gmhz; float* gmrh;                // (steps * rows, H) each
  float* rh; float* hprev;                              // (steps * rows, H): rh_t and h_{t-1}, the left operands of grad_w_hh
  float* gb;                                            // (steps * rows, 3H) per-row bias gradients, or null
  float* gxn;                                           // (steps * rows): dL/d|x_t|
  float* gh0;                                           // (rows, H) or null
  int steps; int64_t rows; int I, H, nonlin;
};

__global__ __launch_bounds__(THREADS) void mobius_gru_bwd_kernel(GruBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int H = a.H, ldh = ld_of(H), ldd = ld_of(2 * H);
  float* hs = smem;                                     // [16][ldh]: h_{t-1}
  float* gs = hs + 16 * ldh;                            // [16][ldh]: the carried dL/dh
  float* qs = gs + 16 * ldh;                            // [16][ldh]: g_mrh W_hh^h
  float* ds = qs + 16 * ldh;                            // [16][ldd]: [g_mrh, then g_mh_r | g_mh_z]
  double* grn = reinterpret_cast<double*>(ds + 16 * ldd);   // [16]: dL/d|rh|
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, a.rows - r0);
  const R br = rowd_load<R>(a.bias, H, lane), bh = rowd_load<R>(a.bias + H, H, lane), bz = rowd_load<R>(a.bias + 2 * H, H, lane);
  tile_for(16, H, [&](int r, int c) { gs[r * ldh + c] = (a.ghl && r < valid) ? a.ghl[(r0 + r) * H + c] : 0.f; });
  for (int t = a.steps - 1; t >= 0; --t) {
    const int64_t tr0 = (int64_t)t * a.rows + r0;
    const float* hsrc = t == 0 ? a.h0 + r0 * H : a.out + ((int64_t)(t - 1) * a.rows + r0) * H;
    __syncthreads();                                    // the last step's readers of hs are done
    tile_load(hs, ldh, hsrc, H, 16, H, valid);
    __syncthreads();
    // ---- pass A: out = h (+) (z (.) delta), delta = (-h) (+) h~, h~, the z gate
#pragma unroll 1
    for (int i = 0; i < RPW; ++i) {
      const int r = wave * RPW + i;
      const bool ok = r < valid;
      const int hv = ok ? H : 0;
      const float* sv = a.saved + (tr0 + (ok ? r : 0)) * 6 * H;
      const R h = rowd_load<R>(hs + r * ldh, H, lane);
      const double hraw = rowd_norm(h), xraw = ok ? global_row_norm(a.x + (tr0 + r) * a.I, a.I, lane) : 0.0;
      R go = rowd_load<R>(gs + r * ldh, H, lane);
      {
        const R g = rowd_load<R>(a.gout + (tr0 + (ok ? r : 0)) * H, hv, lane);
#pragma unroll
        for (int e = 0; e < R::EPL; ++e) go.v[e] += g.v[e];
      }
      const R mxr = rowd_load<R>(sv, hv, lane), mxh = rowd_load<R>(sv + H, hv, lane), mxz = rowd_load<R>(sv + 2 * H, hv, lane);
      const R mhr = rowd_load<R>(sv + 3 * H, hv, lane), mhz = rowd_load<R>(sv + 4 * H, hv, lane), mrh = rowd_load<R>(sv + 5 * H, hv, lane);
      const R yz = rnn_transform_row(mhz, hraw, mxz, xraw, bz);
      const R z = sigmoid_logmap0_d(yz);
      const R rhs = rowd_as_stored(mobius_pointwise_mul_d(sigmoid_logmap0_d(rnn_transform_row(mhr, hraw, mxr, xraw, br)), h));
      const double rhraw = rowd_norm(rhs);
      const R yh = rnn_transform_row(mrh, rhraw, mxh, xraw, bh);
      const R ht = apply_nonlin(yh, a.nonlin);
      const R nh = rowd_neg(h);
      const R dl = mobius_add_d(nh, ht);
      R dh, dzd, dz, ddl, dnh, dht;
      mobius_add_bwd_d(h, mobius_pointwise_mul_d(z, dl), go, dh, dzd);
      mobius_pointwise_mul_bwd_d(z, dl, dzd, dz, ddl);
      mobius_add_bwd_d(nh, ht, ddl, dnh, dht);
      const R dyh = apply_nonlin_bwd(yh, dht, a.nonlin);
      R gmrh, gmxh, gmhz, gmxz, dbh, dbz;
      double grh_n, gxn_h, ghn_z, gxn_z;
      rnn_transform_row_bwd(mrh, rhraw, mxh, xraw, bh, dyh, gmrh, gmxh, dbh, grh_n, gxn_h);
      rnn_transform_row_bwd(mhz, hraw, mxz, xraw, bz, sigmoid_logmap0_bwd_d(yz, dz), gmhz, gmxz, dbz, ghn_z, gxn_z);
      const double ch = ghn_z / fmax(hraw, (double)MIN_NORM);
#pragma unroll
      for (int e = 0; e < R::EPL; ++e) dh.v[e] += ch * h.v[e] - dnh.v[e];
      rowd_store(gs + r * ldh, dh, H, lane);            // dL/dh_{t-1} so far (this wave's own row)
      rowd_store(ds + r * ldd, gmrh, H, lane);
      rowd_store(ds + r * ldd + H, gmhz, H, lane);
      if (lane == 0) grn[r] = grh_n;
      if (ok) {
        const int64_t gr = tr0 + r;
        rowd_store(a.gmrh + gr * H, gmrh, H, lane);
        rowd_store(a.gmhz + gr * H, gmhz, H, lane);
        rowd_store(a.gmx + gr * 3 * H + H, gmxh, H, lane);
        rowd_store(a.gmx + gr * 3 * H + 2 * H, gmxz, H, lane);
        rowd_store(a.rh + gr * H, rhs, H, lane);
        for (int c = lane; c < H; c += 64) a.hprev[gr * H + c] = hs[r * ldh + c];
        if (a.gb) {
          rowd_store(a.gb + gr * 3 * H + H, dbh, H, lane);
          rowd_store(a.gb + gr * 3 * H + 2 * H, dbz, H, lane);
        }
        if (lane == 0) a.gxn[gr] = (float)(gxn_h + gxn_z);   // (pass B adds the r gate's share)
      }
    }
    __syncthreads();
    gemm_nn<1>(ds, ldd, 0, a.w_hh + (size_t)H * H, H, H, identity_map(), H, qs, ldh, false);
    // ---- pass B: rh = r (.) h and the r gate
#pragma unroll 1
    for (int i = 0; i < RPW; ++i) {
      const int r = wave * RPW + i;
      const bool ok = r < valid;
      const int hv = ok ? H : 0;
      const float* sv = a.saved + (tr0 + (ok ? r : 0)) * 6 * H;
      const R h = rowd_load<R>(hs + r * ldh, H, lane);
      const double hraw = rowd_norm(h), xraw = ok ? global_row_norm(a.x + (tr0 + r) * a.I, a.I, lane) : 0.0;
      const R mxr = rowd_load<R>(sv, hv, lane), mhr = rowd_load<R>(sv + 3 * H, hv, lane);
      const R yr = rnn_transform_row(mhr, hraw, mxr, xraw, br);
      const R rg = sigmoid_logmap0_d(yr);
      const R rhs = rowd_as_stored(mobius_pointwise_mul_d(rg, h));
      R drh = rowd_load<R>(qs + r * ldh, H, lane);
      const double crh = grn[r] / fmax(rowd_norm(rhs), (double)MIN_NORM);
#pragma unroll
      for (int e = 0; e < R::EPL; ++e) drh.v[e] += crh * rhs.v[e];
      R drg, dh, gmhr, gmxr, dbr;
      double ghn_r, gxn_r;
      mobius_pointwise_mul_bwd_d(rg, h, drh, drg, dh);
      rnn_transform_row_bwd(mhr, hraw, mxr, xraw, br, sigmoid_logmap0_bwd_d(yr, drg), gmhr, gmxr, dbr, ghn_r, gxn_r);
      const double ch = ghn_r / fmax(hraw, (double)MIN_NORM);
      const R g0 = rowd_load<R>(gs + r * ldh, H, lane);
#pragma unroll
      for (int e = 0; e < R::EPL; ++e) dh.v[e] += ch * h.v[e] + g0.v[e];
      rowd_store(gs + r * ldh, dh, H, lane);
      rowd_store(ds + r * ldd, gmhr, H, lane);
      if (ok) {
        const int64_t gr = tr0 + r;
        rowd_store(a.gmhr + gr * H, gmhr, H, lane);
        rowd_store(a.gmx + gr * 3 * H, gmxr, H, lane);
        if (a.gb) rowd_store(a.gb + gr * 3 * H, dbr, H, lane);
        if (lane == 0) a.gxn[gr] += (float)gxn_r;
      }
    }
    __syncthreads();
    gemm_nn<1>(ds, ldd, 0, a.w_hh, H, 2 * H, RowMap{H, H}, H, gs, ldh, true);
  }
  if (a.gh0) tile_store(a.gh0 + r0 * H, H, gs, ldh, 16, H, valid);
}

// mobius_pointwise_mul on its own: a wave per row
__global__ __launch_bounds__(THREADS) void pointwise_mul_rows(const float* __restrict__ w, const float* __restrict__ x, float* __restrict__ out,
                                                              int64_t rows, int dim, int wbc) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dim, mobius_pointwise_mul_d(rowd_load<R>(w + (wbc ? 0 : r * dim), dim, lane), rowd_load<R>(x + r * dim, dim, lane)), dim,
               lane);
}
__global__ __launch_bounds__(THREADS) void pointwise_mul_rows_bwd(const float* __restrict__ w, const float* __restrict__ x,
                                                                  const float* __restrict__ go, float* __restrict__ gw, float* __restrict__ gx,
                                                                  int64_t rows, int dim, int wbc) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    R dw, dx;
    mobius_pointwise_mul_bwd_d(rowd_load<R>(w + (wbc ? 0 : r * dim), dim, lane), rowd_load<R>(x + r * dim, dim, lane),
                               rowd_load<R>(go + r * dim, dim, lane), dw, dx);
    rowd_store(gw + r * dim, dw, dim, lane);
    rowd_store(gx + r * dim, dx, dim, lane);
  }
}

inline int wave_grid(int64_t rows) {
  const int64_t b = (rows + WAVES - 1) / WAVES;
  return (int)(b > 4096 ? 4096 : b < 1 ? 1 : b);
}
inline int pmul_check(const float* w, const float* x, const void* o, int64_t rows, int dim, int64_t w_rows) {
  if (!w || !x || !o || rows < 0 || dim <= 0 || (w_rows != 1 && w_rows != rows)) return HYPAD_EINVAL;
  return dim > MAX_DIM ? HYPAD_EUNSUPPORTED : HYPAD_OK;
}

// the float offsets of the workspace's parts; tr = steps * rows
struct GruWorkspace { size_t pre, gmx, gmhr, gmhz, gmrh, rh, hprev, gb, scratch, gxn, total; };
inline GruWorkspace gru_workspace(int64_t tr, int H) {
  GruWorkspace w;
  const size_t n = (size_t)tr, h = (size_t)H;
  w.pre = 0;                        // forward: x W_ih^T
  w.gmx = 0;                        // backward: the same 3H columns hold the gradients of x W_ih^T
  w.gmhr = w.gmx + n * 3 * h;
  w.gmhz = w.gmhr + n * h;
  w.gmrh = w.gmhz + n * h;
  w.rh = w.gmrh + n * h;
  w.hprev = w.rh + n * h;
  w.gb = w.hprev + n * h;
  w.scratch = w.gb + n * 3 * h;     // hypad_linear_act_bwd's copy of the gradient it contracts
  w.gxn = w.scratch + n * 3 * h;
  w.total = w.gxn + n;
  return w;
}
inline int gru_check(const float* w_ih, const float* w_hh, const float* bias, int steps, int64_t rows, int I, int H, int nonlin, size_t lds) {
  if (!w_ih || !w_hh || !bias || steps <= 0 || rows < 0 || I <= 0 || H <= 0) return HYPAD_EINVAL;
  if (nonlin < HYPAD_NONLIN_NONE || nonlin > HYPAD_NONLIN_RELU) return HYPAD_EINVAL;
  if (I > MAX_DIM || H > MAX_DIM || (int64_t)steps * rows > 0x7fffffff) return HYPAD_EUNSUPPORTED;
  // (the dense calls' LDS, hypad_linear_act_fwd / _bwd at 3H outputs: refused here, before anything has been written)
  if ((size_t)(16 * (ld_of(I) + ld_of(3 * H)) + WST) * sizeof(float) > 150 * 1024) return HYPAD_EUNSUPPORTED;
  return lds > LDS_LIMIT ? HYPAD_EUNSUPPORTED : HYPAD_OK;
}
inline int zero_floats(float* p, size_t n, hipStream_t s) {
  if (!p) return HYPAD_OK;
  const hipError_t e = hipMemsetAsync(p, 0, n * sizeof(float), s);
  return e == hipSuccess ? HYPAD_OK : (int)e;
}

}  // namespace

extern "C" {

int hypad_mobius_pointwise_mul_fwd(const float* w, const float* x, float* out, int64_t rows, int dim, int64_t w_rows, hypad_stream_t s) {
  const int rc = pmul_check(w, x, out, rows, dim, w_rows);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(pointwise_mul_rows, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, w, x, out, rows, dim,
                     (int)(w_rows == 1 && rows != 1));
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_mobius_pointwise_mul_bwd(const float* w, const float* x, const float* go, float* gw, float* gx, int64_t rows, int dim,
                                   int64_t w_rows, hypad_stream_t s) {
  const int rc = pmul_check(w, x, go, rows, dim, w_rows);
  if (rc) return rc;
  if (!gw || !gx) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  hipLaunchKernelGGL(pointwise_mul_rows_bwd, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, w, x, go, gw, gx, rows, dim,
                     (int)(w_rows == 1 && rows != 1));
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

size_t hypad_mobius_gru_workspace_bytes(int steps, int64_t rows, int in_dim, int hidden) {
  if (steps <= 0 || rows <= 0 || in_dim <= 0 || hidden <= 0) return 0;
  return gru_workspace((int64_t)steps * rows, hidden).total * sizeof(float);
}

int hypad_mobius_gru_fwd(const float* x, const float* h0, const float* w_ih, const float* w_hh, const float* bias, float* out, float* saved,
                         void* workspace, size_t workspace_bytes, int steps, int64_t rows, int in_dim, int hidden, int nonlin,
                         hypad_stream_t s) {
  const size_t lds = gru_fwd_lds(hidden > 0 && hidden <= MAX_DIM ? hidden : 1);
  int rc = gru_check(w_ih, w_hh, bias, steps, rows, in_dim, hidden, nonlin, lds);
  if (rc || rows == 0) return rc;
  if (!x || !h0 || !out) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < hypad_mobius_gru_workspace_bytes(steps, rows, in_dim, hidden)) return HYPAD_EWORKSPACE;
  const int64_t tr = (int64_t)steps * rows;
  float* ws = (float*)workspace;
  const GruWorkspace w = gru_workspace(tr, hidden);
  hipError_t e = allow_lds((const void*)mobius_gru_fwd_kernel, lds);
  if (e != hipSuccess) return HYPAD_EUNSUPPORTED;
  rc = hypad_linear_act_fwd(x, w_ih, nullptr, ws + w.pre, tr, in_dim, 3 * hidden, HYPAD_ACT_NONE, s);
  if (rc) return rc;
  const GruFwdArgs a{x, h0, w_hh, bias, ws + w.pre, out, saved, steps, rows, in_dim, hidden, nonlin};
  hipLaunchKernelGGL(mobius_gru_fwd_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(THREADS), lds, (hipStream_t)s, a);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad_mobius_gru_bwd(const float* x, const float* h0, const float* w_ih, const float* w_hh, const float* bias, const float* out,
                         const float* saved, const float* grad_out, const float* grad_h_last, float* grad_x, float* grad_h0,
                         float* grad_w_ih, float* grad_w_hh, float* grad_bias, void* workspace, size_t workspace_bytes, int steps,
                         int64_t rows, int in_dim, int hidden, int nonlin, hypad_stream_t s) {
  const size_t lds = gru_bwd_lds(hidden > 0 && hidden <= MAX_DIM ? hidden : 1);
  int rc = gru_check(w_ih, w_hh, bias, steps, rows, in_dim, hidden, nonlin, lds);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)s;
  const int I = in_dim, H = hidden;
  if (rows == 0) {                                          // an empty batch: the sums over no rows are zeros
    rc = zero_floats(grad_w_ih, (size_t)3 * H * I, st);
    if (!rc) rc = zero_floats(grad_w_hh, (size_t)3 * H * H, st);
    return rc ? rc : zero_floats(grad_bias, (size_t)3 * H, st);
  }
  if (!x || !h0 || !out || !saved || !grad_out) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < hypad_mobius_gru_workspace_bytes(steps, rows, in_dim, hidden)) return HYPAD_EWORKSPACE;
  if (!grad_x && !grad_h0 && !grad_w_ih && !grad_w_hh && !grad_bias) return HYPAD_OK;
  const int64_t tr = (int64_t)steps * rows;
  float* ws = (float*)workspace;
  const GruWorkspace w = gru_workspace(tr, H);
  hipError_t e = allow_lds((const void*)mobius_gru_bwd_kernel, lds);
  if (e != hipSuccess) return HYPAD_EUNSUPPORTED;
  const GruBwdArgs a{x, h0, w_hh, bias, out, saved, grad_out, grad_h_last, ws + w.gmx, ws + w.gmhr, ws + w.gmhz, ws + w.gmrh, ws + w.rh,
                     ws + w.hprev, grad_bias ? ws + w.gb : nullptr, ws + w.gxn, grad_h0, steps, rows, I, H, nonlin};
  hipLaunchKernelGGL(mobius_gru_bwd_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(THREADS), lds, st, a);
  HYPAD_CHECK_LAUNCH();
  // the dense contractions over all steps * rows rows
  if (grad_x || grad_w_ih) {                                // grad_x = G_mx W_ih (+ dL/d|x| x / |x|), grad_w_ih = G_mx^T x
    rc = hypad_linear_act_bwd(x, w_ih, nullptr, ws + w.gmx, grad_x, grad_w_ih, nullptr, grad_w_ih ? ws + w.scratch : nullptr, tr, I, 3 * H,
                              HYPAD_ACT_NONE, s);
    if (!rc && grad_x) rc = norm_grad_add_launch(x, ws + w.gxn, grad_x, tr, I, s);
    if (rc) return rc;
  }
  if (grad_w_hh) {                                          // its three H x H blocks: g_mh_r^T h_prev, g_mrh^T rh, g_mh_z^T h_prev
    const float* left[3] = {ws + w.gmhr, ws + w.gmrh, ws + w.gmhz};
    const float* right[3] = {ws + w.hprev, ws + w.rh, ws + w.hprev};
    for (int b = 0; b < 3; ++b) {
      rc = hypad_linear_act_bwd(right[b], w_hh + (size_t)b * H * H, nullptr, left[b], nullptr, grad_w_hh + (size_t)b * H * H, nullptr,
                                ws + w.scratch, tr, H, H, HYPAD_ACT_NONE, s);
      if (rc) return rc;
    }
  }
  return grad_bias ? hypad_column_sum(ws + w.gb, grad_bias, tr, 3 * H, s) : HYPAD_OK;
}

}  // extern "C"
