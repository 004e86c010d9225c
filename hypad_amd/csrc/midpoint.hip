// The weighted Moebius gyromidpoint (math_.py:1953-2122, _lambda_x :382-383, at k = -1) in its attention / aggregation form -- below --
// and in its pooling form (the second half of this file: "the reduce form"), and mobius_scalar_mul (math_.py:788-858) on its own.
// Shapes of the bmm form: xs (batch, M, D) on the ball, weights (batch, N, M), out (batch, N, D).
//
//   gamma_j = 2 / max(1 - |x_j|^2, 1e-15)     c_j = gamma_j - 1
//   nom_i = sum_j w_ij gamma_j x_j     den_i = sum_j |w_ij| c_j     alpha_i = sum_j |w_ij|
//   t_i = nom_i / max(den_i, 1e-10)    a_i = t_i / (1 + sqrt(1 - |t_i|^2))    [lincomb: a_i = alpha_i (x) a_i]    out_i = project(a_i)
//
// Forward: ONE launch, a workgroup of four waves per (batch element, 64 output rows).  It walks M in chunks of 64 points: the xs chunk
// is staged in LDS once, 1 - |x_j|^2 is taken from an fp64 sum of the staged fp32 values (the one cancellation among the operands, as
// dist2plane.hip takes 1 - x2) and the rows are scaled to gamma_j x_j in place -- a point is re-formed once per 64 output rows instead
// of being written to and read from a workspace by a pre-pass, which would cost the attention shape (N = M = 100: two row tiles) a
// second launch to save two re-formations.  Each wave multiplies its 16 x 64 weight tile with the chunk on fp32 MFMA (16 rows x all
// D columns of accumulators); den and alpha are fp64 VALU sums of non-negative terms, every lane a fixed quarter of the chunk.  The
// epilogue (rowops.h: midpoint_tail_d) runs in fp64 registers on the fp32 sums, 16 lanes a row.  The training form stores
// saved (batch, N, D + 2) = [nom | den | alpha]; the epilogue always starts from those fp32 values, so inference has the same bits.
//
// Backward: (1) a row pass, a wave per output row, from `saved` and grad_out to g_s = g_t / den', g_d and g_alpha in the workspace;
// (2) grad_w_ij = gamma_j <g_s_i, x_j> + sign(w_ij) (g_d_i c_j + g_alpha_i): 64 x 64 tiles, contraction over D in chunks of 128;
// (3) grad_x_j = gamma_j G_j + gamma_j^2 (<G_j, x_j> + h_j) x_j with G = W^T g_s, h = |W|^T g_d: the forward's kernel body with the
// weight tile read transposed, a workgroup owning all D columns of its 64 points.  (2) and (3) are independent launches: either
// gradient alone has the bits of the run that asks for both.  No atomics: every sum has one owner and a fixed order.
//
// Dynamic LDS of one workgroup, C = 64, 128 or 256 columns for D <= 64, 128, 256:
//   product kernels   4 (64 (C + 4) + 64 68 + 64) + 8 128 bytes    -- the chunk, the weight tile, c_j or g_d, den and alpha;  85 248 at C = 256
//   grad_w            4 (2 64 (min(pad4(D), 128) + 4) + 128)       -- the g_s and x tiles, gamma_j and c_j;                    68 096 at most
// both are checked against gfx950's 160 KiB per workgroup before anything is launched.
#include <hip/hip_runtime.h>

#include "../../include/hypad.h"
#include "rowops.h"

using namespace hypad;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MT = 64;                                  // output rows of a workgroup, 16 per wave
constexpr int KC = 64;                                  // contraction positions staged at a time
constexpr int LDA = KC + 4;
constexpr int GWC = 128;                                // grad_w: columns of D staged at a time
constexpr int MAX_D = 64 * MAX_EPL;
constexpr size_t LDS_LIMIT = 160 * 1024;                // a gfx950 workgroup's LDS
constexpr double GAMMA_EPS = 1e-15;                     // math_.py:383
using RW = RowD<64, MAX_EPL>;                           // a row per wave

// a row of fp32 or fp64 storage to and from the registers of a wave
template <class T>
__device__ __forceinline__ RW load_row(const T* __restrict__ p, int D, int lane) {
  RW r;
#pragma unroll
  for (int e = 0; e < RW::EPL; ++e) { const int c = lane + 64 * e; r.v[e] = c < D ? (double)p[c] : 0.0; }
  return r;
}
template <class T>
__device__ __forceinline__ void store_row(T* __restrict__ p, const RW& r, int D, int lane) {
#pragma unroll
  for (int e = 0; e < RW::EPL; ++e) { const int c = lane + 64 * e; if (c < D) p[c] = (T)r.v[e]; }
}

inline int nt_of(int D) { return D <= 64 ? 4 : D <= 128 ? 8 : 16; }
inline size_t prod_lds(int D) { return (size_t)(KC * (nt_of(D) * 16 + 4) + MT * LDA + KC) * sizeof(float) + 2 * MT * sizeof(double); }
__host__ __device__ inline int gw_ld(int D) { const int d4 = (D + 3) & ~3; return (d4 < GWC ? d4 : GWC) + 4; }
inline size_t gw_lds(int D) { return (size_t)(2 * MT * gw_ld(D) + 2 * MT) * sizeof(float); }

// out rows x contraction positions of one batch element.  GRADX = false, the forward: a(i, j) = W[i][j], the chunk rows are
// gamma_j x_j formed from X (M, D), the side vector is c_j.  GRADX = true: a(j, i) = W[i][j], the chunk rows are g_s_i (N, D), the
// side vector is g_d_i, and the epilogue closes grad_x.  `rows` = output rows, `K` = contraction length, wld = M.
// CV... here and below: the launch's curvature -- nothing at k = -1, one Curv at k = -c (rowops.h), where gamma_j = 2 / max(1 - c |x_j|^2,
// 1e-15), d gamma / d x = c gamma^2 x, and the tail halves by 1 + sqrt(1 - c |t|^2) and projects onto (1 - 4e-3) / sqrt(c).
template <int NT, bool GRADX, class... CV>
__global__ __launch_bounds__(THREADS) void mid_product_kernel(const float* __restrict__ W, const float* __restrict__ B, const float* __restrict__ side,
                                                               const float* __restrict__ X, float* __restrict__ out, float* __restrict__ saved,
                                                               int rows, int K, int wld, int D, int tiles, int lincomb, CV... cv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDB = NT * 16 + 4;
  float* bs = smem;                                     // [KC][LDB]
  float* as = bs + KC * LDB;                            // [MT][LDA]
  float* sv = as + MT * LDA;                            // [KC]
  double* dn = (double*)(sv + KC);                      // [MT] den (h in GRADX), then [MT] alpha
  double* al = dn + MT;
  using R = RowD<16, NT>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / tiles, r0 = (blockIdx.x % tiles) * MT;
  const size_t nN = GRADX ? (size_t)K : (size_t)rows, nM = (size_t)wld;
  W += (size_t)b * nN * nM;
  B += (size_t)b * (size_t)K * D;
  if (GRADX) { side += (size_t)b * K; X += (size_t)b * (size_t)rows * D; }
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  double den = 0.0, alpha = 0.0;
  for (int k0 = 0; k0 < K; k0 += KC) {
    const int kw = K - k0 < KC ? K - k0 : KC, kw4 = (kw + 3) & ~3;
    __syncthreads();                                    // the readers of the previous chunk are done
    for (int r = wave; r < KC; r += WAVES)
      for (int c = lane; c < NT * 16; c += 64) bs[r * LDB + c] = (r < kw && c < D) ? B[(size_t)(k0 + r) * D + c] : 0.f;
    if (GRADX) {
      for (int c = wave; c < KC; c += WAVES)            // as[out row j][position i] = W[i][j]: lanes along j
        as[lane * LDA + c] = (c < kw && r0 + lane < rows) ? W[(size_t)(k0 + c) * nM + r0 + lane] : 0.f;
      if (tid < KC) sv[tid] = tid < kw ? side[k0 + tid] : 0.f;
    } else {
      for (int r = wave; r < MT; r += WAVES) as[r * LDA + lane] = (lane < kw && r0 + r < rows) ? W[(size_t)(r0 + r) * nM + k0 + lane] : 0.f;
    }
    __syncthreads();
    if constexpr (!GRADX) {                             // four threads a point: 1 - |x|^2 in fp64, the row scaled to gamma x
      float* p = bs + (tid >> 2) * LDB;
      double s = 0.0;
      for (int c = tid & 3; c < D; c += 4) { const double v = p[c]; s += v * v; }
      s += __shfl_xor(s, 1, WAVE);
      s += __shfl_xor(s, 2, WAVE);
      const double g = 2.0 / fmax(1.0 - curv_mul(s, cv...), GAMMA_EPS);
      for (int c = tid & 3; c < D; c += 4) p[c] = (float)(g * (double)p[c]);
      if ((tid & 3) == 0) sv[tid >> 2] = (float)(g - 1.0);
      __syncthreads();
    }
    for (int kk = 0; kk < kw4; kk += 4) {
      const float a = as[(wave * 16 + j) * LDA + kk + q];
      const float* bp = bs + (kk + q) * LDB + j;
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[t * 16], acc[t], 0, 0, 0);
    }
    for (int kk = q; kk < kw; kk += 4) {                // row wave * 16 + j, the positions kk = q mod 4
      const double w = fabsf(as[(wave * 16 + j) * LDA + kk]);
      den += w * (double)sv[kk];
      if constexpr (!GRADX) alpha += w;
    }
  }
  den += __shfl_xor(den, 16, WAVE);
  den += __shfl_xor(den, 32, WAVE);
  if constexpr (!GRADX) {
    alpha += __shfl_xor(alpha, 16, WAVE);
    alpha += __shfl_xor(alpha, 32, WAVE);
  }
  if (q == 0) { dn[wave * 16 + j] = den; al[wave * 16 + j] = alpha; }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lr = wave * 16 + 4 * q + r, gr = r0 + lr;
    const bool rv = gr < rows;
    R v;
#pragma unroll
    for (int t = 0; t < NT; ++t) v.v[t] = (double)acc[t][r];
    if constexpr (GRADX) {
      const float* xr = X + (size_t)(rv ? gr : 0) * D;
      R x;
#pragma unroll
      for (int t = 0; t < NT; ++t) x.v[t] = (rv && t * 16 + j < D) ? (double)xr[t * 16 + j] : 0.0;
      const double om = 1.0 - curv_mul(rowd_dot(x, x), cv...);
      const double g = 2.0 / fmax(om, GAMMA_EPS);
      const double s = om >= GAMMA_EPS ? curv_mul(g * g * (rowd_dot(v, x) + dn[lr]), cv...) : 0.0;
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (rv && t * 16 + j < D) out[((size_t)b * rows + gr) * D + t * 16 + j] = (float)(g * v.v[t] + s * x.v[t]);
    } else {
      const float denf = (float)dn[lr], alf = (float)al[lr];
      if (saved && rv) {
        float* sp = saved + ((size_t)b * rows + gr) * (D + 2);
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (t * 16 + j < D) sp[t * 16 + j] = acc[t][r];
        if (j == 0) { sp[D] = denf; sp[D + 1] = alf; }
      }
      const R o = midpoint_tail_d(v, (double)denf, (double)alf, MidpointCfg{true, lincomb != 0, true, false}, cv...);
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (rv && t * 16 + j < D) out[((size_t)b * rows + gr) * D + t * 16 + j] = (float)o.v[t];
    }
  }
}

// The row pass of both backwards: a wave per output row, from saved = [nom | den | alpha] and grad_out to g_nom = g_s (rows, D), g_d and
// g_alpha.  The scalar of lincomb is r = rscale alpha (1 in the bmm form, 1/2 in the reduce form).  T: fp32 in the bmm form, whose
// sums are fp32 MFMA products; fp64 in the reduce form, whose sums are fp64 and where grad_w = gamma <g_nom, x> + (gamma - 1) g_d is
// the difference of two terms 1 / sqrt(1 - |t|^2) times its size when one point carries the row (a single point: exactly zero).
template <class T, class... CV>
__global__ __launch_bounds__(THREADS) void mid_rows_bwd(const T* __restrict__ saved, const float* __restrict__ go, T* __restrict__ gs,
                                                         T* __restrict__ gd, T* __restrict__ ga, int64_t rows, int D, MidpointCfg cfg,
                                                         float rscale, CV... cv) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    const T* sp = saved + r * (D + 2);
    RW gnom;
    double gden, gr;
    midpoint_tail_bwd_d(load_row(sp, D, lane), (double)sp[D], (double)rscale * (double)sp[D + 1], cfg, load_row(go + r * D, D, lane), gnom, gden, gr,
                        cv...);
    store_row(gs + r * D, gnom, D, lane);
    if (lane == 0) { gd[r] = (T)gden; ga[r] = (T)((double)rscale * gr); }
  }
}

// grad_w (N, M) of one batch element, a 64 x 64 tile per workgroup: gamma_j <g_s_i, x_j> + sign(w_ij) (g_d_i c_j + g_alpha_i).
template <class... CV>
__global__ __launch_bounds__(THREADS) void mid_gradw_kernel(const float* __restrict__ W, const float* __restrict__ X, const float* __restrict__ gs,
                                                             const float* __restrict__ gd, const float* __restrict__ ga, float* __restrict__ gw,
                                                             int N, int M, int D, int tn, int tm, int lincomb, CV... cv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ld = gw_ld(D);
  float* gt = smem;                                     // [64][ld] g_s rows
  float* xt = gt + MT * ld;                             // [64][ld] points
  float* gam = xt + MT * ld;                            // [64] gamma_j
  float* cj = gam + MT;                                 // [64] c_j
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / (tn * tm), tile = blockIdx.x % (tn * tm);
  const int i0 = (tile / tm) * MT, j0 = (tile % tm) * MT;
  W += (size_t)b * N * M;
  gw += (size_t)b * N * M;
  X += (size_t)b * M * D;
  gs += (size_t)b * N * D;
  gd += (size_t)b * N;
  ga += (size_t)b * N;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  double x2 = 0.0;                                      // four threads a point, the columns c = tid mod 4
  for (int d0 = 0; d0 < D; d0 += GWC) {
    const int dw = D - d0 < GWC ? D - d0 : GWC, dw4 = (dw + 3) & ~3;
    __syncthreads();
    for (int r = wave; r < MT; r += WAVES)
      for (int c = lane; c < dw4; c += 64) {
        gt[r * ld + c] = (c < dw && i0 + r < N) ? gs[(size_t)(i0 + r) * D + d0 + c] : 0.f;
        xt[r * ld + c] = (c < dw && j0 + r < M) ? X[(size_t)(j0 + r) * D + d0 + c] : 0.f;
      }
    __syncthreads();
    {
      const float* p = xt + (tid >> 2) * ld;
      for (int c = tid & 3; c < dw; c += 4) { const double v = p[c]; x2 += v * v; }
    }
    for (int kk = 0; kk < dw4; kk += 4) {
      const float a = gt[(wave * 16 + j) * ld + kk + q];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xt[(t * 16 + j) * ld + kk + q], acc[t], 0, 0, 0);
    }
  }
  x2 += __shfl_xor(x2, 1, WAVE);
  x2 += __shfl_xor(x2, 2, WAVE);
  if ((tid & 3) == 0) {
    const double g = 2.0 / fmax(1.0 - curv_mul(x2, cv...), GAMMA_EPS);
    gam[tid >> 2] = (float)g;
    cj[tid >> 2] = (float)(g - 1.0);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gi = i0 + wave * 16 + 4 * q + r;
    if (gi >= N) continue;
    const float d = gd[gi], a = lincomb ? ga[gi] : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int lc = t * 16 + j, gj = j0 + lc;
      if (gj >= M) continue;
      const float w = W[(size_t)gi * M + gj];
      const float sg = w > 0.f ? 1.f : w < 0.f ? -1.f : 0.f;
      gw[(size_t)gi * M + gj] = gam[lc] * acc[t][r] + sg * (d * cj[lc] + a);
    }
  }
}

// mobius_scalar_mul on its own: a wave per row; r of one value (rbc) or one per row
__global__ __launch_bounds__(THREADS) void scalar_mul_rows(const float* __restrict__ rr, const float* __restrict__ x, float* __restrict__ out,
                                                           int64_t rows, int dim, int rbc) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dim, mobius_scalar_mul_d((double)rr[rbc ? 0 : r], rowd_load<RW>(x + r * dim, dim, lane)), dim, lane);
}
__global__ __launch_bounds__(THREADS) void scalar_mul_rows_bwd(const float* __restrict__ rr, const float* __restrict__ x, const float* __restrict__ go,
                                                               float* __restrict__ gr, float* __restrict__ gx, int64_t rows, int dim, int rbc) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW dx;
    const double g = mobius_scalar_mul_bwd_d((double)rr[rbc ? 0 : r], rowd_load<RW>(x + r * dim, dim, lane), rowd_load<RW>(go + r * dim, dim, lane), dx);
    if (gx) rowd_store(gx + r * dim, dx, dim, lane);
    if (gr && lane == 0) gr[r] = (float)g;
  }
}

// ---- the reduce form (math_.py:2027-2087): xs (M, R, D) -- M reduced positions of R kept rows -- and weights (M, R), one value, or none.
//   nom = sum_m gamma_m w_m x_m    den = sum_m (gamma_m - 1) |w_m|    alpha = sum_m w_m  (|w_m| with posweight)
//   t = nom / (den + 1e-10)    a = t / (1 + sqrt(1 - |t|^2)), or t with lincomb / coadd    [lincomb: a = (alpha / 2) (x) a]    no project
// posweight moves a negative weight's point to its antipode -x and takes |w|: |w| (-x) = w x, so only alpha changes.
enum { W_NONE = 0, W_SCALAR = 1, W_ELEMENTS = 2 };
__device__ __forceinline__ float red_weight(const float* __restrict__ w, int wkind, int64_t idx) {
  return wkind == W_NONE ? 1.f : w[wkind == W_SCALAR ? 0 : idx];
}
__device__ __forceinline__ MidpointCfg red_cfg(int flags) {
  return MidpointCfg{!(flags & (HYPAD_MID_LINCOMB | HYPAD_MID_COADD)), (flags & HYPAD_MID_LINCOMB) != 0, false, true};
}
// the fp64 sums of a kept row to `saved` and to the row of out
template <class... CV>
__device__ __forceinline__ void red_finish(const RW& nom, double den, double alpha, float* __restrict__ out, double* __restrict__ saved, int64_t rho,
                                           int D, int flags, int lane, CV... cv) {
  if (saved) {
    double* sp = saved + rho * (D + 2);
    store_row(sp, nom, D, lane);
    if (lane == 0) { sp[D] = den; sp[D + 1] = alpha; }
  }
  store_row(out + rho * D, midpoint_tail_d(nom, den, 0.5 * alpha, red_cfg(flags), cv...), D, lane);
}
// A wave per (kept row, slice of the positions): the three sums in fp64 registers.  One slice: the row is finished here; more: the
// partial sums go to part (slices, R, D + 2) and mid_reduce_finish adds them in slice order.
template <class... CV>
__global__ __launch_bounds__(THREADS) void mid_reduce_kernel(const float* __restrict__ xs, const float* __restrict__ w, int wkind,
                                                              double* __restrict__ part, float* __restrict__ out, double* __restrict__ saved, int64_t M,
                                                              int64_t R, int D, int slices, int64_t slice_len, int flags, CV... cv) {
  const int lane = threadIdx.x & 63;
  const bool pos = (flags & HYPAD_MID_POSWEIGHT) != 0;
  for (int64_t task = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); task < R * slices; task += (int64_t)gridDim.x * WAVES) {
    const int64_t rho = task % R, sl = task / R;
    const int64_t m0 = sl * slice_len, m1 = m0 + slice_len < M ? m0 + slice_len : M;
    RW nom;
#pragma unroll
    for (int e = 0; e < RW::EPL; ++e) nom.v[e] = 0.0;
    double den = 0.0, alpha = 0.0;
    for (int64_t m = m0; m < m1; ++m) {
      const int64_t idx = m * R + rho;
      const RW x = rowd_load<RW>(xs + idx * D, D, lane);
      const double wv = red_weight(w, wkind, idx);
      const double g = 2.0 / fmax(1.0 - curv_mul(rowd_dot(x, x), cv...), GAMMA_EPS);
#pragma unroll
      for (int e = 0; e < RW::EPL; ++e) nom.v[e] += g * wv * x.v[e];
      den += (g - 1.0) * fabs(wv);
      alpha += pos ? fabs(wv) : wv;
    }
    if (slices == 1) {
      red_finish(nom, den, alpha, out, saved, rho, D, flags, lane, cv...);
    } else {
      double* p = part + (sl * R + rho) * (D + 2);
#pragma unroll
      for (int e = 0; e < RW::EPL; ++e) { const int c = lane + 64 * e; if (c < D) p[c] = nom.v[e]; }
      if (lane == 0) { p[D] = den; p[D + 1] = alpha; }
    }
  }
}
template <class... CV>
__global__ __launch_bounds__(THREADS) void mid_reduce_finish(const double* __restrict__ part, float* __restrict__ out, double* __restrict__ saved,
                                                              int64_t R, int D, int slices, int flags, CV... cv) {
  const int lane = threadIdx.x & 63;
  for (int64_t rho = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); rho < R; rho += (int64_t)gridDim.x * WAVES) {
    RW nom;
#pragma unroll
    for (int e = 0; e < RW::EPL; ++e) nom.v[e] = 0.0;
    double den = 0.0, alpha = 0.0;
    for (int sl = 0; sl < slices; ++sl) {
      const double* p = part + ((int64_t)sl * R + rho) * (D + 2);
#pragma unroll
      for (int e = 0; e < RW::EPL; ++e) { const int c = lane + 64 * e; nom.v[e] += c < D ? p[c] : 0.0; }
      den += p[D];
      alpha += p[D + 1];
    }
    red_finish(nom, den, alpha, out, saved, rho, D, flags, lane, cv...);
  }
}
// The element-wise pass of the backward, a wave per (position, kept row):
//   grad_x = gamma w g_nom + gamma^2 (w <g_nom, x> + |w| g_d) x        (the second term 0 where gamma is clamped)
//   grad_w = gamma <g_nom, x> + sign(w) (gamma - 1) g_d + g_alpha      (g_alpha times -1 for a negative weight with posweight)
// gw (M, R): the weights' gradient, or the summands of a single weight's.
template <class... CV>
__global__ __launch_bounds__(THREADS) void mid_reduce_elem_bwd(const float* __restrict__ xs, const float* __restrict__ w, int wkind,
                                                                const double* __restrict__ gnom, const double* __restrict__ gd,
                                                                const double* __restrict__ ga, float* __restrict__ gx, float* __restrict__ gw,
                                                                int64_t MR, int64_t R, int D, int flags, CV... cv) {
  const int lane = threadIdx.x & 63;
  const bool pos = (flags & HYPAD_MID_POSWEIGHT) != 0;
  for (int64_t idx = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); idx < MR; idx += (int64_t)gridDim.x * WAVES) {
    const int64_t rho = idx % R;
    const RW x = load_row(xs + idx * D, D, lane), gn = load_row(gnom + rho * D, D, lane);
    const double wv = red_weight(w, wkind, idx), gdv = gd[rho], gav = ga[rho];
    const double om = 1.0 - curv_mul(rowd_dot(x, x), cv...), g = 2.0 / fmax(om, GAMMA_EPS), gnx = rowd_dot(gn, x);
    if (gx) {
      const double s = om >= GAMMA_EPS ? curv_mul(g * g * (wv * gnx + fabs(wv) * gdv), cv...) : 0.0;
      RW o;
#pragma unroll
      for (int e = 0; e < RW::EPL; ++e) o.v[e] = g * wv * gn.v[e] + s * x.v[e];
      rowd_store(gx + idx * D, o, D, lane);
    }
    if (gw && lane == 0) {
      const double sg = wv > 0.0 ? 1.0 : wv < 0.0 ? -1.0 : 0.0;
      gw[idx] = (float)(g * gnx + sg * (g - 1.0) * gdv + (pos && wv < 0.0 ? -gav : gav));
    }
  }
}
// out[0] = the sum of n floats: one workgroup, every thread a fixed stride of the summands in fp64, then a fixed tree
__global__ __launch_bounds__(THREADS) void fixed_sum_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n) {
  __shared__ double sh[THREADS];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += THREADS) s += (double)in[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)sh[0];
}

inline int wave_grid(int64_t rows) {
  const int64_t b = (rows + WAVES - 1) / WAVES;
  return (int)(b > 4096 ? 4096 : b < 1 ? 1 : b);
}
inline int zero_floats(float* p, size_t n, hipStream_t s) {
  if (!p || n == 0) return HYPAD_OK;
  const hipError_t e = hipMemsetAsync(p, 0, n * sizeof(float), s);
  return e == hipSuccess ? HYPAD_OK : (int)e;
}
inline int smul_check(const float* r, const float* x, const void* o, int64_t rows, int dim, int64_t r_rows) {
  if (!r || !x || !o || rows < 0 || dim <= 0 || (r_rows != 1 && r_rows != rows)) return HYPAD_EINVAL;
  return dim > MAX_D ? HYPAD_EUNSUPPORTED : HYPAD_OK;
}

struct BmmWorkspace { size_t gs, gd, ga, total; };      // offsets in floats
inline BmmWorkspace bmm_workspace(int64_t batch, int64_t N, int D) {
  BmmWorkspace w;
  const size_t rows = (size_t)batch * (size_t)N;
  w.gs = 0;                                             // g_s (batch N, D)
  w.gd = w.gs + rows * D;                               // g_d (batch N)
  w.ga = w.gd + rows;                                   // g_alpha (batch N)
  w.total = w.ga + rows;
  return w;
}
constexpr int64_t INT_LIMIT = 0x7fffffff;
inline int bmm_check(const float* xs, const float* w, int64_t batch, int64_t N, int64_t M, int D, int flags) {
  if (!xs || (!w && N > 0) || batch <= 0 || N < 0 || M <= 0 || D <= 0) return HYPAD_EINVAL;      // (no output rows: weights is empty)
  if (flags & ~HYPAD_MID_LINCOMB) return HYPAD_EINVAL;
  if (D > MAX_D) return HYPAD_EUNSUPPORTED;
  if (batch > INT_LIMIT || N > INT_LIMIT || M > INT_LIMIT) return HYPAD_EUNSUPPORTED;
  // every element count and every grid below 2^31
  const int64_t tn = (N + MT - 1) / MT, tm = (M + MT - 1) / MT;
  if (N * M > INT_LIMIT / batch || M * D > INT_LIMIT / batch || (N > 0 && N * (int64_t)(D + 2) > INT_LIMIT / batch)) return HYPAD_EUNSUPPORTED;
  if (tn * tm > INT_LIMIT / batch) return HYPAD_EUNSUPPORTED;
  if (prod_lds(D) > LDS_LIMIT || gw_lds(D) > LDS_LIMIT) return HYPAD_EUNSUPPORTED;
  return HYPAD_OK;
}

// The slices of the reduce form -- a function of the shapes alone: about 1 024 waves where the kept rows alone give fewer, no slice
// below 16 positions, at most 256 slices.  Workspace: the partial sums (doubles), then g_nom (R, D), g_d, g_alpha (R), the summands of a
// single weight's gradient (M, R).  Offsets: part, gnom, gd, ga in doubles from the start; gw in floats after the `doubles` doubles.
struct RedPlan { int slices; int64_t slice_len; size_t gnom, gd, ga, doubles, floats; };
inline RedPlan red_plan(int64_t M, int64_t R, int D) {
  RedPlan p;
  int64_t want = R > 0 ? 1024 / R : 1;
  const int64_t most = (M + 15) / 16;
  want = want > most ? most : want;
  want = want > 256 ? 256 : want < 1 ? 1 : want;
  p.slice_len = (M + want - 1) / want;
  p.slices = (int)((M + p.slice_len - 1) / p.slice_len);
  p.gnom = p.slices > 1 ? (size_t)p.slices * (size_t)R * (D + 2) : 0;     // (the partial sums of the forward come first)
  p.gd = p.gnom + (size_t)R * D;
  p.ga = p.gd + (size_t)R;
  p.doubles = p.ga + (size_t)R;
  p.floats = (size_t)M * (size_t)R;
  return p;
}
inline size_t red_bytes(const RedPlan& p) { return p.doubles * sizeof(double) + p.floats * sizeof(float); }
inline int red_check(const float* xs, const float* w, int64_t w_count, int64_t M, int64_t R, int D, int flags) {
  if ((!xs && R > 0) || M <= 0 || R < 0 || D <= 0) return HYPAD_EINVAL;                             // (no kept rows: xs is empty)
  if (flags & ~(HYPAD_MID_POSWEIGHT | HYPAD_MID_LINCOMB | HYPAD_MID_COADD)) return HYPAD_EINVAL;
  if (w ? (w_count != 1 && w_count != M * R) : w_count != 0) return HYPAD_EINVAL;
  if (D > MAX_D) return HYPAD_EUNSUPPORTED;
  if (M > INT_LIMIT || R > INT_LIMIT || (R > 0 && M * (int64_t)(D + 2) > INT_LIMIT / R)) return HYPAD_EUNSUPPORTED;
  return HYPAD_OK;
}
inline int red_wkind(const float* w, int64_t w_count, int64_t MR) { return !w ? W_NONE : (w_count == 1 && MR != 1) ? W_SCALAR : W_ELEMENTS; }

template <bool GRADX, class... CV>
int launch_product(const float* W, const float* B, const float* side, const float* X, float* out, float* saved, int64_t batch, int rows, int K, int wld,
                   int D, int lincomb, hipStream_t st, CV... cv) {
  const size_t lds = prod_lds(D);
  const int tiles = (rows + MT - 1) / MT;
  const dim3 grid((unsigned)(batch * tiles));
#define HYPAD_MID_LAUNCH(NT)                                                                                                              \
  do {                                                                                                                                     \
    const hipError_t e = allow_lds((const void*)mid_product_kernel<NT, GRADX, CV...>, lds);                                                \
    if (e != hipSuccess) return (int)e;                                                                                                    \
    hipLaunchKernelGGL((mid_product_kernel<NT, GRADX, CV...>), grid, dim3(THREADS), lds, st, W, B, side, X, out, saved, rows, K, wld, D, tiles, lincomb, \
                       cv...);                                                                                                             \
  } while (0)
  if (D <= 64) HYPAD_MID_LAUNCH(4);
  else if (D <= 128) HYPAD_MID_LAUNCH(8);
  else HYPAD_MID_LAUNCH(16);
#undef HYPAD_MID_LAUNCH
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

// the bodies of the bmm and the reduce entry points, at k = -1 (no cv) and at k = -c
template <class... CV>
int bmm_fwd(const float* xs, const float* weights, float* out, float* saved, int64_t batch, int64_t N, int64_t M, int D, int flags, hypad_stream_t s,
            CV... cv) {
  const int rc = bmm_check(xs, weights, batch, N, M, D, flags);
  if (rc || N == 0) return rc;
  if (!out) return HYPAD_EINVAL;
  return launch_product<false>(weights, xs, nullptr, nullptr, out, saved, batch, (int)N, (int)M, (int)M, D, flags & HYPAD_MID_LINCOMB, (hipStream_t)s,
                               cv...);
}

template <class... CV>
int bmm_bwd(const float* xs, const float* weights, const float* saved, const float* grad_out, float* grad_xs, float* grad_weights, void* workspace,
            size_t workspace_bytes, int64_t batch, int64_t N, int64_t M, int D, int flags, hypad_stream_t s, CV... cv) {
  const int rc = bmm_check(xs, weights, batch, N, M, D, flags);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)s;
  if (N == 0) return zero_floats(grad_xs, (size_t)batch * M * D, st);      // a sum over no output rows
  if (!saved || !grad_out) return HYPAD_EINVAL;
  if (!grad_xs && !grad_weights) return HYPAD_OK;
  const BmmWorkspace w = bmm_workspace(batch, N, D);
  if (!workspace || workspace_bytes < w.total * sizeof(float)) return HYPAD_EWORKSPACE;
  float* ws = (float*)workspace;
  const int lincomb = flags & HYPAD_MID_LINCOMB;
  hipLaunchKernelGGL((mid_rows_bwd<float, CV...>), dim3(wave_grid(batch * N)), dim3(THREADS), 0, st, saved, grad_out, ws + w.gs, ws + w.gd, ws + w.ga,
                     batch * N, D, MidpointCfg{true, lincomb != 0, true, false}, 1.f, cv...);
  HYPAD_CHECK_LAUNCH();
  if (grad_weights) {
    const int tn = (int)((N + MT - 1) / MT), tm = (int)((M + MT - 1) / MT);
    const size_t lds = gw_lds(D);
    const hipError_t e = allow_lds((const void*)mid_gradw_kernel<CV...>, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mid_gradw_kernel<CV...>, dim3((unsigned)(batch * tn * tm)), dim3(THREADS), lds, st, weights, xs, ws + w.gs, ws + w.gd, ws + w.ga,
                       grad_weights, (int)N, (int)M, D, tn, tm, lincomb, cv...);
    HYPAD_CHECK_LAUNCH();
  }
  if (grad_xs)
    return launch_product<true>(weights, ws + w.gs, ws + w.gd, xs, grad_xs, nullptr, batch, (int)M, (int)N, (int)M, D, lincomb, st, cv...);
  return HYPAD_OK;
}

template <class... CV>
int red_fwd(const float* xs, const float* weights, int64_t w_count, float* out, double* saved, void* workspace, size_t workspace_bytes, int64_t M,
            int64_t R, int D, int flags, hypad_stream_t s, CV... cv) {
  const int rc = red_check(xs, weights, w_count, M, R, D, flags);
  if (rc || R == 0) return rc;
  if (!out || ((uintptr_t)saved & 7)) return HYPAD_EINVAL;
  const RedPlan p = red_plan(M, R, D);
  if (p.slices > 1 && (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < red_bytes(p))) return HYPAD_EWORKSPACE;
  hipStream_t st = (hipStream_t)s;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(mid_reduce_kernel<CV...>, dim3(wave_grid(R * p.slices)), dim3(THREADS), 0, st, xs, weights, red_wkind(weights, w_count, M * R), part,
                     out, saved, M, R, D, p.slices, p.slice_len, flags, cv...);
  HYPAD_CHECK_LAUNCH();
  if (p.slices > 1) {
    hipLaunchKernelGGL(mid_reduce_finish<CV...>, dim3(wave_grid(R)), dim3(THREADS), 0, st, (const double*)part, out, saved, R, D, p.slices, flags, cv...);
    HYPAD_CHECK_LAUNCH();
  }
  return HYPAD_OK;
}

template <class... CV>
int red_bwd(const float* xs, const float* weights, int64_t w_count, const double* saved, const float* grad_out, float* grad_xs, float* grad_weights,
            void* workspace, size_t workspace_bytes, int64_t M, int64_t R, int D, int flags, hypad_stream_t s, CV... cv) {
  const int rc = red_check(xs, weights, w_count, M, R, D, flags);
  if (rc) return rc;
  if (grad_weights && !weights) return HYPAD_EINVAL;
  hipStream_t st = (hipStream_t)s;
  const int wkind = red_wkind(weights, w_count, M * R);
  if (R == 0) return wkind == W_SCALAR || w_count == 1 ? zero_floats(grad_weights, 1, st) : HYPAD_OK;   // a sum over no rows
  if (!saved || ((uintptr_t)saved & 7) || !grad_out) return HYPAD_EINVAL;
  if (!grad_xs && !grad_weights) return HYPAD_OK;
  const RedPlan p = red_plan(M, R, D);
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < red_bytes(p)) return HYPAD_EWORKSPACE;
  double* wd = (double*)workspace;
  float* wf = (float*)(wd + p.doubles);
  hipLaunchKernelGGL((mid_rows_bwd<double, CV...>), dim3(wave_grid(R)), dim3(THREADS), 0, st, saved, grad_out, wd + p.gnom, wd + p.gd, wd + p.ga, R, D,
                     MidpointCfg{!(flags & (HYPAD_MID_LINCOMB | HYPAD_MID_COADD)), (flags & HYPAD_MID_LINCOMB) != 0, false, true}, 0.5f, cv...);
  HYPAD_CHECK_LAUNCH();
  float* gw = !grad_weights ? nullptr : wkind == W_SCALAR ? wf : grad_weights;
  hipLaunchKernelGGL(mid_reduce_elem_bwd<CV...>, dim3(wave_grid(M * R)), dim3(THREADS), 0, st, xs, weights, wkind, (const double*)(wd + p.gnom),
                     (const double*)(wd + p.gd), (const double*)(wd + p.ga), grad_xs, gw, M * R, R, D, flags, cv...);
  HYPAD_CHECK_LAUNCH();
  if (grad_weights && wkind == W_SCALAR) {
    hipLaunchKernelGGL(fixed_sum_kernel, dim3(1), dim3(THREADS), 0, st, (const float*)wf, grad_weights, M * R);
    HYPAD_CHECK_LAUNCH();
  }
  return HYPAD_OK;
}

}  // namespace

extern "C" {

int hypad_mobius_scalar_mul_fwd(const float* r, const float* x, float* out, int64_t rows, int dim, int64_t r_rows, hypad_stream_t s) {
  const int rc = smul_check(r, x, out, rows, dim, r_rows);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(scalar_mul_rows, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, r, x, out, rows, dim, (int)(r_rows == 1 && rows != 1));
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_mobius_scalar_mul_bwd(const float* r, const float* x, const float* go, float* gr, float* gx, int64_t rows, int dim, int64_t r_rows,
                                hypad_stream_t s) {
  const int rc = smul_check(r, x, go, rows, dim, r_rows);
  if (rc || rows == 0 || (!gr && !gx)) return rc;
  hipLaunchKernelGGL(scalar_mul_rows_bwd, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, r, x, go, gr, gx, rows, dim,
                     (int)(r_rows == 1 && rows != 1));
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

size_t hypad_weighted_midpoint_bmm_workspace_bytes(int64_t batch, int64_t N, int64_t M, int D) {
  if (batch <= 0 || N <= 0 || M <= 0 || D <= 0) return 0;
  return bmm_workspace(batch, N, D).total * sizeof(float);
}

int hypad_weighted_midpoint_bmm_fwd(const float* xs, const float* weights, float* out, float* saved, int64_t batch, int64_t N, int64_t M, int D,
                                    int flags, hypad_stream_t s) {
  return bmm_fwd(xs, weights, out, saved, batch, N, M, D, flags, s);
}
int hypad_weighted_midpoint_bmm_bwd(const float* xs, const float* weights, const float* saved, const float* grad_out, float* grad_xs,
                                    float* grad_weights, void* workspace, size_t workspace_bytes, int64_t batch, int64_t N, int64_t M, int D,
                                    int flags, hypad_stream_t s) {
  return bmm_bwd(xs, weights, saved, grad_out, grad_xs, grad_weights, workspace, workspace_bytes, batch, N, M, D, flags, s);
}

size_t hypad_weighted_midpoint_workspace_bytes(int64_t M, int64_t R, int D) {
  if (M <= 0 || R <= 0 || D <= 0) return 0;
  return red_bytes(red_plan(M, R, D));
}

int hypad_weighted_midpoint_fwd(const float* xs, const float* weights, int64_t w_count, float* out, double* saved, void* workspace,
                                size_t workspace_bytes, int64_t M, int64_t R, int D, int flags, hypad_stream_t s) {
  return red_fwd(xs, weights, w_count, out, saved, workspace, workspace_bytes, M, R, D, flags, s);
}
int hypad_weighted_midpoint_bwd(const float* xs, const float* weights, int64_t w_count, const double* saved, const float* grad_out, float* grad_xs,
                                float* grad_weights, void* workspace, size_t workspace_bytes, int64_t M, int64_t R, int D, int flags,
                                hypad_stream_t s) {
  return red_bwd(xs, weights, w_count, saved, grad_out, grad_xs, grad_weights, workspace, workspace_bytes, M, R, D, flags, s);
}

// the same at k = -c: c is checked first, then everything as above; the *_workspace_bytes functions serve both
int hypad_ball_weighted_midpoint_bmm_fwd(const float* xs, const float* weights, float* out, float* saved, int64_t batch, int64_t N, int64_t M, int D,
                                         int flags, double c, hypad_stream_t s) {
  return curv_invalid(c) ? HYPAD_EINVAL : bmm_fwd(xs, weights, out, saved, batch, N, M, D, flags, s, curv_of(c));
}
int hypad_ball_weighted_midpoint_bmm_bwd(const float* xs, const float* weights, const float* saved, const float* grad_out, float* grad_xs,
                                         float* grad_weights, void* workspace, size_t workspace_bytes, int64_t batch, int64_t N, int64_t M, int D,
                                         int flags, double c, hypad_stream_t s) {
  return curv_invalid(c) ? HYPAD_EINVAL
                  : bmm_bwd(xs, weights, saved, grad_out, grad_xs, grad_weights, workspace, workspace_bytes, batch, N, M, D, flags, s, curv_of(c));
}
int hypad_ball_weighted_midpoint_fwd(const float* xs, const float* weights, int64_t w_count, float* out, double* saved, void* workspace,
                                     size_t workspace_bytes, int64_t M, int64_t R, int D, int flags, double c, hypad_stream_t s) {
  return curv_invalid(c) ? HYPAD_EINVAL : red_fwd(xs, weights, w_count, out, saved, workspace, workspace_bytes, M, R, D, flags, s, curv_of(c));
}
int hypad_ball_weighted_midpoint_bwd(const float* xs, const float* weights, int64_t w_count, const double* saved, const float* grad_out,
                                     float* grad_xs, float* grad_weights, void* workspace, size_t workspace_bytes, int64_t M, int64_t R, int D,
                                     int flags, double c, hypad_stream_t s) {
  return curv_invalid(c) ? HYPAD_EINVAL
                  : red_bwd(xs, weights, w_count, saved, grad_out, grad_xs, grad_weights, workspace, workspace_bytes, M, R, D, flags, s, curv_of(c));
}

}  // extern "C"
