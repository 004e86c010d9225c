// dist2plane_matmul (math_.py:2125-2159) at k = -1: the reference's batched hyperplane read-out in the operand layout of dist_matmul.
// x (batch, N, D) on the ball, the points p and the normals z of the planes (batch, M, D) -- the reference's (batch, D, M) transposed by
// the caller --, out and grad_out (batch, N, M).  It is NOT 2 dist2plane(signed, scaled) of the transposed operands (dist2plane.hip):
//
//   zn_j = |z_j|   zh_j = z_j / max(zn_j, 1e-15)   x2_i = |x_i|^2   p2_j = |p_j|^2   bx_i = max(1 - x2_i, 1e-15)   bp_j = max(1 - p2_j, 1e-15)
//   xp = <x_i, p_j>   xz = <x_i, zh_j>   pz_j = <p_j, zh_j>   alpha = 1 - 2 xp + x2_i
//   t = (2 / bp_j) (xz - (alpha / bx_i) pz_j)        out_ij = 2 asinh(t) zn_j
//
// Forward: ONE launch, a workgroup of four waves per (batch element, 64 x 64 tile of out).  D is staged in chunks of 128 columns; each
// wave multiplies its 16 rows of x with the 64 rows of p and of z on fp32 MFMA from one staged x tile; x2, p2, |z|^2 and <p, z> are
// fp64 sums of the staged fp32 values, four threads a point, and 1 - x2, 1 - p2 come from those sums (both multiply t: a point near the
// rim would lose its digits in fp32); the epilogue (d2pm_pair) runs in fp64 registers and stores fp32.
//
// Backward, per pair with g the incoming gradient; a clamp that holds passes nothing, the norm at 0 has gradient 0:
//   h = 2 g zn / sqrt(1 + t^2)     C_xz = 2 h / bp     C_xp = 4 h pz / (bp bx)
//   c_x2_i = sum_j -2 h pz / (bp bx) - 2 h alpha pz / (bp bx^2)     c_p2_j = sum_i h t / bp     c_pz_j = sum_i -2 h alpha / (bp bx)
//   c_zn_j = sum_i 2 g asinh(t)
//   grad_x = C_xz zh^T + C_xp p^T + 2 c_x2 x      grad_p = x^T C_xp + 2 c_p2 p + c_pz zh      gzh = x^T C_xz + c_pz p
//   grad_z = (gzh - zh <zh, gzh>) / zn + c_zn zh
// Two fused kernel bodies in the form of dist.hip's dist_pair_bwd_kernel, no N x M intermediate and no workspace.  The owner of 64 rows
// of x (d2pm_bwd_x_kernel), or of 64 planes (d2pm_bwd_planes_kernel: grad_p and grad_z share the walk), keeps its operands in LDS and
// its accumulators in registers (NT = 4 / 8 / 16 tiles of 16 columns for D <= 64 / 128 / 256) and walks the other side in chunks of KC
// points: stage the chunk and the g tile, recompute the two 64 x KC products on MFMA, form the two coefficient tiles (fp32) and the
// scalar sums (fp64) from d2pm_pair, multiply the coefficient tiles with the chunk on MFMA.  KC = 64 up to D = 128; at D <= 256 the
// resident tiles leave room for 32 planes (grad_x) and 16 rows (the planes).  No atomics: every sum has one owner and a fixed order.
//
// Dynamic LDS of one workgroup, C = 16 NT:
//   forward    4 (3 64 (min(pad4(D), 128) + 4)) + 8 256                                                              103 424 at most
//   grad_x     4 ((64 + 2 KC) (C + 4) + 128 (KC + 4)) + 8 (64 + 3 KC)       89 088, 138 240, 152 832 for C = 64, 128, 256
//   planes     4 ((128 + KC) (C + 4) + 128 (KC + 4)) + 8 (192 + KC)         89 088, 138 240, 161 664
// each checked against gfx950's 163 840 bytes before anything is launched.
#include <hip/hip_runtime.h>

#include "../../include/hypad.h"
#include "rowops.h"

using namespace hypad;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MT = 64;                                  // rows (or planes) of a workgroup's tile, 16 per wave
constexpr int FWC = 128;                                // forward: columns of D staged at a time
constexpr int MAX_D = 64 * MAX_EPL;
constexpr double EPS = 1e-15;
constexpr size_t LDS_LIMIT = 160 * 1024;                // a gfx950 workgroup's LDS
constexpr int64_t INT_LIMIT = 0x7fffffff;

inline int nt_of(int D) { return D <= 64 ? 4 : D <= 128 ? 8 : 16; }
inline int kc_x(int nt) { return nt == 16 ? 32 : 64; }
inline int kc_planes(int nt) { return nt == 16 ? 16 : 64; }
__host__ __device__ inline int fw_ld(int D) { const int d4 = (D + 3) & ~3; return (d4 < FWC ? d4 : FWC) + 4; }
inline size_t fwd_lds(int D) { return (size_t)(3 * MT * fw_ld(D)) * sizeof(float) + 4 * MT * sizeof(double); }
inline size_t bwd_x_lds(int nt, int kc) {
  return (size_t)((MT + 2 * kc) * (nt * 16 + 4) + 2 * MT * (kc + 4)) * sizeof(float) + (size_t)(MT + 3 * kc) * sizeof(double);
}
inline size_t bwd_planes_lds(int nt, int kc) {
  return (size_t)((2 * MT + kc) * (nt * 16 + 4) + 2 * MT * (kc + 4)) * sizeof(float) + (size_t)(3 * MT + kc) * sizeof(double);
}

// <u_r, w_r> of the first `rows` rows of two staged tiles, four threads a row, in fp64; `s` carries the sum over the chunks of D
__device__ __forceinline__ void tile_dot_add(const float* __restrict__ u, const float* __restrict__ w, int ld, int cols, int rows, int tid, double& s) {
  if ((tid >> 2) >= rows) return;
  const float* a = u + (tid >> 2) * ld;
  const float* b = w + (tid >> 2) * ld;
  for (int c = tid & 3; c < cols; c += 4) s += (double)a[c] * (double)b[c];
}
__device__ __forceinline__ double quad_sum(double s) {
  s += __shfl_xor(s, 1, WAVE);
  return s + __shfl_xor(s, 2, WAVE);
}

// what a plane brings to its pairs, from the fp64 sums p2 = |p|^2, z2 = |z|^2, pzraw = <p, z>
struct D2PMPlane {
  double bp, zn, zc, pz;                                // max(1 - p2, eps), |z|, max(|z|, eps), <p, z / zc>
  bool bp_clamped;
};
__device__ __forceinline__ D2PMPlane d2pm_plane(double p2, double z2, double pzraw) {
  D2PMPlane pl;
  pl.bp_clamped = 1.0 - p2 < EPS;
  pl.bp = pl.bp_clamped ? EPS : 1.0 - p2;
  pl.zn = sqrt(z2);
  pl.zc = fmax(pl.zn, EPS);
  pl.pz = pzraw / pl.zc;
  return pl;
}
struct D2PMCoef { double xz, xp, x2, p2, pz, zn; };     // the gradients of <x, zh>, <x, p>, |x|^2, |p|^2, <p, zh> and |z| under g

// One (row, plane) pair from x2 = |x|^2 (fp64 sum), the plane, and the MFMA products xp = <x, p>, xzraw = <x, z>.
template <bool BWD>
__device__ __forceinline__ double d2pm_pair(double x2, const D2PMPlane& pl, double xp, double xzraw, double g, D2PMCoef& c) {
  const bool bx_clamped = 1.0 - x2 < EPS;
  const double bx = bx_clamped ? EPS : 1.0 - x2;
  const double alpha = 1.0 - 2.0 * xp + x2;
  const double xz = xzraw / pl.zc;
  const double t = (2.0 / pl.bp) * (xz - (alpha / bx) * pl.pz);
  const double as = asinh(t);
  if constexpr (BWD) {
    const double h = 2.0 * g * pl.zn / sqrt(1.0 + t * t);
    const double hb = h / pl.bp;
    c.xz = 2.0 * hb;
    c.xp = 4.0 * hb * pl.pz / bx;
    c.x2 = -2.0 * hb * pl.pz / bx - (bx_clamped ? 0.0 : 2.0 * hb * alpha * pl.pz / (bx * bx));
    c.p2 = pl.bp_clamped ? 0.0 : hb * t;
    c.pz = -2.0 * hb * alpha / bx;
    c.zn = 2.0 * g * as;
  }
  return 2.0 * as * pl.zn;
}

__global__ __launch_bounds__(THREADS) void d2pm_fwd_kernel(const float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ Z,
                                                            float* __restrict__ out, int N, int M, int D, int tn, int tm) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ld = fw_ld(D);
  float* xt = smem;                                     // [64][ld] rows of x
  float* pt = xt + MT * ld;                             // [64][ld] points of the planes
  float* zt = pt + MT * ld;                             // [64][ld] normals of the planes
  double* x2s = (double*)(zt + MT * ld);                // [64] each: |x|^2, |p|^2, |z|^2, <p, z>
  double* p2s = x2s + MT;
  double* z2s = p2s + MT;
  double* pzs = z2s + MT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / (tn * tm), tile = blockIdx.x % (tn * tm);
  const int i0 = (tile / tm) * MT, j0 = (tile % tm) * MT;
  X += (size_t)b * N * D;
  P += (size_t)b * M * D;
  Z += (size_t)b * M * D;
  out += (size_t)b * N * M;
  f32x4 axp[4], axz[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) { axp[t] = f32x4{0.f, 0.f, 0.f, 0.f}; axz[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  double x2 = 0.0, p2 = 0.0, z2 = 0.0, pz = 0.0;        // four threads a point, the columns c = tid mod 4
  for (int d0 = 0; d0 < D; d0 += FWC) {
    const int dw = D - d0 < FWC ? D - d0 : FWC, dw4 = (dw + 3) & ~3;
    __syncthreads();
    for (int r = wave; r < MT; r += WAVES)
      for (int c = lane; c < dw4; c += 64) {
        xt[r * ld + c] = (c < dw && i0 + r < N) ? X[(size_t)(i0 + r) * D + d0 + c] : 0.f;
        const bool pv = c < dw && j0 + r < M;
        pt[r * ld + c] = pv ? P[(size_t)(j0 + r) * D + d0 + c] : 0.f;
        zt[r * ld + c] = pv ? Z[(size_t)(j0 + r) * D + d0 + c] : 0.f;
      }
    __syncthreads();
    tile_dot_add(xt, xt, ld, dw, MT, tid, x2);
    tile_dot_add(pt, pt, ld, dw, MT, tid, p2);
    tile_dot_add(zt, zt, ld, dw, MT, tid, z2);
    tile_dot_add(pt, zt, ld, dw, MT, tid, pz);
    for (int kk = 0; kk < dw4; kk += 4) {
      const float a = xt[(wave * 16 + j) * ld + kk + q];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        axp[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pt[(t * 16 + j) * ld + kk + q], axp[t], 0, 0, 0);
        axz[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, zt[(t * 16 + j) * ld + kk + q], axz[t], 0, 0, 0);
      }
    }
  }
  x2 = quad_sum(x2);
  p2 = quad_sum(p2);
  z2 = quad_sum(z2);
  pz = quad_sum(pz);
  if ((tid & 3) == 0) { x2s[tid >> 2] = x2; p2s[tid >> 2] = p2; z2s[tid >> 2] = z2; pzs[tid >> 2] = pz; }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int lc = t * 16 + j, gj = j0 + lc;
    if (gj >= M) continue;
    const D2PMPlane pl = d2pm_plane(p2s[lc], z2s[lc], pzs[lc]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = wave * 16 + 4 * q + r, gi = i0 + lr;
      D2PMCoef unused;
      if (gi < N) out[(size_t)gi * M + gj] = (float)d2pm_pair<false>(x2s[lr], pl, (double)axp[t][r], (double)axz[t][r], 0.0, unused);
    }
  }
}

// grad_x of the 64 rows r0.. of x (N, D) against the M planes (P, Z: (M, D)) of one batch element; G is (N, M) row-major.
template <int NT, int KC>
__global__ __launch_bounds__(THREADS) void d2pm_bwd_x_kernel(const float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ Z,
                                                              const float* __restrict__ G, float* __restrict__ gx, int N, int M, int D, int tiles) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDB = NT * 16 + 4, LDP = KC + 4, KT = KC / 16;
  float* xt = smem;                                     // [MT][LDB] the own rows, resident
  float* pc = xt + MT * LDB;                            // [KC][LDB] the chunk's points
  float* zc = pc + KC * LDB;                            // [KC][LDB] the chunk's normals
  float* c1 = zc + KC * LDB;                            // [MT][LDP] g, then C_xp
  float* c2 = c1 + MT * LDP;                            // [MT][LDP] C_xz / max(|z|, eps)
  double* x2s = (double*)(c2 + MT * LDP);               // [MT] |x_i|^2, then [KC] each: |p|^2, |z|^2, <p, z> of the chunk
  double* p2s = x2s + MT;
  double* z2s = p2s + KC;
  double* pzs = z2s + KC;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / tiles, r0 = (blockIdx.x % tiles) * MT;
  X += (size_t)b * N * D;
  P += (size_t)b * M * D;
  Z += (size_t)b * M * D;
  G += (size_t)b * (size_t)N * M;
  gx += (size_t)b * N * D;
  for (int r = wave; r < MT; r += WAVES)
    for (int c = lane; c < NT * 16; c += 64) xt[r * LDB + c] = (r0 + r < N && c < D) ? X[(size_t)(r0 + r) * D + c] : 0.f;
  __syncthreads();
  {
    double s = 0.0;
    tile_dot_add(xt, xt, LDB, D, MT, tid, s);
    s = quad_sum(s);
    if ((tid & 3) == 0) x2s[tid >> 2] = s;
  }
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  double rs[4] = {0.0, 0.0, 0.0, 0.0};                  // the |x|^2 coefficient of the rows wave * 16 + 4 q + r, the columns j mod 16
  const int d4 = (D + 3) & ~3;
  for (int k0 = 0; k0 < M; k0 += KC) {
    const int kw = M - k0 < KC ? M - k0 : KC, kw4 = (kw + 3) & ~3;
    __syncthreads();                                    // the readers of the previous chunk are done
    for (int r = wave; r < KC; r += WAVES)
      for (int c = lane; c < NT * 16; c += 64) {
        const bool v = r < kw && c < D;
        pc[r * LDB + c] = v ? P[(size_t)(k0 + r) * D + c] : 0.f;
        zc[r * LDB + c] = v ? Z[(size_t)(k0 + r) * D + c] : 0.f;
      }
    for (int r = wave; r < MT; r += WAVES)
      for (int c = lane; c < KC; c += 64) c1[r * LDP + c] = (c < kw && r0 + r < N) ? G[(size_t)(r0 + r) * M + k0 + c] : 0.f;
    __syncthreads();
    {
      double sp = 0.0, sz = 0.0, spz = 0.0;
      tile_dot_add(pc, pc, LDB, D, KC, tid, sp);
      tile_dot_add(zc, zc, LDB, D, KC, tid, sz);
      tile_dot_add(pc, zc, LDB, D, KC, tid, spz);
      sp = quad_sum(sp);
      sz = quad_sum(sz);
      spz = quad_sum(spz);
      if ((tid & 3) == 0 && (tid >> 2) < KC) { p2s[tid >> 2] = sp; z2s[tid >> 2] = sz; pzs[tid >> 2] = spz; }
    }
    f32x4 xp[KT], xz[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) { xp[t] = f32x4{0.f, 0.f, 0.f, 0.f}; xz[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int kk = 0; kk < d4; kk += 4) {
      const float a = xt[(wave * 16 + j) * LDB + kk + q];
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        xp[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, pc[(t * 16 + j) * LDB + kk + q], xp[t], 0, 0, 0);
        xz[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, zc[(t * 16 + j) * LDB + kk + q], xz[t], 0, 0, 0);
      }
    }
    __syncthreads();                                    // the chunk's sums are in LDS
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const int lc = t * 16 + j;
      const D2PMPlane pl = d2pm_plane(p2s[lc], z2s[lc], pzs[lc]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = wave * 16 + 4 * q + r;
        D2PMCoef c;
        d2pm_pair<true>(x2s[lr], pl, (double)xp[t][r], (double)xz[t][r], (double)c1[lr * LDP + lc], c);   // (g = 0 past either edge: nothing)
        c1[lr * LDP + lc] = (float)c.xp;
        c2[lr * LDP + lc] = (float)(c.xz / pl.zc);
        rs[r] += c.x2;
      }
    }
    __syncthreads();                                    // the coefficients are in LDS
    for (int kk = 0; kk < kw4; kk += 4) {
      const float a1 = c1[(wave * 16 + j) * LDP + kk + q], a2 = c2[(wave * 16 + j) * LDP + kk + q];
      const float* bp = pc + (kk + q) * LDB + j;
      const float* bz = zc + (kk + q) * LDB + j;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bp[t * 16], acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, bz[t * 16], acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double s = 2.0 * groupd_sum<16>(rs[r]);
    const int lr = wave * 16 + 4 * q + r, gr = r0 + lr;
    if (gr >= N) continue;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = t * 16 + j;
      if (c < D) gx[(size_t)gr * D + c] = (float)((double)acc[t][r] + s * (double)xt[lr * LDB + c]);
    }
  }
}

// grad_p and grad_z (either may be NULL) of the 64 planes r0.. against the N rows of x of one batch element: one walk for both.
template <int NT, int KC>
__global__ __launch_bounds__(THREADS) void d2pm_bwd_planes_kernel(const float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ Z,
                                                                   const float* __restrict__ G, float* __restrict__ gp, float* __restrict__ gz, int N,
                                                                   int M, int D, int tiles) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDB = NT * 16 + 4, LDP = KC + 4, KT = KC / 16;
  float* pt = smem;                                     // [MT][LDB] the own points, resident
  float* zt = pt + MT * LDB;                            // [MT][LDB] the own normals, resident
  float* xc = zt + MT * LDB;                            // [KC][LDB] the chunk of x
  float* c1 = xc + KC * LDB;                            // [MT][LDP] g read transposed, then C_xp
  float* c2 = c1 + MT * LDP;                            // [MT][LDP] C_xz
  double* p2s = (double*)(c2 + MT * LDP);               // [MT] each: |p|^2, |z|^2, <p, z>; then [KC] |x|^2 of the chunk
  double* z2s = p2s + MT;
  double* pzs = z2s + MT;
  double* x2s = pzs + MT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / tiles, r0 = (blockIdx.x % tiles) * MT;
  X += (size_t)b * N * D;
  P += (size_t)b * M * D;
  Z += (size_t)b * M * D;
  G += (size_t)b * (size_t)N * M;
  if (gp) gp += (size_t)b * M * D;
  if (gz) gz += (size_t)b * M * D;
  for (int r = wave; r < MT; r += WAVES)
    for (int c = lane; c < NT * 16; c += 64) {
      const bool v = r0 + r < M && c < D;
      pt[r * LDB + c] = v ? P[(size_t)(r0 + r) * D + c] : 0.f;
      zt[r * LDB + c] = v ? Z[(size_t)(r0 + r) * D + c] : 0.f;
    }
  __syncthreads();
  {
    double sp = 0.0, sz = 0.0, spz = 0.0;
    tile_dot_add(pt, pt, LDB, D, MT, tid, sp);
    tile_dot_add(zt, zt, LDB, D, MT, tid, sz);
    tile_dot_add(pt, zt, LDB, D, MT, tid, spz);
    sp = quad_sum(sp);
    sz = quad_sum(sz);
    spz = quad_sum(spz);
    if ((tid & 3) == 0) { p2s[tid >> 2] = sp; z2s[tid >> 2] = sz; pzs[tid >> 2] = spz; }
  }
  __syncthreads();
  D2PMPlane pl[4];                                      // the own planes wave * 16 + 4 q + r
#pragma unroll
  for (int r = 0; r < 4; ++r) { const int lr = wave * 16 + 4 * q + r; pl[r] = d2pm_plane(p2s[lr], z2s[lr], pzs[lr]); }
  f32x4 accp[NT], accz[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) { accp[t] = f32x4{0.f, 0.f, 0.f, 0.f}; accz[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  double sp2[4] = {0.0, 0.0, 0.0, 0.0}, spz[4] = {0.0, 0.0, 0.0, 0.0}, szn[4] = {0.0, 0.0, 0.0, 0.0};
  const int d4 = (D + 3) & ~3;
  for (int k0 = 0; k0 < N; k0 += KC) {
    const int kw = N - k0 < KC ? N - k0 : KC, kw4 = (kw + 3) & ~3;
    __syncthreads();                                    // the readers of the previous chunk are done
    for (int r = wave; r < KC; r += WAVES)
      for (int c = lane; c < NT * 16; c += 64) xc[r * LDB + c] = (r < kw && c < D) ? X[(size_t)(k0 + r) * D + c] : 0.f;
    for (int c = wave; c < KC; c += WAVES)              // c1[own plane j][position i] = G[i][j]: lanes along j
      c1[lane * LDP + c] = (c < kw && r0 + lane < M) ? G[(size_t)(k0 + c) * M + r0 + lane] : 0.f;
    __syncthreads();
    {
      double s = 0.0;
      tile_dot_add(xc, xc, LDB, D, KC, tid, s);
      s = quad_sum(s);
      if ((tid & 3) == 0 && (tid >> 2) < KC) x2s[tid >> 2] = s;
    }
    f32x4 px[KT], zx[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) { px[t] = f32x4{0.f, 0.f, 0.f, 0.f}; zx[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int kk = 0; kk < d4; kk += 4) {
      const float ap = pt[(wave * 16 + j) * LDB + kk + q], az = zt[(wave * 16 + j) * LDB + kk + q];
#pragma unroll
      for (int t = 0; t < KT; ++t) {
        const float bx = xc[(t * 16 + j) * LDB + kk + q];
        px[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap, bx, px[t], 0, 0, 0);
        zx[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(az, bx, zx[t], 0, 0, 0);
      }
    }
    __syncthreads();                                    // |x|^2 of the chunk is in LDS
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const int lc = t * 16 + j;
      const double xx = x2s[lc];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = wave * 16 + 4 * q + r;
        D2PMCoef c;
        d2pm_pair<true>(xx, pl[r], (double)px[t][r], (double)zx[t][r], (double)c1[lr * LDP + lc], c);     // (g = 0 past either edge: nothing)
        c1[lr * LDP + lc] = (float)c.xp;
        c2[lr * LDP + lc] = (float)c.xz;
        sp2[r] += c.p2;
        spz[r] += c.pz;
        szn[r] += c.zn;
      }
    }
    __syncthreads();                                    // the coefficients are in LDS
    for (int kk = 0; kk < kw4; kk += 4) {
      const float a1 = c1[(wave * 16 + j) * LDP + kk + q], a2 = c2[(wave * 16 + j) * LDP + kk + q];
      const float* bx = xc + (kk + q) * LDB + j;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float bv = bx[t * 16];
        accp[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, accp[t], 0, 0, 0);
        accz[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, bv, accz[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double cp2 = groupd_sum<16>(sp2[r]), cpz = groupd_sum<16>(spz[r]), czn = groupd_sum<16>(szn[r]);
    const int lr = wave * 16 + 4 * q + r, gr = r0 + lr;
    double dot = 0.0;                                   // <zh, gzh>, this lane's columns
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = t * 16 + j;
      const double zh = (double)zt[lr * LDB + c] / pl[r].zc;
      dot += zh * ((double)accz[t][r] + cpz * (double)pt[lr * LDB + c]);
    }
    dot = groupd_sum<16>(dot);
    if (gr >= M) continue;
    const double izn = pl[r].zn > EPS ? 1.0 / pl[r].zn : 0.0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = t * 16 + j;
      if (c >= D) continue;
      const double pv = (double)pt[lr * LDB + c], zh = (double)zt[lr * LDB + c] / pl[r].zc;
      if (gp) gp[(size_t)gr * D + c] = (float)((double)accp[t][r] + 2.0 * cp2 * pv + cpz * zh);
      if (gz) gz[(size_t)gr * D + c] = (float)((((double)accz[t][r] + cpz * pv) - zh * dot) * izn + czn * zh);
    }
  }
}

inline int zero_floats(float* p, size_t n, hipStream_t s) {
  if (!p || n == 0) return HYPAD_OK;
  const hipError_t e = hipMemsetAsync(p, 0, n * sizeof(float), s);
  return e == hipSuccess ? HYPAD_OK : (int)e;
}
// every element count and every grid below 2^31, the LDS of every launch within the limit
inline int sizes_check(int64_t batch, int64_t N, int64_t M, int D) {
  if (batch < 0 || N < 0 || M < 0 || D <= 0) return HYPAD_EINVAL;
  if (D > MAX_D) return HYPAD_EUNSUPPORTED;
  if (batch > INT_LIMIT || N > INT_LIMIT || M > INT_LIMIT) return HYPAD_EUNSUPPORTED;
  if (batch > 0 && (N * M > INT_LIMIT / batch || N * D > INT_LIMIT / batch || M * D > INT_LIMIT / batch)) return HYPAD_EUNSUPPORTED;
  const int nt = nt_of(D);
  if (fwd_lds(D) > LDS_LIMIT || bwd_x_lds(nt, kc_x(nt)) > LDS_LIMIT || bwd_planes_lds(nt, kc_planes(nt)) > LDS_LIMIT) return HYPAD_EUNSUPPORTED;
  return HYPAD_OK;
}
// an operand may be NULL only where it has no elements (x: batch N rows; p, z: batch M rows; g = out or grad_out: batch N M)
inline bool missing(const float* x, const float* p, const float* z, const float* g, int64_t batch, int64_t N, int64_t M) {
  return (!x && batch * N > 0) || ((!p || !z) && batch * M > 0) || (!g && batch * N > 0 && M > 0);
}

template <int NT, int KC>
int launch_bwd_x(const float* x, const float* p, const float* z, const float* g, float* gx, int64_t batch, int N, int M, int D, hipStream_t st) {
  const size_t lds = bwd_x_lds(NT, KC);
  const int tiles = (N + MT - 1) / MT;
  const hipError_t e = allow_lds((const void*)d2pm_bwd_x_kernel<NT, KC>, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((d2pm_bwd_x_kernel<NT, KC>), dim3((unsigned)(batch * tiles)), dim3(THREADS), lds, st, x, p, z, g, gx, N, M, D, tiles);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <int NT, int KC>
int launch_bwd_planes(const float* x, const float* p, const float* z, const float* g, float* gp, float* gz, int64_t batch, int N, int M, int D,
                      hipStream_t st) {
  const size_t lds = bwd_planes_lds(NT, KC);
  const int tiles = (M + MT - 1) / MT;
  const hipError_t e = allow_lds((const void*)d2pm_bwd_planes_kernel<NT, KC>, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((d2pm_bwd_planes_kernel<NT, KC>), dim3((unsigned)(batch * tiles)), dim3(THREADS), lds, st, x, p, z, g, gp, gz, N, M, D, tiles);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

}  // namespace

extern "C" {

int hypad_dist2plane_matmul_fwd(const float* x, const float* p, const float* z, float* out, int64_t batch, int64_t N, int64_t M, int D,
                                hypad_stream_t s) {
  const int rc = sizes_check(batch, N, M, D);
  if (rc) return rc;
  if (missing(x, p, z, out, batch, N, M)) return HYPAD_EINVAL;
  if (batch == 0 || N == 0 || M == 0) return HYPAD_OK;
  const int tn = (int)((N + MT - 1) / MT), tm = (int)((M + MT - 1) / MT);
  if ((int64_t)tn * tm > INT_LIMIT / batch) return HYPAD_EUNSUPPORTED;
  const size_t lds = fwd_lds(D);
  const hipError_t e = allow_lds((const void*)d2pm_fwd_kernel, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(d2pm_fwd_kernel, dim3((unsigned)(batch * tn * tm)), dim3(THREADS), lds, (hipStream_t)s, x, p, z, out, (int)N, (int)M, D, tn, tm);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad_dist2plane_matmul_bwd(const float* x, const float* p, const float* z, const float* grad_out, float* grad_x, float* grad_p, float* grad_z,
                                int64_t batch, int64_t N, int64_t M, int D, hypad_stream_t s) {
  const int rc = sizes_check(batch, N, M, D);
  if (rc) return rc;
  if (missing(x, p, z, grad_out, batch, N, M)) return HYPAD_EINVAL;
  hipStream_t st = (hipStream_t)s;
  if (batch == 0 || N == 0 || M == 0) {                 // sums over no pairs
    int r = zero_floats(grad_x, (size_t)batch * N * D, st);
    if (!r) r = zero_floats(grad_p, (size_t)batch * M * D, st);
    return r ? r : zero_floats(grad_z, (size_t)batch * M * D, st);
  }
  const int n = (int)N, m = (int)M;
  if (grad_x) {
    const int r = D <= 64    ? launch_bwd_x<4, 64>(x, p, z, grad_out, grad_x, batch, n, m, D, st)
                  : D <= 128 ? launch_bwd_x<8, 64>(x, p, z, grad_out, grad_x, batch, n, m, D, st)
                             : launch_bwd_x<16, 32>(x, p, z, grad_out, grad_x, batch, n, m, D, st);
    if (r) return r;
  }
  if (grad_p || grad_z)
    return D <= 64    ? launch_bwd_planes<4, 64>(x, p, z, grad_out, grad_p, grad_z, batch, n, m, D, st)
           : D <= 128 ? launch_bwd_planes<8, 64>(x, p, z, grad_out, grad_p, grad_z, batch, n, m, D, st)
                      : launch_bwd_planes<16, 16>(x, p, z, grad_out, grad_p, grad_z, batch, n, m, D, st);
  return HYPAD_OK;
}

}  // extern "C"
