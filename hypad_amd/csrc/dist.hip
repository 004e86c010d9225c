// Geodesic distances on the Poincare ball at k = -1: dist_matmul (math_.py:905-947), every x_i against every y_j -- below -- and the
// row forms dist (:861-902) and dist0 (:950-975) at the end of this file.  Shapes of the pair form: x (batch, N, D), y (batch, M, D)
// -- the reference's (batch, D, M) transposed by the caller --, out and grad_out (batch, N, M).
//
//   x2_i = |x_i|^2   y2_j = |y_j|^2   xy_ij = <x_i, y_j>
//   num = x2 - 2 xy + y2    den = max(1 - 2 xy + x2 y2, 1e-15)    u = num / den    s = sqrt(max(u, 1e-15))    out_ij = 2 artanh(min(s, 1 - 1e-7))
//
// Forward: ONE launch, a workgroup of four waves per (batch element, 64 x 64 tile of out).  D is staged in chunks of 128 columns; each
// wave multiplies its 16 rows of x with the 64 rows of y on fp32 MFMA; x2 and y2 are fp64 sums of the staged fp32 values, four threads
// a point; the epilogue (rowops.h: dist_pair_d) runs in fp64 registers and stores fp32.
//
// Backward, per pair with g the incoming gradient (rowops.h: dist_pair_bwd_d): a = dL/dnum, b = dL/dden, P = -2 (a + b) = dL/dxy,
//   grad_x_i = sum_j P_ij y_j + 2 x_i sum_j (a_ij + b_ij y2_j)        grad_y_j = sum_i P_ij x_i + 2 y_j sum_i (a_ij + b_ij x2_i)
// One fused kernel body, no N x M intermediate and no workspace.  A workgroup owns 64 rows of its operand with all D columns of
// accumulators (NT = 4 / 8 / 16 tiles of 16 columns for D <= 64 / 128 / 256, the layout of midpoint.hip's product kernel), keeps them
// in LDS and walks the other operand in chunks of 64 points: stage the chunk and the g tile, recompute the 64 x 64 xy tile on MFMA,
// form P in place of g (fp32) and the row sums (fp64) from dist_pair_bwd_d, multiply P with the chunk on MFMA.  The row sums: every lane
// adds its four columns of each chunk for its four rows, the sixteen lanes of a row are combined by a butterfly after the walk.
// grad_y is the same body with the operands exchanged and the g tile read transposed.  Two independent launches: either gradient alone
// has the bits of the run that asks for both.  No atomics: every sum has one owner and a fixed order.
//
// Dynamic LDS of one workgroup:
//   forward    4 (2 64 (min(pad4(D), 128) + 4)) + 8 128 bytes          -- the x and y tiles, x2 and y2;                       68 608 at most
//   backward   4 (2 64 (C + 4) + 64 68) + 8 128 bytes, C = 64, 128, 256 -- the own tile, the chunk, g / P, the two norm vectors:
//              53 248, 86 016, 151 552 -- below gfx950's 160 KiB per workgroup at every D, so the xy product needs no chunking of D.
// Both are checked against that limit before anything is launched.
#include <hip/hip_runtime.h>

#include "../../include/hypad.h"
#include "rowops.h"

using namespace hypad;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MT = 64;                                  // rows of a workgroup's tile, 16 per wave
constexpr int KC = 64;                                  // points of the other operand staged at a time
constexpr int LDP = KC + 4;
constexpr int FWC = 128;                                // forward: columns of D staged at a time
constexpr int MAX_D = 64 * MAX_EPL;
constexpr size_t LDS_LIMIT = 160 * 1024;                // a gfx950 workgroup's LDS
constexpr int64_t INT_LIMIT = 0x7fffffff;
using RW = RowD<64, MAX_EPL>;                           // a row per wave

inline int nt_of(int D) { return D <= 64 ? 4 : D <= 128 ? 8 : 16; }
__host__ __device__ inline int fw_ld(int D) { const int d4 = (D + 3) & ~3; return (d4 < FWC ? d4 : FWC) + 4; }
inline size_t fwd_lds(int D) { return (size_t)(2 * MT * fw_ld(D)) * sizeof(float) + 2 * MT * sizeof(double); }
inline size_t bwd_lds(int D) { return (size_t)(2 * MT * (nt_of(D) * 16 + 4) + MT * LDP) * sizeof(float) + 2 * MT * sizeof(double); }

// |row|^2 of the 64 rows of a staged tile, four threads a row, in fp64; `s` carries the sum over the chunks of D
__device__ __forceinline__ void tile_sq_add(const float* __restrict__ tile, int ld, int cols, int tid, double& s) {
  const float* p = tile + (tid >> 2) * ld;
  for (int c = tid & 3; c < cols; c += 4) { const double v = p[c]; s += v * v; }
}
__device__ __forceinline__ double quad_sum(double s) {
  s += __shfl_xor(s, 1, WAVE);
  return s + __shfl_xor(s, 2, WAVE);
}

// CV... here and below: the launch's curvature -- nothing at k = -1, one Curv at k = -c (rowops.h)
template <class... CV>
__global__ __launch_bounds__(THREADS) void dist_pair_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Y, float* __restrict__ out,
                                                                 int N, int M, int D, int tn, int tm, CV... cv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ld = fw_ld(D);
  float* xt = smem;                                     // [64][ld] rows of x
  float* yt = xt + MT * ld;                             // [64][ld] rows of y
  double* x2s = (double*)(yt + MT * ld);                // [64], then y2 [64]
  double* y2s = x2s + MT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / (tn * tm), tile = blockIdx.x % (tn * tm);
  const int i0 = (tile / tm) * MT, j0 = (tile % tm) * MT;
  X += (size_t)b * N * D;
  Y += (size_t)b * M * D;
  out += (size_t)b * N * M;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  double x2 = 0.0, y2 = 0.0;                            // four threads a point, the columns c = tid mod 4
  for (int d0 = 0; d0 < D; d0 += FWC) {
    const int dw = D - d0 < FWC ? D - d0 : FWC, dw4 = (dw + 3) & ~3;
    __syncthreads();
    for (int r = wave; r < MT; r += WAVES)
      for (int c = lane; c < dw4; c += 64) {
        xt[r * ld + c] = (c < dw && i0 + r < N) ? X[(size_t)(i0 + r) * D + d0 + c] : 0.f;
        yt[r * ld + c] = (c < dw && j0 + r < M) ? Y[(size_t)(j0 + r) * D + d0 + c] : 0.f;
      }
    __syncthreads();
    tile_sq_add(xt, ld, dw, tid, x2);
    tile_sq_add(yt, ld, dw, tid, y2);
    for (int kk = 0; kk < dw4; kk += 4) {
      const float a = xt[(wave * 16 + j) * ld + kk + q];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, yt[(t * 16 + j) * ld + kk + q], acc[t], 0, 0, 0);
    }
  }
  x2 = quad_sum(x2);
  y2 = quad_sum(y2);
  if ((tid & 3) == 0) { x2s[tid >> 2] = x2; y2s[tid >> 2] = y2; }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lr = wave * 16 + 4 * q + r, gi = i0 + lr;
    if (gi >= N) continue;
    const double xx = x2s[lr];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int lc = t * 16 + j, gj = j0 + lc;
      if (gj < M) out[(size_t)gi * M + gj] = (float)dist_pair_d(xx, y2s[lc], (double)acc[t][r], cv...);
    }
  }
}

// The gradient of the `rows` rows of A (rows, D) against the K rows of B (K, D) of one batch element.  GRADY = false: A = x, B = y,
// g(i, k) = G[i][k]; GRADY = true: A = y, B = x, g(j, k) = G[k][j].  G is (N, M) row-major: gld = M.
template <int NT, bool GRADY, class... CV>
__global__ __launch_bounds__(THREADS) void dist_pair_bwd_kernel(const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ G,
                                                                 float* __restrict__ grad, int rows, int K, int gld, int D, int tiles, CV... cv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDB = NT * 16 + 4;
  float* at = smem;                                     // [MT][LDB] the own rows, resident
  float* bs = at + MT * LDB;                            // [KC][LDB] the chunk
  float* ps = bs + KC * LDB;                            // [MT][LDP] g, then P
  double* a2s = (double*)(ps + MT * LDP);               // [MT] |a_i|^2, then [KC] |b_k|^2 of the chunk
  double* b2s = a2s + MT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / tiles, r0 = (blockIdx.x % tiles) * MT;
  A += (size_t)b * rows * D;
  B += (size_t)b * K * D;
  G += (size_t)b * (size_t)rows * K;
  grad += (size_t)b * rows * D;
  for (int r = wave; r < MT; r += WAVES)
    for (int c = lane; c < NT * 16; c += 64) at[r * LDB + c] = (r0 + r < rows && c < D) ? A[(size_t)(r0 + r) * D + c] : 0.f;
  __syncthreads();
  {
    double s = 0.0;
    tile_sq_add(at, LDB, D, tid, s);
    s = quad_sum(s);
    if ((tid & 3) == 0) a2s[tid >> 2] = s;
  }
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  double rs[4] = {0.0, 0.0, 0.0, 0.0};                  // sum_k (a + b |b_k|^2) of the rows wave * 16 + 4 q + r, the columns k = j mod 16
  const int d4 = (D + 3) & ~3;
  for (int k0 = 0; k0 < K; k0 += KC) {
    const int kw = K - k0 < KC ? K - k0 : KC, kw4 = (kw + 3) & ~3;
    __syncthreads();                                    // the readers of the previous chunk are done
    for (int r = wave; r < KC; r += WAVES)
      for (int c = lane; c < NT * 16; c += 64) bs[r * LDB + c] = (r < kw && c < D) ? B[(size_t)(k0 + r) * D + c] : 0.f;
    if (GRADY) {
      for (int c = wave; c < KC; c += WAVES)            // ps[own row j][position i] = G[i][j]: lanes along j
        ps[lane * LDP + c] = (c < kw && r0 + lane < rows) ? G[(size_t)(k0 + c) * gld + r0 + lane] : 0.f;
    } else {
      for (int r = wave; r < MT; r += WAVES) ps[r * LDP + lane] = (lane < kw && r0 + r < rows) ? G[(size_t)(r0 + r) * gld + k0 + lane] : 0.f;
    }
    __syncthreads();
    {
      double s = 0.0;
      tile_sq_add(bs, LDB, D, tid, s);
      s = quad_sum(s);
      if ((tid & 3) == 0) b2s[tid >> 2] = s;
    }
    f32x4 xy[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) xy[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < d4; kk += 4) {
      const float a = at[(wave * 16 + j) * LDB + kk + q];
#pragma unroll
      for (int t = 0; t < 4; ++t) xy[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bs[(t * 16 + j) * LDB + kk + q], xy[t], 0, 0, 0);
    }
    __syncthreads();                                    // |b_k|^2 of the chunk is in LDS
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = wave * 16 + 4 * q + r;
      const double aa = a2s[lr];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int lc = t * 16 + j;
        const double bb = b2s[lc];
        double da, db;
        dist_pair_bwd_d(aa, bb, (double)xy[t][r], (double)ps[lr * LDP + lc], da, db, cv...);      // (g = 0 past either edge: nothing)
        ps[lr * LDP + lc] = (float)(-2.0 * (da + db));
        rs[r] += da + db * curv_mul(bb, cv...);
      }
    }
    __syncthreads();                                    // P is in LDS
    for (int kk = 0; kk < kw4; kk += 4) {
      const float a = ps[(wave * 16 + j) * LDP + kk + q];
      const float* bp = bs + (kk + q) * LDB + j;
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[t * 16], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double s = 2.0 * groupd_sum<16>(rs[r]);
    const int lr = wave * 16 + 4 * q + r, gr = r0 + lr;
    if (gr >= rows) continue;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = t * 16 + j;
      if (c < D) grad[(size_t)gr * D + c] = (float)((double)acc[t][r] + s * (double)at[lr * LDB + c]);
    }
  }
}

// ---- the row forms: a wave per row
__global__ __launch_bounds__(THREADS) void dist_rows(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out, int64_t rows, int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    const double d = dist_row_d(rowd_load<RW>(x + r * dim, dim, lane), rowd_load<RW>(y + r * dim, dim, lane));
    if (lane == 0) out[r] = (float)d;
  }
}
__global__ __launch_bounds__(THREADS) void dist_rows_bwd(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ go,
                                                         float* __restrict__ gx, float* __restrict__ gy, int64_t rows, int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW dx, dy;
    dist_row_bwd_d(rowd_load<RW>(x + r * dim, dim, lane), rowd_load<RW>(y + r * dim, dim, lane), (double)go[r], dx, dy);
    if (gx) rowd_store(gx + r * dim, dx, dim, lane);
    if (gy) rowd_store(gy + r * dim, dy, dim, lane);
  }
}
__global__ __launch_bounds__(THREADS) void dist0_rows(const float* __restrict__ x, float* __restrict__ out, int64_t rows, int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    const double d = dist0_row_d(rowd_load<RW>(x + r * dim, dim, lane));
    if (lane == 0) out[r] = (float)d;
  }
}
__global__ __launch_bounds__(THREADS) void dist0_rows_bwd(const float* __restrict__ x, const float* __restrict__ go, float* __restrict__ gx, int64_t rows,
                                                          int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(gx + r * dim, dist0_row_bwd_d(rowd_load<RW>(x + r * dim, dim, lane), (double)go[r]), dim, lane);
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
// sizes of the pair form: every element count and every grid below 2^31, the LDS of every launch within the limit
inline int pair_check(int64_t batch, int64_t N, int64_t M, int D) {
  if (batch < 0 || N < 0 || M < 0 || D <= 0) return HYPAD_EINVAL;
  if (D > MAX_D) return HYPAD_EUNSUPPORTED;
  if (batch > INT_LIMIT || N > INT_LIMIT || M > INT_LIMIT) return HYPAD_EUNSUPPORTED;
  if (batch > 0 && (N * M > INT_LIMIT / batch || N * D > INT_LIMIT / batch || M * D > INT_LIMIT / batch)) return HYPAD_EUNSUPPORTED;
  if (fwd_lds(D) > LDS_LIMIT || bwd_lds(D) > LDS_LIMIT) return HYPAD_EUNSUPPORTED;
  return HYPAD_OK;
}
// an operand may be NULL only where it has no elements (x: batch N rows, y: batch M rows, g = out or grad_out: batch N M)
inline bool pair_missing(const float* x, const float* y, const float* g, int64_t batch, int64_t N, int64_t M) {
  return (!x && batch * N > 0) || (!y && batch * M > 0) || (!g && batch * N > 0 && M > 0);
}
inline int rows_check(int64_t rows, int dim) {
  if (rows < 0 || dim <= 0) return HYPAD_EINVAL;
  return dim > MAX_D ? HYPAD_EUNSUPPORTED : HYPAD_OK;
}

template <bool GRADY, class... CV>
int launch_pair_bwd(const float* A, const float* B, const float* G, float* grad, int64_t batch, int rows, int K, int gld, int D, hipStream_t st,
                    CV... cv) {
  const size_t lds = bwd_lds(D);
  const int tiles = (rows + MT - 1) / MT;
  const dim3 grid((unsigned)(batch * tiles));
#define HYPAD_DIST_LAUNCH(NT)                                                                                                      \
  do {                                                                                                                              \
    const hipError_t e = allow_lds((const void*)dist_pair_bwd_kernel<NT, GRADY, CV...>, lds);                                       \
    if (e != hipSuccess) return (int)e;                                                                                             \
    hipLaunchKernelGGL((dist_pair_bwd_kernel<NT, GRADY, CV...>), grid, dim3(THREADS), lds, st, A, B, G, grad, rows, K, gld, D, tiles, cv...); \
  } while (0)
  if (D <= 64) HYPAD_DIST_LAUNCH(4);
  else if (D <= 128) HYPAD_DIST_LAUNCH(8);
  else HYPAD_DIST_LAUNCH(16);
#undef HYPAD_DIST_LAUNCH
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

template <class... CV>
int pair_fwd(const float* x, const float* y, float* out, int64_t batch, int64_t N, int64_t M, int D, hypad_stream_t s, CV... cv) {
  const int rc = pair_check(batch, N, M, D);
  if (rc) return rc;
  if (pair_missing(x, y, out, batch, N, M)) return HYPAD_EINVAL;
  if (batch == 0 || N == 0 || M == 0) return HYPAD_OK;
  const int tn = (int)((N + MT - 1) / MT), tm = (int)((M + MT - 1) / MT);
  if ((int64_t)tn * tm > INT_LIMIT / batch) return HYPAD_EUNSUPPORTED;
  const size_t lds = fwd_lds(D);
  const hipError_t e = allow_lds((const void*)dist_pair_fwd_kernel<CV...>, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(dist_pair_fwd_kernel<CV...>, dim3((unsigned)(batch * tn * tm)), dim3(THREADS), lds, (hipStream_t)s, x, y, out, (int)N, (int)M, D, tn,
                     tm, cv...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

template <class... CV>
int pair_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t batch, int64_t N, int64_t M, int D,
             hypad_stream_t s, CV... cv) {
  const int rc = pair_check(batch, N, M, D);
  if (rc) return rc;
  if (pair_missing(x, y, grad_out, batch, N, M)) return HYPAD_EINVAL;
  hipStream_t st = (hipStream_t)s;
  if (batch == 0 || N == 0 || M == 0) {                 // sums over no pairs
    const int rx = zero_floats(grad_x, (size_t)batch * N * D, st);
    return rx ? rx : zero_floats(grad_y, (size_t)batch * M * D, st);
  }
  if (grad_x) {
    const int r = launch_pair_bwd<false>(x, y, grad_out, grad_x, batch, (int)N, (int)M, (int)M, D, st, cv...);
    if (r) return r;
  }
  if (grad_y) return launch_pair_bwd<true>(y, x, grad_out, grad_y, batch, (int)M, (int)N, (int)M, D, st, cv...);
  return HYPAD_OK;
}

}  // namespace

extern "C" {

int hypad_dist_matmul_fwd(const float* x, const float* y, float* out, int64_t batch, int64_t N, int64_t M, int D, hypad_stream_t s) {
  return pair_fwd(x, y, out, batch, N, M, D, s);
}
int hypad_dist_matmul_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t batch, int64_t N, int64_t M,
                          int D, hypad_stream_t s) {
  return pair_bwd(x, y, grad_out, grad_x, grad_y, batch, N, M, D, s);
}
// the same at k = -c: c is checked first, then everything as above
int hypad_ball_dist_matmul_fwd(const float* x, const float* y, float* out, int64_t batch, int64_t N, int64_t M, int D, double c, hypad_stream_t s) {
  return curv_invalid(c) ? HYPAD_EINVAL : pair_fwd(x, y, out, batch, N, M, D, s, curv_of(c));
}
int hypad_ball_dist_matmul_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t batch, int64_t N,
                               int64_t M, int D, double c, hypad_stream_t s) {
  return curv_invalid(c) ? HYPAD_EINVAL : pair_bwd(x, y, grad_out, grad_x, grad_y, batch, N, M, D, s, curv_of(c));
}

int hypad_dist_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, hypad_stream_t s) {
  const int rc = rows_check(rows, dim);
  if (rc) return rc;
  if (rows > 0 && (!x || !y || !out)) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  hipLaunchKernelGGL(dist_rows, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, x, y, out, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_dist_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, hypad_stream_t s) {
  const int rc = rows_check(rows, dim);
  if (rc) return rc;
  if (rows > 0 && (!x || !y || !grad_out)) return HYPAD_EINVAL;
  if (rows == 0 || (!grad_x && !grad_y)) return HYPAD_OK;
  hipLaunchKernelGGL(dist_rows_bwd, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, x, y, grad_out, grad_x, grad_y, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_dist0_fwd(const float* x, float* out, int64_t rows, int dim, hypad_stream_t s) {
  const int rc = rows_check(rows, dim);
  if (rc) return rc;
  if (rows > 0 && (!x || !out)) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  hipLaunchKernelGGL(dist0_rows, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, x, out, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_dist0_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, hypad_stream_t s) {
  const int rc = rows_check(rows, dim);
  if (rc) return rc;
  if (rows > 0 && (!x || !grad_out || !grad_x)) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  hipLaunchKernelGGL(dist0_rows_bwd, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, x, grad_out, grad_x, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

}  // extern "C"
