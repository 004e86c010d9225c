// Signed geodesic distance of ball-valued rows to hyperplanes of the ball (hyperspace/hyrnn_nets.py:210-245, math_.py:1645-1666 at
// k = -1): the hyperbolic counterpart of the logits of a linear layer.  Everything the distance of row x to the plane (p, a) needs is a
// function of the two products <p,x>, <x,a> and of per-row / per-plane scalars, so the forward is the pair-wise distance kernel's
// shape (ops_hyper.hip: pairdist_kernel): a 64 x 64 tile of x P^T and of x A^T on fp32 MFMA from one staged x tile, and the epilogue in
// registers.  The backward recomputes the two products with the same kernel body, turns grad_out into the per-element coefficients of
// <p,x> and <x,a> and the row / column sums of the scalar coefficients; the grad_x contraction goes through hypad_linear_act_bwd,
// the two C^T x contractions through a row-sliced MFMA kernel.
//
//   px = <p,x>  xa = <x,a>  x2 = |x|^2  p2 = |p|^2  pa = <p,a>  an = |a|
//   alpha = 1 - 2 px + x2     beta = 1 - p2     D = max(1 - 2 px + p2 x2, 1e-15)
//   s  = (beta xa - alpha pa) / D                                   = <(-p) (+) x, a>
//   n2 = max((alpha^2 p2 - 2 alpha beta px + beta^2 x2) / D^2, 1e-15)  = |(-p) (+) x|^2
//   d  = asinh(2 s' / clamp_abs((1 - n2) an))      s' = s or |s|;  d an if scaled;  times exp(log_scale)
//
// 1 - n2 is where a row near the rim loses its digits (1 - 1e-3 leaves fp32 four of them), and it has a closed form,
//   1 - |(-p) (+) x|^2 = beta (1 - x2) / D,
// in which only 1 - x2 and beta = 1 - p2 cancel: the kernels take those two from fp64 sums over the staged tiles (the squares of fp32
// numbers are exact in fp64) and evaluate 1 - n2 by the closed form; the products and the rest of the epilogue are fp32.
//
// LDS of one workgroup: 4 (192 (min(pad4(K), 128) + 4) + 448) bytes forward, 4096 more in the backward -- at most 107 264: K is
// staged in chunks of 128 columns, so every K <= 256 runs (three 64 x 260 tiles would not fit).
#include <hip/hip_runtime.h>

#include "../../include/hypad.h"
#include "device_utils.h"

using namespace hypad;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int DT = 64;            // rows and planes of a tile
constexpr int DKC = 128;          // columns of K staged at a time
constexpr int MAX_K = 256;        // 64 * MAX_EPL, the limit of the other row ops
constexpr float D2P_EPS = 1e-15f;

__host__ __device__ inline int d2p_ld(int K) { const int k4 = (K + 3) & ~3; return (k4 < DKC ? k4 : DKC) + 4; }
inline size_t d2p_lds(int K, bool bwd) { return (size_t)(3 * DT * d2p_ld(K) + 7 * DT + (bwd ? 16 * DT : 0)) * sizeof(float); }

struct D2PCoef { float px, xa, x2, p2, pa, an, sc; };

// One (row, plane) pair; gamma = 1 - x2 and beta = 1 - p2 come rounded from fp64.  Returns the output element; BWD: c = the
// gradients of the scalars under grad_out g (c.x2 and c.p2 include what flows through gamma and beta; c.sc = g * out, the summand of
// grad_log_scale).  On a clamp nothing flows through the clamped quantity.
template <bool BWD>
__device__ __forceinline__ float d2p_elem(float px, float xa, float x2, float gamma, float p2, float beta, float pa, float an, float E,
                                          bool sgn, bool scaled, float g, D2PCoef& c) {
  const float alpha = 1.f - 2.f * px + x2;
  const float Draw = 1.f - 2.f * px + p2 * x2;
  const float rD = 1.f / fmaxf(Draw, D2P_EPS);
  const float s = (beta * xa - alpha * pa) * rD;
  const float om_raw = beta * gamma * rD;                          // 1 - n2 before the clamp n2 >= 1e-15
  const bool clamped = 1.f - om_raw < D2P_EPS;
  const float om = clamped ? 1.f - D2P_EPS : om_raw;
  const float sp = sgn ? s : fabsf(s);
  const float v = om * an;
  const float den = v >= 0.f ? v + D2P_EPS : v - D2P_EPS;          // clamp_abs: sign'(v) (|v| + 1e-15), sign'(0) = +1
  const float t = 2.f * sp / den;
  const float d = asinhf(t);
  const float o = d * (scaled ? an : 1.f) * E;
  if constexpr (BWD) {
    const float gd = g * (scaled ? an : 1.f) * E;
    const float gt = gd / sqrtf(1.f + t * t);
    const float gsp = 2.f * gt / den, gv = -gt * t / den;
    const float gs = sgn ? gsp : (s > 0.f ? gsp : (s < 0.f ? -gsp : 0.f));
    const float gom = clamped ? 0.f : gv * an;
    c.an = gv * om + (scaled ? g * d * E : 0.f);
    const float gnums = gs * rD;
    const float gD = -(gom * om_raw + gs * s) * rD;
    const float gDraw = Draw >= D2P_EPS ? gD : 0.f;
    const float galpha = -gnums * pa;
    c.xa = gnums * beta;
    c.pa = -gnums * alpha;
    c.px = -2.f * (gDraw + galpha);
    c.x2 = gDraw * p2 + galpha - gom * beta * rD;
    c.p2 = gDraw * x2 - gnums * xa - gom * gamma * rD;
    c.sc = g * o;
  }
  return o;
}

// Forward (BWD = false): out[r][n] for a 64-row tile (blockIdx.x) and the plane tiles blockIdx.y, blockIdx.y + gridDim.y, ...
// Backward (BWD = true, gridDim.y == 1: the workgroup walks every plane tile of its rows): ccat (rows, 2N) = [C_px | C_xa],
// cx2 (rows) = the row sums of the |x|^2 coefficient, part (row tiles, 4, N) = this row tile's column sums of the |p|^2, <p,a>, |a|
// coefficients and of grad_out * out.  No atomics: every sum has one owner and a fixed order.
template <bool BWD>
__global__ __launch_bounds__(THREADS) void d2p_kernel(const float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ A,
                                                       const float* __restrict__ log_scale, float* __restrict__ out,
                                                       const float* __restrict__ gout, float* __restrict__ ccat,
                                                       float* __restrict__ cx2, float* __restrict__ part, int64_t rows, int K, int N,
                                                       int flags) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ld = d2p_ld(K);
  float* xs = smem;                  // [64][ld]
  float* ps = xs + DT * ld;          // [64][ld]
  float* as = ps + DT * ld;          // [64][ld]
  float* st = as + DT * ld;          // [4][64]: x2 of the rows; p2, pa, |a| of the planes
  float* es = st + 4 * DT;           // [64]: exp(log_scale) of the planes
  float* gm = es + DT;               // [64]: 1 - x2 of the rows, rounded from fp64
  float* bt = gm + DT;               // [64]: 1 - p2 of the planes, rounded from fp64
  float* cr = bt + DT;               // BWD: [4 waves][4][64] column sums of a wave's 16 rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * DT;
  const bool sgn = (flags & HYPAD_D2P_SIGNED) != 0, scaled = (flags & HYPAD_D2P_SCALED) != 0;
  const bool one_chunk = K <= DKC;
  const int nct = (N + DT - 1) / DT;
  float rx2[4] = {0.f, 0.f, 0.f, 0.f};
  bool x_staged = false;
  for (int ct = blockIdx.y; ct < nct; ct += gridDim.y) {
    const int c0 = ct * DT;
    f32x4 apx[4], axa[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { apx[t] = f32x4{0.f, 0.f, 0.f, 0.f}; axa[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    double stat = 0.0;                                             // wave 0: x2 of row `lane`; 1, 2, 3: p2, pa, |a|^2 of plane `lane`
    for (int kc = 0; kc < K; kc += DKC) {
      const int kw = K - kc < DKC ? K - kc : DKC, kw4 = (kw + 3) & ~3;
      __syncthreads();                                             // the readers of the previous tiles are done
      for (int r = wave; r < DT; r += THREADS / 64)
        for (int c = lane; c < kw4; c += 64) {
          const bool cv = c < kw;
          if (!x_staged) xs[r * ld + c] = (cv && r0 + r < rows) ? X[(size_t)(r0 + r) * K + kc + c] : 0.f;
          const bool pv = cv && c0 + r < N;
          ps[r * ld + c] = pv ? P[(size_t)(c0 + r) * K + kc + c] : 0.f;
          as[r * ld + c] = pv ? A[(size_t)(c0 + r) * K + kc + c] : 0.f;
        }
      x_staged = one_chunk;                                        // one chunk: the x tile serves every plane tile
      __syncthreads();
      {
        const float* u = (wave == 0 ? xs : wave == 3 ? as : ps) + lane * ld;
        const float* w = (wave == 0 ? xs : wave == 1 ? ps : as) + lane * ld;
        for (int c = 0; c < kw; ++c) stat += (double)u[c] * (double)w[c];
      }
      for (int k0 = 0; k0 < kw4; k0 += 4) {
        const int k = k0 + q;
        const float a = xs[(wave * 16 + j) * ld + k];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          apx[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ps[(t * 16 + j) * ld + k], apx[t], 0, 0, 0);
          axa[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, as[(t * 16 + j) * ld + k], axa[t], 0, 0, 0);
        }
      }
    }
    st[tid] = wave == 3 ? (float)sqrt(stat) : (float)stat;
    if (wave == 0) gm[lane] = (float)(1.0 - stat);
    if (wave == 1) bt[lane] = (float)(1.0 - stat);
    if (wave == 1) es[lane] = (log_scale && c0 + lane < N) ? expf(log_scale[c0 + lane]) : 1.f;
    __syncthreads();
    float cs[4][4];                                                // BWD: [quantity][t], summed over this lane's four rows
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int lc = t * 16 + j, gc = c0 + lc;
      const float p2 = st[DT + lc], beta = bt[lc], pa = st[2 * DT + lc], an = st[3 * DT + lc], E = es[lc];
      if constexpr (BWD) cs[0][t] = cs[1][t] = cs[2][t] = cs[3][t] = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = wave * 16 + 4 * q + r;
        const int64_t gr = r0 + lr;
        const bool valid = gr < rows && gc < N;
        D2PCoef c;
        float g = 0.f;
        if constexpr (BWD) g = valid ? gout[(size_t)gr * N + gc] : 0.f;
        const float o = d2p_elem<BWD>(apx[t][r], axa[t][r], st[lr], gm[lr], p2, beta, pa, an, E, sgn, scaled, g, c);
        if constexpr (BWD) {
          if (valid) {
            ccat[(size_t)gr * 2 * N + gc] = c.px;
            ccat[(size_t)gr * 2 * N + N + gc] = c.xa;
          }
          rx2[r] += valid ? c.x2 : 0.f;
          cs[0][t] += valid ? c.p2 : 0.f;
          cs[1][t] += valid ? c.pa : 0.f;
          cs[2][t] += valid ? c.an : 0.f;
          cs[3][t] += valid ? c.sc : 0.f;
        } else if (valid) {
          out[(size_t)gr * N + gc] = o;
        }
      }
    }
    if constexpr (BWD) {
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float v = cs[u][t];
          v += __shfl_xor(v, 16, WAVE);
          v += __shfl_xor(v, 32, WAVE);
          if (q == 0) cr[(wave * 4 + u) * DT + t * 16 + j] = v;
        }
      __syncthreads();
      if (c0 + lane < N) {                                         // thread (u = wave, column = lane): the four waves in order
        const float v = ((cr[(0 * 4 + wave) * DT + lane] + cr[(1 * 4 + wave) * DT + lane]) + cr[(2 * 4 + wave) * DT + lane]) +
                        cr[(3 * 4 + wave) * DT + lane];
        part[((size_t)blockIdx.x * 4 + wave) * N + c0 + lane] = v;
      }
    }
  }
  if constexpr (BWD) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = row16_sum(rx2[r]);
      const int64_t gr = r0 + wave * 16 + 4 * q + r;
      if (j == 0 && gr < rows) cx2[gr] = v;
    }
  }
}

// wpart[sl] (2N, K) = [C_px | C_xa]^T x over the rows of slice sl (blockIdx.y): a 16 x 16 tile per wave on fp32 MFMA, as
// ops_dense.hip: outer_sum_kernel, but with the rows split over up to 64 slices -- one wave per tile walking every row is a serial
// chain of rows / 4 MFMAs on a handful of CUs.  The slices are added by d2p_finish_planes, in order.
__global__ __launch_bounds__(THREADS) void d2p_outer_kernel(const float* __restrict__ ccat, const float* __restrict__ X,
                                                             float* __restrict__ wpart, int64_t rows, int64_t slice_rows, int K, int N2) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int tk = (K + 15) >> 4, tn = (N2 + 15) >> 4;
  const int tile = blockIdx.x * (THREADS / 64) + wave;
  if (tile >= tn * tk) return;
  const int n0 = (tile / tk) * 16, k0 = (tile % tk) * 16;
  const int64_t rbeg = (int64_t)blockIdx.y * slice_rows;
  const int64_t rend = rbeg + slice_rows < rows ? rbeg + slice_rows : rows;
  const bool nv = n0 + j < N2, kv = k0 + j < K;
  const float* cp = ccat + (nv ? n0 + j : 0);
  const float* xp = X + (kv ? k0 + j : 0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int64_t rr = rbeg; rr < rend; rr += 4) {
    const int64_t r = rr + q;
    const bool rv = r < rend;
    const float a = (rv && nv) ? cp[(size_t)r * N2] : 0.f;
    const float b = (rv && kv) ? xp[(size_t)r * K] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + 4 * q + r, k = k0 + j;
    if (n < N2 && k < K) wpart[((size_t)blockIdx.y * N2 + n) * K + k] = acc[r];
  }
}

// One wave per plane n: the column sums over the row tiles and the slices of the products in a fixed order, then
//   grad_p[n] = (C_px^T x)[n] + 2 c_p2 p[n] + c_pa a[n]     grad_a[n] = (C_xa^T x)[n] + c_pa p[n] + c_an a[n] / |a[n]|
// (wpart: slices of [C_px^T x ; C_xa^T x], each (2N, K); a zero normal takes the zero subgradient of its norm) and grad_log_scale[n].
__global__ __launch_bounds__(THREADS) void d2p_finish_planes(const float* __restrict__ P, const float* __restrict__ A,
                                                              const float* __restrict__ wpart, int slices,
                                                              const float* __restrict__ part, int64_t ntiles, float* __restrict__ gp, float* __restrict__ ga,
                                                              float* __restrict__ gscale, int K, int N) {
  const int lane = threadIdx.x & 63;
  for (int n = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); n < N; n += gridDim.x * (THREADS / 64)) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t b = lane; b < ntiles; b += 64)
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] += part[((size_t)b * 4 + u) * N + n];
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = wave_sum(s[u]);
    float a2 = 0.f;
    for (int c = lane; c < K; c += 64) { const float v = A[(size_t)n * K + c]; a2 += v * v; }
    const float an = sqrtf(wave_sum(a2));
    const float ia = an > 0.f ? s[2] / an : 0.f;
    for (int c = lane; c < K; c += 64) {
      const float pv = P[(size_t)n * K + c], av = A[(size_t)n * K + c];
      float wp = 0.f, wa = 0.f;
      for (int sl = 0; sl < slices; ++sl) {
        if (gp) wp += wpart[((size_t)sl * 2 * N + n) * K + c];
        if (ga) wa += wpart[((size_t)sl * 2 * N + N + n) * K + c];
      }
      if (gp) gp[(size_t)n * K + c] = wp + 2.f * s[0] * pv + s[1] * av;
      if (ga) ga[(size_t)n * K + c] = wa + s[1] * pv + ia * av;
    }
    if (gscale && lane == 0) gscale[n] = s[3];
  }
}

// grad_x += 2 c_x2 x, row by row
__global__ __launch_bounds__(THREADS) void d2p_finish_rows(const float* __restrict__ X, const float* __restrict__ cx2,
                                                            float* __restrict__ gx, int64_t rows, int K) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * (THREADS / 64)) {
    const float c = 2.f * cx2[r];
    for (int k = lane; k < K; k += 64) gx[(size_t)r * K + k] += c * X[(size_t)r * K + k];
  }
}

// wcat (2N, K) = [P ; A], nk = N K floats each.  A kernel, not two hipMemcpyAsync: a call may be captured into a graph, and this
// library puts no non-kernel node between the kernels of a captured sequence (scoring.hip: launch_quantiles).
__global__ __launch_bounds__(THREADS) void d2p_stack_kernel(const float* __restrict__ P, const float* __restrict__ A,
                                                             float* __restrict__ wcat, size_t nk) {
  for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < 2 * nk; i += (size_t)gridDim.x * THREADS)
    wcat[i] = i < nk ? P[i] : A[i - nk];
}

struct D2PWorkspace {
  size_t wcat, wpart, ccat, cx2, part, total;                      // offsets in floats
  int slices;
  int64_t slice_rows;
};
inline D2PWorkspace d2p_workspace(int64_t rows, int K, int N) {
  D2PWorkspace w;
  const size_t nk = (size_t)2 * N * K, rn = (size_t)rows * 2 * N, tiles = (size_t)((rows + DT - 1) / DT);
  const int64_t want = (rows + 255) / 256;                          // slices of at least 256 rows, at most 64 of them
  w.slices = (int)(want > 64 ? 64 : want < 1 ? 1 : want);
  w.slice_rows = (((rows + w.slices - 1) / w.slices) + 3) & ~(int64_t)3;
  w.wcat = 0;                 // [P ; A] (2N, K)
  w.wpart = w.wcat + nk;      // slices of [C_px^T x ; C_xa^T x], each (2N, K)
  w.ccat = w.wpart + (size_t)w.slices * nk;   // [C_px | C_xa] (rows, 2N)
  w.cx2 = w.ccat + rn;        // (rows)
  w.part = w.cx2 + (size_t)rows;   // (row tiles, 4, N)
  w.total = w.part + tiles * 4 * N;
  return w;
}

inline int d2p_check(const float* p, const float* a, int64_t rows, int K, int N, int flags) {
  if (!p || !a || rows < 0 || K <= 0 || N <= 0) return HYPAD_EINVAL;
  if (flags & ~(HYPAD_D2P_SIGNED | HYPAD_D2P_SCALED)) return HYPAD_EINVAL;
  if (K > MAX_K) return HYPAD_EUNSUPPORTED;
  if ((rows + DT - 1) / DT > 0x7fffffff || (N + DT - 1) / DT > 65535) return HYPAD_EUNSUPPORTED;
  return HYPAD_OK;
}
inline int d2p_zero(float* p, size_t n, hipStream_t s) {
  if (!p) return HYPAD_OK;
  const hipError_t e = hipMemsetAsync(p, 0, n * sizeof(float), s);
  return e == hipSuccess ? HYPAD_OK : (int)e;
}
inline int row_blocks(int64_t n) {
  int64_t b = (n + THREADS / 64 - 1) / (THREADS / 64);
  return (int)(b > 4096 ? 4096 : b < 1 ? 1 : b);
}

}  // namespace

extern "C" {

size_t hypad_dist2plane_workspace_bytes(int64_t rows, int K, int N) {
  if (rows < 0 || K <= 0 || N <= 0) return 0;
  return d2p_workspace(rows, K, N).total * sizeof(float);
}

int hypad_dist2plane_fwd(const float* x, const float* p, const float* a, const float* log_scale, float* out, int64_t rows, int K, int N,
                         int flags, hypad_stream_t s) {
  int rc = d2p_check(p, a, rows, K, N, flags);
  if (rc) return rc;
  if (rows == 0) return HYPAD_OK;
  if (!x || !out) return HYPAD_EINVAL;
  const size_t lds = d2p_lds(K, false);
  hipError_t e = allow_lds((const void*)d2p_kernel<false>, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(d2p_kernel<false>, dim3((unsigned)((rows + DT - 1) / DT), (unsigned)((N + DT - 1) / DT)), dim3(THREADS), lds,
                     (hipStream_t)s, x, p, a, log_scale, out, (const float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                     rows, K, N, flags);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad_dist2plane_bwd(const float* x, const float* p, const float* a, const float* log_scale, const float* out, const float* grad_out,
                         float* grad_x, float* grad_p, float* grad_a, float* grad_log_scale, void* workspace, size_t workspace_bytes,
                         int64_t rows, int K, int N, int flags, hypad_stream_t s) {
  (void)out;                                               // (the coefficients need the un-scaled distance: recomputed with them)
  int rc = d2p_check(p, a, rows, K, N, flags);
  if (rc) return rc;
  if (grad_log_scale && !log_scale) return HYPAD_EINVAL;
  // (the contractions' LDS is that of hypad_linear_act_bwd at 2N outputs: refused here, before anything has been written)
  if ((size_t)16 * ((size_t)((K + 3) & ~3) + 4 + (size_t)((2 * (size_t)N + 3) & ~(size_t)3) + 4) * sizeof(float) > 150 * 1024) return HYPAD_EUNSUPPORTED;
  hipStream_t st = (hipStream_t)s;
  if (rows == 0) {                                         // an empty batch: the sums over no rows are zeros
    rc = d2p_zero(grad_p, (size_t)N * K, st);
    if (!rc) rc = d2p_zero(grad_a, (size_t)N * K, st);
    return rc ? rc : d2p_zero(grad_log_scale, (size_t)N, st);
  }
  if (!x || !grad_out) return HYPAD_EINVAL;
  if (!grad_x && !grad_p && !grad_a && !grad_log_scale) return HYPAD_OK;
  const D2PWorkspace w = d2p_workspace(rows, K, N);
  if (!workspace || workspace_bytes < w.total * sizeof(float)) return HYPAD_EWORKSPACE;
  float* ws = (float*)workspace;
  const size_t lds = d2p_lds(K, true);
  hipError_t e = allow_lds((const void*)d2p_kernel<true>, lds);
  if (e != hipSuccess) return (int)e;
  const int64_t tiles = (rows + DT - 1) / DT;
  hipLaunchKernelGGL(d2p_kernel<true>, dim3((unsigned)tiles, 1), dim3(THREADS), lds, st, x, p, a, log_scale, (float*)nullptr, grad_out,
                     ws + w.ccat, ws + w.cx2, ws + w.part, rows, K, N, flags);
  HYPAD_CHECK_LAUNCH();
  const bool planes = grad_p || grad_a;
  if (grad_x) {
    // grad_x = [C_px | C_xa] [P ; A]
    const size_t nk = (size_t)N * K;
    const size_t blocks = (2 * nk + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(d2p_stack_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(THREADS), 0, st, p, a, ws + w.wcat, nk);
    HYPAD_CHECK_LAUNCH();
    rc = hypad_linear_act_bwd(nullptr, ws + w.wcat, nullptr, ws + w.ccat, grad_x, nullptr, nullptr, nullptr, rows, K, 2 * N,
                              HYPAD_ACT_NONE, s);
    if (rc) return rc;
    hipLaunchKernelGGL(d2p_finish_rows, dim3(row_blocks(rows)), dim3(THREADS), 0, st, x, ws + w.cx2, grad_x, rows, K);
    HYPAD_CHECK_LAUNCH();
  }
  if (planes) {
    const int ntile = ((2 * N + 15) / 16) * ((K + 15) / 16);
    hipLaunchKernelGGL(d2p_outer_kernel, dim3((ntile + THREADS / 64 - 1) / (THREADS / 64), w.slices), dim3(THREADS), 0, st, ws + w.ccat, x,
                       ws + w.wpart, rows, w.slice_rows, K, 2 * N);
    HYPAD_CHECK_LAUNCH();
  }
  if (planes || grad_log_scale) {
    hipLaunchKernelGGL(d2p_finish_planes, dim3(row_blocks(N)), dim3(THREADS), 0, st, p, a, ws + w.wpart, w.slices, ws + w.part, tiles,
                       grad_p, grad_a, grad_log_scale, K, N);
    HYPAD_CHECK_LAUNCH();
  }
  return HYPAD_OK;
}

}  // extern "C"
