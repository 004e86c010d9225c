// Hyperbolic attention at k = -1: per query the gyromidpoint of the values under softmax_j(-beta d(q_i, keys_j) + bias_ij) -- the
// composition of dist_matmul (math_.py:905-947), a softmax over the keys and weighted_midpoint_bmm without lincomb (:2090-2122) with no
// N x M tensor in memory, forward or backward.  q (batch, N, D), keys (batch, M, D), values (batch, M, E), bias NULL or (N, M) at a batch
// stride in elements (0: one bias for every batch element; -inf is the mask), out (batch, N, E).
//
//   d_ij = dist_pair_d(|q_i|^2, |keys_j|^2, <q_i, keys_j>)     s_ij = -beta d_ij + bias_ij     L_i = logsumexp_j s_ij     p_ij = exp(s_ij - L_i)
//   gamma_j = 2 / max(1 - |v_j|^2, 1e-15)    c_j = gamma_j - 1    nom_i = sum_j p_ij gamma_j v_j    den_i = sum_j p_ij c_j
//   out_i = midpoint_tail_d(nom_i, den_i): halve, no lincomb, project, max(den, 1e-10)
// A row whose every s_ij is -inf: out_i = 0, L_i = -inf, nothing to any gradient (the composition gives NaN there).
//
// The shape of a workgroup.  The pair terms (a division, a square root, two log1p and an exp in fp64 per pair) bound these kernels, so
// the pairs are spread over as many waves as the shape gives: a workgroup of four waves owns SIXTEEN rows, and the four waves split the
// 64 points of a chunk among them -- wave w forms the pair terms of the points 16 w .. 16 w + 15, one 16 x 16 MFMA tile -- and split the
// columns of the accumulators in the products (wave w: the 16-column tiles w, w + 4, ...).  What a row needs from all four waves goes
// through LDS in a fixed order.  (With dist.hip's shape, 64 rows a workgroup and 16 rows x 64 points a wave, batch 8, N = M = 1024 gives
// 512 waves for 1 024 SIMDs and ran 398 us forward; 32 rows a workgroup with the same 16 x 64 a wave, still 512 waves: 551 us.)
//
// Forward: ONE launch, a workgroup per (batch element, 16 query rows), the query tile resident in LDS.  It walks keys and values in
// chunks of 64 points: both chunks staged once, |k_j|^2 and 1 - |v_j|^2 from fp64 sums of the staged fp32, the values scaled to
// gamma_j v_j in place, <q, k> on fp32 MFMA, d, s and exp in fp64 registers, the weights tile as fp32 in LDS, weights x values on MFMA.
// ONE walk with a running maximum: the maximum of a row over the chunk is combined over the sixteen lanes and then over the four waves
// (LDS); every thread keeps the running maximum m_i of its four rows and its own share of the running sum and of den in fp64; when m_i
// rises, the accumulators of the row and the two sums are multiplied by exp(m_old - m_new).  nom / den does not depend on the scale, so
// the division by the sum comes once, in the epilogue.  The training form stores saved (batch, N, E + 1) = [nom | den] (of the
// normalised weights) and L (batch, N); the epilogue starts from those fp32 values in either form, so inference has the same bits.
//
// Backward, with g_s_i (E values) and g_d_i the gradients of nom_i and den_i (rowops.h: midpoint_tail_bwd_d):
//   delta_i = <g_s_i, nom_i> + g_d_i den_i       gw_ij = gamma_j <g_s_i, v_j> + g_d_i c_j       gs_ij = p_ij (gw_ij - delta_i)       g_ij = -beta gs_ij
//   grad_v_j = gamma_j G_j + gamma_j^2 (<G_j, v_j> + h_j) v_j,   G_j = sum_i p_ij g_s_i,   h_j = sum_i p_ij g_d_i   (second term 0 on the clamp)
//   grad_q_i = sum_j P_ij k_j + 2 q_i sum_j (a_ij + b_ij |k_j|^2)      grad_k_j = sum_i P_ij q_i + 2 k_j sum_i (a_ij + b_ij |q_i|^2)
// with a, b, P = -2 (a + b) of dist_pair_bwd_d under g_ij.  (1) a row pass, a wave per query row, writes [g_s | g_d | delta] to the
// workspace (batch, N, E + 2); (2) one launch for grad_q: a workgroup owns 16 query rows and their g_s rows and walks keys and values;
// (3) one launch for grad_keys and grad_values: a workgroup owns 16 keys and values and walks the queries and their g_s rows -- p is
// recomputed once for both, the weights tile holds p for the product with g_s and then P for the product with q.  A gradient that is
// not asked for skips its product and changes nothing in the others.  No atomics: every sum has one owner and a fixed order.
//
// Dynamic LDS of one workgroup, C = 64 or 128 columns for max(D, E) <= 64, 128:
//   forward             4 ((16 + 2 64) (C + 4) + 16 68 + 32) + 8 336 bytes          -- q, keys chunk, values chunk, weights, den and L; the norms, c_j, the waves' row terms:   83 200 at C = 128
//   grad_q              4 ((2 16 + 2 64) (C + 4) + 16 68) + 8 272 bytes             -- q, g_s, the two chunks, weights; the norms, gamma, c, the waves' row sums:                 91 008
//   grad_keys / values  4 ((2 16 + 2 64) (C + 4) + 16 68 + 3 64) + 8 240 bytes      -- keys, values, q chunk, g_s chunk, weights; L, g_d, delta; norms and row sums:              91 520
// checked against gfx950's 160 KiB per workgroup before anything is launched.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/hypad.h"
#include "rowops.h"

using namespace hypad;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MT = 16;                                  // rows of a workgroup's tile
constexpr int KC = 16 * WAVES;                          // points of the walked operands staged at a time, 16 per wave
constexpr int LDP = KC + 4;
constexpr int MAX_W = 128;                              // D and E
constexpr size_t LDS_LIMIT = 160 * 1024;                // a gfx950 workgroup's LDS
constexpr int64_t INT_LIMIT = 0x7fffffff;
constexpr double GAMMA_EPS = 1e-15;                     // math_.py:383
using RW = RowD<64, 2>;                                 // a row of at most 128 elements per wave
#define HYPAD_NEG_INF (-__builtin_huge_val())

inline int nt_of(int D, int E) { return (D > E ? D : E) <= 64 ? 4 : 8; }
inline size_t fwd_lds(int nt) { return (size_t)((MT + 2 * KC) * (nt * 16 + 4) + MT * LDP + 2 * MT) * sizeof(float) + (MT + 5 * KC) * sizeof(double); }
inline size_t gq_lds(int nt) { return (size_t)((2 * MT + 2 * KC) * (nt * 16 + 4) + MT * LDP) * sizeof(float) + (MT + 4 * KC) * sizeof(double); }
inline size_t gkv_lds(int nt) {
  return (size_t)((2 * MT + 2 * KC) * (nt * 16 + 4) + MT * LDP + 3 * KC) * sizeof(float) + (3 * MT + 3 * KC) * sizeof(double);
}

// ROWS rows of `width` columns from row `first` of a (count, ld) matrix into a [ROWS][LDB] tile, zeros past either edge
template <int NT, int ROWS>
__device__ __forceinline__ void stage_rows(float* __restrict__ tile, const float* __restrict__ src, int first, int count, int width, size_t ld, int wave,
                                           int lane) {
  constexpr int LDB = NT * 16 + 4;
  for (int r = wave; r < ROWS; r += WAVES)
    for (int c = lane; c < NT * 16; c += 64) tile[r * LDB + c] = (first + r < count && c < width) ? src[(size_t)(first + r) * ld + c] : 0.f;
}
// |row|^2 of row tid / 4 of a staged tile, four threads a row, in fp64 (complete in every one of the four)
__device__ __forceinline__ double tile_row_sq(const float* __restrict__ tile, int ld, int cols, int tid) {
  const float* p = tile + (tid >> 2) * ld;
  double s = 0.0;
  for (int c = tid & 3; c < cols; c += 4) { const double v = p[c]; s += v * v; }
  s += __shfl_xor(s, 1, WAVE);
  return s + __shfl_xor(s, 2, WAVE);
}
__device__ __forceinline__ double group16_max(double v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, WAVE));
  return v;
}
// the sum over the four waves of what each left for row `row`, in wave order
__device__ __forceinline__ double waves_sum(const double* __restrict__ w, int row) { return ((w[row] + w[MT + row]) + w[2 * MT + row]) + w[3 * MT + row]; }
// the 16 own rows x the 16 rows b0 .. b0 + 15 of the other tile, contraction over the first `cols4` columns: [r] = (row 4 q + r, row b0 + j of b)
template <int LDB>
__device__ __forceinline__ f32x4 tile_dots(const float* __restrict__ a, const float* __restrict__ b, int cols4, int b0, int j, int q) {
  f32x4 xy = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kk = 0; kk < cols4; kk += 4) xy = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j * LDB + kk + q], b[(b0 + j) * LDB + kk + q], xy, 0, 0, 0);
  return xy;
}
// acc += weights tile (the 16 own rows x positions) times the chunk (positions x columns), the column tiles wave, wave + 4, ...
template <int NT>
__device__ __forceinline__ void tile_product(const float* __restrict__ ps, const float* __restrict__ bs, int kw4, int wave, int j, int q,
                                             f32x4 (&acc)[NT / WAVES]) {
  constexpr int LDB = NT * 16 + 4;
  for (int kk = 0; kk < kw4; kk += 4) {
    const float a = ps[j * LDP + kk + q];
    const float* bp = bs + (kk + q) * LDB + wave * 16 + j;
#pragma unroll
    for (int t = 0; t < NT / WAVES; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[t * WAVES * 16], acc[t], 0, 0, 0);
  }
}
// the (N, M) bias tile of the rows i0 .. and the columns k0 .. into ps[row][column], threads along the columns
__device__ __forceinline__ void stage_bias(float* __restrict__ ps, const float* __restrict__ bias, int i0, int N, int k0, int kw, int M, int tid) {
  for (int e = tid; e < MT * KC; e += THREADS) {
    const int r = e / KC, c = e % KC;
    ps[r * LDP + c] = (c < kw && i0 + r < N) ? bias[(size_t)(i0 + r) * M + k0 + c] : 0.f;
  }
}

// CV... here and below: the launch's curvature -- nothing at k = -1, one Curv at k = -c (rowops.h): d_c in the scores, gamma_j = 2 / max(1 -
// c |v_j|^2, 1e-15) with d gamma / d v = c gamma^2 v, the tail of the midpoint at c, dL/dxy = -2 (a + b) and dL/d|q|^2 = a + b (c |k|^2).
template <int NT, class... CV>
__global__ __launch_bounds__(THREADS) void attn_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                            const float* __restrict__ bias, int64_t bias_bs, double beta, float* __restrict__ out,
                                                            float* __restrict__ saved, float* __restrict__ lse, int N, int M, int D, int E, int tiles,
                                                            CV... cv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDB = NT * 16 + 4, NA = NT / WAVES;
  float* qt = smem;                                     // [MT][LDB] the query rows, resident
  float* ks = qt + MT * LDB;                            // [KC][LDB] keys of the chunk; after the walk [MT][LDB] nom
  float* vs = ks + KC * LDB;                            // [KC][LDB] values of the chunk, then gamma_j v_j
  float* ps = vs + KC * LDB;                            // [MT][LDP] bias, then the weights exp(s - m)
  float* dens = ps + MT * LDP;                          // [MT] den, [MT] L
  float* Lrow = dens + MT;
  double* q2s = (double*)(Lrow + MT);                   // [MT] |q_i|^2, [KC] |k_j|^2, [KC] c_j
  double* k2s = q2s + MT;
  double* cjs = k2s + KC;
  double* wmx = cjs + KC;                               // [WAVES][MT] each: the waves' row maxima of the chunk, their shares of the sum and of den
  double* wls = wmx + WAVES * MT;
  double* wdn = wls + WAVES * MT;
  using R = RowD<16, NT>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / tiles, i0 = (blockIdx.x % tiles) * MT;
  Q += (size_t)b * N * D;
  K += (size_t)b * M * D;
  V += (size_t)b * M * E;
  if (bias) bias += (size_t)b * (size_t)bias_bs;
  stage_rows<NT, MT>(qt, Q, i0, N, D, (size_t)D, wave, lane);
  __syncthreads();
  if (wave == 0) {
    const double s = tile_row_sq(qt, LDB, D, tid);
    if ((tid & 3) == 0) q2s[tid >> 2] = s;
  }
  f32x4 acc[NA];
#pragma unroll
  for (int t = 0; t < NA; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  double mx[4], ls[4], dn[4];                           // of the rows 4 q + r: the running maximum; this thread's share (its point of every chunk) of the two sums
#pragma unroll
  for (int r = 0; r < 4; ++r) { mx[r] = HYPAD_NEG_INF; ls[r] = 0.0; dn[r] = 0.0; }
  const int d4 = (D + 3) & ~3, lc = wave * 16 + j;
  for (int k0 = 0; k0 < M; k0 += KC) {
    const int kw = M - k0 < KC ? M - k0 : KC, kw4 = (kw + 3) & ~3;
    __syncthreads();                                    // the readers of the previous chunk are done
    stage_rows<NT, KC>(ks, K, k0, M, D, (size_t)D, wave, lane);
    stage_rows<NT, KC>(vs, V, k0, M, E, (size_t)E, wave, lane);
    if (bias) stage_bias(ps, bias, i0, N, k0, kw, M, tid);
    __syncthreads();
    {                                                   // four threads a point
      const double s = tile_row_sq(ks, LDB, D, tid);
      float* p = vs + (tid >> 2) * LDB;
      const double g = 2.0 / fmax(1.0 - curv_mul(tile_row_sq(vs, LDB, E, tid), cv...), GAMMA_EPS);
      for (int c = tid & 3; c < E; c += 4) p[c] = (float)(g * (double)p[c]);
      if ((tid & 3) == 0) { k2s[tid >> 2] = s; cjs[tid >> 2] = g - 1.0; }
    }
    const f32x4 xy = tile_dots<LDB>(qt, ks, d4, wave * 16, j, q);
    __syncthreads();                                    // |q_i|^2, |k_j|^2, c_j and gamma_j v_j are in LDS
    double sv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = 4 * q + r;
      sv[r] = HYPAD_NEG_INF;
      if (lc < kw) sv[r] = -beta * dist_pair_d(q2s[lr], k2s[lc], (double)xy[r], cv...) + (bias ? (double)ps[lr * LDP + lc] : 0.0);
      const double top = group16_max(sv[r]);
      if (j == 0) wmx[wave * MT + lr] = top;
    }
    __syncthreads();                                    // the four waves' maxima are in LDS
    const double cj = cjs[lc];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = 4 * q + r;
      const double mn = fmax(fmax(mx[r], fmax(wmx[lr], wmx[MT + lr])), fmax(wmx[2 * MT + lr], wmx[3 * MT + lr]));
      const bool none = mn == HYPAD_NEG_INF;            // nothing but -inf so far: the sums are zero and stay
      const double sc = (none || mn == mx[r]) ? 1.0 : exp(mx[r] - mn);
      const float pf = none ? 0.f : (float)exp(sv[r] - mn);
      ps[lr * LDP + lc] = pf;
      ls[r] = ls[r] * sc + (double)pf;
      dn[r] = dn[r] * sc + (double)pf * cj;
      if (sc != 1.0) {
        const float scf = (float)sc;
#pragma unroll
        for (int t = 0; t < NA; ++t) acc[t][r] *= scf;
      }
      mx[r] = mn;
    }
    __syncthreads();                                    // the weights are in LDS
    tile_product<NT>(ps, vs, kw4, wave, j, q, acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double lsum = groupd_sum<16>(ls[r]), dsum = groupd_sum<16>(dn[r]);
    if (j == 0) { wls[wave * MT + 4 * q + r] = lsum; wdn[wave * MT + 4 * q + r] = dsum; }
  }
  __syncthreads();                                      // the waves' shares are in LDS; the last chunk's readers are done
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lr = 4 * q + r;
    const double lsum = waves_sum(wls, lr), dsum = waves_sum(wdn, lr);
    const double inv = lsum > 0.0 ? 1.0 / lsum : 0.0;
#pragma unroll
    for (int t = 0; t < NA; ++t) ks[lr * LDB + (wave + t * WAVES) * 16 + j] = (float)((double)acc[t][r] * inv);
    if (wave == 0 && j == 0) {
      dens[lr] = (float)(dsum * inv);
      Lrow[lr] = lsum > 0.0 ? (float)(mx[r] + log(lsum)) : (float)HYPAD_NEG_INF;
    }
  }
  __syncthreads();                                      // nom, den and L of the 16 rows are in LDS
  {                                                     // row 4 wave + q, sixteen lanes a row
    const int lr = 4 * wave + q, gi = i0 + lr;
    const bool rv = gi < N;
    const float denf = dens[lr];
    R v;
#pragma unroll
    for (int t = 0; t < NT; ++t) v.v[t] = (double)ks[lr * LDB + t * 16 + j];
    if (saved && rv) {
      float* sp = saved + ((size_t)b * N + gi) * (E + 1);
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t * 16 + j < E) sp[t * 16 + j] = (float)v.v[t];
      if (j == 0) { sp[E] = denf; lse[(size_t)b * N + gi] = Lrow[lr]; }
    }
    const R o = midpoint_tail_d(v, (double)denf, 0.0, MidpointCfg{true, false, true, false}, cv...);
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (rv && t * 16 + j < E) out[((size_t)b * N + gi) * E + t * 16 + j] = (float)o.v[t];
  }
}

// The row pass of the backward, a wave per query row: from saved = [nom | den], L and grad_out to [g_s | g_d | delta] (rows, E + 2).
// A row without a finite score (L = -inf) gets zeros.
template <class... CV>
__global__ __launch_bounds__(THREADS) void attn_rows_bwd(const float* __restrict__ saved, const float* __restrict__ lse, const float* __restrict__ go,
                                                          float* __restrict__ ws, int64_t rows, int E, CV... cv) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    const float* sp = saved + r * (E + 1);
    const RW nom = rowd_load<RW>(sp, E, lane);
    const double den = (double)sp[E];
    RW gnom;
    double gden, gr;
    midpoint_tail_bwd_d(nom, den, 0.0, MidpointCfg{true, false, true, false}, rowd_load<RW>(go + r * E, E, lane), gnom, gden, gr, cv...);
    double delta = rowd_dot(gnom, nom) + gden * den;
    if (lse[r] == (float)HYPAD_NEG_INF) {
#pragma unroll
      for (int e = 0; e < RW::EPL; ++e) gnom.v[e] = 0.0;
      gden = 0.0;
      delta = 0.0;
    }
    float* wp = ws + r * (E + 2);
    rowd_store(wp, gnom, E, lane);
    if (lane == 0) { wp[E] = (float)gden; wp[E + 1] = (float)delta; }
  }
}

// One pair of the backward: the weight p, and under g = -beta p (gw - delta) the pair terms a, b of dist_pair_bwd_d.  x2 is the query's.
template <class... CV>
__device__ __forceinline__ float pair_bwd(double x2, double y2, double xy, double bias, double beta, double L, double gw, double delta, double& a,
                                          double& b, CV... cv) {
  const float pf = (float)exp(-beta * dist_pair_d(x2, y2, xy, cv...) + bias - L);
  dist_pair_bwd_d(x2, y2, xy, -beta * (double)pf * (gw - delta), a, b, cv...);
  return pf;
}

template <int NT, class... CV>
__global__ __launch_bounds__(THREADS) void attn_gradq_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                              const float* __restrict__ bias, int64_t bias_bs, double beta,
                                                              const float* __restrict__ lse, const float* __restrict__ ws, float* __restrict__ grad,
                                                              int N, int M, int D, int E, int tiles, CV... cv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDB = NT * 16 + 4, NA = NT / WAVES;
  float* qt = smem;                                     // [MT][LDB] the query rows, resident
  float* gt = qt + MT * LDB;                            // [MT][LDB] their g_s rows, resident
  float* ks = gt + MT * LDB;                            // [KC][LDB] keys of the chunk
  float* vs = ks + KC * LDB;                            // [KC][LDB] values of the chunk
  float* ps = vs + KC * LDB;                            // [MT][LDP] bias, then P
  double* q2s = (double*)(ps + MT * LDP);               // [MT] |q_i|^2, then [KC] each: |k_j|^2, gamma_j, c_j
  double* k2s = q2s + MT;
  double* gms = k2s + KC;
  double* cjs = gms + KC;
  double* wrs = cjs + KC;                               // [WAVES][MT] the waves' shares of the row sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / tiles, i0 = (blockIdx.x % tiles) * MT;
  Q += (size_t)b * N * D;
  K += (size_t)b * M * D;
  V += (size_t)b * M * E;
  ws += (size_t)b * N * (E + 2);
  lse += (size_t)b * N;
  if (bias) bias += (size_t)b * (size_t)bias_bs;
  stage_rows<NT, MT>(qt, Q, i0, N, D, (size_t)D, wave, lane);
  stage_rows<NT, MT>(gt, ws, i0, N, E, (size_t)(E + 2), wave, lane);
  __syncthreads();
  if (wave == 0) {
    const double s = tile_row_sq(qt, LDB, D, tid);
    if ((tid & 3) == 0) q2s[tid >> 2] = s;
  }
  double Lr[4], gdr[4], dlr[4];                         // of the rows 4 q + r
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gi = i0 + 4 * q + r;
    const bool rv = gi < N;
    Lr[r] = rv ? (double)lse[gi] : HYPAD_NEG_INF;
    gdr[r] = rv ? (double)ws[(size_t)gi * (E + 2) + E] : 0.0;
    dlr[r] = rv ? (double)ws[(size_t)gi * (E + 2) + E + 1] : 0.0;
  }
  f32x4 acc[NA];
#pragma unroll
  for (int t = 0; t < NA; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  double rs[4] = {0.0, 0.0, 0.0, 0.0};                  // sum_j (a + b |k_j|^2) of the rows, this thread's point of every chunk
  const int d4 = (D + 3) & ~3, e4 = (E + 3) & ~3, lc = wave * 16 + j;
  for (int k0 = 0; k0 < M; k0 += KC) {
    const int kw = M - k0 < KC ? M - k0 : KC, kw4 = (kw + 3) & ~3;
    __syncthreads();                                    // the readers of the previous chunk are done
    stage_rows<NT, KC>(ks, K, k0, M, D, (size_t)D, wave, lane);
    stage_rows<NT, KC>(vs, V, k0, M, E, (size_t)E, wave, lane);
    if (bias) stage_bias(ps, bias, i0, N, k0, kw, M, tid);
    __syncthreads();
    {                                                   // four threads a point
      const double s = tile_row_sq(ks, LDB, D, tid);
      const double g = 2.0 / fmax(1.0 - curv_mul(tile_row_sq(vs, LDB, E, tid), cv...), GAMMA_EPS);
      if ((tid & 3) == 0) { k2s[tid >> 2] = s; gms[tid >> 2] = g; cjs[tid >> 2] = g - 1.0; }
    }
    const f32x4 xy = tile_dots<LDB>(qt, ks, d4, wave * 16, j, q), gv = tile_dots<LDB>(gt, vs, e4, wave * 16, j, q);
    __syncthreads();                                    // the norms are in LDS
    const double kk2 = k2s[lc], gm = gms[lc], cj = cjs[lc];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = 4 * q + r;
      const double bv = bias ? (double)ps[lr * LDP + lc] : 0.0;
      float P = 0.f;
      if (Lr[r] != HYPAD_NEG_INF && lc < kw && bv != HYPAD_NEG_INF) {
        double da, db;
        pair_bwd(q2s[lr], kk2, (double)xy[r], bv, beta, Lr[r], gm * (double)gv[r] + gdr[r] * cj, dlr[r], da, db, cv...);
        P = (float)(-2.0 * (da + db));
        rs[r] += da + db * curv_mul(kk2, cv...);
      }
      ps[lr * LDP + lc] = P;
    }
    __syncthreads();                                    // P is in LDS
    tile_product<NT>(ps, ks, kw4, wave, j, q, acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double s = groupd_sum<16>(rs[r]);
    if (j == 0) wrs[wave * MT + 4 * q + r] = s;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lr = 4 * q + r, gi = i0 + lr;
    const double s = 2.0 * waves_sum(wrs, lr);
#pragma unroll
    for (int t = 0; t < NA; ++t) {
      const int c = (wave + t * WAVES) * 16 + j;
      if (gi < N && c < D) grad[((size_t)b * N + gi) * D + c] = (float)((double)acc[t][r] + s * (double)qt[lr * LDB + c]);
    }
  }
}

// grad_keys and grad_values of 16 keys and values against the N queries of their batch element; either may be NULL.
template <int NT, class... CV>
__global__ __launch_bounds__(THREADS) void attn_gradkv_kernel(const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
                                                               const float* __restrict__ bias, int64_t bias_bs, double beta,
                                                               const float* __restrict__ lse, const float* __restrict__ ws, float* __restrict__ gk,
                                                               float* __restrict__ gvl, int N, int M, int D, int E, int tiles, CV... cv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LDB = NT * 16 + 4, NA = NT / WAVES;
  float* kt = smem;                                     // [MT][LDB] the keys, resident
  float* vt = kt + MT * LDB;                            // [MT][LDB] the values, resident
  float* qs = vt + MT * LDB;                            // [KC][LDB] queries of the chunk; after the walk [MT][LDB] G
  float* gs = qs + KC * LDB;                            // [KC][LDB] their g_s rows
  float* ps = gs + KC * LDB;                            // [MT][LDP] bias (read transposed), then p, then P
  float* Ls = ps + MT * LDP;                            // [KC] L_i, g_d_i, delta_i of the chunk
  float* gds = Ls + KC;
  float* dls = gds + KC;
  double* k2s = (double*)(dls + KC);                    // [MT] |k_j|^2, gamma_j, c_j, [KC] |q_i|^2
  double* gms = k2s + MT;
  double* cjs = gms + MT;
  double* q2s = cjs + MT;
  double* wrs = q2s + KC;                               // [WAVES][MT] each: the waves' shares of the two row sums
  double* whs = wrs + WAVES * MT;
  using R = RowD<16, NT>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, q = lane >> 4;
  const int b = blockIdx.x / tiles, j0 = (blockIdx.x % tiles) * MT;
  Q += (size_t)b * N * D;
  K += (size_t)b * M * D;
  V += (size_t)b * M * E;
  ws += (size_t)b * N * (E + 2);
  lse += (size_t)b * N;
  if (bias) bias += (size_t)b * (size_t)bias_bs;
  stage_rows<NT, MT>(kt, K, j0, M, D, (size_t)D, wave, lane);
  stage_rows<NT, MT>(vt, V, j0, M, E, (size_t)E, wave, lane);
  __syncthreads();
  if (wave == 0) {
    const double s = tile_row_sq(kt, LDB, D, tid);
    const double g = 2.0 / fmax(1.0 - curv_mul(tile_row_sq(vt, LDB, E, tid), cv...), GAMMA_EPS);
    if ((tid & 3) == 0) { k2s[tid >> 2] = s; gms[tid >> 2] = g; cjs[tid >> 2] = g - 1.0; }
  }
  f32x4 ack[NA], acv[NA];
#pragma unroll
  for (int t = 0; t < NA; ++t) { ack[t] = f32x4{0.f, 0.f, 0.f, 0.f}; acv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  double rs[4] = {0.0, 0.0, 0.0, 0.0}, hs[4] = {0.0, 0.0, 0.0, 0.0};      // sum_i (a + b |q_i|^2) and sum_i p g_d_i of the rows, this thread's query of every chunk
  const int d4 = (D + 3) & ~3, e4 = (E + 3) & ~3, lc = wave * 16 + j;
  for (int n0 = 0; n0 < N; n0 += KC) {
    const int kw = N - n0 < KC ? N - n0 : KC, kw4 = (kw + 3) & ~3;
    __syncthreads();                                    // the readers of the previous chunk are done (and the own norms are in LDS)
    stage_rows<NT, KC>(qs, Q, n0, N, D, (size_t)D, wave, lane);
    stage_rows<NT, KC>(gs, ws, n0, N, E, (size_t)(E + 2), wave, lane);
    if (bias)
      for (int e = tid; e < MT * KC; e += THREADS) {      // ps[own key j][query i] = bias[i][j]: threads along j
        const int jj = e % MT, c = e / MT;
        ps[jj * LDP + c] = (c < kw && j0 + jj < M) ? bias[(size_t)(n0 + c) * M + j0 + jj] : 0.f;
      }
    if (tid < KC) {
      const bool v = tid < kw;
      Ls[tid] = v ? lse[n0 + tid] : (float)HYPAD_NEG_INF;
      gds[tid] = v ? ws[(size_t)(n0 + tid) * (E + 2) + E] : 0.f;
      dls[tid] = v ? ws[(size_t)(n0 + tid) * (E + 2) + E + 1] : 0.f;
    }
    __syncthreads();
    {                                                   // four threads a query
      const double s = tile_row_sq(qs, LDB, D, tid);
      if ((tid & 3) == 0) q2s[tid >> 2] = s;
    }
    const f32x4 xy = tile_dots<LDB>(kt, qs, d4, wave * 16, j, q), gv = tile_dots<LDB>(vt, gs, e4, wave * 16, j, q);
    __syncthreads();                                    // |q_i|^2 of the chunk is in LDS
    const double L = (double)Ls[lc], qq = q2s[lc], gd = (double)gds[lc], dl = (double)dls[lc];
    f32x4 Pr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = 4 * q + r;
      const double bv = bias ? (double)ps[lr * LDP + lc] : 0.0;
      float pf = 0.f, P = 0.f;
      if (L != HYPAD_NEG_INF && bv != HYPAD_NEG_INF) {
        const double kk2 = k2s[lr];
        double da, db;
        pf = pair_bwd(qq, kk2, (double)xy[r], bv, beta, L, gms[lr] * (double)gv[r] + gd * cjs[lr], dl, da, db, cv...);
        P = (float)(-2.0 * (da + db));
        rs[r] += da + db * curv_mul(qq, cv...);
        hs[r] += (double)pf * gd;
      }
      ps[lr * LDP + lc] = pf;
      Pr[r] = P;
    }
    __syncthreads();                                    // p is in LDS
    if (gvl) tile_product<NT>(ps, gs, kw4, wave, j, q, acv);
    if (gk) {
      __syncthreads();                                  // the readers of p are done
#pragma unroll
      for (int r = 0; r < 4; ++r) ps[(4 * q + r) * LDP + lc] = Pr[r];
      __syncthreads();                                  // P is in LDS
      tile_product<NT>(ps, qs, kw4, wave, j, q, ack);
    }
  }
  __syncthreads();                                      // the last chunk's readers are done
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lr = 4 * q + r;
    const double s = groupd_sum<16>(rs[r]), h = groupd_sum<16>(hs[r]);
    if (j == 0) { wrs[wave * MT + lr] = s; whs[wave * MT + lr] = h; }
#pragma unroll
    for (int t = 0; t < NA; ++t) qs[lr * LDB + (wave + t * WAVES) * 16 + j] = acv[t][r];
  }
  __syncthreads();                                      // the row sums and G are in LDS
  if (gk) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = 4 * q + r, gj = j0 + lr;
      const double s = 2.0 * waves_sum(wrs, lr);
#pragma unroll
      for (int t = 0; t < NA; ++t) {
        const int c = (wave + t * WAVES) * 16 + j;
        if (gj < M && c < D) gk[((size_t)b * M + gj) * D + c] = (float)((double)ack[t][r] + s * (double)kt[lr * LDB + c]);
      }
    }
  }
  if (gvl) {                                            // row 4 wave + q, sixteen lanes a row
    const int lr = 4 * wave + q, gj = j0 + lr;
    const double h = waves_sum(whs, lr);
    R G, x;
#pragma unroll
    for (int t = 0; t < NT; ++t) { G.v[t] = (double)qs[lr * LDB + t * 16 + j]; x.v[t] = (double)vt[lr * LDB + t * 16 + j]; }
    const double om = 1.0 - curv_mul(rowd_dot(x, x), cv...);
    const double g = 2.0 / fmax(om, GAMMA_EPS);
    const double s2 = om >= GAMMA_EPS ? curv_mul(g * g * (rowd_dot(G, x) + h), cv...) : 0.0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int c = t * 16 + j;
      if (gj < M && c < E) gvl[((size_t)b * M + gj) * E + c] = (float)(g * G.v[t] + s2 * x.v[t]);
    }
  }
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
// the sizes: every element count and every grid below 2^31, the LDS of every launch within the limit
inline int attn_check(int64_t batch, int64_t N, int64_t M, int D, int E, double beta) {
  if (batch < 0 || N < 0 || M < 0 || D <= 0 || E <= 0 || !std::isfinite(beta)) return HYPAD_EINVAL;
  if (M == 0 && batch > 0 && N > 0) return HYPAD_EINVAL;                 // a midpoint of no points
  if (D > MAX_W || E > MAX_W) return HYPAD_EUNSUPPORTED;
  if (batch > INT_LIMIT || N > INT_LIMIT || M > INT_LIMIT) return HYPAD_EUNSUPPORTED;
  const int64_t w = (D > E ? D : E) + 2;
  if (batch > 0 && (N * M > INT_LIMIT / batch || N * w > INT_LIMIT / batch || M * w > INT_LIMIT / batch)) return HYPAD_EUNSUPPORTED;
  const int nt = nt_of(D, E);
  if (fwd_lds(nt) > LDS_LIMIT || gq_lds(nt) > LDS_LIMIT || gkv_lds(nt) > LDS_LIMIT) return HYPAD_EUNSUPPORTED;
  return HYPAD_OK;
}
inline size_t attn_workspace_floats(int64_t batch, int64_t N, int E) { return (size_t)batch * (size_t)N * (size_t)(E + 2); }

#define HYPAD_ATTN_LAUNCH(kernel, lds, grid, st, ...)                                        \
  do {                                                                                       \
    if (nt == 4) {                                                                           \
      const hipError_t e = allow_lds((const void*)kernel<4, CV...>, lds);                    \
      if (e != hipSuccess) return (int)e;                                                    \
      hipLaunchKernelGGL((kernel<4, CV...>), grid, dim3(THREADS), lds, st, __VA_ARGS__);     \
    } else {                                                                                 \
      const hipError_t e = allow_lds((const void*)kernel<8, CV...>, lds);                    \
      if (e != hipSuccess) return (int)e;                                                    \
      hipLaunchKernelGGL((kernel<8, CV...>), grid, dim3(THREADS), lds, st, __VA_ARGS__);     \
    }                                                                                        \
    HYPAD_CHECK_LAUNCH();                                                                    \
  } while (0)

// the bodies of the entry points, at k = -1 (no cv) and at k = -c
template <class... CV>
int attn_fwd(const float* q, const float* keys, const float* values, const float* bias, int64_t bias_batch_stride, double beta, float* out,
             float* saved, float* lse, int64_t batch, int64_t N, int64_t M, int D, int E, hypad_stream_t s, CV... cv) {
  const int rc = attn_check(batch, N, M, D, E, beta);
  if (rc) return rc;
  if (bias && bias_batch_stride != 0 && bias_batch_stride != N * M) return HYPAD_EINVAL;
  if (batch == 0 || N == 0) return HYPAD_OK;
  if (!q || !keys || !values || !out || (saved == nullptr) != (lse == nullptr)) return HYPAD_EINVAL;
  const int64_t tiles = (N + MT - 1) / MT;
  if (tiles > INT_LIMIT / batch) return HYPAD_EUNSUPPORTED;
  const int nt = nt_of(D, E);
  const size_t lds = fwd_lds(nt);
  const dim3 grid((unsigned)(batch * tiles));
  HYPAD_ATTN_LAUNCH(attn_fwd_kernel, lds, grid, (hipStream_t)s, q, keys, values, bias, bias_batch_stride, beta, out, saved, lse, (int)N, (int)M, D, E,
                    (int)tiles, cv...);
  return HYPAD_OK;
}

template <class... CV>
int attn_bwd(const float* q, const float* keys, const float* values, const float* bias, int64_t bias_batch_stride, double beta, const float* saved,
             const float* lse, const float* grad_out, float* grad_q, float* grad_keys, float* grad_values, void* workspace, size_t workspace_bytes,
             int64_t batch, int64_t N, int64_t M, int D, int E, hypad_stream_t s, CV... cv) {
  const int rc = attn_check(batch, N, M, D, E, beta);
  if (rc) return rc;
  if (bias && bias_batch_stride != 0 && bias_batch_stride != N * M) return HYPAD_EINVAL;
  hipStream_t st = (hipStream_t)s;
  if (batch == 0 || N == 0) {                           // sums over no queries
    const int rk = zero_floats(grad_keys, (size_t)batch * M * D, st);
    return rk ? rk : zero_floats(grad_values, (size_t)batch * M * E, st);
  }
  if (!q || !keys || !values || !saved || !lse || !grad_out) return HYPAD_EINVAL;
  if (!grad_q && !grad_keys && !grad_values) return HYPAD_OK;
  if (!workspace || workspace_bytes < attn_workspace_floats(batch, N, E) * sizeof(float)) return HYPAD_EWORKSPACE;
  const int64_t tq = (N + MT - 1) / MT, tk = (M + MT - 1) / MT;
  if (tq > INT_LIMIT / batch || tk > INT_LIMIT / batch) return HYPAD_EUNSUPPORTED;
  const int nt = nt_of(D, E);
  float* ws = (float*)workspace;
  hipLaunchKernelGGL(attn_rows_bwd<CV...>, dim3(wave_grid(batch * N)), dim3(THREADS), 0, st, saved, lse, grad_out, ws, batch * N, E, cv...);
  HYPAD_CHECK_LAUNCH();
  if (grad_q) {
    const size_t lds = gq_lds(nt);
    const dim3 grid((unsigned)(batch * tq));
    HYPAD_ATTN_LAUNCH(attn_gradq_kernel, lds, grid, st, q, keys, values, bias, bias_batch_stride, beta, lse, (const float*)ws, grad_q, (int)N, (int)M,
                      D, E, (int)tq, cv...);
  }
  if (grad_keys || grad_values) {
    const size_t lds = gkv_lds(nt);
    const dim3 grid((unsigned)(batch * tk));
    HYPAD_ATTN_LAUNCH(attn_gradkv_kernel, lds, grid, st, q, keys, values, bias, bias_batch_stride, beta, lse, (const float*)ws, grad_keys,
                      grad_values, (int)N, (int)M, D, E, (int)tk, cv...);
  }
  return HYPAD_OK;
}

}  // namespace

extern "C" {

size_t hypad_hyp_attention_workspace_bytes(int64_t batch, int64_t N, int64_t M, int D, int E) {
  if (batch <= 0 || N <= 0 || M <= 0 || D <= 0 || E <= 0) return 0;
  return attn_workspace_floats(batch, N, E) * sizeof(float);
}

int hypad_hyp_attention_fwd(const float* q, const float* keys, const float* values, const float* bias, int64_t bias_batch_stride, double beta,
                            float* out, float* saved, float* lse, int64_t batch, int64_t N, int64_t M, int D, int E, hypad_stream_t s) {
  return attn_fwd(q, keys, values, bias, bias_batch_stride, beta, out, saved, lse, batch, N, M, D, E, s);
}
int hypad_hyp_attention_bwd(const float* q, const float* keys, const float* values, const float* bias, int64_t bias_batch_stride, double beta,
                            const float* saved, const float* lse, const float* grad_out, float* grad_q, float* grad_keys, float* grad_values,
                            void* workspace, size_t workspace_bytes, int64_t batch, int64_t N, int64_t M, int D, int E, hypad_stream_t s) {
  return attn_bwd(q, keys, values, bias, bias_batch_stride, beta, saved, lse, grad_out, grad_q, grad_keys, grad_values, workspace, workspace_bytes,
                  batch, N, M, D, E, s);
}
// the same at k = -c: c is checked first, then everything as above; hypad_hyp_attention_workspace_bytes serves both
int hypad_ball_hyp_attention_fwd(const float* q, const float* keys, const float* values, const float* bias, int64_t bias_batch_stride, double beta,
                                 float* out, float* saved, float* lse, int64_t batch, int64_t N, int64_t M, int D, int E, double c,
                                 hypad_stream_t s) {
  return curv_invalid(c) ? HYPAD_EINVAL
                  : attn_fwd(q, keys, values, bias, bias_batch_stride, beta, out, saved, lse, batch, N, M, D, E, s, curv_of(c));
}
int hypad_ball_hyp_attention_bwd(const float* q, const float* keys, const float* values, const float* bias, int64_t bias_batch_stride, double beta,
                                 const float* saved, const float* lse, const float* grad_out, float* grad_q, float* grad_keys, float* grad_values,
                                 void* workspace, size_t workspace_bytes, int64_t batch, int64_t N, int64_t M, int D, int E, double c,
                                 hypad_stream_t s) {
  return curv_invalid(c) ? HYPAD_EINVAL
                  : attn_bwd(q, keys, values, bias, bias_batch_stride, beta, saved, lse, grad_out, grad_q, grad_keys, grad_values, workspace,
                             workspace_bytes, batch, N, M, D, E, s, curv_of(c));
}

}  // extern "C"
