// Window-scoring kernels: utils/anomaly_detection_utils.py on the GPU.
// Post-processing arithmetic is fp64 because the reference computes it in NumPy/pandas fp64.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "../../include/hypad.h"
#include "device_utils.h"

using namespace hypad;

namespace {

// Occupancy (waves per SIMD the register allocator is asked to fit).
constexpr int UNROLL_WPE = 4;

constexpr int THREADS = 256;
constexpr int MAX_WINDOW = 256;

inline int grid_for(int64_t n, int per_block) {
  int64_t b = (n + per_block - 1) / per_block;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (int)b;
}

// ---- S1: anti-diagonal un-roll (:918-935).  One wave per output timestep: gather <= window values, rank them
// by counting (ties broken by position), scatter into sorted order in LDS, read the order statistics.
__device__ __forceinline__ float np_lerp(float a, float b, float t) {
  // numpy.lib._function_base_impl._lerp, evaluated in the data's precision (float32) as NumPy does
#pragma clang fp contract(off)                   // numpy rounds the product before the sum: no fused multiply-add here
  float diff = b - a;
  float r = a + diff * t;
  if (t >= 0.5f) r = b - diff * (1.0f - t);
  return r;
}
// EPL: anti-diagonal values per lane (window <= 64 EPL); the rank-by-counting loop is the kernel's arithmetic (window^2 / 64
// compares per timestep and lane), so it is instantiated for the window class and reads the broadcast values four at a time.
//
// Memory side: timestep t gathers y_hat[t - j][j] -- one 4-byte element from each of `window` rows, 4 of every 64-byte sector
// (7.9x the algorithmic bytes when each wave gathered its own anti-diagonal).  A workgroup now owns UT consecutive timesteps and
// stages their anti-diagonals through LDS: row r contributes the contiguous run j in [t0 - r, t0 + UT - r) to this tile, read
// with lane-consecutive (coalesced) loads, every element of y_hat by exactly one workgroup; the element lands at
// tile[t - t0][j - j0(t)], i.e. each timestep's values end up as one contiguous LDS row (row stride = window rounded up to a
// multiple of 4, so consecutive j of one source row -- consecutive t -- fall into different banks: stride + 1 is odd).
//
// FILTER (median only, no summary): a full rank count is window^2 compares although only the middle is wanted.  Two pivots are
// taken from the ranks of a 32-value sample (the 11th and 22nd smallest: the median of 100 lies between them in ~96 % of
// draws), the values below / not above them are counted with two ballots per slot, and if the middle position(s) fall between
// the pivots and at most 64 values do, only those candidates are ranked against each other (~33^2 compares).  Anything else --
// pivots that miss, ties among the candidates, short edge diagonals -- takes the full count: the result is the exact order
// statistic either way.
#if HYPAD_DIAG
long long* g_unroll_stamps = nullptr;        // development aid (dev library): [0..3] shader-clock stamps of one workgroup's first tile, [8] filter hits, [9] full counts
#define USTAMP(k) do { if (stamps && blockIdx.x == 37 && threadIdx.x == 0 && t0 == (int64_t)blockIdx.x * UT) stamps[k] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#define UCOUNT(k) do { if (ucount && lane == 0) atomicAdd((unsigned long long*)stamps + (k), 1ull); } while (0)
#else
#define USTAMP(k) do { } while (0)
#define UCOUNT(k) do { } while (0)
#endif
// UT: timesteps per workgroup tile, one wave per 16 of them (UT = 64: 256 threads, 128: 512).  A longer tile reads longer runs
// of every source row (fewer partly used 128-byte lines at the runs' ends: the tile's triangle rows) for twice the LDS.
template <int EPL, bool FILTER, int UT>
__global__ __launch_bounds__(UT * 4) __attribute__((amdgpu_waves_per_eu(UNROLL_WPE, UNROLL_WPE))) void unroll_median_kernel(const float* __restrict__ y_hat, float* __restrict__ median,
                                                                double* __restrict__ summary, int64_t n, int W, long long* stamps) {
  constexpr int THREADS = UT * 4;                           // (shadows the file's 256: this kernel's block size follows its tile)
  constexpr int RUN = UT / 64;                               // elements per lane of one source row's run
  extern __shared__ __attribute__((aligned(16))) float usm[];
  const int WS = (W + 3) & ~3;                              // tile row stride (floats)
  float* tile = usm;                                        // [UT][WS]
  float* sorted = usm + UT * WS;                            // [waves][MAX_WINDOW]   (summary / candidates)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  constexpr int NWV = THREADS / 64;
  const int64_t T = n + W - 1;
  float* s = sorted + wave_s * MAX_WINDOW;
  const float INF = __int_as_float(0x7f800000);
#if HYPAD_DIAG
  const bool ucount = stamps && stamps[14] != 0;             // (counting costs one contended atomic per timestep: a run of its own)
#endif
  for (int64_t t0 = (int64_t)blockIdx.x * UT; t0 < T; t0 += (int64_t)gridDim.x * UT) {
    USTAMP(0);
    // ---- stage: rows r in [t0 - (W - 1), t0 + UT) (clipped to the matrix), their runs of this tile's timesteps
    constexpr int RB = 8 / RUN;                              // rows in flight per wave (8 loads per lane either way)
    if (t0 >= W - 1 && t0 + UT <= n) {
      // interior tile (all but the first and last two of a long series): no clipping, j0 == 0, 32-bit indices relative to the
      // tile's first row, the row number a scalar -- ~9 vector instructions per row and lane instead of ~30 of 64-bit arithmetic
      const float* base = y_hat + (t0 - (W - 1)) * W;
      const int nrows = W + UT - 1;
      for (int kb = wave_s * RB; kb < nrows; kb += NWV * RB) {
        float val[RB][RUN];
        int dst[RB][RUN];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
          const int k = kb + u;                              // (scalar) row of the tile's parallelogram
          const int jb = W - 1 - k > 0 ? W - 1 - k : 0;
#pragma unroll
          for (int h = 0; h < RUN; ++h) {
            const int j = jb + lane + 64 * h, tt = k - (W - 1) + j;
            const bool ok = k < nrows && j < W && tt < UT;
            dst[u][h] = ok ? tt * WS + j : -1;
            val[u][h] = ok ? base[k * W + j] : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < RB; ++u)
#pragma unroll
          for (int h = 0; h < RUN; ++h)
            if (dst[u][h] >= 0) tile[dst[u][h]] = val[u][h];
      }
    } else {
      const int64_t r_lo = t0 - (W - 1) > 0 ? t0 - (W - 1) : 0;
      const int64_t r_hi = t0 + UT < n ? t0 + UT : n;         // exclusive
      for (int64_t rb = r_lo + wave * RB; rb < r_hi; rb += NWV * RB) {
        float val[RB][RUN];
        int dst[RB][RUN];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
          const int64_t r = rb + u;
          const int jb = (int)(t0 - r > 0 ? t0 - r : 0);       // first column of row r inside the tile
#pragma unroll
          for (int h = 0; h < RUN; ++h) {
            const int j = jb + lane + 64 * h;                  // (a run is at most UT columns: RUN elements per lane)
            const int64_t t = r + j;
            dst[u][h] = -1; val[u][h] = 0.f;
            if (r < r_hi && j < W && t < t0 + UT && t < T) {
              const int j0 = (int)(t - n + 1 > 0 ? t - n + 1 : 0);
              dst[u][h] = (int)(t - t0) * WS + (j - j0);
              val[u][h] = y_hat[r * W + j];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < RB; ++u)
#pragma unroll
          for (int h = 0; h < RUN; ++h)
            if (dst[u][h] >= 0) tile[dst[u][h]] = val[u][h];
      }
    }
    USTAMP(1);
    __syncthreads();
    USTAMP(2);
    // (round 6: the timestep a wave works on is a scalar -- as a vector value every count, address and "wave-uniform" branch below was
    // vector arithmetic and exec-mask code)
    for (int tt = wave_s; tt < UT; tt += NWV) {
      const int64_t t = t0 + tt;
      if (t >= T) break;
      const int j0 = (int)(t - n + 1 > 0 ? t - n + 1 : 0);
      const int j1 = (int)(t + 1 < W ? t + 1 : W);
      const int cnt = j1 - j0;
      float* v = tile + tt * WS;
      // pad the row to a multiple of 4 with +inf (never below or equal to a finite value)
      if (lane < 4 && cnt + lane < ((cnt + 3) & ~3)) v[cnt + lane] = INF;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): LDS writes of this wave landed
      float mine[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) { const int i = lane + 64 * e; mine[e] = i < cnt ? v[i] : INF; }
      const int m1 = (cnt - 1) >> 1, m2 = cnt >> 1;
      float lo_med = 0.f, hi_med = 0.f;
      bool done = false;
      if (FILTER && !summary && cnt >= 64) {                 // wave-uniform
        // ranks inside the sample v[0 .. 31] (lanes >= 32 idle along)
        const float sv = v[lane & 31];
        int less = 0;
#pragma unroll
        for (int k0 = 0; k0 < 32; k0 += 4) {
          const float4 q = *reinterpret_cast<const float4*>(v + k0);
          less += (q.x < sv ? 1 : 0) + (q.y < sv ? 1 : 0) + (q.z < sv ? 1 : 0) + (q.w < sv ? 1 : 0);
        }
        float plo = less <= 10 ? sv : -INF, phi = less >= 21 ? sv : INF;     // 11th smallest (largest with <= 10 below), 22nd smallest
        plo = hypad::wave_max(plo); phi = hypad::wave_min(phi);                // (DPP butterflies: no LDS round trips on this chain)
        int c_lt = 0, c_le = 0;
        unsigned long long cm[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const bool in = lane + 64 * e < cnt;
          c_lt += __builtin_popcountll(__ballot(in && mine[e] < plo));
          c_le += __builtin_popcountll(__ballot(in && mine[e] <= phi));
          cm[e] = __ballot(in && mine[e] >= plo && mine[e] <= phi);
        }
        const int nc = c_le - c_lt;
        if (c_lt <= m1 && m2 < c_le && nc <= 64 && nc > 0) {
          // compact the candidates into the wave's slab, rank them against each other
          int base = 0;
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(cm[e] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)cm[e], 0u));
            if ((cm[e] >> lane) & 1ull) s[pos] = mine[e];
            base += __builtin_popcountll(cm[e]);
          }
          if (lane < 4 && nc + lane < ((nc + 3) & ~3)) s[nc + lane] = INF;
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_s_waitcnt(0xc07f);
          const float c = lane < nc ? s[lane] : INF;
          int rk = 0;
          for (int k0 = 0; k0 < nc; k0 += 4) {
            const float4 q = *reinterpret_cast<const float4*>(s + k0);
            rk += (q.x < c ? 1 : 0) + (q.y < c ? 1 : 0) + (q.z < c ? 1 : 0) + (q.w < c ? 1 : 0);
          }
          // without ties the "less" counts are a permutation of 0 .. nc - 1 (their sum tells): then the lanes holding local ranks
          // m1 - c_lt and m2 - c_lt hold the two middle values
          const float rsum = hypad::wave_sum(lane < nc ? (float)rk : 0.f);
          if (rsum == 0.5f * (float)nc * (float)(nc - 1)) {
            const unsigned long long k1 = __ballot(lane < nc && rk == m1 - c_lt), k2 = __ballot(lane < nc && rk == m2 - c_lt);
            lo_med = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), (int)__builtin_ctzll(k1)));
            hi_med = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), (int)__builtin_ctzll(k2)));
            done = true;
            UCOUNT(8);
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
      if (!done) {
        UCOUNT(9);
        // rank = #{k : v[k] < mine} + #{k < i : v[k] == mine}.  Fast pass: count "less" only (one compare + add-carry per value).
        // Without ties those counts are a permutation of 0 .. cnt-1, with ties two values share a count and the counts' sum falls
        // short of cnt (cnt - 1) / 2: only then is the ordered tie count needed.  (The sum is exact in fp32: < 2^15 at window 256.)
        int rank[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) rank[e] = 0;
        for (int k0 = 0; k0 < cnt; k0 += 4) {
          const float4 q = *reinterpret_cast<const float4*>(v + k0);
          const float vk[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < EPL; ++e) rank[e] += vk[u] < mine[e] ? 1 : 0;
        }
        float rsum = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) rsum += lane + 64 * e < cnt ? (float)rank[e] : 0.f;
        const bool ties = hypad::wave_sum(rsum) != 0.5f * (float)cnt * (float)(cnt - 1);
        if (ties) {                                      // wave-uniform
#pragma unroll
          for (int e = 0; e < EPL; ++e) rank[e] = 0;
          for (int k = 0; k < cnt; ++k) {
            const float vk = v[k];
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
              const int i = lane + 64 * e;
              rank[e] += (vk < mine[e]) || (vk == mine[e] && k < i);
            }
          }
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e)
          if (lane + 64 * e < cnt) s[rank[e]] = mine[e];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        lo_med = s[m1]; hi_med = s[m2];
      }
      if (lane == 0) {
        median[t] = (cnt & 1) ? lo_med : (lo_med + hi_med) * 0.5f;     // np.median of float32 stays float32
        if (summary) {
          double* o = summary + t * 5;
          o[0] = (double)s[0];
          const double qs[3] = {0.25, 0.5, 0.75};
          for (int qi = 0; qi < 3; ++qi) {
            double pos = qs[qi] * (double)(cnt - 1);
            int a = (int)floor(pos);
            int b = a + 1 < cnt ? a + 1 : cnt - 1;
            o[1 + qi] = (double)np_lerp(s[a], s[b], (float)(pos - (double)a));
          }
          o[4] = (double)s[cnt - 1];
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    USTAMP(3);
    __syncthreads();
  }
}

template <class TIn>
__global__ __launch_bounds__(THREADS) void unroll_true_kernel(const TIn* __restrict__ y, int64_t ld, double* __restrict__ out, int64_t n, int W) {
  const int64_t T = n + W - 1;
  for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < T; t += (int64_t)gridDim.x * THREADS)
    out[t] = (double)(t < n ? y[t * ld] : y[(n - 1) * ld + (t - n + 1)]);
}

__global__ __launch_bounds__(THREADS) void point_error_kernel(const double* __restrict__ y, const float* __restrict__ yh,
                                                               double* __restrict__ out, int64_t T) {
  for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < T; t += (int64_t)gridDim.x * THREADS)
    out[t] = fabs(y[t] - (double)yh[t]);
}

// pandas centred window of size w at i: [i + off - w + 1, i + off], off = (w - 1) / 2, clipped to the array
__device__ __forceinline__ void centred_window(int64_t i, int w, int64_t T, int64_t& lo, int64_t& hi) {
  const int off = (w - 1) / 2;
  lo = i + off - w + 1; hi = i + off;
  if (lo < 0) lo = 0;
  if (hi > T - 1) hi = T - 1;
}

__global__ __launch_bounds__(THREADS) void area_error_kernel(const double* __restrict__ y, const float* __restrict__ yh,
                                                              double* __restrict__ out, int64_t T, int w) {
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < T; i += (int64_t)gridDim.x * THREADS) {
    int64_t lo, hi;
    centred_window(i, w, T, lo, hi);
    if (hi - lo + 1 < w / 2) { out[i] = NAN; continue; }
    double a = 0.0, b = 0.0;
    for (int64_t k = lo; k < hi; ++k) {
      a += (y[k] + y[k + 1]) * 0.5;
      b += ((double)yh[k] + (double)yh[k + 1]) * 0.5;
    }
    out[i] = fabs(a - b);
  }
}

template <int LEN>
__global__ __launch_bounds__(THREADS) void dtw_error_kernel(const double* __restrict__ y, const float* __restrict__ yh,
                                                             double* __restrict__ out, int64_t T) {
  constexpr int HALF = LEN / 2;
  for (int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x; p < T; p += (int64_t)gridDim.x * THREADS) {
    const int64_t i = p - HALF;                 // window start in padded coordinates
    if (i < 0 || i >= T - LEN) { out[p] = 0.0; continue; }
    double a[LEN], b[LEN], row[LEN];
#pragma unroll
    for (int k = 0; k < LEN; ++k) {
      int64_t src = i + k - HALF;               // y_pad[i + k] = y[i + k - HALF]
      bool ok = src >= 0 && src < T;
      a[k] = ok ? y[src] : 0.0;
      b[k] = ok ? (double)yh[src] : 0.0;
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < LEN; ++j) { double d = a[0] - b[j]; acc += d * d; row[j] = acc; }
#pragma unroll
    for (int r = 1; r < LEN; ++r) {
      double diag = row[0];
      double d0 = a[r] - b[0];
      row[0] = row[0] + d0 * d0;
#pragma unroll
      for (int j = 1; j < LEN; ++j) {
        double up = row[j];
        double d = a[r] - b[j];
        double m = fmin(fmin(up, row[j - 1]), diag);
        row[j] = d * d + m;
        diag = up;
      }
    }
    out[p] = sqrt(row[LEN - 1]);
  }
}

// ---- centred rolling mean (pandas rolling(w, center=True, min_periods=w/2).mean(), NaNs skipped).
// A window's sum is O(w) additions per output if taken element by element: 1 250 per timestep at 125 000 windows (the reference's
// smoothing window is 1 % of the windows), 10^4 at 10^6.  It is taken from two levels of pre-summed chunks instead -- 16 and 256
// elements, aligned to the ABSOLUTE index (origin + local index) -- in one canonical order: the elements up to the next multiple of
// 16, 16-chunks up to the next multiple of 256, 256-chunks, 16-chunks, the remaining elements; <= 30 + 30 + w/256 additions.
// Canonical and absolute: a rank that smooths only a slice of the series (parallel.sharded_euclidean_scores passes the slice's
// position as `origin`) performs exactly the additions the un-sharded pass performs for the same timestep -- same bits.
// Windows up to 32 wide are summed directly (also position-independent).
constexpr int RC1 = 16, RC2 = 256, ROLL_DIRECT_MAX = 32;
struct RollSrc {                                   // element i of the smoothed series: in[i], or the point-wise error |in[i] - sub[i]| (:761-777) fused
  const double* in; const float* sub;
  __device__ __forceinline__ double operator()(int64_t i) const { const double v = in[i]; return sub ? fabs(v - (double)sub[i]) : v; }
};
struct RollWs { double* s1; double* s2; int* c1; int* c2; int64_t n1, n2; };
__host__ __device__ inline void roll_counts(int64_t T, int64_t origin, int64_t& n1, int64_t& n2) {
  n1 = ((origin + T - 1) >> 4) - (origin >> 4) + 1;
  n2 = ((origin + T - 1) >> 8) - (origin >> 8) + 1;
}
// level 1: one thread per 16-chunk, ascending
// (one launch for both levels: a workgroup owns 16 consecutive 256-chunks and the 256 16-chunks they consist of -- the slots are
// counted from the level-2 chunk's own first 16-chunk, so no 256-chunk straddles two workgroups; level 2 adds its 16 level-1 sums in
// ascending order out of LDS: the additions of the two-launch form, hence its bits)
__global__ __launch_bounds__(THREADS) void roll_chunks_kernel(RollSrc src, RollWs ws, int64_t T, int64_t origin) {
  __shared__ double sh_s[THREADS];
  __shared__ int sh_c[THREADS];
  const int64_t c2_0 = (int64_t)blockIdx.x * 16;                                     // this workgroup's first 256-chunk
  const int64_t first1 = (((origin >> 8) + c2_0) << 4) - (origin >> 4);             // level-1 slot of its first 16-chunk (may be < 0 at the left edge)
  const int64_t j = first1 + threadIdx.x;
  double s = 0.0; int cnt = 0;
  if (j >= 0 && j < ws.n1) {
    const int64_t g0 = ((origin >> 4) + j) << 4;
#pragma unroll 4
    for (int k = 0; k < RC1; ++k) {
      const int64_t i = g0 + k - origin;
      if (i >= 0 && i < T) { const double v = src(i); if (v == v) { s += v; ++cnt; } }
    }
    ws.s1[j] = s; ws.c1[j] = cnt;
  }
  sh_s[threadIdx.x] = s; sh_c[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x < 16 && c2_0 + threadIdx.x < ws.n2) {
    double s2 = 0.0; int c2 = 0;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
      const int64_t jj = first1 + 16 * threadIdx.x + k;
      if (jj >= 0 && jj < ws.n1) { s2 += sh_s[16 * threadIdx.x + k]; c2 += sh_c[16 * threadIdx.x + k]; }
    }
    ws.s2[c2_0 + threadIdx.x] = s2; ws.c2[c2_0 + threadIdx.x] = c2;
  }
}
template <bool CHUNKED>
__global__ __launch_bounds__(THREADS) void rolling_mean_kernel(RollSrc src, RollWs ws, double* __restrict__ out, int64_t T, int w, int64_t origin) {
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < T; i += (int64_t)gridDim.x * THREADS) {
    int64_t lo, hi;
    centred_window(i, w, T, lo, hi);
    int cnt = 0;
    double s = 0.0;
    if constexpr (!CHUNKED) {
      for (int64_t k = lo; k <= hi; ++k) {
        const double v = src(k);
        if (v == v) { s += v; ++cnt; }            // pandas skips NaN
      }
    } else {
      const int64_t b1 = origin >> 4, b2 = origin >> 8, end = origin + hi + 1;
      int64_t p = origin + lo;
      auto elems = [&](int64_t to) { for (; p < to; ++p) { const double v = src(p - origin); if (v == v) { s += v; ++cnt; } } };
      const int64_t a16 = (p + RC1 - 1) & ~(int64_t)(RC1 - 1);
      elems(a16 < end ? a16 : end);
      while (p + RC1 <= end && (p & (RC2 - 1))) { s += ws.s1[(p >> 4) - b1]; cnt += ws.c1[(p >> 4) - b1]; p += RC1; }
      while (p + RC2 <= end) { s += ws.s2[(p >> 8) - b2]; cnt += ws.c2[(p >> 8) - b2]; p += RC2; }
      while (p + RC1 <= end) { s += ws.s1[(p >> 4) - b1]; cnt += ws.c1[(p >> 4) - b1]; p += RC1; }
      elems(end);
    }
    out[i] = cnt >= w / 2 && cnt > 0 ? s / (double)cnt : NAN;
  }
}

// ---- z-score statistics in two levels (scipy.stats.zscore: mean, population std).  Level 1: up to STAT_G blocks, each over one
// contiguous slice: (n, mean, M2 = sum (x - mean)^2) two-pass inside the slice; level 2: every block of the elementwise kernel
// that follows merges the <= 256 partials itself with the pairwise update (Chan et al.) in one fixed tree order -- no third
// launch, the same bits in every block.  (The one-block serial form took 41 us per 10^5 values: 1 % of the HBM rate.)
constexpr int STAT_G = 256;
struct StatPart { double n, mean, m2, rsum, rcnt; };          // rsum / rcnt: sum and count of the values inside [lo, hi] (critic score)
__device__ __forceinline__ double block_sum_256(double v, double* sh) {      // fixed order: wave butterflies, then the 4 wave sums ascending
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
template <bool RANGE>
__global__ __launch_bounds__(256) void stat_partials_kernel(const double* __restrict__ in, StatPart* __restrict__ parts, int64_t T, double lo, double hi,
                                                              const double* __restrict__ range_dev = nullptr) {      // range_dev: [lo, hi] left on the device by hypad_quantiles
  __shared__ double sh[4];
  if (RANGE && range_dev) { lo = range_dev[0]; hi = range_dev[1]; }
  const int64_t len = (T + gridDim.x - 1) / gridDim.x;
  const int64_t b = (int64_t)blockIdx.x * len, e = b + len < T ? b + len : T;
  double s = 0.0, rs = 0.0, rc = 0.0;
  for (int64_t i = b + threadIdx.x; i < e; i += 256) {
    const double x = in[i];
    s += x;
    if (RANGE && x >= lo && x <= hi) { rs += x; rc += 1.0; }
  }
  const double n = e > b ? (double)(e - b) : 0.0;
  const double mean = n > 0.0 ? block_sum_256(s, sh) / n : 0.0;
  double q = 0.0;
  for (int64_t i = b + threadIdx.x; i < e; i += 256) { const double d = in[i] - mean; q += d * d; }
  q = block_sum_256(q, sh);
  if (RANGE) { rs = block_sum_256(rs, sh); rc = block_sum_256(rc, sh); }
  if (threadIdx.x == 0) { StatPart p; p.n = n; p.mean = mean; p.m2 = q; p.rsum = rs; p.rcnt = rc; parts[blockIdx.x] = p; }
}
__device__ __forceinline__ StatPart stat_merge(const StatPart& a, const StatPart& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  StatPart r;
  r.n = a.n + b.n;
  const double d = b.mean - a.mean;
  r.mean = a.mean + d * (b.n / r.n);
  r.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / r.n);
  r.rsum = a.rsum + b.rsum; r.rcnt = a.rcnt + b.rcnt;
  return r;
}
// every thread of a 256-thread block gets the merged statistics of `g` partials (fixed binary tree over the slots)
__device__ __forceinline__ StatPart stat_merge_all(const StatPart* __restrict__ parts, int g, StatPart* sh) {
  StatPart p; p.n = 0.0; p.mean = 0.0; p.m2 = 0.0; p.rsum = 0.0; p.rcnt = 0.0;
  if ((int)threadIdx.x < g) p = parts[threadIdx.x];
  sh[threadIdx.x] = p;
  __syncthreads();
  for (int st = 1; st < STAT_G; st <<= 1) {
    if ((threadIdx.x & (2 * st - 1)) == 0) sh[threadIdx.x] = stat_merge(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  return sh[0];
}
__global__ __launch_bounds__(256) void zscore_apply_kernel(const double* __restrict__ in, const StatPart* __restrict__ parts, int g,
                                                            double* __restrict__ out, int64_t T) {
  __shared__ StatPart sh[STAT_G];
  const StatPart st = stat_merge_all(parts, g, sh);
  const double mean = st.mean, sd = sqrt(st.m2 / st.n);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
    double z = (in[i] - mean) / sd;
    out[i] = (z != z) ? z : fmax(z, 0.0) + 1.0;  // np.clip keeps NaN
  }
}

// ---- critic smoothing: final_critic_scores :365-404.  Timestep t sees the critic values of the
// windows covering it, critic[t - j] for the valid j (each window's score repeated along the window, un-rolled along
// anti-diagonals).  Its score is the sample at which a Scott-bandwidth Gaussian KDE of those values is largest
// (scipy.stats.gaussian_kde(v)(v), first arg-max), the median when fewer than two values or a singular covariance.
constexpr int KDE_WPE = 7;     // (round 6, re-swept on the final kernel: 5 -> 0.233, 6 -> 0.229, 7 -> 0.224 ms per 125 000 windows at 70 registers, none spilled; 8 spills 4)
constexpr int KDE_CB = 2;                    // candidates per pass-2 batch.  Its term buffer is the kernel's largest LDS array (4 KB per wave at 2): with 2
                                             // and five waves per SIMD (96 registers) the kernel takes 0.354 ms per 125 000 windows; 0.438 at 4 / three waves
//
// Selection in two passes.  The result is a SAMPLE (the arg-max's value), so only the arg-max must be exact, not the densities:
// pass 1 evaluates every density in fp32 (v_exp_f32: cnt^2 = 10^4 exponentials per timestep at window 100 -- in fp64 this pass
// was 97 % of the kernel, 1.7 ms for 125 000 windows); pass 2 re-evaluates in fp64, exactly as before, only the samples whose
// fp32 density lies within 4e-5 of the fp32 maximum -- a superset of the true arg-max set (the fp32 density's relative error is
// below 7.1e-6: the budget is written out at the threshold below) -- with the same first-maximum tie rule.  Clustered samples (many near-equal densities) simply put more candidates into pass 2.
// KPL: sample slots of 64 per lane = ceil(window / 64), a template parameter: the fp32 pass keeps four partial sums per slot.
template <int KPL>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(KDE_WPE, KDE_WPE))) void kde_mode_kernel(const float* __restrict__ critic, double* __restrict__ modes,
                                                            int64_t n, int W) {
  constexpr int WMAX = 64 * KPL;                            // the window class: 9 KB of LDS per workgroup and slot, 18 KB at window 100
  __shared__ double vals[THREADS / 64][WMAX];
  __shared__ __attribute__((aligned(16))) float vals32[THREADS / 64][WMAX + 4];      // + the padding the fp32 pass reads past the end
  __shared__ __attribute__((aligned(16))) float nsq32[THREADS / 64][WMAX + 4];       // -(value^2) for the factored form of the fp32 pass
  __shared__ double terms[THREADS / 64][KDE_CB * WMAX];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t T = n + W - 1;
  double* v = vals[wave];
  float* vf = vals32[wave];
  float* nf = nsq32[wave];
  // per-thread constants of the timestep loop, held in SCALAR registers (they are wave-uniform; as vector values the compiler kept them
  // in scratch memory across the loop: 20 bytes of private segment per lane and two scratch loads per timestep)
  auto uniform = [](double x) __attribute__((always_inline)) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
  };
  // Scott's factor n^(-2/5) for every sample count 1 .. W, one power per thread, once (the 2 (W - 1) edge timesteps have fewer than W
  // samples; a double-precision pow inside the loop -- ~200 instructions, its 40 polynomial constants hoisted into vector registers
  // across the loop -- was what this kernel spilled around)
  __shared__ double scott[WMAX];
  for (int c = threadIdx.x; c < W && c < WMAX; c += THREADS) scott[c] = pow((double)(c + 1), -0.4);
  __syncthreads();
  const double rW1 = uniform(W > 1 ? 1.0 / (double)(W - 1) : 0.0);
  for (int64_t t = (int64_t)blockIdx.x * (THREADS / 64) + wave; t < T; t += (int64_t)gridDim.x * (THREADS / 64)) {
    const int j0 = (int)(t - n + 1 > 0 ? t - n + 1 : 0);
    const int j1 = (int)(t + 1 < W ? t + 1 : W);
    const int cnt = __builtin_amdgcn_readfirstlane(j1 - j0);      // (wave-uniform: the pair loops below run on scalar counters)
    double s = 0.0;
    for (int k = lane; k < cnt; k += 64) {
      const float xf = critic[t - (j0 + k)];
      v[k] = (double)xf;
      vf[k] = xf;
      s += (double)xf;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    const double mean = wave_sum(s) / (double)cnt;
    double q = 0.0;
    for (int k = lane; k < cnt; k += 64) { const double d = v[k] - mean; q += d * d; }
    const double var = cnt > 1 ? wave_sum(q) * (cnt == W ? rW1 : 1.0 / (double)(cnt - 1)) : 0.0;      // np.cov: ddof = 1, `c *= 1 / fact`
    // Scott: factor = n^(-1/5), squared.  (All but the 2 (W - 1) edge timesteps have cnt == W: that power is taken once per
    // thread, not once per timestep -- a double-precision pow is ~200 instructions.)
    const double cov = var * uniform(scott[cnt - 1]);
    double out;
    if (cnt > 1 && cov > 0.0 && cov == cov) {
      // pass 1: fp32 densities of this lane's samples.  exp(-d^2 inv) = exp2(-(c d)^2) with c = sqrt(inv log2 e): the samples are
      // centred and rescaled once (pass 2 reads the fp64 copies), so a pair costs a subtract, a multiply, an exp2 and an add; the
      // slab is padded with +inf to a multiple of four (a padded pair contributes exp2(-inf) = 0) and read four values at a
      // time, every value once for all of the lane's samples.
      // The samples are CENTRED first, in fp64 (densities depend on differences only): rescaling the raw values would leave the
      // fp32 copies with an absolute error of |value| 2^-24 c, which at |mean| / bandwidth beyond ~1e4 exceeds the screen's margin.
      // The scale itself only has to be good to fp32 (an error in it is a slightly different bandwidth for every sample alike: 2e-7
      // relative in the densities): one v_rsq_f32 instead of an fp64 division and square root per timestep; the fp64 1 / (2 cov) that
      // pass 2 uses is taken only when pass 2 runs.  (A covariance outside the fp32 range makes the screen all-NaN or all-equal: pass 2
      // then sees every sample, as before.)
      const double c64 = (double)__builtin_amdgcn_rsqf((float)cov * 1.3862943611198906f);     // sqrt(log2 e / (2 cov))
      float amax = 0.f;
      for (int k = lane; k < cnt; k += 64) {
        const float y = (float)((v[k] - mean) * c64);
        vf[k] = y; nf[k] = -(y * y);
        amax = fmaxf(amax, fabsf(y));
      }
      amax = wave_max(amax);
      // (Measured and dropped in round 3, twice: using the kernel matrix's symmetry -- each unordered pair evaluated once.  With the
      // partner's share delivered by ds_add_f32: 3.28 ms against 0.42 ms for 125 000 windows (LDS float atomics).  With the values
      // parked in a small LDS matrix in chunks of eight steps and collected by the partners after a wave barrier (no atomics,
      // conflict-free strides, immediate offsets): 0.69 ms -- three per-lane LDS operations per pair cost more issue time than the
      // quarter-rate exponential they save; the broadcast form below reads each value once for all 64 lanes.)
      const bool factored = amax <= 8.f;                   // (wave-uniform; NaN -> the direct form)
      if (lane < 4 && cnt + lane < ((cnt + 3) & ~3)) {      // padding to a multiple of four: a pair that contributes exp2(-inf) = 0 in either form
        vf[cnt + lane] = factored ? 0.f : __int_as_float(0x7f800000);
        nf[cnt + lane] = __int_as_float(0xff800000);
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xc07f);
      // (Measured and dropped in round 3: giving the cnt % 64 samples of the last slot 64 / b lanes each -- groups of b = 32, 16, ..
      // samples by the binary digits of the remainder, each lane a share of the values, shares added by xor shuffles: 25 + 13 + 2 steps
      // of four values per lane at window 100 instead of 25 + 25, 20 % fewer exponentials by counter, and no faster: 0.292 against
      // 0.287 ms.  Per-lane LDS addresses and the shuffles cost what the idle lanes did.)
      float d32[KPL], xs[KPL];
      float acc[KPL][4];                                   // one accumulator per position in the group of four: <= ceil(cnt / 4) terms each
#pragma unroll
      for (int u = 0; u < KPL; ++u) {
        const int k = lane + 64 * u;
        xs[u] = vf[k < cnt ? k : 0];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[u][c] = 0.f;
      }
      const int nu = (cnt + 63) >> 6;                                             // sample slots in use (wave-uniform)
      if (factored) {
        // exp2(-(x - v)^2) = exp2(-x^2) exp2(2 x v - v^2): the pair costs a fused multiply-add (2 x in a register, v and -v^2 from
        // LDS), an exp2 and an add -- three issue slots instead of four -- and exp2(-x^2) multiplies the finished sum once.
        // |x|, |v| <= 8 keeps 2 x v - v^2 <= x^2 <= 64 inside the fp32 exponent range and its rounding (the product's and
        // -v^2's: 2^-24 x 64 each at the very worst) inside the budget written out at the threshold below.
        float x2[KPL];
#pragma unroll
        for (int u = 0; u < KPL; ++u) x2[u] = 2.f * xs[u];
        for (int m = 0; m < cnt; m += 4) {
          const float4 q4 = *reinterpret_cast<const float4*>(vf + m);
          const float4 n4 = *reinterpret_cast<const float4*>(nf + m);
          const float vm[4] = {q4.x, q4.y, q4.z, q4.w}, nm[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            if (u >= nu) continue;
            // (two fused multiply-adds per instruction: v_pk_fma_f32 -- the same roundings)
            typedef float v2f __attribute__((ext_vector_type(2)));
            const v2f xx = {x2[u], x2[u]};
            const v2f a01 = __builtin_elementwise_fma(xx, v2f{vm[0], vm[1]}, v2f{nm[0], nm[1]});
            const v2f a23 = __builtin_elementwise_fma(xx, v2f{vm[2], vm[3]}, v2f{nm[2], nm[3]});
            acc[u][0] += __builtin_amdgcn_exp2f(a01.x); acc[u][1] += __builtin_amdgcn_exp2f(a01.y);
            acc[u][2] += __builtin_amdgcn_exp2f(a23.x); acc[u][3] += __builtin_amdgcn_exp2f(a23.y);
          }
        }
#pragma unroll
        for (int u = 0; u < KPL; ++u) d32[u] = ((acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3])) * __builtin_amdgcn_exp2f(-(xs[u] * xs[u]));
      } else {
        for (int m = 0; m < cnt; m += 4) {
          const float4 q4 = *reinterpret_cast<const float4*>(vf + m);
          const float vm[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            if (u >= nu) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) { const float d = xs[u] - vm[c]; acc[u][c] += __builtin_amdgcn_exp2f(-(d * d)); }
          }
        }
#pragma unroll
        for (int u = 0; u < KPL; ++u) d32[u] = (acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3]);
      }
      float mx = -1.f;
#pragma unroll
      for (int u = 0; u < KPL; ++u) {
        if (lane + 64 * u >= cnt) d32[u] = -1.f;
        mx = fmaxf(mx, d32[u]);
      }
      mx = wave_max(mx);
      // Relative error of an fp32 density D~ against the exact D, all terms positive.  Direct form, exp2(-(x - v)^2):
      //  * arguments: a centred, rescaled sample y carries 2^-24 |y| <= 1e-6 (|y| < 32 for every pair that contributes: two of <= 256
      //    samples within a few units of each other lie at most 2.6 sqrt(255 / 2) = 29 units from the mean; a lone outlier beyond that
      //    sees only its own term, exactly 1), a difference d twice that, d^2 an absolute 2 |d| 2e-6 (+ 2^-24 d^2 from the product);
      //    a term's relative error is ln 2 times that, and weighted by the terms themselves (|d| 2^(-d^2) <= 0.52, the self term is 1)
      //    the sum's is <= 3e-6;
      //  * v_exp_f32: 1 ulp = 1.2e-7;
      //  * accumulation: four partial sums of <= 64 terms, each add 2^-24 of a partial sum that never exceeds the result: 3.8e-6, + 1.2e-7
      //    for the two combining adds
      // -> eps <= 7.1e-6 at window 256 (4.8e-6 at 100).  Factored form (all |y| <= 8), exp2(-x^2) exp2(2 x v - v^2):
      //  * the samples' own rounding (|y| <= 8: 2^-24 x 8): 0.7e-6 by the same weighting;
      //  * the argument 2 x v - v^2 (|.| <= 64): -v^2 rounded once, the fused multiply-add once, 2^-24 x 64 = 3.8e-6 absolute together
      //    at the very worst -> ln 2 x 3.8e-6 = 2.6e-6;  exp2(-x^2): x^2 rounded (1.9e-6 absolute -> 1.3e-6) + 1 ulp;
      //  * v_exp_f32 1.2e-7, accumulation 3.9e-6 as above, the closing product 6e-8
      // -> eps <= 8.8e-6.  If k* is the true arg-max, D~[k*] >= (1 - eps) D[k*] >= (1 - eps) D[j] >= (1 - eps) / (1 + eps) D~[j] for
      // every j: the screen keeps k* as long as its margin exceeds 2 eps = 1.8e-5.  Margin 4e-5 (rounds 2-3 used 2e-4 with one
      // accumulator per sample: 1.7 fp64 evaluations per timestep on random-normal values, 0.6 now).
      const float thr = mx * (1.f - 4e-5f);
      // pass 2: fp64 densities of the candidates, in ascending sample order (the first maximum is kept); of every sample if
      // pass 1 produced no candidate (a bandwidth so small that its reciprocal leaves the fp32 range makes the screen NaN).
      // A wave pays for a sequential sum as if all 64 lanes ran it, so a candidate's sum is NOT given to one lane with its
      // exponentials: the lanes compute a candidate's cnt exponentials side by side into LDS (two per lane at window 100), four
      // candidates per batch, then lane c adds candidate c's terms in index order -- the same additions in the same order as
      // the one-lane loop, hence the same bits, at 1/20 of its cycles.
      double best = -1.0;
      int besti = 0x7fffffff;
      double* tm = terms[wave];
      {
        // one candidate only: the screen has decided (its margin is far above the fp32 pass's error), no fp64 sum is needed
        int ncand = 0, first = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < KPL; ++u) {
          const unsigned long long mk = __ballot(lane + 64 * u < cnt && d32[u] >= thr);
          ncand += __builtin_popcountll(mk);
          if (mk && first == 0x7fffffff) first = __builtin_ctzll(mk) + 64 * u;
        }
        if (ncand == 1) besti = first;
      }
      double inv = 0.0;
      if (__builtin_amdgcn_readfirstlane(besti) == 0x7fffffff) inv = 0.5 / cov;          // (only the fp64 pass needs it)
      for (int round = 0; round < 2 && besti == 0x7fffffff; ++round) {
        // First the candidates' fp64 densities as TREE sums (a lane's own terms, then the wave's butterfly: no LDS, no sequential add):
        // either order of adding <= 256 positive terms is within 3e-14 of the exact sum, so a candidate more than 1e-12 below the
        // largest tree sum cannot be the arg-max of the ordered sums either.  One survivor (the usual case): it is the arg-max, and
        // the ordered sums -- a lane adding 100 terms one after the other: half of this pass's time -- are not taken at all; several
        // (equal samples, true near-ties): only those go through the ordered sums below, which decide as before.
        bool keep[KPL];
        {
          double dq[KPL];
#pragma unroll
          for (int u = 0; u < KPL; ++u) dq[u] = -1.0;
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            unsigned long long mask = __ballot(lane + 64 * u < cnt && (round == 1 || d32[u] >= thr));
            while (mask) {                                                        // wave-uniform
              const int k = __builtin_ctzll(mask) + 64 * u;
              mask &= mask - 1;
              const double xk = v[k];
              double loc = 0.0;
              for (int m = lane; m < cnt; m += 64) { const double d = xk - v[m]; loc += exp(-d * d * inv); }
              const double dp = wave_sum(loc);
              if (lane == (k & 63)) dq[u] = dp;
            }
          }
          double mx2 = -1.0;
#pragma unroll
          for (int u = 0; u < KPL; ++u) mx2 = fmax(mx2, dq[u]);
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) mx2 = fmax(mx2, __shfl_xor(mx2, off, WAVE));
          const double thr2 = mx2 * (1.0 - 1e-12);
          int nkeep = 0, first = 0x7fffffff;
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            keep[u] = dq[u] >= thr2 && dq[u] > 0.0;
            const unsigned long long mk = __ballot(keep[u]);
            nkeep += __builtin_popcountll(mk);
            if (mk && first == 0x7fffffff) first = __builtin_ctzll(mk) + 64 * u;
          }
          if (nkeep == 1) { besti = first; break; }
        }
#pragma unroll
        for (int u = 0; u < KPL; ++u) {
          unsigned long long mask = __ballot(keep[u]);
          while (mask) {                                                          // wave-uniform
            int kc[KDE_CB];
            int nb = 0;
#pragma unroll
            for (int c = 0; c < KDE_CB; ++c) {
              kc[c] = -1;
              if (mask) { kc[c] = __builtin_ctzll(mask) + 64 * u; mask &= mask - 1; nb = c + 1; }
            }
#pragma unroll
            for (int c = 0; c < KDE_CB; ++c) {
              if (kc[c] < 0) continue;
              const double xk = v[kc[c]];
              for (int m = lane; m < cnt; m += 64) { const double d = xk - v[m]; tm[c * WMAX + m] = exp(-d * d * inv); }
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);
            double dens = -1.0;
            if (lane < nb) {
              dens = 0.0;
              const double* tp = tm + lane * WMAX;
              int m = 0;
              for (; m + 8 <= cnt; m += 8) {                 // (the terms of eight steps requested together; added in index order)
                double t8[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) t8[x] = tp[m + x];
#pragma unroll
                for (int x = 0; x < 8; ++x) dens += t8[x];
              }
              for (; m < cnt; ++m) dens += tp[m];
            }
#pragma unroll
            for (int c = 0; c < KDE_CB; ++c) {
              const double dc = __shfl(dens, c, WAVE);
              if (c < nb && dc > best) { best = dc; besti = kc[c]; }
            }
            __builtin_amdgcn_wave_barrier();
          }
        }
      }
      out = v[besti < cnt ? besti : 0];                    // (all densities NaN -- a covariance whose reciprocal overflows: scipy's arg-max of NaNs is 0)
    } else {
      // median by rank counting (cnt <= 256)
      double lo = 0.0, hi = 0.0;
      for (int k = lane; k < cnt; k += 64) {
        const double xk = v[k];
        int rank = 0;
        for (int m = 0; m < cnt; ++m) rank += (v[m] < xk) || (v[m] == xk && m < k);
        if (rank == (cnt - 1) / 2) lo = xk;
        if (rank == cnt / 2) hi = xk;
      }
      out = 0.5 * (wave_sum(lo) + wave_sum(hi));
    }
    if (lane == 0) modes[t] = out;
    __builtin_amdgcn_wave_barrier();
  }
}

// _compute_critic_score :307-333 without the rolling mean: out = |x - mean of the values inside [lo, hi]| / population std of all
// values + 1 (the statistics in two levels, as for the z-score above).
__global__ __launch_bounds__(256) void critic_apply_kernel(const double* __restrict__ in, const StatPart* __restrict__ parts, int g,
                                                            double* __restrict__ out, int64_t T) {
  __shared__ StatPart sh[STAT_G];
  const StatPart st = stat_merge_all(parts, g, sh);
  const double mean = st.rsum / st.rcnt, sd = sqrt(st.m2 / st.n);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256)
    out[i] = fabs((in[i] - mean) / sd) + 1.0;
}

// ---- np.quantile (method "linear") of an fp64 vector without a sort: exact order statistics by radix selection on the keys.
// _compute_critic_score :307-322 needs the 25 % and 75 % quantiles of the (T,) critic modes; torch.quantile sorted them (a device
// radix sort + seven merge passes + ~15 elementwise launches, ~0.15 ms per 125 000 values, and the two results went through the
// host).  Here: a double maps to a 64-bit key whose unsigned order is the numeric order; the key of the element of rank k is
// fixed 11 bits at a time -- one pass over the data per level histograms the next digit of the elements that still match the
// prefix (LDS histogram per workgroup, non-empty bins added to the level's global histogram), the next level's launch starts by
// scanning that histogram for the bin that holds the rank.  Up to four ranks at once (floor and floor + 1 of two quantiles;
// wave s of a workgroup scans for rank s).  Six levels (11 + 11 + 11 + 11 + 11 + 9 bits), then one workgroup interpolates as
// numpy does.  Any NaN makes every quantile NaN (numpy).  Nothing returns to the host.
constexpr int QS_BITS = 11, QS_BINS = 1 << QS_BITS, QS_LEVELS = 6, QS_SEL = 4;
struct QsState { unsigned long long prefix; long long rank; };
// Round 5: after QS_PRE = THREE levels (33 bits: sign, exponent, 21 mantissa bits) the elements that still match a rank's prefix are a
// handful -- so the fourth launch COMPACTS them (their keys into a per-rank candidate list, with the list's minimum and maximum) and
// one workgroup of 1 024 threads finishes: 256 threads per rank run the three remaining radix levels over its list, then numpy's
// interpolation.  Five launches instead of seven (each is a chain of dependent memory round trips: ~9 us of stream time apiece).
// (Two levels were measured first: critic scores cluster around a non-zero mean -- bench.py's sit in a band 2 % wide -- and a 22-bit bin,
// 2^-10 of the magnitude wide, then held 3 % of the values: 3 000 candidates per rank at 125 000 values, 30 000 at 10^6.)
// A list whose keys are all equal (heavy ties, constant input) needs no list at all (minimum == maximum is the answer); a list longer
// than QS_CAND (all values inside a band 2^-21 of their magnitude wide, not all equal) falls back to the same three levels over the
// input itself, 256 threads per rank with four loads in flight each -- exact, ~0.1 ms per million values and level.
constexpr int QS_CAND = 4096, QS_PRE = 3;
struct QsWs {                       // layout of the workspace (hypad_quantile_workspace_bytes)
  unsigned int* hist;               // [QS_LEVELS][QS_SEL][QS_BINS] (levels 0 and 1 in use), zeroed by the call's memset
  QsState* state;                   // [QS_LEVELS + 1][QS_SEL]
  unsigned int* nan_count;          // [1] (inside the zeroed region)
  unsigned int* cand_count;         // [QS_SEL] (zeroed)
  unsigned long long* kmax;         // [QS_SEL] largest candidate key (zeroed)
  unsigned long long* kinv;         // [QS_SEL] largest ~key = ~(smallest candidate key) (zeroed)
  unsigned long long* cand;         // [QS_SEL][QS_CAND]
};
constexpr size_t QS_HIST_BYTES = (size_t)QS_LEVELS * QS_SEL * QS_BINS * sizeof(unsigned int);
constexpr size_t QS_ZERO_BYTES = QS_HIST_BYTES + 128;
constexpr size_t QS_STATE_BYTES = (QS_LEVELS + 1) * QS_SEL * sizeof(QsState) + 64;
constexpr size_t QS_WS_BYTES = QS_ZERO_BYTES + QS_STATE_BYTES + (size_t)QS_SEL * QS_CAND * sizeof(unsigned long long);
__host__ __device__ inline int qs_shift(int level) { const int sh = 64 - QS_BITS * (level + 1); return sh < 0 ? 0 : sh; }
__host__ __device__ inline int qs_bins(int level) { return level == QS_LEVELS - 1 ? 1 << (64 - QS_BITS * (QS_LEVELS - 1)) : QS_BINS; }
__device__ __forceinline__ unsigned long long qs_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}
__device__ __forceinline__ double qs_value(unsigned long long k) {
  const unsigned long long b = k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull);
  return __longlong_as_double((long long)b);
}
// Wave `sel` of the block: which bin of hist[level][sel] holds rank st.rank?  The histogram row is first copied to LDS (`stage`,
// >= qs_bins(level) words, private to the wave) with lane-consecutive loads that leave together -- walking it in global memory
// cost one dependent L2 round trip per bin.  Every lane returns the new state.
__device__ __forceinline__ QsState qs_descend_staged(const unsigned int* stage, int level, const QsState st);
__device__ __forceinline__ QsState qs_descend(const unsigned int* __restrict__ hist, int level, const QsState st, unsigned int* stage) {
  const int lane = threadIdx.x & 63, bins = qs_bins(level);
  for (int i = lane; i < bins; i += 64) stage[i] = hist[i];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  return qs_descend_staged(stage, level, st);
}
// ... the same with the level's histogram already in `stage` (LDS)
__device__ __forceinline__ QsState qs_descend_staged(const unsigned int* stage, int level, const QsState st) {
  const int lane = threadIdx.x & 63, bins = qs_bins(level), per = bins / 64;       // 32 (or 8) consecutive bins per lane
  unsigned long long mine = 0;
  for (int i = 0; i < per; ++i) mine += stage[lane * per + i];
  unsigned long long incl = mine;                                                   // inclusive wave scan
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const unsigned long long o = __shfl_up(incl, off, WAVE); if (lane >= off) incl += o; }
  const unsigned long long before = incl - mine, r = (unsigned long long)st.rank;
  const bool here = r >= before && r < incl;                                        // exactly one lane (the ranks are < n)
  int bin = 0; unsigned long long cum = 0;
  if (here) {
    cum = before;
    for (int i = 0; i < per; ++i) { const unsigned int c = stage[lane * per + i]; if (r < cum + c) { bin = lane * per + i; break; } cum += c; }
  }
  const unsigned long long mask = __ballot(here);
  const int src = mask ? __builtin_ctzll(mask) : 0;
  bin = __shfl(bin, src, WAVE); cum = __shfl(cum, src, WAVE);
  QsState nx; nx.prefix = st.prefix | ((unsigned long long)bin << qs_shift(level)); nx.rank = (long long)(r - cum);
  return nx;
}
__global__ __launch_bounds__(256) void qs_level_kernel(const double* __restrict__ in, int64_t n, QsWs ws, int level, int nsel,
                                                         long long r0, long long r1, long long r2, long long r3) {
  __shared__ unsigned int h[QS_SEL][QS_BINS];
  __shared__ QsState cur[QS_SEL];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // The kernel is a chain of dependent memory round trips (previous state -> previous histogram -> data -> histogram update), about a
  // microsecond each; the first round's values do not depend on the scan, so they are requested before it.
  constexpr int PER = 4;                                  // values per thread and round: requested together, then filed
  double x[PER];
  int64_t base = (int64_t)blockIdx.x * (256 * PER);
#pragma unroll
  for (int u = 0; u < PER; ++u) { const int64_t i = base + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  if (wave < nsel) {
    QsState st;
    if (level == 0) { st.prefix = 0; st.rank = wave == 0 ? r0 : wave == 1 ? r1 : wave == 2 ? r2 : r3; }
    else st = qs_descend(ws.hist + ((size_t)(level - 1) * QS_SEL + wave) * QS_BINS, level - 1, ws.state[(level - 1) * QS_SEL + wave], h[wave]);
    if (lane == 0) { cur[wave] = st; if (blockIdx.x == 0) ws.state[level * QS_SEL + wave] = st; }
  }
  __syncthreads();                                                                  // (h doubled as the scan's staging rows)
  for (int i = threadIdx.x; i < QS_SEL * QS_BINS; i += 256) (&h[0][0])[i] = 0u;
  __syncthreads();
  const int sh = qs_shift(level), bins = qs_bins(level);
  const int hi_sh = sh + (level == QS_LEVELS - 1 ? 64 - QS_BITS * (QS_LEVELS - 1) : QS_BITS);     // bits above the digit
  unsigned long long pre[QS_SEL];
  for (int s2 = 0; s2 < QS_SEL; ++s2) pre[s2] = s2 < nsel ? cur[s2].prefix : 0;
  unsigned int nans = 0;
  for (; base < n; base += (int64_t)gridDim.x * (256 * PER)) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      if (base + u * 256 + threadIdx.x >= n) continue;
      if (level == 0 && x[u] != x[u]) ++nans;
      const unsigned long long k = qs_key(x[u]);
      const unsigned int digit = (unsigned int)(k >> sh) & (unsigned int)(bins - 1);
#pragma unroll
      for (int s2 = 0; s2 < QS_SEL; ++s2)
        if (s2 < nsel && (hi_sh >= 64 || ((k ^ pre[s2]) >> hi_sh) == 0)) atomicAdd(&h[s2][digit], 1u);
    }
    const int64_t nb = base + (int64_t)gridDim.x * (256 * PER);
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int64_t i = nb + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  }
  if (level == 0 && nans) atomicAdd(ws.nan_count, nans);
  __syncthreads();
  unsigned int* g = ws.hist + (size_t)level * QS_SEL * QS_BINS;
  for (int i = threadIdx.x; i < nsel * QS_BINS; i += 256) {
    const unsigned int c = (&h[0][0])[i];
    if (c) atomicAdd(g + i, c);
  }
}
// launch QS_PRE + 1: the keys that match a rank's 33-bit prefix -> that rank's candidate list (+ the list's extremes)
__global__ __launch_bounds__(256) void qs_compact_kernel(const double* __restrict__ in, int64_t n, QsWs ws, int nsel) {
  __shared__ unsigned int h[QS_SEL][QS_BINS];
  __shared__ QsState cur[QS_SEL];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int PER = 4;
  double x[PER];
  int64_t base = (int64_t)blockIdx.x * (256 * PER);
#pragma unroll
  for (int u = 0; u < PER; ++u) { const int64_t i = base + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  if (wave < nsel) {
    const QsState st = qs_descend(ws.hist + ((size_t)(QS_PRE - 1) * QS_SEL + wave) * QS_BINS, QS_PRE - 1, ws.state[(QS_PRE - 1) * QS_SEL + wave], h[wave]);
    if (lane == 0) { cur[wave] = st; if (blockIdx.x == 0) ws.state[QS_PRE * QS_SEL + wave] = st; }
  }
  __syncthreads();
  const int hi_sh = qs_shift(QS_PRE - 1);                 // the 33 bits fixed so far sit above it
  unsigned long long pre[QS_SEL];
  for (int s2 = 0; s2 < QS_SEL; ++s2) pre[s2] = s2 < nsel ? cur[s2].prefix : 0;
  for (; base < n; base += (int64_t)gridDim.x * (256 * PER)) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      if (base + u * 256 + threadIdx.x >= n) continue;
      const unsigned long long k = qs_key(x[u]);
#pragma unroll
      for (int s2 = 0; s2 < QS_SEL; ++s2)
        if (s2 < nsel && ((k ^ pre[s2]) >> hi_sh) == 0) {
          const unsigned int pos = atomicAdd(ws.cand_count + s2, 1u);
          if (pos < (unsigned int)QS_CAND) ws.cand[(size_t)s2 * QS_CAND + pos] = k;
          atomicMax(ws.kmax + s2, k);
          atomicMax(ws.kinv + s2, ~k);
        }
    }
    const int64_t nb = base + (int64_t)gridDim.x * (256 * PER);
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int64_t i = nb + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  }
}
__device__ __forceinline__ double np_lerp64(double a, double b, double t) {     // numpy.lib._function_base_impl._lerp
#pragma clang fp contract(off)                   // numpy rounds the product before the sum: no fused multiply-add here
  const double diff = b - a;
  double r = a + diff * t;
  if (t >= 0.5) r = b - diff * (1.0 - t);
  return r;
}
// one workgroup of 1 024 threads: threads [256 s, 256 s + 256) fix the remaining 31 bits of rank s's key from its candidate list (see
// QS_CAND), the four groups in lock step; then out[j] = lerp(x[floor], x[floor + 1], frac) for the nq quantiles
__global__ __launch_bounds__(1024) void qs_final_kernel(const double* __restrict__ in, int64_t n, QsWs ws, int nsel, double t0, double t1,
                                                          double* __restrict__ out) {
  __shared__ unsigned long long keys[QS_SEL];
  __shared__ unsigned int stage[QS_SEL][QS_BINS];
  __shared__ QsState cur[QS_SEL];
  const int grp = threadIdx.x >> 8, tg = threadIdx.x & 255, lane = threadIdx.x & 63;
  const bool live = grp < nsel;
  QsState st = ws.state[QS_PRE * QS_SEL + (live ? grp : 0)];
  const unsigned int c = live ? ws.cand_count[grp] : 0u;
  const unsigned long long kmx = live ? ws.kmax[grp] : 0ull, kmn = live ? ~ws.kinv[grp] : 0ull;
  const bool decided = !live || kmx == kmn;                // (group-uniform) every candidate is the same key
  const bool listed = c <= (unsigned int)QS_CAND;
  const unsigned long long* cand = ws.cand + (size_t)(live ? grp : 0) * QS_CAND;
  const int64_t m = decided ? 0 : (listed ? (int64_t)c : n);
  unsigned int* hst = stage[live ? grp : 0];
  for (int level = QS_PRE; level < QS_LEVELS; ++level) {   // (block-uniform trip count; a decided group only keeps the barriers)
    const int bins = qs_bins(level), sh = qs_shift(level);
    const int hi_sh = sh + (level == QS_LEVELS - 1 ? 64 - QS_BITS * (QS_LEVELS - 1) : QS_BITS);     // bits above the digit (<= 31)
    for (int i = tg; i < bins; i += 256) hst[i] = 0u;
    __syncthreads();
    for (int64_t i0 = 0; i0 < m; i0 += 4 * 256) {          // four loads in flight per thread
      unsigned long long k[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + u * 256 + tg;
        k[u] = i < m ? (listed ? cand[i] : qs_key(in[i])) : ~st.prefix;      // (~prefix never matches)
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (((k[u] ^ st.prefix) >> hi_sh) == 0) atomicAdd(hst + ((unsigned int)(k[u] >> sh) & (unsigned int)(bins - 1)), 1u);
    }
    __syncthreads();
    if (tg < 64 && !decided) {                             // the group's first wave scans its histogram
      const QsState nx = qs_descend_staged(hst, level, st);
      if (lane == 0) cur[grp] = nx;
    }
    __syncthreads();
    if (!decided) st = cur[grp];
  }
  if (live && tg == 0) keys[grp] = decided ? kmx : st.prefix;
  __syncthreads();
  if (threadIdx.x < nsel / 2) {
    const int j = threadIdx.x;
    double r = np_lerp64(qs_value(keys[2 * j]), qs_value(keys[2 * j + 1]), j == 0 ? t0 : t1);
    if (*ws.nan_count) r = __longlong_as_double(0x7ff8000000000000ll);
    out[j] = r;
  }
}
QsWs qs_ws(void* workspace) {
  QsWs w; char* p = (char*)workspace;
  w.hist = (unsigned int*)p; w.nan_count = (unsigned int*)(p + QS_HIST_BYTES); w.state = (QsState*)(p + QS_ZERO_BYTES);
  w.cand_count = (unsigned int*)(p + QS_HIST_BYTES + 16);
  w.kmax = (unsigned long long*)(p + QS_HIST_BYTES + 32); w.kinv = (unsigned long long*)(p + QS_HIST_BYTES + 64);      // (all inside the zeroed region)
  w.cand = (unsigned long long*)(p + QS_ZERO_BYTES + QS_STATE_BYTES);
  return w;
}
// numpy (_function_base_impl._quantile, method "linear"): virtual index (n - 1) q, neighbours floor and floor + 1 (both the last
// element once the index reaches n - 1), weight = index - floor
inline void qs_position(int64_t n, double q, long long* lo, long long* hi, double* frac) {
  const double pos = (double)(n - 1) * q;
  const double f = floor(pos);
  long long l = (long long)f;
  *frac = pos - f;
  if (pos >= (double)(n - 1)) { *lo = n - 1; *hi = n - 1; return; }
  if (l < 0) l = 0;
  *lo = l; *hi = l + 1 > n - 1 ? n - 1 : l + 1;
}
__global__ __launch_bounds__(256) void qs_zero_kernel(unsigned* __restrict__ p, int words) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < words) p[i] = 0u;
}
int launch_quantiles(const double* in, int64_t n, const double* q, int nq, double* out, void* workspace, hipStream_t s) {
  const QsWs ws = qs_ws(workspace);
  // (a kernel, not hipMemsetAsync: captured into a graph a memset node between kernels proved unreliably ordered on ROCm 7.2 --
  // critic_fused.hip run_critic_phase, round 6; the scoring pass is replayed from a graph too)
  static_assert(QS_ZERO_BYTES % 4 == 0, "whole words");
  hipLaunchKernelGGL(qs_zero_kernel, dim3((unsigned)((QS_ZERO_BYTES / 4 + 255) / 256)), dim3(256), 0, s, (unsigned*)workspace, (int)(QS_ZERO_BYTES / 4));
  HYPAD_CHECK_LAUNCH();
  long long r[QS_SEL] = {0, 0, 0, 0};
  double t[2] = {0.0, 0.0};
  for (int j = 0; j < nq; ++j) qs_position(n, q[j], &r[2 * j], &r[2 * j + 1], &t[j]);
  const int nsel = 2 * nq;
  int64_t g = (n + 1023) / 1024;
  g = g < 1 ? 1 : (g > 1024 ? 1024 : g);
  for (int level = 0; level < QS_PRE; ++level) {
    hipLaunchKernelGGL(qs_level_kernel, dim3((unsigned)g), dim3(256), 0, s, in, n, ws, level, nsel, r[0], r[1], r[2], r[3]);
    HYPAD_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(qs_compact_kernel, dim3((unsigned)g), dim3(256), 0, s, in, n, ws, nsel);
  HYPAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(qs_final_kernel, dim3(1), dim3(1024), 0, s, in, n, ws, nsel, t[0], t[1], out);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

__global__ __launch_bounds__(THREADS) void row_norms_kernel(const float* __restrict__ x, double* __restrict__ out, int64_t rows, int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * (THREADS / 64)) {
    float s = 0.f;    // np.linalg.norm on float32 reduces in float32
    for (int c = lane; c < dim; c += 64) { float v = x[r * dim + c]; s += v * v; }
    s = wave_sum(s);
    if (lane == 0) out[r] = (double)sqrtf(s);
  }
}

__global__ __launch_bounds__(THREADS) void combine_kernel(int mode, const double* __restrict__ c, const double* __restrict__ r,
                                                           const double* __restrict__ u, double* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
    double cv = c ? c[i] : 0.0, rv = r ? r[i] : 0.0, uv = u ? u[i] : 0.0, o;
    switch (mode) {
      case HYPAD_COMB_SUM: o = 0.2 * cv + 0.8 * rv; break;
      case HYPAD_COMB_MULT: o = cv * rv; break;
      case HYPAD_COMB_UNCERTAINTY: o = cv * rv * uv; break;
      case HYPAD_COMB_CRITIC: o = cv; break;
      case HYPAD_COMB_CRITIC_UNCERTAINTY: o = cv * uv; break;
      case HYPAD_COMB_SUM_UNCERTAINTY: o = 0.5 * cv * uv + 0.5 * rv * uv; break;
      case HYPAD_COMB_REC: o = rv; break;
      case HYPAD_COMB_REC_UNCERTAINTY: o = rv * uv; break;
      case HYPAD_COMB_EUCL_MULT: o = cv * rv; break;
      default: o = 0.5 * (cv - 1.0) + 0.5 * (rv - 1.0); break;   // HYPAD_COMB_EUCL_SUM, lambda_rec = 0.5
    }
    out[i] = o;
  }
}

// ------------------------------------------------------------------------------------------------ signal groups
// Segmented combine (hypad_combine_scores_signals): grid (blocks, segments of the launch); segment blockIdx.y (a scalar) writes its rows
// row_off[s] .. row_off[s + 1] from critic scores that start at row_off[s] + s * (window - 1) -- each segment's critic scores are
// the n_s + window - 1 timesteps of its own final_critic_scores.  Per element combine_kernel's arithmetic.
constexpr int SEG_CHUNK = 64;
struct SegTable { int n, seg0; int64_t off[SEG_CHUNK + 1]; };
__global__ __launch_bounds__(THREADS) void combine_signals_kernel(int mode, const double* __restrict__ c, const double* __restrict__ r,
                                                                   const double* __restrict__ u, double* __restrict__ out, SegTable t, int window) {
  const int sl = blockIdx.y;
  const int64_t o = t.off[sl], n = t.off[sl + 1] - o, co = o + (int64_t)(t.seg0 + sl) * (window - 1);
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
    double cv = c ? c[co + i] : 0.0, rv = r ? r[o + i] : 0.0, uv = u ? u[o + i] : 0.0, v;
    switch (mode) {
      case HYPAD_COMB_SUM: v = 0.2 * cv + 0.8 * rv; break;
      case HYPAD_COMB_MULT: v = cv * rv; break;
      case HYPAD_COMB_UNCERTAINTY: v = cv * rv * uv; break;
      case HYPAD_COMB_CRITIC: v = cv; break;
      case HYPAD_COMB_CRITIC_UNCERTAINTY: v = cv * uv; break;
      case HYPAD_COMB_SUM_UNCERTAINTY: v = 0.5 * cv * uv + 0.5 * rv * uv; break;
      case HYPAD_COMB_REC: v = rv; break;
      case HYPAD_COMB_REC_UNCERTAINTY: v = rv * uv; break;
      case HYPAD_COMB_EUCL_MULT: v = cv * rv; break;
      default: v = 0.5 * (cv - 1.0) + 0.5 * (rv - 1.0); break;   // HYPAD_COMB_EUCL_SUM, lambda_rec = 0.5
    }
    out[o + i] = v;
  }
}
__global__ __launch_bounds__(THREADS) void fill_nan_kernel(double* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) out[i] = __builtin_nan("");
}
// offsets of a group: row_off[0] = 0, every segment > 0 rows
int seg_check(int n_signals, const int64_t* row_off) {
  if (n_signals < 1 || !row_off || row_off[0] != 0) return HYPAD_EINVAL;
  for (int i = 0; i < n_signals; ++i) if (row_off[i + 1] <= row_off[i]) return HYPAD_EINVAL;
  return HYPAD_OK;
}

// ---- Euclidean (TadGAN) scores of a group: score_anomalies :407-576 for every segment at once, in TIMESTEP LAYOUT (include/hypad.h).
// Every kernel below takes its segment from blockIdx.y -- a scalar: the segment's offsets come out of the kernel arguments with scalar
// loads and every clip is against the segment's own ends -- and does, per output element, what the single-signal kernel above does
// on that segment alone.
__device__ __forceinline__ int64_t seg_toff(const SegTable& t, int sl, int window) { return t.off[sl] + (int64_t)(t.seg0 + sl) * (window - 1); }

// unroll_median_kernel<EPL, true, UT> without the summary, per segment: grid (tiles, segments).  A tile lies inside one segment (the
// tile loop runs over the segment's own timesteps), the interior fast path holds for tiles inside it, n / T are the segment's.
// (The tile loop is a copy, not a shared function: with the loop moved into one the single-signal kernels' register allocation
// changed -- their code objects are held identical.)
template <int EPL, int UT>
__global__ __launch_bounds__(UT * 4) __attribute__((amdgpu_waves_per_eu(UNROLL_WPE, UNROLL_WPE))) void unroll_median_signals_kernel(
    const float* __restrict__ y_all, float* __restrict__ median_all, SegTable tab, int W) {
  const int sl = blockIdx.y;
  const int64_t n = tab.off[sl + 1] - tab.off[sl];
  const float* __restrict__ y_hat = y_all + tab.off[sl] * W;
  float* __restrict__ median = median_all + seg_toff(tab, sl, W);
  constexpr int THREADS = UT * 4;                           // (shadows the file's 256: this kernel's block size follows its tile)
  constexpr int RUN = UT / 64;                               // elements per lane of one source row's run
  extern __shared__ __attribute__((aligned(16))) float usm[];
  const int WS = (W + 3) & ~3;                              // tile row stride (floats)
  float* tile = usm;                                        // [UT][WS]
  float* sorted = usm + UT * WS;                            // [waves][MAX_WINDOW]   (summary / candidates)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  constexpr int NWV = THREADS / 64;
  const int64_t T = n + W - 1;
  float* s = sorted + (wave_s) * MAX_WINDOW;
  const float INF = __int_as_float(0x7f800000);
  for (int64_t t0 = (int64_t)blockIdx.x * UT; t0 < T; t0 += (int64_t)gridDim.x * UT) {
    // ---- stage: rows r in [t0 - (W - 1), t0 + UT) (clipped to the matrix), their runs of this tile's timesteps
    constexpr int RB = 8 / RUN;                              // rows in flight per wave (8 loads per lane either way)
    if (t0 >= W - 1 && t0 + UT <= n) {
      // interior tile (all but the first and last two of a long series): no clipping, j0 == 0, 32-bit indices relative to the
      // tile's first row, the row number a scalar -- ~9 vector instructions per row and lane instead of ~30 of 64-bit arithmetic
      const float* base = y_hat + (t0 - (W - 1)) * W;
      const int nrows = W + UT - 1;
      for (int kb = wave_s * RB; kb < nrows; kb += NWV * RB) {
        float val[RB][RUN];
        int dst[RB][RUN];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
          const int k = kb + u;                              // (scalar) row of the tile's parallelogram
          const int jb = W - 1 - k > 0 ? W - 1 - k : 0;
#pragma unroll
          for (int h = 0; h < RUN; ++h) {
            const int j = jb + lane + 64 * h, tt = k - (W - 1) + j;
            const bool ok = k < nrows && j < W && tt < UT;
            dst[u][h] = ok ? tt * WS + j : -1;
            val[u][h] = ok ? base[k * W + j] : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < RB; ++u)
#pragma unroll
          for (int h = 0; h < RUN; ++h)
            if (dst[u][h] >= 0) tile[dst[u][h]] = val[u][h];
      }
    } else {
      const int64_t r_lo = t0 - (W - 1) > 0 ? t0 - (W - 1) : 0;
      const int64_t r_hi = t0 + UT < n ? t0 + UT : n;         // exclusive
      for (int64_t rb = r_lo + wave * RB; rb < r_hi; rb += NWV * RB) {
        float val[RB][RUN];
        int dst[RB][RUN];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
          const int64_t r = rb + u;
          const int jb = (int)(t0 - r > 0 ? t0 - r : 0);       // first column of row r inside the tile
#pragma unroll
          for (int h = 0; h < RUN; ++h) {
            const int j = jb + lane + 64 * h;                  // (a run is at most UT columns: RUN elements per lane)
            const int64_t t = r + j;
            dst[u][h] = -1; val[u][h] = 0.f;
            if (r < r_hi && j < W && t < t0 + UT && t < T) {
              const int j0 = (int)(t - n + 1 > 0 ? t - n + 1 : 0);
              dst[u][h] = (int)(t - t0) * WS + (j - j0);
              val[u][h] = y_hat[r * W + j];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < RB; ++u)
#pragma unroll
          for (int h = 0; h < RUN; ++h)
            if (dst[u][h] >= 0) tile[dst[u][h]] = val[u][h];
      }
    }
    __syncthreads();
    // (round 6: the timestep a wave works on is a scalar -- as a vector value every count, address and "wave-uniform" branch below was
    // vector arithmetic and exec-mask code)
    for (int tt = wave_s; tt < UT; tt += NWV) {
      const int64_t t = t0 + tt;
      if (t >= T) break;
      const int j0 = (int)(t - n + 1 > 0 ? t - n + 1 : 0);
      const int j1 = (int)(t + 1 < W ? t + 1 : W);
      const int cnt = j1 - j0;
      float* v = tile + tt * WS;
      // pad the row to a multiple of 4 with +inf (never below or equal to a finite value)
      if (lane < 4 && cnt + lane < ((cnt + 3) & ~3)) v[cnt + lane] = INF;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): LDS writes of this wave landed
      float mine[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) { const int i = lane + 64 * e; mine[e] = i < cnt ? v[i] : INF; }
      const int m1 = (cnt - 1) >> 1, m2 = cnt >> 1;
      float lo_med = 0.f, hi_med = 0.f;
      bool done = false;
      if (cnt >= 64) {                                       // wave-uniform (FILTER: median only)
        // ranks inside the sample v[0 .. 31] (lanes >= 32 idle along)
        const float sv = v[lane & 31];
        int less = 0;
#pragma unroll
        for (int k0 = 0; k0 < 32; k0 += 4) {
          const float4 q = *reinterpret_cast<const float4*>(v + k0);
          less += (q.x < sv ? 1 : 0) + (q.y < sv ? 1 : 0) + (q.z < sv ? 1 : 0) + (q.w < sv ? 1 : 0);
        }
        float plo = less <= 10 ? sv : -INF, phi = less >= 21 ? sv : INF;     // 11th smallest (largest with <= 10 below), 22nd smallest
        plo = hypad::wave_max(plo); phi = hypad::wave_min(phi);                // (DPP butterflies: no LDS round trips on this chain)
        int c_lt = 0, c_le = 0;
        unsigned long long cm[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const bool in = lane + 64 * e < cnt;
          c_lt += __builtin_popcountll(__ballot(in && mine[e] < plo));
          c_le += __builtin_popcountll(__ballot(in && mine[e] <= phi));
          cm[e] = __ballot(in && mine[e] >= plo && mine[e] <= phi);
        }
        const int nc = c_le - c_lt;
        if (c_lt <= m1 && m2 < c_le && nc <= 64 && nc > 0) {
          // compact the candidates into the wave's slab, rank them against each other
          int base = 0;
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(cm[e] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)cm[e], 0u));
            if ((cm[e] >> lane) & 1ull) s[pos] = mine[e];
            base += __builtin_popcountll(cm[e]);
          }
          if (lane < 4 && nc + lane < ((nc + 3) & ~3)) s[nc + lane] = INF;
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_s_waitcnt(0xc07f);
          const float c = lane < nc ? s[lane] : INF;
          int rk = 0;
          for (int k0 = 0; k0 < nc; k0 += 4) {
            const float4 q = *reinterpret_cast<const float4*>(s + k0);
            rk += (q.x < c ? 1 : 0) + (q.y < c ? 1 : 0) + (q.z < c ? 1 : 0) + (q.w < c ? 1 : 0);
          }
          // without ties the "less" counts are a permutation of 0 .. nc - 1 (their sum tells): then the lanes holding local ranks
          // m1 - c_lt and m2 - c_lt hold the two middle values
          const float rsum = hypad::wave_sum(lane < nc ? (float)rk : 0.f);
          if (rsum == 0.5f * (float)nc * (float)(nc - 1)) {
            const unsigned long long k1 = __ballot(lane < nc && rk == m1 - c_lt), k2 = __ballot(lane < nc && rk == m2 - c_lt);
            lo_med = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), (int)__builtin_ctzll(k1)));
            hi_med = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), (int)__builtin_ctzll(k2)));
            done = true;
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
      if (!done) {
        // rank = #{k : v[k] < mine} + #{k < i : v[k] == mine}.  Fast pass: count "less" only (one compare + add-carry per value).
        // Without ties those counts are a permutation of 0 .. cnt-1, with ties two values share a count and the counts' sum falls
        // short of cnt (cnt - 1) / 2: only then is the ordered tie count needed.  (The sum is exact in fp32: < 2^15 at window 256.)
        int rank[EPL];
#pragma unroll
        for (int e = 0; e < EPL; ++e) rank[e] = 0;
        for (int k0 = 0; k0 < cnt; k0 += 4) {
          const float4 q = *reinterpret_cast<const float4*>(v + k0);
          const float vk[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < EPL; ++e) rank[e] += vk[u] < mine[e] ? 1 : 0;
        }
        float rsum = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) rsum += lane + 64 * e < cnt ? (float)rank[e] : 0.f;
        const bool ties = hypad::wave_sum(rsum) != 0.5f * (float)cnt * (float)(cnt - 1);
        if (ties) {                                      // wave-uniform
#pragma unroll
          for (int e = 0; e < EPL; ++e) rank[e] = 0;
          for (int k = 0; k < cnt; ++k) {
            const float vk = v[k];
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
              const int i = lane + 64 * e;
              rank[e] += (vk < mine[e]) || (vk == mine[e] && k < i);
            }
          }
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e)
          if (lane + 64 * e < cnt) s[rank[e]] = mine[e];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xc07f);
        lo_med = s[m1]; hi_med = s[m2];
      }
      if (lane == 0) {
        median[t] = (cnt & 1) ? lo_med : (lo_med + hi_med) * 0.5f;     // np.median of float32 stays float32
      }
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
  }
}


// area_error_kernel per segment
__global__ __launch_bounds__(THREADS) void area_error_signals_kernel(const double* __restrict__ y_all, const float* __restrict__ yh_all,
                                                                      double* __restrict__ out_all, SegTable tab, int window, int w) {
  const int sl = blockIdx.y;
  const int64_t to = seg_toff(tab, sl, window), T = tab.off[sl + 1] - tab.off[sl] + window - 1;
  const double* __restrict__ y = y_all + to;
  const float* __restrict__ yh = yh_all + to;
  double* __restrict__ out = out_all + to;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < T; i += (int64_t)gridDim.x * THREADS) {
    int64_t lo, hi;
    centred_window(i, w, T, lo, hi);
    if (hi - lo + 1 < w / 2) { out[i] = NAN; continue; }
    double a = 0.0, b = 0.0;
    for (int64_t k = lo; k < hi; ++k) {
      a += (y[k] + y[k + 1]) * 0.5;
      b += ((double)yh[k] + (double)yh[k + 1]) * 0.5;
    }
    out[i] = fabs(a - b);
  }
}
// dtw_error_kernel<LEN> per segment (the zero framing against the segment's T)
template <int LEN>
__global__ __launch_bounds__(THREADS) void dtw_error_signals_kernel(const double* __restrict__ y_all, const float* __restrict__ yh_all,
                                                                     double* __restrict__ out_all, SegTable tab, int window) {
  constexpr int HALF = LEN / 2;
  const int sl = blockIdx.y;
  const int64_t to = seg_toff(tab, sl, window), T = tab.off[sl + 1] - tab.off[sl] + window - 1;
  const double* __restrict__ y = y_all + to;
  const float* __restrict__ yh = yh_all + to;
  double* __restrict__ out = out_all + to;
  for (int64_t p = (int64_t)blockIdx.x * THREADS + threadIdx.x; p < T; p += (int64_t)gridDim.x * THREADS) {
    const int64_t i = p - HALF;                 // window start in padded coordinates
    if (i < 0 || i >= T - LEN) { out[p] = 0.0; continue; }
    double a[LEN], b[LEN], row[LEN];
#pragma unroll
    for (int k = 0; k < LEN; ++k) {
      int64_t src = i + k - HALF;               // y_pad[i + k] = y[i + k - HALF]
      bool ok = src >= 0 && src < T;
      a[k] = ok ? y[src] : 0.0;
      b[k] = ok ? (double)yh[src] : 0.0;
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < LEN; ++j) { double d = a[0] - b[j]; acc += d * d; row[j] = acc; }
#pragma unroll
    for (int r = 1; r < LEN; ++r) {
      double diag = row[0];
      double d0 = a[r] - b[0];
      row[0] = row[0] + d0 * d0;
#pragma unroll
      for (int j = 1; j < LEN; ++j) {
        double up = row[j];
        double d = a[r] - b[j];
        double m = fmin(fmin(up, row[j - 1]), diag);
        row[j] = d * d + m;
        diag = up;
      }
    }
    out[p] = sqrt(row[LEN - 1]);
  }
}

// The smoothing, statistics and z-score of up to three error kinds (blockIdx.z) of every segment (blockIdx.y).  Kind k smooths src[k]
// (the point-wise error fused as in RollSrc) into out[k], which the z-score then rewrites in place.  Per segment: the smoothing window
// trunc(n_s * 0.01) of score_anomalies (0: all NaN, rolling_mean's fill), the chunk sums aligned to the segment's start (origin 0),
// stat_blocks(T_s) slices.  Chunk sums of segment s start at slot (toff_s >> 4) + 2 s resp. (toff_s >> 8) + 2 s of the kind's arrays
// (segments need at most T_s / 16 + 1 resp. T_s / 256 + 1 slots: no overlap), its partials at [(kind, s)][STAT_G].
struct RecKinds { RollSrc src[3]; double* out[3]; double* s1[3]; double* s2[3]; int* c1[3]; int* c2[3]; StatPart* parts[3]; };
__host__ __device__ inline int seg_smooth_window(int64_t n) { return (int)((double)n * 0.01); }        // math.trunc(n * 0.01), n > 0
__host__ __device__ inline int stat_blocks(int64_t t) { int64_t g = (t + 1023) / 1024; return (int)(g < 1 ? 1 : (g > STAT_G ? STAT_G : g)); }
struct SegRoll {                                   // one segment of one kind, as the single-signal kernels see it
  RollSrc src; RollWs ws; double* out; StatPart* parts; int64_t T; int w;
};
__device__ __forceinline__ SegRoll seg_roll(const RecKinds& kd, const SegTable& tab, int window) {
  const int sl = blockIdx.y, kz = blockIdx.z, sg = tab.seg0 + sl;
  const int64_t n = tab.off[sl + 1] - tab.off[sl], to = seg_toff(tab, sl, window);
  SegRoll r;
  r.T = n + window - 1; r.w = seg_smooth_window(n);
  r.src.in = kd.src[kz].in + to; r.src.sub = kd.src[kz].sub ? kd.src[kz].sub + to : nullptr;
  r.out = kd.out[kz] + to;
  const int64_t b1 = (to >> 4) + 2 * sg, b2 = (to >> 8) + 2 * sg;
  r.ws.s1 = kd.s1[kz] + b1; r.ws.c1 = kd.c1[kz] + b1; r.ws.s2 = kd.s2[kz] + b2; r.ws.c2 = kd.c2[kz] + b2;
  roll_counts(r.T, 0, r.ws.n1, r.ws.n2);
  r.parts = kd.parts[kz] + (size_t)sg * STAT_G;
  return r;
}
// roll_chunks_kernel at origin 0, for the segments whose window takes the chunked path
__global__ __launch_bounds__(THREADS) void roll_chunks_signals_kernel(RecKinds kd, SegTable tab, int window) {
  __shared__ double sh_s[THREADS];
  __shared__ int sh_c[THREADS];
  const SegRoll g = seg_roll(kd, tab, window);
  const int64_t c2_0 = (int64_t)blockIdx.x * 16;                                     // this workgroup's first 256-chunk
  if (g.w <= ROLL_DIRECT_MAX || c2_0 >= g.ws.n2) return;                             // (workgroup-uniform)
  const RollSrc src = g.src; const RollWs ws = g.ws; const int64_t T = g.T;
  const int64_t first1 = c2_0 << 4;                                                  // level-1 slot of its first 16-chunk
  const int64_t j = first1 + threadIdx.x;
  double s = 0.0; int cnt = 0;
  if (j >= 0 && j < ws.n1) {
    const int64_t g0 = j << 4;
#pragma unroll 4
    for (int k = 0; k < RC1; ++k) {
      const int64_t i = g0 + k;
      if (i >= 0 && i < T) { const double v = src(i); if (v == v) { s += v; ++cnt; } }
    }
    ws.s1[j] = s; ws.c1[j] = cnt;
  }
  sh_s[threadIdx.x] = s; sh_c[threadIdx.x] = cnt;
  __syncthreads();
  if (threadIdx.x < 16 && c2_0 + threadIdx.x < ws.n2) {
    double s2 = 0.0; int c2 = 0;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
      const int64_t jj = first1 + 16 * threadIdx.x + k;
      if (jj >= 0 && jj < ws.n1) { s2 += sh_s[16 * threadIdx.x + k]; c2 += sh_c[16 * threadIdx.x + k]; }
    }
    ws.s2[c2_0 + threadIdx.x] = s2; ws.c2[c2_0 + threadIdx.x] = c2;
  }
}
// rolling_mean_kernel<false / true> by the segment's window (workgroup-uniform), fill_nan_kernel's value at window 0
__global__ __launch_bounds__(THREADS) void rolling_mean_signals_kernel(RecKinds kd, SegTable tab, int window) {
  const SegRoll g = seg_roll(kd, tab, window);
  const RollSrc src = g.src; const RollWs ws = g.ws; const int64_t T = g.T; const int w = g.w;
  double* __restrict__ out = g.out;
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < T; i += (int64_t)gridDim.x * THREADS) {
    if (w == 0) { out[i] = __builtin_nan(""); continue; }
    int64_t lo, hi;
    centred_window(i, w, T, lo, hi);
    int cnt = 0;
    double s = 0.0;
    if (w <= ROLL_DIRECT_MAX) {
      for (int64_t k = lo; k <= hi; ++k) {
        const double v = src(k);
        if (v == v) { s += v; ++cnt; }            // pandas skips NaN
      }
    } else {
      const int64_t end = hi + 1;
      int64_t p = lo;
      auto elems = [&](int64_t to) { for (; p < to; ++p) { const double v = src(p); if (v == v) { s += v; ++cnt; } } };
      const int64_t a16 = (p + RC1 - 1) & ~(int64_t)(RC1 - 1);
      elems(a16 < end ? a16 : end);
      while (p + RC1 <= end && (p & (RC2 - 1))) { s += ws.s1[p >> 4]; cnt += ws.c1[p >> 4]; p += RC1; }
      while (p + RC2 <= end) { s += ws.s2[p >> 8]; cnt += ws.c2[p >> 8]; p += RC2; }
      while (p + RC1 <= end) { s += ws.s1[p >> 4]; cnt += ws.c1[p >> 4]; p += RC1; }
      elems(end);
    }
    out[i] = cnt >= w / 2 && cnt > 0 ? s / (double)cnt : NAN;
  }
}
// stat_partials_kernel<false> with the segment cut into stat_blocks(T_s) slices (grid.x = STAT_G: the blocks beyond them leave)
__global__ __launch_bounds__(256) void stat_partials_signals_kernel(RecKinds kd, SegTable tab, int window) {
  __shared__ double sh[4];
  const SegRoll g = seg_roll(kd, tab, window);
  const int64_t T = g.T;
  const int nb = stat_blocks(T);
  if ((int)blockIdx.x >= nb) return;                                                  // (workgroup-uniform)
  const double* __restrict__ in = g.out;
  const int64_t len = (T + nb - 1) / nb;
  const int64_t b = (int64_t)blockIdx.x * len, e = b + len < T ? b + len : T;
  double s = 0.0;
  for (int64_t i = b + threadIdx.x; i < e; i += 256) {
    const double x = in[i];
    s += x;
  }
  const double n = e > b ? (double)(e - b) : 0.0;
  const double mean = n > 0.0 ? block_sum_256(s, sh) / n : 0.0;
  double q = 0.0;
  for (int64_t i = b + threadIdx.x; i < e; i += 256) { const double d = in[i] - mean; q += d * d; }
  q = block_sum_256(q, sh);
  if (threadIdx.x == 0) { StatPart p; p.n = n; p.mean = mean; p.m2 = q; p.rsum = 0.0; p.rcnt = 0.0; g.parts[blockIdx.x] = p; }
}
// zscore_apply_kernel per segment, in place
__global__ __launch_bounds__(256) void zscore_apply_signals_kernel(RecKinds kd, SegTable tab, int window) {
  __shared__ StatPart sh[STAT_G];
  const SegRoll g = seg_roll(kd, tab, window);
  const int64_t T = g.T;
  const StatPart st = stat_merge_all(g.parts, stat_blocks(T), sh);
  const double mean = st.mean, sd = sqrt(st.m2 / st.n);
  double* io = g.out;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
    double z = (io[i] - mean) / sd;
    io[i] = (z != z) ? z : fmax(z, 0.0) + 1.0;  // np.clip keeps NaN
  }
}
// ---- The critic-score chain of a group (hypad_critic_chain_signals): final_critic_scores :365-404 for every segment at once.  As above,
// every kernel takes its segment from blockIdx.y (qs_final_signals_kernel: blockIdx.x) and does on it what the single-signal kernel
// does on that segment alone; the bodies are copies for the reason given at unroll_median_signals_kernel.

// kde_mode_kernel<KPL> per segment: grid (workgroups of the longest segment, segments).  n, the critic values and the modes are the
// segment's (scalars out of the kernel arguments); a timestep's mode depends on its own segment's values only, so the partition of
// the timesteps over workgroups does not matter.
template <int KPL>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(KDE_WPE, KDE_WPE))) void kde_mode_signals_kernel(
    const float* __restrict__ critic_all, double* __restrict__ modes_all, SegTable tab, int W) {
  const int sl = blockIdx.y;
  const int64_t n = tab.off[sl + 1] - tab.off[sl];
  if ((int64_t)blockIdx.x * (THREADS / 64) >= n + W - 1) return;                     // (workgroup-uniform: beyond a short segment's end)
  const float* __restrict__ critic = critic_all + tab.off[sl];
  double* __restrict__ modes = modes_all + seg_toff(tab, sl, W);
  constexpr int WMAX = 64 * KPL;                            // the window class: 9 KB of LDS per workgroup and slot, 18 KB at window 100
  __shared__ double vals[THREADS / 64][WMAX];
  __shared__ __attribute__((aligned(16))) float vals32[THREADS / 64][WMAX + 4];      // + the padding the fp32 pass reads past the end
  __shared__ __attribute__((aligned(16))) float nsq32[THREADS / 64][WMAX + 4];       // -(value^2) for the factored form of the fp32 pass
  __shared__ double terms[THREADS / 64][KDE_CB * WMAX];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t T = n + W - 1;
  double* v = vals[wave];
  float* vf = vals32[wave];
  float* nf = nsq32[wave];
  // per-thread constants of the timestep loop, held in SCALAR registers (they are wave-uniform; as vector values the compiler kept them
  // in scratch memory across the loop: 20 bytes of private segment per lane and two scratch loads per timestep)
  auto uniform = [](double x) __attribute__((always_inline)) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
  };
  // Scott's factor n^(-2/5) for every sample count 1 .. W, one power per thread, once (the 2 (W - 1) edge timesteps have fewer than W
  // samples; a double-precision pow inside the loop -- ~200 instructions, its 40 polynomial constants hoisted into vector registers
  // across the loop -- was what this kernel spilled around)
  __shared__ double scott[WMAX];
  for (int c = threadIdx.x; c < W && c < WMAX; c += THREADS) scott[c] = pow((double)(c + 1), -0.4);
  __syncthreads();
  const double rW1 = uniform(W > 1 ? 1.0 / (double)(W - 1) : 0.0);
  for (int64_t t = (int64_t)blockIdx.x * (THREADS / 64) + wave; t < T; t += (int64_t)gridDim.x * (THREADS / 64)) {
    const int j0 = (int)(t - n + 1 > 0 ? t - n + 1 : 0);
    const int j1 = (int)(t + 1 < W ? t + 1 : W);
    const int cnt = __builtin_amdgcn_readfirstlane(j1 - j0);      // (wave-uniform: the pair loops below run on scalar counters)
    double s = 0.0;
    for (int k = lane; k < cnt; k += 64) {
      const float xf = critic[t - (j0 + k)];
      v[k] = (double)xf;
      vf[k] = xf;
      s += (double)xf;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    const double mean = wave_sum(s) / (double)cnt;
    double q = 0.0;
    for (int k = lane; k < cnt; k += 64) { const double d = v[k] - mean; q += d * d; }
    const double var = cnt > 1 ? wave_sum(q) * (cnt == W ? rW1 : 1.0 / (double)(cnt - 1)) : 0.0;      // np.cov: ddof = 1, `c *= 1 / fact`
    // Scott: factor = n^(-1/5), squared.  (All but the 2 (W - 1) edge timesteps have cnt == W: that power is taken once per
    // thread, not once per timestep -- a double-precision pow is ~200 instructions.)
    const double cov = var * uniform(scott[cnt - 1]);
    double out;
    if (cnt > 1 && cov > 0.0 && cov == cov) {
      // pass 1: fp32 densities of this lane's samples.  exp(-d^2 inv) = exp2(-(c d)^2) with c = sqrt(inv log2 e): the samples are
      // centred and rescaled once (pass 2 reads the fp64 copies), so a pair costs a subtract, a multiply, an exp2 and an add; the
      // slab is padded with +inf to a multiple of four (a padded pair contributes exp2(-inf) = 0) and read four values at a
      // time, every value once for all of the lane's samples.
      // The samples are CENTRED first, in fp64 (densities depend on differences only): rescaling the raw values would leave the
      // fp32 copies with an absolute error of |value| 2^-24 c, which at |mean| / bandwidth beyond ~1e4 exceeds the screen's margin.
      // The scale itself only has to be good to fp32 (an error in it is a slightly different bandwidth for every sample alike: 2e-7
      // relative in the densities): one v_rsq_f32 instead of an fp64 division and square root per timestep; the fp64 1 / (2 cov) that
      // pass 2 uses is taken only when pass 2 runs.  (A covariance outside the fp32 range makes the screen all-NaN or all-equal: pass 2
      // then sees every sample, as before.)
      const double c64 = (double)__builtin_amdgcn_rsqf((float)cov * 1.3862943611198906f);     // sqrt(log2 e / (2 cov))
      float amax = 0.f;
      for (int k = lane; k < cnt; k += 64) {
        const float y = (float)((v[k] - mean) * c64);
        vf[k] = y; nf[k] = -(y * y);
        amax = fmaxf(amax, fabsf(y));
      }
      amax = wave_max(amax);
      // (Measured and dropped in round 3, twice: using the kernel matrix's symmetry -- each unordered pair evaluated once.  With the
      // partner's share delivered by ds_add_f32: 3.28 ms against 0.42 ms for 125 000 windows (LDS float atomics).  With the values
      // parked in a small LDS matrix in chunks of eight steps and collected by the partners after a wave barrier (no atomics,
      // conflict-free strides, immediate offsets): 0.69 ms -- three per-lane LDS operations per pair cost more issue time than the
      // quarter-rate exponential they save; the broadcast form below reads each value once for all 64 lanes.)
      const bool factored = amax <= 8.f;                   // (wave-uniform; NaN -> the direct form)
      if (lane < 4 && cnt + lane < ((cnt + 3) & ~3)) {      // padding to a multiple of four: a pair that contributes exp2(-inf) = 0 in either form
        vf[cnt + lane] = factored ? 0.f : __int_as_float(0x7f800000);
        nf[cnt + lane] = __int_as_float(0xff800000);
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xc07f);
      // (Measured and dropped in round 3: giving the cnt % 64 samples of the last slot 64 / b lanes each -- groups of b = 32, 16, ..
      // samples by the binary digits of the remainder, each lane a share of the values, shares added by xor shuffles: 25 + 13 + 2 steps
      // of four values per lane at window 100 instead of 25 + 25, 20 % fewer exponentials by counter, and no faster: 0.292 against
      // 0.287 ms.  Per-lane LDS addresses and the shuffles cost what the idle lanes did.)
      float d32[KPL], xs[KPL];
      float acc[KPL][4];                                   // one accumulator per position in the group of four: <= ceil(cnt / 4) terms each
#pragma unroll
      for (int u = 0; u < KPL; ++u) {
        const int k = lane + 64 * u;
        xs[u] = vf[k < cnt ? k : 0];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[u][c] = 0.f;
      }
      const int nu = (cnt + 63) >> 6;                                             // sample slots in use (wave-uniform)
      if (factored) {
        // exp2(-(x - v)^2) = exp2(-x^2) exp2(2 x v - v^2): the pair costs a fused multiply-add (2 x in a register, v and -v^2 from
        // LDS), an exp2 and an add -- three issue slots instead of four -- and exp2(-x^2) multiplies the finished sum once.
        // |x|, |v| <= 8 keeps 2 x v - v^2 <= x^2 <= 64 inside the fp32 exponent range and its rounding (the product's and
        // -v^2's: 2^-24 x 64 each at the very worst) inside the budget written out at the threshold below.
        float x2[KPL];
#pragma unroll
        for (int u = 0; u < KPL; ++u) x2[u] = 2.f * xs[u];
        for (int m = 0; m < cnt; m += 4) {
          const float4 q4 = *reinterpret_cast<const float4*>(vf + m);
          const float4 n4 = *reinterpret_cast<const float4*>(nf + m);
          const float vm[4] = {q4.x, q4.y, q4.z, q4.w}, nm[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            if (u >= nu) continue;
            // (two fused multiply-adds per instruction: v_pk_fma_f32 -- the same roundings)
            typedef float v2f __attribute__((ext_vector_type(2)));
            const v2f xx = {x2[u], x2[u]};
            const v2f a01 = __builtin_elementwise_fma(xx, v2f{vm[0], vm[1]}, v2f{nm[0], nm[1]});
            const v2f a23 = __builtin_elementwise_fma(xx, v2f{vm[2], vm[3]}, v2f{nm[2], nm[3]});
            acc[u][0] += __builtin_amdgcn_exp2f(a01.x); acc[u][1] += __builtin_amdgcn_exp2f(a01.y);
            acc[u][2] += __builtin_amdgcn_exp2f(a23.x); acc[u][3] += __builtin_amdgcn_exp2f(a23.y);
          }
        }
#pragma unroll
        for (int u = 0; u < KPL; ++u) d32[u] = ((acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3])) * __builtin_amdgcn_exp2f(-(xs[u] * xs[u]));
      } else {
        for (int m = 0; m < cnt; m += 4) {
          const float4 q4 = *reinterpret_cast<const float4*>(vf + m);
          const float vm[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            if (u >= nu) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) { const float d = xs[u] - vm[c]; acc[u][c] += __builtin_amdgcn_exp2f(-(d * d)); }
          }
        }
#pragma unroll
        for (int u = 0; u < KPL; ++u) d32[u] = (acc[u][0] + acc[u][1]) + (acc[u][2] + acc[u][3]);
      }
      float mx = -1.f;
#pragma unroll
      for (int u = 0; u < KPL; ++u) {
        if (lane + 64 * u >= cnt) d32[u] = -1.f;
        mx = fmaxf(mx, d32[u]);
      }
      mx = wave_max(mx);
      // Relative error of an fp32 density D~ against the exact D, all terms positive.  Direct form, exp2(-(x - v)^2):
      //  * arguments: a centred, rescaled sample y carries 2^-24 |y| <= 1e-6 (|y| < 32 for every pair that contributes: two of <= 256
      //    samples within a few units of each other lie at most 2.6 sqrt(255 / 2) = 29 units from the mean; a lone outlier beyond that
      //    sees only its own term, exactly 1), a difference d twice that, d^2 an absolute 2 |d| 2e-6 (+ 2^-24 d^2 from the product);
      //    a term's relative error is ln 2 times that, and weighted by the terms themselves (|d| 2^(-d^2) <= 0.52, the self term is 1)
      //    the sum's is <= 3e-6;
      //  * v_exp_f32: 1 ulp = 1.2e-7;
      //  * accumulation: four partial sums of <= 64 terms, each add 2^-24 of a partial sum that never exceeds the result: 3.8e-6, + 1.2e-7
      //    for the two combining adds
      // -> eps <= 7.1e-6 at window 256 (4.8e-6 at 100).  Factored form (all |y| <= 8), exp2(-x^2) exp2(2 x v - v^2):
      //  * the samples' own rounding (|y| <= 8: 2^-24 x 8): 0.7e-6 by the same weighting;
      //  * the argument 2 x v - v^2 (|.| <= 64): -v^2 rounded once, the fused multiply-add once, 2^-24 x 64 = 3.8e-6 absolute together
      //    at the very worst -> ln 2 x 3.8e-6 = 2.6e-6;  exp2(-x^2): x^2 rounded (1.9e-6 absolute -> 1.3e-6) + 1 ulp;
      //  * v_exp_f32 1.2e-7, accumulation 3.9e-6 as above, the closing product 6e-8
      // -> eps <= 8.8e-6.  If k* is the true arg-max, D~[k*] >= (1 - eps) D[k*] >= (1 - eps) D[j] >= (1 - eps) / (1 + eps) D~[j] for
      // every j: the screen keeps k* as long as its margin exceeds 2 eps = 1.8e-5.  Margin 4e-5 (rounds 2-3 used 2e-4 with one
      // accumulator per sample: 1.7 fp64 evaluations per timestep on random-normal values, 0.6 now).
      const float thr = mx * (1.f - 4e-5f);
      // pass 2: fp64 densities of the candidates, in ascending sample order (the first maximum is kept); of every sample if
      // pass 1 produced no candidate (a bandwidth so small that its reciprocal leaves the fp32 range makes the screen NaN).
      // A wave pays for a sequential sum as if all 64 lanes ran it, so a candidate's sum is NOT given to one lane with its
      // exponentials: the lanes compute a candidate's cnt exponentials side by side into LDS (two per lane at window 100), four
      // candidates per batch, then lane c adds candidate c's terms in index order -- the same additions in the same order as
      // the one-lane loop, hence the same bits, at 1/20 of its cycles.
      double best = -1.0;
      int besti = 0x7fffffff;
      double* tm = terms[wave];
      {
        // one candidate only: the screen has decided (its margin is far above the fp32 pass's error), no fp64 sum is needed
        int ncand = 0, first = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < KPL; ++u) {
          const unsigned long long mk = __ballot(lane + 64 * u < cnt && d32[u] >= thr);
          ncand += __builtin_popcountll(mk);
          if (mk && first == 0x7fffffff) first = __builtin_ctzll(mk) + 64 * u;
        }
        if (ncand == 1) besti = first;
      }
      double inv = 0.0;
      if (__builtin_amdgcn_readfirstlane(besti) == 0x7fffffff) inv = 0.5 / cov;          // (only the fp64 pass needs it)
      for (int round = 0; round < 2 && besti == 0x7fffffff; ++round) {
        // First the candidates' fp64 densities as TREE sums (a lane's own terms, then the wave's butterfly: no LDS, no sequential add):
        // either order of adding <= 256 positive terms is within 3e-14 of the exact sum, so a candidate more than 1e-12 below the
        // largest tree sum cannot be the arg-max of the ordered sums either.  One survivor (the usual case): it is the arg-max, and
        // the ordered sums -- a lane adding 100 terms one after the other: half of this pass's time -- are not taken at all; several
        // (equal samples, true near-ties): only those go through the ordered sums below, which decide as before.
        bool keep[KPL];
        {
          double dq[KPL];
#pragma unroll
          for (int u = 0; u < KPL; ++u) dq[u] = -1.0;
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            unsigned long long mask = __ballot(lane + 64 * u < cnt && (round == 1 || d32[u] >= thr));
            while (mask) {                                                        // wave-uniform
              const int k = __builtin_ctzll(mask) + 64 * u;
              mask &= mask - 1;
              const double xk = v[k];
              double loc = 0.0;
              for (int m = lane; m < cnt; m += 64) { const double d = xk - v[m]; loc += exp(-d * d * inv); }
              const double dp = wave_sum(loc);
              if (lane == (k & 63)) dq[u] = dp;
            }
          }
          double mx2 = -1.0;
#pragma unroll
          for (int u = 0; u < KPL; ++u) mx2 = fmax(mx2, dq[u]);
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) mx2 = fmax(mx2, __shfl_xor(mx2, off, WAVE));
          const double thr2 = mx2 * (1.0 - 1e-12);
          int nkeep = 0, first = 0x7fffffff;
#pragma unroll
          for (int u = 0; u < KPL; ++u) {
            keep[u] = dq[u] >= thr2 && dq[u] > 0.0;
            const unsigned long long mk = __ballot(keep[u]);
            nkeep += __builtin_popcountll(mk);
            if (mk && first == 0x7fffffff) first = __builtin_ctzll(mk) + 64 * u;
          }
          if (nkeep == 1) { besti = first; break; }
        }
#pragma unroll
        for (int u = 0; u < KPL; ++u) {
          unsigned long long mask = __ballot(keep[u]);
          while (mask) {                                                          // wave-uniform
            int kc[KDE_CB];
            int nb = 0;
#pragma unroll
            for (int c = 0; c < KDE_CB; ++c) {
              kc[c] = -1;
              if (mask) { kc[c] = __builtin_ctzll(mask) + 64 * u; mask &= mask - 1; nb = c + 1; }
            }
#pragma unroll
            for (int c = 0; c < KDE_CB; ++c) {
              if (kc[c] < 0) continue;
              const double xk = v[kc[c]];
              for (int m = lane; m < cnt; m += 64) { const double d = xk - v[m]; tm[c * WMAX + m] = exp(-d * d * inv); }
            }
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);
            double dens = -1.0;
            if (lane < nb) {
              dens = 0.0;
              const double* tp = tm + lane * WMAX;
              int m = 0;
              for (; m + 8 <= cnt; m += 8) {                 // (the terms of eight steps requested together; added in index order)
                double t8[8];
#pragma unroll
                for (int x = 0; x < 8; ++x) t8[x] = tp[m + x];
#pragma unroll
                for (int x = 0; x < 8; ++x) dens += t8[x];
              }
              for (; m < cnt; ++m) dens += tp[m];
            }
#pragma unroll
            for (int c = 0; c < KDE_CB; ++c) {
              const double dc = __shfl(dens, c, WAVE);
              if (c < nb && dc > best) { best = dc; besti = kc[c]; }
            }
            __builtin_amdgcn_wave_barrier();
          }
        }
      }
      out = v[besti < cnt ? besti : 0];                    // (all densities NaN -- a covariance whose reciprocal overflows: scipy's arg-max of NaNs is 0)
    } else {
      // median by rank counting (cnt <= 256)
      double lo = 0.0, hi = 0.0;
      for (int k = lane; k < cnt; k += 64) {
        const double xk = v[k];
        int rank = 0;
        for (int m = 0; m < cnt; ++m) rank += (v[m] < xk) || (v[m] == xk && m < k);
        if (rank == (cnt - 1) / 2) lo = xk;
        if (rank == cnt / 2) hi = xk;
      }
      out = 0.5 * (wave_sum(lo) + wave_sum(hi));
    }
    if (lane == 0) modes[t] = out;
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- np.quantile of every segment at once: the radix selection above with one workspace slice per segment of the launch.  Histogram
// counts are integers and the result an exact order statistic: the grid shape cannot change it.  Workspace of a call (slices = the
// segments of one launch, at most SEG_CHUNK; the chunks of a larger group run one after the other through the same slices):
// [slices x (histograms of the QS_PRE global levels | 128 bytes: NaN count, list lengths, list extremes)]  -- zeroed by qs_zero_kernel,
// [slices x (QsState table | candidate lists)].
constexpr size_t QSS_HIST_BYTES = (size_t)QS_PRE * QS_SEL * QS_BINS * sizeof(unsigned int);
constexpr size_t QSS_ZERO_BYTES = QSS_HIST_BYTES + 128;
constexpr size_t QSS_REST_BYTES = QS_STATE_BYTES + (size_t)QS_SEL * QS_CAND * sizeof(unsigned long long);
static_assert(QSS_ZERO_BYTES % 8 == 0 && QSS_REST_BYTES % 8 == 0, "slices keep 8-byte alignment");
struct QsSegs { char* ws; int slices; int nsel; double q0, q1; };
__device__ __forceinline__ QsWs qs_ws_seg(const QsSegs& a, int sl) {
  QsWs w;
  char* z = a.ws + (size_t)sl * QSS_ZERO_BYTES;
  char* r = a.ws + (size_t)a.slices * QSS_ZERO_BYTES + (size_t)sl * QSS_REST_BYTES;
  w.hist = (unsigned int*)z; w.nan_count = (unsigned int*)(z + QSS_HIST_BYTES); w.cand_count = (unsigned int*)(z + QSS_HIST_BYTES + 16);
  w.kmax = (unsigned long long*)(z + QSS_HIST_BYTES + 32); w.kinv = (unsigned long long*)(z + QSS_HIST_BYTES + 64);
  w.state = (QsState*)r; w.cand = (unsigned long long*)(r + QS_STATE_BYTES);
  return w;
}
// qs_position on the device: the same fp64 operations, each rounded on its own (the product must not fuse into the subtraction)
__device__ __forceinline__ void qs_position_dev(int64_t n, double q, long long* lo, long long* hi, double* frac) {
#pragma clang fp contract(off)
  const double pos = (double)(n - 1) * q;
  const double f = floor(pos);
  long long l = (long long)f;
  *frac = pos - f;
  if (pos >= (double)(n - 1)) { *lo = n - 1; *hi = n - 1; return; }
  if (l < 0) l = 0;
  *lo = l; *hi = l + 1 > n - 1 ? n - 1 : l + 1;
}
// qs_level_kernel per segment: grid (blocks of the longest segment, segments); a block with no value of its segment leaves (block 0
// always has one and writes the level's state)
__global__ __launch_bounds__(256) void qs_level_signals_kernel(const double* __restrict__ in_all, QsSegs a, SegTable tab, int window, int level) {
  __shared__ unsigned int h[QS_SEL][QS_BINS];
  __shared__ QsState cur[QS_SEL];
  const int sl = blockIdx.y;
  const int64_t n = tab.off[sl + 1] - tab.off[sl] + window - 1;
  constexpr int PER = 4;                                  // values per thread and round: requested together, then filed
  int64_t base = (int64_t)blockIdx.x * (256 * PER);
  if (base >= n) return;                                  // (workgroup-uniform)
  const double* __restrict__ in = in_all + seg_toff(tab, sl, window);
  const QsWs ws = qs_ws_seg(a, sl);
  const int nsel = a.nsel;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double x[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) { const int64_t i = base + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  if (wave < nsel) {
    QsState st;
    if (level == 0) {
      long long lo, hi; double fr;
      qs_position_dev(n, wave < 2 ? a.q0 : a.q1, &lo, &hi, &fr);
      st.prefix = 0; st.rank = (wave & 1) ? hi : lo;
    }
    else st = qs_descend(ws.hist + ((size_t)(level - 1) * QS_SEL + wave) * QS_BINS, level - 1, ws.state[(level - 1) * QS_SEL + wave], h[wave]);
    if (lane == 0) { cur[wave] = st; if (blockIdx.x == 0) ws.state[level * QS_SEL + wave] = st; }
  }
  __syncthreads();                                                                  // (h doubled as the scan's staging rows)
  for (int i = threadIdx.x; i < QS_SEL * QS_BINS; i += 256) (&h[0][0])[i] = 0u;
  __syncthreads();
  const int sh = qs_shift(level), bins = qs_bins(level);
  const int hi_sh = sh + (level == QS_LEVELS - 1 ? 64 - QS_BITS * (QS_LEVELS - 1) : QS_BITS);     // bits above the digit
  unsigned long long pre[QS_SEL];
  for (int s2 = 0; s2 < QS_SEL; ++s2) pre[s2] = s2 < nsel ? cur[s2].prefix : 0;
  unsigned int nans = 0;
  for (; base < n; base += (int64_t)gridDim.x * (256 * PER)) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      if (base + u * 256 + threadIdx.x >= n) continue;
      if (level == 0 && x[u] != x[u]) ++nans;
      const unsigned long long k = qs_key(x[u]);
      const unsigned int digit = (unsigned int)(k >> sh) & (unsigned int)(bins - 1);
#pragma unroll
      for (int s2 = 0; s2 < QS_SEL; ++s2)
        if (s2 < nsel && (hi_sh >= 64 || ((k ^ pre[s2]) >> hi_sh) == 0)) atomicAdd(&h[s2][digit], 1u);
    }
    const int64_t nb = base + (int64_t)gridDim.x * (256 * PER);
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int64_t i = nb + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  }
  if (level == 0 && nans) atomicAdd(ws.nan_count, nans);
  __syncthreads();
  unsigned int* g = ws.hist + (size_t)level * QS_SEL * QS_BINS;
  for (int i = threadIdx.x; i < nsel * QS_BINS; i += 256) {
    const unsigned int c = (&h[0][0])[i];
    if (c) atomicAdd(g + i, c);
  }
}
// qs_compact_kernel per segment
__global__ __launch_bounds__(256) void qs_compact_signals_kernel(const double* __restrict__ in_all, QsSegs a, SegTable tab, int window) {
  __shared__ unsigned int h[QS_SEL][QS_BINS];
  __shared__ QsState cur[QS_SEL];
  const int sl = blockIdx.y;
  const int64_t n = tab.off[sl + 1] - tab.off[sl] + window - 1;
  constexpr int PER = 4;
  int64_t base = (int64_t)blockIdx.x * (256 * PER);
  if (base >= n) return;                                  // (workgroup-uniform)
  const double* __restrict__ in = in_all + seg_toff(tab, sl, window);
  const QsWs ws = qs_ws_seg(a, sl);
  const int nsel = a.nsel;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double x[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) { const int64_t i = base + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  if (wave < nsel) {
    const QsState st = qs_descend(ws.hist + ((size_t)(QS_PRE - 1) * QS_SEL + wave) * QS_BINS, QS_PRE - 1, ws.state[(QS_PRE - 1) * QS_SEL + wave], h[wave]);
    if (lane == 0) { cur[wave] = st; if (blockIdx.x == 0) ws.state[QS_PRE * QS_SEL + wave] = st; }
  }
  __syncthreads();
  const int hi_sh = qs_shift(QS_PRE - 1);                 // the 33 bits fixed so far sit above it
  unsigned long long pre[QS_SEL];
  for (int s2 = 0; s2 < QS_SEL; ++s2) pre[s2] = s2 < nsel ? cur[s2].prefix : 0;
  for (; base < n; base += (int64_t)gridDim.x * (256 * PER)) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      if (base + u * 256 + threadIdx.x >= n) continue;
      const unsigned long long k = qs_key(x[u]);
#pragma unroll
      for (int s2 = 0; s2 < QS_SEL; ++s2)
        if (s2 < nsel && ((k ^ pre[s2]) >> hi_sh) == 0) {
          const unsigned int pos = atomicAdd(ws.cand_count + s2, 1u);
          if (pos < (unsigned int)QS_CAND) ws.cand[(size_t)s2 * QS_CAND + pos] = k;
          atomicMax(ws.kmax + s2, k);
          atomicMax(ws.kinv + s2, ~k);
        }
    }
    const int64_t nb = base + (int64_t)gridDim.x * (256 * PER);
#pragma unroll
    for (int u = 0; u < PER; ++u) { const int64_t i = nb + u * 256 + threadIdx.x; x[u] = i < n ? in[i] : 0.0; }
  }
}
// qs_final_kernel, one workgroup of 1 024 threads per segment (blockIdx.x): segment s's quantiles go to out[(seg0 + s) * nq ..]; a list
// longer than QS_CAND falls back to the segment's own input range
__global__ __launch_bounds__(1024) void qs_final_signals_kernel(const double* __restrict__ in_all, QsSegs a, SegTable tab, int window,
                                                                  double* __restrict__ out_all) {
  __shared__ unsigned long long keys[QS_SEL];
  __shared__ unsigned int stage[QS_SEL][QS_BINS];
  __shared__ QsState cur[QS_SEL];
  const int sl = blockIdx.x;
  const int64_t n = tab.off[sl + 1] - tab.off[sl] + window - 1;
  const double* __restrict__ in = in_all + seg_toff(tab, sl, window);
  const QsWs ws = qs_ws_seg(a, sl);
  const int nsel = a.nsel;
  double* __restrict__ out = out_all + (size_t)(tab.seg0 + sl) * (nsel / 2);
  const int grp = threadIdx.x >> 8, tg = threadIdx.x & 255, lane = threadIdx.x & 63;
  const bool live = grp < nsel;
  QsState st = ws.state[QS_PRE * QS_SEL + (live ? grp : 0)];
  const unsigned int c = live ? ws.cand_count[grp] : 0u;
  const unsigned long long kmx = live ? ws.kmax[grp] : 0ull, kmn = live ? ~ws.kinv[grp] : 0ull;
  const bool decided = !live || kmx == kmn;                // (group-uniform) every candidate is the same key
  const bool listed = c <= (unsigned int)QS_CAND;
  const unsigned long long* cand = ws.cand + (size_t)(live ? grp : 0) * QS_CAND;
  const int64_t m = decided ? 0 : (listed ? (int64_t)c : n);
  unsigned int* hst = stage[live ? grp : 0];
  for (int level = QS_PRE; level < QS_LEVELS; ++level) {   // (block-uniform trip count; a decided group only keeps the barriers)
    const int bins = qs_bins(level), sh = qs_shift(level);
    const int hi_sh = sh + (level == QS_LEVELS - 1 ? 64 - QS_BITS * (QS_LEVELS - 1) : QS_BITS);     // bits above the digit (<= 31)
    for (int i = tg; i < bins; i += 256) hst[i] = 0u;
    __syncthreads();
    for (int64_t i0 = 0; i0 < m; i0 += 4 * 256) {          // four loads in flight per thread
      unsigned long long k[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + u * 256 + tg;
        k[u] = i < m ? (listed ? cand[i] : qs_key(in[i])) : ~st.prefix;      // (~prefix never matches)
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (((k[u] ^ st.prefix) >> hi_sh) == 0) atomicAdd(hst + ((unsigned int)(k[u] >> sh) & (unsigned int)(bins - 1)), 1u);
    }
    __syncthreads();
    if (tg < 64 && !decided) {                             // the group's first wave scans its histogram
      const QsState nx = qs_descend_staged(hst, level, st);
      if (lane == 0) cur[grp] = nx;
    }
    __syncthreads();
    if (!decided) st = cur[grp];
  }
  if (live && tg == 0) keys[grp] = decided ? kmx : st.prefix;
  __syncthreads();
  if (threadIdx.x < nsel / 2) {
    const int j = threadIdx.x;
    long long lo, hi; double fr;
    qs_position_dev(n, j == 0 ? a.q0 : a.q1, &lo, &hi, &fr);
    double r = np_lerp64(qs_value(keys[2 * j]), qs_value(keys[2 * j + 1]), fr);
    if (*ws.nan_count) r = __longlong_as_double(0x7ff8000000000000ll);
    out[j] = r;
  }
}

// stat_partials_kernel<true> per segment: the segment cut into stat_blocks(T_s) slices (grid.x = STAT_G: the blocks beyond them leave),
// [lo, hi] = the segment's quantiles in the device table `range` ((seg0 + s) * 2), partials at [s][STAT_G]
__global__ __launch_bounds__(256) void critic_partials_signals_kernel(const double* __restrict__ in_all, const double* __restrict__ range,
                                                                        StatPart* __restrict__ parts_all, SegTable tab, int window) {
  __shared__ double sh[4];
  const int sl = blockIdx.y;
  const int64_t T = tab.off[sl + 1] - tab.off[sl] + window - 1;
  const int nb = stat_blocks(T);
  if ((int)blockIdx.x >= nb) return;                                                  // (workgroup-uniform)
  const double* __restrict__ in = in_all + seg_toff(tab, sl, window);
  const double lo = range[2 * (tab.seg0 + sl)], hi = range[2 * (tab.seg0 + sl) + 1];
  const int64_t len = (T + nb - 1) / nb;
  const int64_t b = (int64_t)blockIdx.x * len, e = b + len < T ? b + len : T;
  double s = 0.0, rs = 0.0, rc = 0.0;
  for (int64_t i = b + threadIdx.x; i < e; i += 256) {
    const double x = in[i];
    s += x;
    if (x >= lo && x <= hi) { rs += x; rc += 1.0; }
  }
  const double n = e > b ? (double)(e - b) : 0.0;
  const double mean = n > 0.0 ? block_sum_256(s, sh) / n : 0.0;
  double q = 0.0;
  for (int64_t i = b + threadIdx.x; i < e; i += 256) { const double d = in[i] - mean; q += d * d; }
  q = block_sum_256(q, sh);
  rs = block_sum_256(rs, sh); rc = block_sum_256(rc, sh);
  if (threadIdx.x == 0) { StatPart p; p.n = n; p.mean = mean; p.m2 = q; p.rsum = rs; p.rcnt = rc; parts_all[(size_t)sl * STAT_G + blockIdx.x] = p; }
}
// critic_apply_kernel per segment
__global__ __launch_bounds__(256) void critic_apply_signals_kernel(const double* __restrict__ in_all, const StatPart* __restrict__ parts_all,
                                                                     double* __restrict__ out_all, SegTable tab, int window) {
  __shared__ StatPart sh[STAT_G];
  const int sl = blockIdx.y;
  const int64_t to = seg_toff(tab, sl, window), T = tab.off[sl + 1] - tab.off[sl] + window - 1;
  if ((int64_t)blockIdx.x * 256 >= T) return;                                         // (workgroup-uniform)
  const double* __restrict__ in = in_all + to;
  double* __restrict__ out = out_all + to;
  const StatPart st = stat_merge_all(parts_all + (size_t)sl * STAT_G, stat_blocks(T), sh);
  const double mean = st.rsum / st.rcnt, sd = sqrt(st.m2 / st.n);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256)
    out[i] = fabs((in[i] - mean) / sd) + 1.0;
}
inline SegTable seg_table(const int64_t* row_off, int c0, int n_signals) {
  SegTable t{};
  t.n = std::min(SEG_CHUNK, n_signals - c0); t.seg0 = c0;
  for (int i = 0; i <= t.n; ++i) t.off[i] = row_off[c0 + i];
  return t;
}
inline int64_t seg_longest(const SegTable& t) {
  int64_t most = 0;
  for (int i = 0; i < t.n; ++i) most = std::max<int64_t>(most, t.off[i + 1] - t.off[i]);
  return most;
}
inline bool segs_fit_2_31(int n_signals, const int64_t* row_off, int window) {      // every segment's timesteps within what a quantile launch indexes
  for (int i = 0; i < n_signals; ++i) if (row_off[i + 1] - row_off[i] + window - 1 > ((int64_t)1 << 31)) return false;
  return true;
}
// The template families: f(std::integral_constant<int, N>) launches the instantiation the run-time value picks, single or segmented.
template <int N> using IntC = std::integral_constant<int, N>;
template <class F> bool dtw_len_dispatch(int len, F&& f) {          // false: no instantiation for this length
  switch (len) {
    case 3: f(IntC<3>{}); return true;
    case 5: f(IntC<5>{}); return true;
    case 7: f(IntC<7>{}); return true;
    case 9: f(IntC<9>{}); return true;
    case 11: f(IntC<11>{}); return true;   // reference default
    case 21: f(IntC<21>{}); return true;
    default: return false;
  }
}
template <class F> void kde_kpl_dispatch(int window, F&& f) {       // (window <= MAX_WINDOW)
  switch ((window + 63) / 64) {
    case 1: f(IntC<1>{}); break;
    case 2: f(IntC<2>{}); break;
    case 3: f(IntC<3>{}); break;
    default: f(IntC<4>{}); break;
  }
}
template <class F> auto unroll_epl_dispatch(int window, F&& f) {    // (returns what f does)
  if (window <= 64) return f(IntC<1>{}); else if (window <= 128) return f(IntC<2>{}); else return f(IntC<4>{});
}
inline size_t unroll_lds_bytes(int ut, int window) { return (size_t)(ut * ((window + 3) & ~3) + (ut / 16) * MAX_WINDOW) * sizeof(float); }      // tile 128: 59 KB at window 100, 139 KB at 256
struct GroupTotals { int64_t total, cap1, cap2; };      // timesteps of a group (timestep layout), slots of its rolling mean's 16- and 256-chunk sums
inline GroupTotals group_totals(int n_signals, const int64_t* row_off, int window) {
  const int64_t total = row_off[n_signals] + (int64_t)n_signals * (window - 1);
  return {total, (total >> 4) + 2 * (int64_t)n_signals + 2, (total >> 8) + 2 * (int64_t)n_signals + 2};
}
// kind k of a RecKinds: its chunk sums and counts are slot k of the arrays at `sums` / `counts`
inline void rec_kind(RecKinds& kd, int k, RollSrc src, double* out, char* sums, char* counts, const GroupTotals& g) {
  kd.src[k] = src; kd.out[k] = out;
  kd.s1[k] = (double*)sums + (size_t)k * (g.cap1 + g.cap2); kd.s2[k] = kd.s1[k] + g.cap1;
  kd.c1[k] = (int*)counts + (size_t)k * (g.cap1 + g.cap2); kd.c2[k] = kd.c1[k] + g.cap1;
}
// workspace of hypad_quantiles_signals (the layout is written out at QSS_HIST_BYTES)
inline int qs_slices(int n_signals) { return std::min(n_signals, SEG_CHUNK); }
inline size_t qss_bytes(int n_signals) { return (size_t)qs_slices(n_signals) * (QSS_ZERO_BYTES + QSS_REST_BYTES); }
// the six launches of launch_quantiles for the segments of one table (timestep layout), quantiles to out[(seg0 + s) * nq ..]
int launch_quantiles_signals(const double* in, const SegTable& t, int slices, int window, const double* q, int nq, double* out, void* workspace,
                             hipStream_t s) {
  const QsSegs a{(char*)workspace, slices, 2 * nq, q[0], nq > 1 ? q[1] : 0.0};
  // (a kernel, not a memset node: see launch_quantiles; the zeroed regions of the launch's slices are contiguous)
  const int words = (int)((size_t)t.n * QSS_ZERO_BYTES / 4);
  hipLaunchKernelGGL(qs_zero_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, (unsigned*)workspace, words);
  HYPAD_CHECK_LAUNCH();
  int64_t g = (seg_longest(t) + window - 1 + 1023) / 1024;
  g = g < 1 ? 1 : (g > 1024 ? 1024 : g);
  const dim3 grid((unsigned)g, (unsigned)t.n);
  for (int level = 0; level < QS_PRE; ++level) {
    hipLaunchKernelGGL(qs_level_signals_kernel, grid, dim3(256), 0, s, in, a, t, window, level);
    HYPAD_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(qs_compact_signals_kernel, grid, dim3(256), 0, s, in, a, t, window);
  HYPAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(qs_final_signals_kernel, dim3((unsigned)t.n), dim3(1024), 0, s, in, a, t, window, out);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
// workspace of hypad_critic_chain_signals: [quantile slices | [q25, q75] per segment | STAT_G partials per slice | the rolling mean's
// 16- and 256-chunk sums, then their counts (slots as in RecKinds) | the unsmoothed scores | the modes when the caller keeps none]
struct ChainWsLayout : GroupTotals { int slices; size_t qs, range, parts, sums, counts, tmp, modes, bytes; };
ChainWsLayout chain_ws_layout(int n_signals, const int64_t* row_off, int window) {
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  ChainWsLayout l;
  static_cast<GroupTotals&>(l) = group_totals(n_signals, row_off, window);
  l.slices = qs_slices(n_signals);
  l.qs = 0;
  l.range = up(qss_bytes(n_signals));
  l.parts = l.range + up((size_t)n_signals * 2 * sizeof(double));
  l.sums = l.parts + up((size_t)l.slices * STAT_G * sizeof(StatPart));
  l.counts = l.sums + (size_t)(l.cap1 + l.cap2) * sizeof(double);
  l.tmp = up(l.counts + (size_t)(l.cap1 + l.cap2) * sizeof(int));
  l.modes = l.tmp + up((size_t)l.total * sizeof(double));
  l.bytes = l.modes + up((size_t)l.total * sizeof(double));
  return l;
}
// workspace of hypad_rec_scores_signals: [area errors | dtw errors] (timestep layout) | per kind [16-chunk sums | 256-chunk sums] | their
// counts | per kind and segment STAT_G partials
struct RecWsLayout : GroupTotals { size_t err, sums, counts, parts, bytes; };
RecWsLayout rec_ws_layout(int n_signals, const int64_t* row_off, int window) {
  RecWsLayout l;
  static_cast<GroupTotals&>(l) = group_totals(n_signals, row_off, window);
  l.err = 0;
  l.sums = l.err + 2 * (size_t)l.total * sizeof(double);
  l.counts = l.sums + 3 * (size_t)(l.cap1 + l.cap2) * sizeof(double);
  l.parts = (l.counts + 3 * (size_t)(l.cap1 + l.cap2) * sizeof(int) + 63) & ~(size_t)63;
  l.bytes = l.parts + 3 * (size_t)n_signals * STAT_G * sizeof(StatPart);
  return l;
}

}  // namespace

extern "C" {

int hypad_unroll_median(const float* y_hat, float* median, double* summary, int64_t n, int window, hypad_stream_t s) {
  if (!y_hat || !median || n <= 0 || window <= 0) return HYPAD_EINVAL;
  if (window > MAX_WINDOW) return HYPAD_EUNSUPPORTED;
  const int64_t T = n + window - 1;
  const bool filter = HYPAD_TUNE_INT("HYPAD_UNROLL_FILTER", 1) != 0;
  const int ut = HYPAD_TUNE_INT("HYPAD_UNROLL_TILE", 128) == 64 ? 64 : 128;
  const size_t lds = unroll_lds_bytes(ut, window);
  const dim3 grid(grid_for(T, ut)), block(ut * 4);
  long long* stamps = nullptr;
#if HYPAD_DIAG
  stamps = g_unroll_stamps;
#endif
  auto launch = [&](auto kf) -> int {
    if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return HYPAD_EUNSUPPORTED;
    hipLaunchKernelGGL(kf, grid, block, lds, (hipStream_t)s, y_hat, median, summary, n, window, stamps);
    return HYPAD_OK;
  };
  const int rc = unroll_epl_dispatch(window, [&](auto epl) -> int {
    constexpr int EPL = decltype(epl)::value;
    if constexpr (HYPAD_DIAG != 0) {       // (the unfiltered form and the 64-timestep tile exist in the development library only)
      if (ut == 64) return filter ? launch(unroll_median_kernel<EPL, true, 64>) : launch(unroll_median_kernel<EPL, false, 64>);
      return filter ? launch(unroll_median_kernel<EPL, true, 128>) : launch(unroll_median_kernel<EPL, false, 128>);
    } else return launch(unroll_median_kernel<EPL, true, 128>);
  });
  if (rc) return rc;
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_unroll_true(const double* y, double* out, int64_t n, int window, hypad_stream_t s) {
  if (!y || !out || n <= 0 || window <= 0) return HYPAD_EINVAL;
  hipLaunchKernelGGL(unroll_true_kernel<double>, dim3(grid_for(n + window - 1, THREADS)), dim3(THREADS), 0, (hipStream_t)s, y, (int64_t)window, out, n, window);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_unroll_true_f32(const float* y, int64_t row_stride, double* out, int64_t n, int window, hypad_stream_t s) {
  if (!y || !out || n <= 0 || window <= 0 || row_stride < 1) return HYPAD_EINVAL;
  hipLaunchKernelGGL(unroll_true_kernel<float>, dim3(grid_for(n + window - 1, THREADS)), dim3(THREADS), 0, (hipStream_t)s, y, row_stride, out, n, window);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_point_error(const double* y, const float* yh, double* out, int64_t t, hypad_stream_t s) {
  if (!y || !yh || !out || t < 0) return HYPAD_EINVAL;
  if (t == 0) return HYPAD_OK;
  hipLaunchKernelGGL(point_error_kernel, dim3(grid_for(t, THREADS)), dim3(THREADS), 0, (hipStream_t)s, y, yh, out, t);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_area_error(const double* y, const float* yh, double* out, int64_t t, int score_window, hypad_stream_t s) {
  if (!y || !yh || !out || t < 0 || score_window < 2) return HYPAD_EINVAL;
  if (t == 0) return HYPAD_OK;
  hipLaunchKernelGGL(area_error_kernel, dim3(grid_for(t, THREADS)), dim3(THREADS), 0, (hipStream_t)s, y, yh, out, t, score_window);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_dtw_error(const double* y, const float* yh, double* out, int64_t t, int score_window, hypad_stream_t s) {
  if (!y || !yh || !out || t < 0 || score_window < 2) return HYPAD_EINVAL;
  if (t == 0) return HYPAD_OK;
  const int len = (score_window / 2) * 2 + 1;
  dim3 g(grid_for(t, THREADS)), b(THREADS);
  if (!dtw_len_dispatch(len, [&](auto L) { hipLaunchKernelGGL(dtw_error_kernel<decltype(L)::value>, g, b, 0, (hipStream_t)s, y, yh, out, t); })) return HYPAD_EUNSUPPORTED;
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
size_t hypad_rolling_workspace_bytes(int64_t t) {
  if (t <= 0) return 0;
  const int64_t n1 = t / RC1 + 3, n2 = t / RC2 + 3;               // (>= the chunk counts for any origin)
  return (size_t)(n1 + n2) * (sizeof(double) + sizeof(int)) + 64;
}
int hypad_rolling_mean(const double* in, const float* sub, double* out, int64_t t, int window, int64_t origin, void* workspace,
                       size_t workspace_bytes, hypad_stream_t s) {
  if (!in || !out || t < 0 || window < 1 || origin < 0) return HYPAD_EINVAL;
  if (t == 0) return HYPAD_OK;
  RollSrc src{in, sub};
  RollWs ws{};
  if (window <= ROLL_DIRECT_MAX) {
    hipLaunchKernelGGL(rolling_mean_kernel<false>, dim3(grid_for(t, THREADS)), dim3(THREADS), 0, (hipStream_t)s, src, ws, out, t, window, origin);
    HYPAD_CHECK_LAUNCH();
    return HYPAD_OK;
  }
  if (!workspace || workspace_bytes < hypad_rolling_workspace_bytes(t)) return HYPAD_EWORKSPACE;
  roll_counts(t, origin, ws.n1, ws.n2);
  const int64_t cap1 = t / RC1 + 3, cap2 = t / RC2 + 3;
  ws.s1 = (double*)workspace; ws.s2 = ws.s1 + cap1;
  ws.c1 = (int*)(ws.s2 + cap2); ws.c2 = ws.c1 + cap1;
  hipLaunchKernelGGL(roll_chunks_kernel, dim3((unsigned)((ws.n2 + 15) / 16)), dim3(THREADS), 0, (hipStream_t)s, src, ws, t, origin);
  HYPAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(rolling_mean_kernel<true>, dim3(grid_for(t, THREADS)), dim3(THREADS), 0, (hipStream_t)s, src, ws, out, t, window, origin);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_zscore_clip(const double* in, double* out, int64_t t, void* workspace, size_t workspace_bytes, hypad_stream_t s) {
  if (!in || !out || t <= 0) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < HYPAD_STATS_WORKSPACE_BYTES) return HYPAD_EWORKSPACE;
  const int g = stat_blocks(t);
  hipLaunchKernelGGL(stat_partials_kernel<false>, dim3(g), dim3(256), 0, (hipStream_t)s, in, (StatPart*)workspace, t, 0.0, 0.0, (const double*)nullptr);
  HYPAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(zscore_apply_kernel, dim3(grid_for(t, 1024)), dim3(256), 0, (hipStream_t)s, in, (const StatPart*)workspace, g, out, t);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_kde_mode(const float* critic, double* modes, int64_t n, int window, hypad_stream_t s) {
  if (!critic || !modes || n <= 0 || window <= 0) return HYPAD_EINVAL;
  if (window > MAX_WINDOW) return HYPAD_EUNSUPPORTED;
  // (A resident grid -- 256 x KDE_WPE workgroups whose waves stride over ~100 timesteps each -- was measured and dropped: 0.33 ms
  // against 0.30 ms for 8 192 workgroups of ~4 timesteps per wave at 125 000 windows; HYPAD_KDE_GRID caps the grid for such trials.)
  static const int kde_grid = HYPAD_TUNE_INT("HYPAD_KDE_GRID", 8192);
  int gw = grid_for(n + window - 1, THREADS / 64);
  if (gw > kde_grid) gw = kde_grid;
  const dim3 grid(gw);
  kde_kpl_dispatch(window, [&](auto K) { hipLaunchKernelGGL(kde_mode_kernel<decltype(K)::value>, grid, dim3(THREADS), 0, (hipStream_t)s, critic, modes, n, window); });
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_critic_zscore(const double* in, double q25, double q75, double* out, int64_t t, void* workspace, size_t workspace_bytes,
                        hypad_stream_t s) {
  if (!in || !out || t <= 0) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < HYPAD_STATS_WORKSPACE_BYTES) return HYPAD_EWORKSPACE;
  const int g = stat_blocks(t);
  hipLaunchKernelGGL(stat_partials_kernel<true>, dim3(g), dim3(256), 0, (hipStream_t)s, in, (StatPart*)workspace, t, q25, q75, (const double*)nullptr);
  HYPAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(critic_apply_kernel, dim3(grid_for(t, 1024)), dim3(256), 0, (hipStream_t)s, in, (const StatPart*)workspace, g, out, t);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
size_t hypad_quantile_workspace_bytes(void) { return QS_WS_BYTES; }
int hypad_quantiles(const double* in, int64_t n, const double* q, int nq, double* out, void* workspace, size_t workspace_bytes, hypad_stream_t s) {
  if (!in || !q || !out || n <= 0 || nq < 1) return HYPAD_EINVAL;
  if (nq > 2 || n > ((int64_t)1 << 31)) return HYPAD_EUNSUPPORTED;
  for (int j = 0; j < nq; ++j) if (!(q[j] >= 0.0 && q[j] <= 1.0)) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < QS_WS_BYTES) return HYPAD_EWORKSPACE;
  return launch_quantiles(in, n, q, nq, out, workspace, (hipStream_t)s);
}
int hypad_critic_score(const double* in, double* out, int64_t t, void* workspace, size_t workspace_bytes, hypad_stream_t s) {
  if (!in || !out || t <= 0) return HYPAD_EINVAL;
  if (t > ((int64_t)1 << 31)) return HYPAD_EUNSUPPORTED;
  if (!workspace || workspace_bytes < hypad_critic_score_workspace_bytes()) return HYPAD_EWORKSPACE;
  char* p = (char*)workspace;
  double* range = (double*)p;                                     // [q25, q75]
  void* stats = p + 64; void* qws = p + 64 + HYPAD_STATS_WORKSPACE_BYTES;
  const double q[2] = {0.25, 0.75};
  const int rc = launch_quantiles(in, t, q, 2, range, qws, (hipStream_t)s);
  if (rc) return rc;
  const int g = stat_blocks(t);
  hipLaunchKernelGGL(stat_partials_kernel<true>, dim3(g), dim3(256), 0, (hipStream_t)s, in, (StatPart*)stats, t, 0.0, 0.0, (const double*)range);
  HYPAD_CHECK_LAUNCH();
  hipLaunchKernelGGL(critic_apply_kernel, dim3(grid_for(t, 1024)), dim3(256), 0, (hipStream_t)s, in, (const StatPart*)stats, g, out, t);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
size_t hypad_critic_score_workspace_bytes(void) { return 64 + HYPAD_STATS_WORKSPACE_BYTES + QS_WS_BYTES; }
int hypad_row_norms(const float* x, double* out, int64_t rows, int dim, hypad_stream_t s) {
  if (!x || !out || rows < 0 || dim <= 0) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  hipLaunchKernelGGL(row_norms_kernel, dim3(grid_for(rows, THREADS / 64)), dim3(THREADS), 0, (hipStream_t)s, x, out, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_combine_scores(int mode, const double* c, const double* r, const double* u, double* out, int64_t n, hypad_stream_t s) {
  if (!out || n < 0 || mode < 0 || mode > HYPAD_COMB_EUCL_SUM) return HYPAD_EINVAL;
  if (n == 0) return HYPAD_OK;
  hipLaunchKernelGGL(combine_kernel, dim3(grid_for(n, THREADS)), dim3(THREADS), 0, (hipStream_t)s, mode, c, r, u, out, n);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad_kde_mode_signals(const float* critic, double* modes, int n_signals, const int64_t* row_off, int window, hypad_stream_t s) {
  int rc = seg_check(n_signals, row_off);
  if (rc) return rc;
  if (!critic || !modes || window <= 0) return HYPAD_EINVAL;
  if (window > MAX_WINDOW) return HYPAD_EUNSUPPORTED;
  for (int i = 0; i < n_signals && !rc; ++i)          // (each segment as hypad_kde_mode partitions it: the same modes bit for bit)
    rc = hypad_kde_mode(critic + row_off[i], modes + row_off[i] + (int64_t)i * (window - 1), row_off[i + 1] - row_off[i], window, s);
  return rc;
}
// workspace: [critic_score's | rolling mean's for the longest segment | the unsmoothed scores of all segments]
static size_t seg_roll_bytes(int n_signals, const int64_t* row_off, int window) {
  int64_t t = 0;
  for (int i = 0; i < n_signals; ++i) t = std::max<int64_t>(t, row_off[i + 1] - row_off[i] + window - 1);
  return (hypad_rolling_workspace_bytes(t) + 255) & ~(size_t)255;
}
size_t hypad_critic_score_signals_workspace_bytes(int n_signals, const int64_t* row_off, int window) {
  if (seg_check(n_signals, row_off) || window <= 0) return 0;
  const size_t head = (hypad_critic_score_workspace_bytes() + 255) & ~(size_t)255;
  return head + seg_roll_bytes(n_signals, row_off, window) + (size_t)(row_off[n_signals] + (int64_t)n_signals * (window - 1)) * sizeof(double);
}
int hypad_critic_score_signals(const double* modes, double* out, int n_signals, const int64_t* row_off, int window, void* workspace,
                               size_t workspace_bytes, hypad_stream_t s) {
  int rc = seg_check(n_signals, row_off);
  if (rc) return rc;
  if (!modes || !out || window <= 0) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < hypad_critic_score_signals_workspace_bytes(n_signals, row_off, window)) return HYPAD_EWORKSPACE;
  const size_t head = (hypad_critic_score_workspace_bytes() + 255) & ~(size_t)255, roll = seg_roll_bytes(n_signals, row_off, window);
  char* ws = (char*)workspace;
  double* tmp = (double*)(ws + head + roll);
  for (int i = 0; i < n_signals && !rc; ++i) {
    const int64_t n = row_off[i + 1] - row_off[i], t = n + window - 1, o = row_off[i] + (int64_t)i * (window - 1);
    rc = hypad_critic_score(modes + o, tmp + o, t, ws, head, s);
    if (rc) break;
    const int w = (int)std::trunc((double)n * 0.01);       // final_critic_scores :404: math.trunc(n * 0.01), the segment's own n
    if (w == 0) {                                            // pandas' rolling(0): all NaN (hypad_amd rolling_mean)
      hipLaunchKernelGGL(fill_nan_kernel, dim3(grid_for(t, THREADS)), dim3(THREADS), 0, (hipStream_t)s, out + o, t);
      HYPAD_CHECK_LAUNCH();
    } else {
      rc = hypad_rolling_mean(tmp + o, nullptr, out + o, t, w, 0, ws + head, roll, s);
    }
  }
  return rc;
}
int hypad_combine_scores_signals(int mode, const double* c, const double* r, const double* u, double* out, int n_signals, const int64_t* row_off,
                                 int window, hypad_stream_t s) {
  int rc = seg_check(n_signals, row_off);
  if (rc) return rc;
  if (!out || window <= 0 || mode < 0 || mode > HYPAD_COMB_EUCL_SUM) return HYPAD_EINVAL;
  for (int c0 = 0; c0 < n_signals; c0 += SEG_CHUNK) {        // (SEG_CHUNK segments per launch: the table is a kernel argument)
    const SegTable t = seg_table(row_off, c0, n_signals);
    hipLaunchKernelGGL(combine_signals_kernel, dim3(grid_for(seg_longest(t), THREADS), (unsigned)t.n), dim3(THREADS), 0, (hipStream_t)s, mode, c, r, u, out, t, window);
    HYPAD_CHECK_LAUNCH();
  }
  return HYPAD_OK;
}

int hypad_unroll_median_signals(const float* y_hat, float* median, int n_signals, const int64_t* row_off, int window, hypad_stream_t s) {
  const int rc = seg_check(n_signals, row_off);
  if (rc) return rc;
  if (!y_hat || !median || window <= 0) return HYPAD_EINVAL;
  if (window > MAX_WINDOW) return HYPAD_EUNSUPPORTED;
  constexpr int UT = 128;
  const size_t lds = unroll_lds_bytes(UT, window);          // hypad_unroll_median's
  const auto kf = unroll_epl_dispatch(window, [](auto epl) { return &unroll_median_signals_kernel<decltype(epl)::value, UT>; });
  if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();                                  // (the refusal is reported by the status, not left behind)
    return HYPAD_EUNSUPPORTED;
  }
  for (int c0 = 0; c0 < n_signals; c0 += SEG_CHUNK) {
    const SegTable t = seg_table(row_off, c0, n_signals);
    const dim3 grid(grid_for(seg_longest(t) + window - 1, UT), (unsigned)t.n), block(UT * 4);
    hipLaunchKernelGGL(kf, grid, block, lds, (hipStream_t)s, y_hat, median, t, window);
    HYPAD_CHECK_LAUNCH();
  }
  return HYPAD_OK;
}
size_t hypad_rec_scores_signals_workspace_bytes(int n_signals, const int64_t* row_off, int window) {
  if (seg_check(n_signals, row_off) || window <= 0) return 0;
  return rec_ws_layout(n_signals, row_off, window).bytes;
}
int hypad_rec_scores_signals(int kinds, const double* true_unrolled, const float* median, double* out_point, double* out_area, double* out_dtw,
                             int n_signals, const int64_t* row_off, int window, int score_window, void* workspace, size_t workspace_bytes,
                             hypad_stream_t s) {
  const int rc = seg_check(n_signals, row_off);
  if (rc) return rc;
  if (!true_unrolled || !median || window <= 0 || kinds < 1 || kinds > (HYPAD_REC_POINT | HYPAD_REC_AREA | HYPAD_REC_DTW)) return HYPAD_EINVAL;
  if (((kinds & HYPAD_REC_POINT) && !out_point) || ((kinds & HYPAD_REC_AREA) && !out_area) || ((kinds & HYPAD_REC_DTW) && !out_dtw)) return HYPAD_EINVAL;
  if ((kinds & (HYPAD_REC_AREA | HYPAD_REC_DTW)) && score_window < 2) return HYPAD_EINVAL;
  const int len = (score_window / 2) * 2 + 1;
  if ((kinds & HYPAD_REC_DTW) && !dtw_len_dispatch(len, [](auto) {})) return HYPAD_EUNSUPPORTED;
  const RecWsLayout l = rec_ws_layout(n_signals, row_off, window);
  if (!workspace || workspace_bytes < l.bytes) return HYPAD_EWORKSPACE;
  char* ws = (char*)workspace;
  double* err_area = (double*)(ws + l.err);
  double* err_dtw = err_area + l.total;
  RecKinds kd{};
  int nk = 0;
  auto add = [&](const double* in, const float* sub, double* out) {
    rec_kind(kd, nk, RollSrc{in, sub}, out, ws + l.sums, ws + l.counts, l);
    kd.parts[nk] = (StatPart*)(ws + l.parts) + (size_t)nk * n_signals * STAT_G;
    ++nk;
  };
  if (kinds & HYPAD_REC_POINT) add(true_unrolled, median, out_point);       // |true - median| inside the smoothing, as rolling_mean(minus=) does
  if (kinds & HYPAD_REC_AREA) add(err_area, nullptr, out_area);
  if (kinds & HYPAD_REC_DTW) add(err_dtw, nullptr, out_dtw);
  const hipStream_t st = (hipStream_t)s;
  for (int c0 = 0; c0 < n_signals; c0 += SEG_CHUNK) {
    const SegTable t = seg_table(row_off, c0, n_signals);
    const int64_t most = seg_longest(t) + window - 1;
    const dim3 ge(grid_for(most, THREADS), (unsigned)t.n), b(THREADS);
    if (kinds & HYPAD_REC_AREA) {
      hipLaunchKernelGGL(area_error_signals_kernel, ge, b, 0, st, true_unrolled, median, err_area, t, window, score_window);
      HYPAD_CHECK_LAUNCH();
    }
    if (kinds & HYPAD_REC_DTW) {
      dtw_len_dispatch(len, [&](auto L) { hipLaunchKernelGGL(dtw_error_signals_kernel<decltype(L)::value>, ge, b, 0, st, true_unrolled, median, err_dtw, t, window); });
      HYPAD_CHECK_LAUNCH();
    }
    // (always the same launches, whatever the segments' windows: a segment that does not take the chunked path leaves at once)
    const unsigned gc = (unsigned)((((most - 1) >> 8) + 1 + 15) / 16);
    hipLaunchKernelGGL(roll_chunks_signals_kernel, dim3(gc, (unsigned)t.n, (unsigned)nk), b, 0, st, kd, t, window);
    HYPAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(rolling_mean_signals_kernel, dim3(ge.x, (unsigned)t.n, (unsigned)nk), b, 0, st, kd, t, window);
    HYPAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(stat_partials_signals_kernel, dim3(STAT_G, (unsigned)t.n, (unsigned)nk), dim3(256), 0, st, kd, t, window);
    HYPAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(zscore_apply_signals_kernel, dim3(grid_for(most, 1024), (unsigned)t.n, (unsigned)nk), dim3(256), 0, st, kd, t, window);
    HYPAD_CHECK_LAUNCH();
  }
  return HYPAD_OK;
}

size_t hypad_quantiles_signals_workspace_bytes(int n_signals) { return n_signals < 1 ? 0 : qss_bytes(n_signals); }
int hypad_quantiles_signals(const double* in, int n_signals, const int64_t* row_off, int window, const double* q, int nq, double* out,
                            void* workspace, size_t workspace_bytes, hypad_stream_t s) {
  const int rc = seg_check(n_signals, row_off);
  if (rc) return rc;
  if (!in || !q || !out || window <= 0 || nq < 1) return HYPAD_EINVAL;
  if (nq > 2) return HYPAD_EUNSUPPORTED;
  if (!segs_fit_2_31(n_signals, row_off, window)) return HYPAD_EUNSUPPORTED;
  for (int j = 0; j < nq; ++j) if (!(q[j] >= 0.0 && q[j] <= 1.0)) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < qss_bytes(n_signals)) return HYPAD_EWORKSPACE;
  for (int c0 = 0; c0 < n_signals; c0 += SEG_CHUNK) {
    const int r = launch_quantiles_signals(in, seg_table(row_off, c0, n_signals), qs_slices(n_signals), window, q, nq, out, workspace, (hipStream_t)s);
    if (r) return r;
  }
  return HYPAD_OK;
}
size_t hypad_critic_chain_signals_workspace_bytes(int n_signals, const int64_t* row_off, int window) {
  if (seg_check(n_signals, row_off) || window <= 0) return 0;
  return chain_ws_layout(n_signals, row_off, window).bytes;
}
int hypad_critic_chain_signals(const float* critic, double* modes_out, double* out, int n_signals, const int64_t* row_off, int window,
                               void* workspace, size_t workspace_bytes, hypad_stream_t s) {
  const int rc = seg_check(n_signals, row_off);
  if (rc) return rc;
  if (!critic || !out || window <= 0) return HYPAD_EINVAL;
  if (window > MAX_WINDOW) return HYPAD_EUNSUPPORTED;
  if (!segs_fit_2_31(n_signals, row_off, window)) return HYPAD_EUNSUPPORTED;
  const ChainWsLayout l = chain_ws_layout(n_signals, row_off, window);
  if (!workspace || workspace_bytes < l.bytes) return HYPAD_EWORKSPACE;
  char* ws = (char*)workspace;
  double* modes = modes_out ? modes_out : (double*)(ws + l.modes);
  double* range = (double*)(ws + l.range);
  double* tmp = (double*)(ws + l.tmp);
  StatPart* parts = (StatPart*)(ws + l.parts);
  RecKinds kd{};                                               // one kind: the unsmoothed scores, no subtrahend
  rec_kind(kd, 0, RollSrc{tmp, nullptr}, out, ws + l.sums, ws + l.counts, l);
  const hipStream_t st = (hipStream_t)s;
  const double q[2] = {0.25, 0.75};
  for (int c0 = 0; c0 < n_signals; c0 += SEG_CHUNK) {          // eleven launches per SEG_CHUNK signals
    const SegTable t = seg_table(row_off, c0, n_signals);
    const int64_t most = seg_longest(t) + window - 1;
    const dim3 gk(grid_for(most, THREADS / 64), (unsigned)t.n), b(THREADS);
    kde_kpl_dispatch(window, [&](auto K) { hipLaunchKernelGGL(kde_mode_signals_kernel<decltype(K)::value>, gk, b, 0, st, critic, modes, t, window); });
    HYPAD_CHECK_LAUNCH();
    const int r = launch_quantiles_signals(modes, t, l.slices, window, q, 2, range, ws + l.qs, st);
    if (r) return r;
    hipLaunchKernelGGL(critic_partials_signals_kernel, dim3(STAT_G, (unsigned)t.n), dim3(256), 0, st, modes, range, parts, t, window);
    HYPAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(critic_apply_signals_kernel, dim3(grid_for(most, 1024), (unsigned)t.n), dim3(256), 0, st, modes, parts, tmp, t, window);
    HYPAD_CHECK_LAUNCH();
    // (the smoothing of hypad_rec_scores_signals with one kind: each segment's own window trunc(n_s * 0.01), NaN fill at 0)
    const unsigned gc = (unsigned)((((most - 1) >> 8) + 1 + 15) / 16);
    hipLaunchKernelGGL(roll_chunks_signals_kernel, dim3(gc, (unsigned)t.n, 1), b, 0, st, kd, t, window);
    HYPAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(rolling_mean_signals_kernel, dim3(grid_for(most, THREADS), (unsigned)t.n, 1), b, 0, st, kd, t, window);
    HYPAD_CHECK_LAUNCH();
  }
  return HYPAD_OK;
}

}  // extern "C"

#if HYPAD_DIAG
extern "C" __attribute__((visibility("default"))) void hypad_diag_set_unroll_stamps(long long* p) { g_unroll_stamps = p; }
#endif
