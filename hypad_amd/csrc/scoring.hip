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
#include "unroll_median_body.inc"
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
#include "dtw_error_body.inc"
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
#include "kde_mode_body.inc"
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
#include "qs_level_body.inc"
}
// launch QS_PRE + 1: the keys that match a rank's 33-bit prefix -> that rank's candidate list (+ the list's extremes)
__global__ __launch_bounds__(256) void qs_compact_kernel(const double* __restrict__ in, int64_t n, QsWs ws, int nsel) {
  __shared__ unsigned int h[QS_SEL][QS_BINS];
  __shared__ QsState cur[QS_SEL];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int PER = 4;
  double x[PER];
  int64_t base = (int64_t)blockIdx.x * (256 * PER);
#include "qs_compact_body.inc"
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
#include "qs_final_body.inc"
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

// row_norms_kernel on the difference a - b, formed in fp32 as it is read (multivariate_anomaly_detection's Euclidean reconstruction
// score, utils/anomaly_detection_utils.py:157): the same lane partition and the same order of additions, hence the bits of
// hypad_row_norms on the fp32 difference matrix.
__global__ __launch_bounds__(THREADS) void row_diff_norms_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ out,
                                                                  int64_t rows, int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * (THREADS / 64)) {
    float s = 0.f;
    for (int c = lane; c < dim; c += 64) { float v = a[r * dim + c] - b[r * dim + c]; s += v * v; }
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
// The tile loop is the single-signal kernel's, shared as TEXT: <name>_body.inc holds what a single-signal kernel and its segmented
// twin both do after their prologues, and each of the two includes it.  Not a shared __device__ function: with the loop moved into
// one the single-signal kernels' register allocation changed (unroll_median_kernel: 5 spilled scalar registers instead of 12; all
// eight kde_mode kernels other bytes), and the code objects of the timed kernels are held identical.  An included text is compiled
// in each kernel as if written there: same bytes as the copies it replaced (docs/history/scoring_shared_bodies.md).
template <int EPL, int UT>
__global__ __launch_bounds__(UT * 4) __attribute__((amdgpu_waves_per_eu(UNROLL_WPE, UNROLL_WPE))) void unroll_median_signals_kernel(
    const float* __restrict__ y_all, float* __restrict__ median_all, SegTable tab, int W) {
  const int sl = blockIdx.y;
  const int64_t n = tab.off[sl + 1] - tab.off[sl];
  const float* __restrict__ y_hat = y_all + tab.off[sl] * W;
  float* __restrict__ median = median_all + seg_toff(tab, sl, W);
  constexpr bool FILTER = true;                              // medians only: no summary, and none of the development library's stamps
  double* const summary = nullptr;
  [[maybe_unused]] long long* const stamps = nullptr;
#include "unroll_median_body.inc"
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
#include "dtw_error_body.inc"
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
// ---- hypad_zscore_clip per segment of a plain segmented vector (hypad_zscore_clip_signals: WINDOW LAYOUT, segment s at off[s]; the
// multivariate detector's rec_scores, utils/anomaly_detection_utils.py:160-161, 177-178).  The two kernels above without the
// rolling-mean workspace: the partials of segment seg0 + blockIdx.y are slots (seg0 + blockIdx.y) * STAT_G .. of `parts_all`.
__global__ __launch_bounds__(256) void zscore_partials_segments_kernel(const double* __restrict__ in_all, StatPart* __restrict__ parts_all, SegTable tab) {
  __shared__ double sh[4];
  const int sl = blockIdx.y;
  const int64_t T = tab.off[sl + 1] - tab.off[sl];
  const int nb = stat_blocks(T);
  if ((int)blockIdx.x >= nb) return;                                                  // (workgroup-uniform)
  const double* __restrict__ in = in_all + tab.off[sl];
  const int64_t len = (T + nb - 1) / nb;
  const int64_t b = (int64_t)blockIdx.x * len, e = b + len < T ? b + len : T;
  double s = 0.0;
  for (int64_t i = b + threadIdx.x; i < e; i += 256) s += in[i];
  const double n = e > b ? (double)(e - b) : 0.0;
  const double mean = n > 0.0 ? block_sum_256(s, sh) / n : 0.0;
  double q = 0.0;
  for (int64_t i = b + threadIdx.x; i < e; i += 256) { const double d = in[i] - mean; q += d * d; }
  q = block_sum_256(q, sh);
  if (threadIdx.x == 0) { StatPart p; p.n = n; p.mean = mean; p.m2 = q; p.rsum = 0.0; p.rcnt = 0.0; parts_all[(size_t)(tab.seg0 + sl) * STAT_G + blockIdx.x] = p; }
}
// (in and out: no __restrict__, in == out is allowed -- every element is read and written by the same thread)
__global__ __launch_bounds__(256) void zscore_apply_segments_kernel(const double* in_all, const StatPart* __restrict__ parts_all, double* out_all, SegTable tab) {
  __shared__ StatPart sh[STAT_G];
  const int sl = blockIdx.y;
  const int64_t o = tab.off[sl], T = tab.off[sl + 1] - o;
  const StatPart st = stat_merge_all(parts_all + (size_t)(tab.seg0 + sl) * STAT_G, stat_blocks(T), sh);
  const double mean = st.mean, sd = sqrt(st.m2 / st.n);
  const double* in = in_all + o;
  double* out = out_all + o;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < T; i += (int64_t)gridDim.x * 256) {
    double z = (in[i] - mean) / sd;
    out[i] = (z != z) ? z : fmax(z, 0.0) + 1.0;  // np.clip keeps NaN
  }
}
// ---- The critic-score chain of a group (hypad_critic_chain_signals): final_critic_scores :365-404 for every segment at once.  As above,
// every kernel takes its segment from blockIdx.y (qs_final_signals_kernel: blockIdx.x) and does on it what the single-signal kernel
// does on that segment alone.  The KDE and the three radix-selection kernels include the single-signal kernels' bodies (*_body.inc: shared
// as text, for the reason given at unroll_median_signals_kernel); the statistics kernels, a dozen lines each, are written out.

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
#include "kde_mode_body.inc"
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
#include "qs_level_body.inc"
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
#include "qs_compact_body.inc"
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
#include "qs_final_body.inc"
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
int hypad_row_diff_norms(const float* a, const float* b, double* out, int64_t rows, int dim, hypad_stream_t s) {
  if (!a || !b || !out || rows <= 0 || dim <= 0) return HYPAD_EINVAL;
  hipLaunchKernelGGL(row_diff_norms_kernel, dim3(grid_for(rows, THREADS / 64)), dim3(THREADS), 0, (hipStream_t)s, a, b, out, rows, dim);
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

size_t hypad_zscore_clip_signals_workspace_bytes(int n_signals) { return n_signals < 1 ? 0 : (size_t)n_signals * STAT_G * sizeof(StatPart); }
int hypad_zscore_clip_signals(const double* in, double* out, int n_signals, const int64_t* seg_off, void* workspace, size_t workspace_bytes,
                              hypad_stream_t s) {
  const int rc = seg_check(n_signals, seg_off);
  if (rc) return rc;
  if (!in || !out) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < hypad_zscore_clip_signals_workspace_bytes(n_signals)) return HYPAD_EWORKSPACE;
  StatPart* parts = (StatPart*)workspace;
  for (int c0 = 0; c0 < n_signals; c0 += SEG_CHUNK) {
    const SegTable t = seg_table(seg_off, c0, n_signals);
    hipLaunchKernelGGL(zscore_partials_segments_kernel, dim3(STAT_G, (unsigned)t.n), dim3(256), 0, (hipStream_t)s, in, parts, t);
    HYPAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(zscore_apply_segments_kernel, dim3(grid_for(seg_longest(t), 1024), (unsigned)t.n), dim3(256), 0, (hipStream_t)s, in, (const StatPart*)parts, out, t);
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
