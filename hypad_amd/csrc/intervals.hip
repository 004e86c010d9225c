// Anomalous intervals of a group of score vectors (hypad_find_anomalies_signals): the fixed-threshold find_anomalies of
// utils/anomaly_detection_utils.py :1363-1472 (helpers :1098-1114, :1117-1313) on the GPU, for every signal of a group at once.
//
// Work items are the (signal, window[, mirrored]) triples.  Launches per 64 signals, whatever the number of windows:
//   fa_reduce_kernel<0>   sum x                         per 4 096-element chunk of every window   -> mean
//   fa_reduce_kernel<1>   sum (x - mean)^2, sum x'      (x' = mean - (x - mean), the mirrored window of lower_threshold)
//   fa_reduce_kernel<2>   sum (x' - mean')^2            only with lower_threshold
//   fa_window_kernel      one workgroup per item: threshold, padded runs, run maxima, max_below, sort, prune, scores
//   fa_merge_kernel       one workgroup per signal: _merge_sequences
// A window's chunks depend on its own length alone and every partial sum is reduced in a fixed order (no floating-point atomics), so
// a signal's table does not depend on the group it is scored in.  fp64 throughout, no fused multiply-add (NumPy has none).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/hypad.h"
#include "device_utils.h"

#pragma clang fp contract(off)

using namespace hypad;

namespace {

typedef unsigned long long u64;
constexpr int FA_CHUNK = 64;          // signals per launch: their table is a kernel argument
constexpr int RED_T = 256;            // threads of a reduction workgroup
constexpr int RED_ELEMS = 4096;       // elements of a reduction chunk
constexpr int BT = 1024;              // threads of the per-window and per-signal workgroups
constexpr int LDS_SORT = 4096;        // keys an LDS sort holds; larger sorts run in the workspace
constexpr long long FAR = 1LL << 62;

// The signals of one launch.  size / step are clamped to the segment length by the host (a longer window is the whole segment, a
// longer step leaves the segment at once), woff is the running number of windows, wsb each signal's workspace offset in bytes.
struct FaTable {
  int n, seg0, passes, pad_;
  int64_t off[FA_CHUNK + 1];
  int size[FA_CHUNK], step[FA_CHUNK];
  int woff[FA_CHUNK + 1];
  int64_t wsb[FA_CHUNK];
};

__host__ __device__ inline int64_t up8(int64_t b) { return (b + 7) & ~(int64_t)7; }
__host__ __device__ inline int64_t pow2ceil(int64_t v) { int64_t p = 1; while (p < v) p <<= 1; return p; }

// Workspace of one signal: [4 partial sums per (window, chunk) | kept count per item | its offset in the signal's candidate list |
// item blocks | the candidate list and its sort].  An item block: the values above the threshold (position, value, run number;
// reused for the kept (start, stop, score) rows), the runs (start, end, maximum as an ordered key), their sort, the left-cover bits.
// cap: more than window / 16 values cannot lie above mean + 4 std (Chebyshev), hence no more runs either.
struct FaLayout {
  int cap, nch, words;
  int64_t P, NI, gcap, Pg;
  int64_t part, icnt, ioff, items, IB, i_val, i_key, i_sa, i_mask, i_pos, i_rid, i_rs, i_re, i_sb;
  int64_t g_sc, g_sa, g_s, g_e, g_first, g_sb, bytes;
};
__host__ __device__ inline FaLayout fa_layout(int size, int nw, int passes) {
  FaLayout l;
  l.cap = size / 16 + 2; l.P = pow2ceil(l.cap);
  l.nch = (size + RED_ELEMS - 1) / RED_ELEMS;
  l.words = ((size + BT - 1) / BT) * (BT / 64);
  l.NI = (int64_t)nw * passes; l.gcap = l.NI * l.cap; l.Pg = pow2ceil(l.gcap);
  int64_t b = 0;
  l.i_val = b; b += (int64_t)l.cap * 8;
  l.i_key = b; b += (int64_t)l.cap * 8;
  l.i_sa = b; b += l.P * 8;
  l.i_mask = b; b += (int64_t)l.words * 8;
  l.i_pos = b; b += (int64_t)l.cap * 4;
  l.i_rid = b; b += (int64_t)l.cap * 4;
  l.i_rs = b; b += (int64_t)l.cap * 4;
  l.i_re = b; b += (int64_t)l.cap * 4;
  l.i_sb = b; b += l.P * 4;
  l.IB = up8(b);
  int64_t o = 0;
  l.part = o; o += (int64_t)nw * l.nch * 4 * 8;
  l.icnt = o; o += up8(l.NI * 4);
  l.ioff = o; o += up8(l.NI * 4);
  l.items = o; o += l.NI * l.IB;
  l.g_sc = o; o += l.gcap * 8;
  l.g_sa = o; o += l.Pg * 8;
  l.g_s = o; o += up8(l.gcap * 4);
  l.g_e = o; o += up8(l.gcap * 4);
  l.g_first = o; o += up8(l.gcap * 4);
  l.g_sb = o; o += up8(l.Pg * 4);
  l.bytes = (o + 255) & ~(int64_t)255;
  return l;
}
// windows of a segment of n values: the reference's `while window_end < n` (:1437-1466)
inline int64_t fa_windows(int64_t n, int64_t size, int64_t step) { return n > size ? (n - size + step - 1) / step + 1 : 1; }

__device__ __forceinline__ int fa_signal(const FaTable& t, int w) {
  int lo = 0, hi = t.n - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.woff[mid] <= w) lo = mid; else hi = mid - 1; }
  return lo;
}
// a double as an unsigned key of the same order (no NaN gets here), and back
__device__ __forceinline__ u64 dkey(double v) { const u64 b = (u64)__double_as_longlong(v); return (b >> 63) ? ~b : b ^ (1ULL << 63); }
__device__ __forceinline__ double undkey(u64 k) { return __longlong_as_double((long long)((k >> 63) ? k ^ (1ULL << 63) : ~k)); }

struct OpSum { __device__ long long operator()(long long a, long long b) const { return a + b; } };
struct OpMax { __device__ long long operator()(long long a, long long b) const { return a > b ? a : b; } };
struct OpMin { __device__ long long operator()(long long a, long long b) const { return a < b ? a : b; } };
// Inclusive scan over the workgroup's threads in thread order, continued from `carry` (the same value in every thread), which
// becomes the total.  sh: one slot per wave.  Two barriers.
template <class Op>
__device__ __forceinline__ long long block_scan(long long v, Op op, long long* sh, long long& carry) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwv = blockDim.x >> 6;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const long long o = __shfl_up(v, off, WAVE); if (lane >= off) v = op(v, o); }
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  long long pre = carry, tot = carry;
  for (int w2 = 0; w2 < nwv; ++w2) { const long long x = sh[w2]; if (w2 < wave) pre = op(pre, x); tot = op(tot, x); }
  __syncthreads();
  carry = tot;
  return op(pre, v);
}
// (a, b) ascending, lexicographic; P a power of two; a / b in LDS or in the workspace (one workgroup either way)
__device__ void bitonic_sort(u64* a, unsigned* b, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const int x = i ^ j;
        if (x > i) {
          const u64 ai = a[i], ax = a[x];
          const unsigned bi = b[i], bx = b[x];
          const bool gt = ai > ax || (ai == ax && bi > bx);
          if (gt == ((i & k) == 0)) { a[i] = ax; a[x] = ai; b[i] = bx; b[x] = bi; }
        }
      }
    }
  __syncthreads();
}

struct FaWin { int s, k; int64_t n, start, L; };
__device__ __forceinline__ FaWin fa_window(const FaTable& t, int w) {
  FaWin r;
  r.s = fa_signal(t, w); r.k = w - t.woff[r.s];
  r.n = t.off[r.s + 1] - t.off[r.s];
  r.start = (int64_t)r.k * t.step[r.s];
  r.L = r.n - r.start < t.size[r.s] ? r.n - r.start : t.size[r.s];
  return r;
}
// the statistics of a window from its chunk partials, summed in chunk order (every thread the same numbers)
struct FaStats { double mean0, mean, sd, thr; };
__device__ __forceinline__ FaStats fa_stats(const double* part, int64_t L, int pass) {
  const int nch = (int)((L + RED_ELEMS - 1) / RED_ELEMS);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int c = 0; c < nch; ++c) { s0 += part[c * 4]; s1 += part[c * 4 + 1]; s2 += part[c * 4 + 2]; s3 += part[c * 4 + 3]; }
  FaStats st;
  st.mean0 = s0 / (double)L;
  st.mean = pass ? s2 / (double)L : st.mean0;
  st.sd = sqrt((pass ? s3 : s1) / (double)L);
  st.thr = st.mean + 4.0 * st.sd;                    // _fixed_threshold :1098-1114
  return st;
}

// STAGE 0: sum x.  1: sum (x - mean)^2 and the sum of the mirrored window.  2: sum (x' - mean')^2.  grid (windows, chunks).
template <int STAGE>
__global__ __launch_bounds__(RED_T) void fa_reduce_kernel(const double* __restrict__ in, char* __restrict__ ws, FaTable t) {
  __shared__ double sh[2][RED_T / 64];
  const FaWin w = fa_window(t, blockIdx.x);
  const int64_t c0 = (int64_t)blockIdx.y * RED_ELEMS;
  if (c0 >= w.L) return;
  const int nw = t.woff[w.s + 1] - t.woff[w.s];
  const FaLayout l = fa_layout(t.size[w.s], nw, t.passes);
  double* part = (double*)(ws + t.wsb[w.s] + l.part) + (int64_t)w.k * l.nch * 4;
  const double* x = in + t.off[w.s] + w.start;
  const int nch = (int)((w.L + RED_ELEMS - 1) / RED_ELEMS);
  double mean = 0.0, mean2 = 0.0;
  if (STAGE >= 1) { double s = 0.0; for (int c = 0; c < nch; ++c) s += part[c * 4]; mean = s / (double)w.L; }
  if (STAGE >= 2) { double s = 0.0; for (int c = 0; c < nch; ++c) s += part[c * 4 + 2]; mean2 = s / (double)w.L; }
  const int64_t c1 = c0 + RED_ELEMS < w.L ? c0 + RED_ELEMS : w.L;
  double a = 0.0, b = 0.0;
  for (int64_t i = c0 + threadIdx.x; i < c1; i += RED_T) {
    const double v = x[i];
    if (STAGE == 0) a += v;
    if (STAGE == 1) { const double d = v - mean; a += d * d; b += mean - d; }
    if (STAGE == 2) { const double d = (mean - (v - mean)) - mean2; a += d * d; }
  }
  a = wave_sum(a); b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double ta = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]), tb = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
    double* p = part + (int64_t)blockIdx.y * 4;
    if (STAGE == 0) { p[0] = ta; p[1] = 0.0; p[2] = 0.0; p[3] = 0.0; }
    if (STAGE == 1) { p[1] = ta; p[2] = tb; }
    if (STAGE == 2) p[3] = ta;
  }
}

// One workgroup per item (window, pass): _find_window_sequences :1316-1360 with the fixed threshold.
__global__ __launch_bounds__(BT) void fa_window_kernel(const double* __restrict__ in, char* __restrict__ ws, FaTable t, long long pad, double min_percent) {
  __shared__ u64 s_a[LDS_SORT];
  __shared__ unsigned s_b[LDS_SORT];
  __shared__ long long s_scan[BT / 64];
  __shared__ double s_red[BT / 64];
  __shared__ int s_last[BT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int pass = blockIdx.x % t.passes;
  const FaWin w = fa_window(t, blockIdx.x / t.passes);
  const int nw = t.woff[w.s + 1] - t.woff[w.s];
  const FaLayout l = fa_layout(t.size[w.s], nw, t.passes);
  char* base = ws + t.wsb[w.s];
  const int64_t it = (int64_t)w.k * t.passes + pass;
  int* icnt = (int*)(base + l.icnt) + it;
  if (w.L <= 0) { if (tid == 0) *icnt = 0; return; }            // (a step beyond the window: the reference slices nothing)
  const FaStats st = fa_stats((const double*)(base + l.part) + (int64_t)w.k * l.nch * 4, w.L, pass);
  if (!(st.thr == st.thr)) { if (tid == 0) *icnt = 0; return; }  // a NaN in the window: nothing lies above a NaN threshold
  char* ib = base + l.items + it * l.IB;
  double* lv = (double*)(ib + l.i_val);
  u64* key = (u64*)(ib + l.i_key);
  u64* mask = (u64*)(ib + l.i_mask);
  int* pos = (int*)(ib + l.i_pos);
  int* rid = (int*)(ib + l.i_rid);
  int* rs = (int*)(ib + l.i_rs);
  int* re = (int*)(ib + l.i_re);
  const double* x = in + t.off[w.s] + w.start;
  const int L = (int)w.L;
  const double mean0 = st.mean0, thr = st.thr;
  auto value = [&](int i) { double v = x[i]; if (pass) v = mean0 - (v - mean0); return v + 0.0; };

  // 1. the values above the threshold, in order; bit i of `mask`: a value above within `pad` positions to the left of i (or at i)
  long long count = 0, prev = -1;
  for (int b0 = 0; b0 < L; b0 += BT) {
    const int i = b0 + tid;
    const bool in_w = i < L;
    const double v = in_w ? value(i) : 0.0;
    const bool ab = in_w && v > thr;
    const long long incl = block_scan(ab ? 1LL : 0LL, OpSum(), s_scan, count);
    if (ab && incl - 1 < l.cap) { pos[incl - 1] = i; lv[incl - 1] = v; }
    const long long pa = block_scan(ab ? (long long)i : -1LL, OpMax(), s_scan, prev);
    const u64 bal = __ballot(in_w && pa >= 0 && i - pa <= pad);
    if (lane == 0) mask[(b0 >> 6) + wave] = bal;
  }
  const bool clipped = count > l.cap;                            // (cannot happen: see FaLayout)
  const int m = (int)(clipped ? l.cap : count);
  if (m == 0) { if (tid == 0) *icnt = 0; return; }
  __syncthreads();

  // 2. runs of the dilated mask (_find_sequences :1117-1166): two values above belong to one run when at most 2 pad + 1 apart
  const long long gap = 2 * pad + 1;
  long long runs = 0;
  for (int b0 = 0; b0 < m; b0 += BT) {
    const int j = b0 + tid;
    const bool in_l = j < m;
    int p = 0;
    bool first = false;
    if (in_l) { p = pos[j]; first = j == 0 || (long long)p - pos[j - 1] > gap; }
    const long long incl = block_scan(first ? 1LL : 0LL, OpSum(), s_scan, runs);
    if (in_l) {
      const int r = (int)incl - 1;
      rid[j] = r;
      if (first) { rs[r] = (int)(p - pad > 0 ? p - pad : 0); key[r] = 0ULL; }
      if (j == m - 1 || (long long)pos[j + 1] - p > gap) re[r] = (int)(p + pad < L - 1 ? p + pad : L - 1);
    }
  }
  const int R = (int)runs;
  __syncthreads();
  for (int j = tid; j < m; j += BT) atomicMax(&key[rid[j]], dkey(lv[j]));      // run maxima (_get_max_errors :1169-1200): an integer maximum
  // 3. max_below: the largest value outside the dilated mask, 0 when it covers the window
  double mb = -INFINITY;
  int any = 0;
  long long next = FAR;
  for (int tile = (L - 1) / BT; tile >= 0; --tile) {
    const int i = tile * BT + (BT - 1 - tid);
    const bool in_w = i < L;
    const double v = in_w ? value(i) : 0.0;
    const long long na = block_scan(in_w && v > thr ? (long long)i : FAR, OpMin(), s_scan, next);
    if (in_w && !((mask[i >> 6] >> (i & 63)) & 1ULL) && !(na - i <= pad)) { any = 1; mb = fmax(mb, v); }
  }
  for (int off = 32; off > 0; off >>= 1) mb = fmax(mb, __shfl_xor(mb, off, WAVE));
  if (lane == 0) s_red[wave] = mb;
  any = __syncthreads_or(any);
  for (int w2 = 0; w2 < BT / 64; ++w2) mb = fmax(mb, s_red[w2]);
  const double max_below = any ? mb : 0.0;

  // 4. the runs by descending maximum, stably by start (:1196-1199)
  const int P = (int)pow2ceil(R);
  u64* a = P <= LDS_SORT ? s_a : (u64*)(ib + l.i_sa);
  unsigned* b = P <= LDS_SORT ? s_b : (unsigned*)(ib + l.i_sb);
  for (int j = tid; j < P; j += BT) {
    a[j] = j < R ? ~__hip_atomic_load(&key[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ULL;
    b[j] = j < R ? (unsigned)j : ~0u;
  }
  bitonic_sort(a, b, P);
  // 5. _prune_anomalies :1203-1237: keep down to the last run that stands out from its successor (the sentinel behind the last)
  int last = -1;
  for (int i = tid; i < R; i += BT) {
    const double cur = undkey(~a[i]), nxt = i + 1 < R ? undkey(~a[i + 1]) : max_below;
    if (!((cur - nxt) / cur < min_percent)) last = i;
  }
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(last, off, WAVE); last = o > last ? o : last; }
  if (lane == 0) s_last[wave] = last;
  __syncthreads();
  for (int w2 = 0; w2 < BT / 64; ++w2) last = s_last[w2] > last ? s_last[w2] : last;
  const int keep = last + 1;
  // 6. _compute_scores :1240-1269, into the item's (dead) list arrays
  const double denom = st.mean + st.sd;
  // A covered window is one run (0, L - 1), and its sentinel is (-1, -1, 0).  The reference's stable sort (:1196-1199) puts the sentinel
  // in front of a run whose maximum is <= 0; (0 - max) / 0 is +inf or NaN, never below min_percent, so the prune keeps exactly the
  // sentinel's row and drops the run behind it.
  if (!any && !(undkey(~a[0]) > 0.0)) {
    if (tid == 0) { pos[0] = (int)w.start - 1; rid[0] = (int)w.start - 1; lv[0] = (0.0 - thr) / denom; *icnt = clipped ? -2 : 1; }
    return;
  }
  for (int i = tid; i < keep; i += BT) {
    const int r = (int)b[i];
    pos[i] = rs[r] + (int)w.start;
    rid[i] = re[r] + (int)w.start;
    lv[i] = (undkey(~a[i]) - thr) / denom;
  }
  if (tid == 0) *icnt = clipped ? -(keep + 1) : keep;
}

// One workgroup per signal: _merge_sequences :1272-1313 over the kept rows of its items, in order of production.
__global__ __launch_bounds__(BT) void fa_merge_kernel(char* __restrict__ ws, FaTable t, double* __restrict__ out, int* __restrict__ counts,
                                                       int* __restrict__ status, int capacity) {
  __shared__ u64 s_a[LDS_SORT];
  __shared__ unsigned s_b[LDS_SORT];
  __shared__ long long s_scan[BT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.x, sg = t.seg0 + s;
  const int nw = t.woff[s + 1] - t.woff[s];
  const FaLayout l = fa_layout(t.size[s], nw, t.passes);
  char* base = ws + t.wsb[s];
  const int* icnt = (const int*)(base + l.icnt);
  int* ioff = (int*)(base + l.ioff);
  double* gsc = (double*)(base + l.g_sc);
  int* gs = (int*)(base + l.g_s);
  int* ge = (int*)(base + l.g_e);
  int* gfirst = (int*)(base + l.g_first);
  long long total = 0;
  int bad = 0;
  for (int64_t b0 = 0; b0 < l.NI; b0 += BT) {
    const int64_t it = b0 + tid;
    int c = 0;
    if (it < l.NI) { c = icnt[it]; if (c < 0) { bad = 1; c = -c - 1; } }
    const long long incl = block_scan((long long)c, OpSum(), s_scan, total);
    if (it < l.NI) ioff[it] = (int)(incl - c);
  }
  bad = __syncthreads_or(bad);
  const int C = (int)total;
  if (C == 0) { if (tid == 0) { counts[sg] = 0; status[sg] = bad ? HYPAD_FA_INTERNAL : 0; } return; }
  for (int64_t it = wave; it < l.NI; it += BT / 64) {
    int c = icnt[it];
    c = c < 0 ? -c - 1 : c;
    const int o = ioff[it];
    const char* ib = base + l.items + it * l.IB;
    const int* cs = (const int*)(ib + l.i_pos);
    const int* ce = (const int*)(ib + l.i_rid);
    const double* csc = (const double*)(ib + l.i_val);
    for (int i = lane; i < c; i += 64) { gs[o + i] = cs[i]; ge[o + i] = ce[i]; gsc[o + i] = csc[i]; }
  }
  __syncthreads();
  // by start, stably in order of production (:1290)
  const int P = (int)pow2ceil(C);
  u64* a = P <= LDS_SORT ? s_a : (u64*)(base + l.g_sa);
  unsigned* b = P <= LDS_SORT ? s_b : (unsigned*)(base + l.g_sb);
  // (the key is start + 1: the sentinel's row of a signal's first window starts at -1)
  for (int j = tid; j < P; j += BT) { a[j] = j < C ? (u64)(gs[j] + 1LL) : ~0ULL; b[j] = j < C ? (unsigned)j : ~0u; }
  bitonic_sort(a, b, P);
  // a row opens a group when it starts beyond the largest stop so far + 1 (:1296)
  long long far = -1, groups = 0;
  for (int b0 = 0; b0 < C; b0 += BT) {
    const int j = b0 + tid;
    const bool in_l = j < C;
    const long long before = block_scan(in_l && j > 0 ? (long long)ge[b[j - 1]] : -1LL, OpMax(), s_scan, far);
    const bool first = in_l && (j == 0 || (long long)a[j] - 1 > before + 1);
    const long long incl = block_scan(first ? 1LL : 0LL, OpSum(), s_scan, groups);
    if (first) gfirst[incl - 1] = j;
  }
  const int G = (int)groups;
  __syncthreads();
  int zero = 0;
  for (int g = tid; g < G; g += BT) {
    const int j0 = gfirst[g], j1 = g + 1 < G ? gfirst[g + 1] : C;
    const int q0 = (int)b[j0];
    int stop = ge[q0];
    double score = gsc[q0];
    if (j1 - j0 > 1) {                                            // np.average(scores, weights = stop - start) (:1302)
      double sw = 0.0, sws = 0.0;
      for (int j = j0; j < j1; ++j) {
        const int q = (int)b[j];
        const double wq = (double)(ge[q] - gs[q]);
        sws += gsc[q] * wq; sw += wq;
        stop = ge[q] > stop ? ge[q] : stop;
        if (j == j0 + 1 && sw == 0.0) zero = 1;                   // the reference divides at every join: the first two decide
      }
      score = sws / sw;
    }
    if (g < capacity) {
      double* row = out + ((int64_t)sg * capacity + g) * 3;
      row[0] = (double)gs[q0]; row[1] = (double)stop; row[2] = score;
    }
  }
  zero = __syncthreads_or(zero);
  if (tid == 0) {
    counts[sg] = G;
    status[sg] = (zero ? HYPAD_FA_ZERO_WEIGHT : 0) | (G > capacity ? HYPAD_FA_OVERFLOW : 0) | (bad ? HYPAD_FA_INTERNAL : 0);
  }
}

// argument checks and the plan: per signal the clamped window / step, its windows and its workspace offset
struct FaPlan { int64_t bytes; };
int fa_check(int n_signals, const int64_t* seg_off, const int64_t* window_size, const int64_t* window_step, int lower_threshold, size_t* bytes) {
  if (n_signals < 1 || !seg_off || !window_size || !window_step || seg_off[0] != 0) return HYPAD_EINVAL;
  for (int i = 0; i < n_signals; ++i) if (seg_off[i + 1] <= seg_off[i] || window_size[i] < 1 || window_step[i] < 1) return HYPAD_EINVAL;
  const int passes = lower_threshold ? 2 : 1;
  size_t total = 0;
  for (int c0 = 0; c0 < n_signals; c0 += FA_CHUNK) {
    int64_t wsum = 0;
    for (int i = c0; i < std::min(n_signals, c0 + FA_CHUNK); ++i) {
      const int64_t n = seg_off[i + 1] - seg_off[i];
      if (n > INT_MAX) return HYPAD_EUNSUPPORTED;
      const int64_t size = std::min(window_size[i], n), step = std::min(window_step[i], n), nw = fa_windows(n, size, step);
      wsum += nw;
      if (wsum * passes > INT_MAX) return HYPAD_EUNSUPPORTED;
      const FaLayout l = fa_layout((int)size, (int)nw, passes);
      if (l.gcap > INT_MAX / 2 || l.nch > 65535) return HYPAD_EUNSUPPORTED;
      total += (size_t)l.bytes;
    }
  }
  *bytes = total;
  return HYPAD_OK;
}

}  // namespace

extern "C" {

size_t hypad_find_anomalies_signals_workspace_bytes(int n_signals, const int64_t* seg_off, const int64_t* window_size, const int64_t* window_step,
                                                    int lower_threshold) {
  size_t bytes = 0;
  return fa_check(n_signals, seg_off, window_size, window_step, lower_threshold, &bytes) ? 0 : bytes;
}

int hypad_find_anomalies_signals(const double* scores, int n_signals, const int64_t* seg_off, const int64_t* window_size,
                                 const int64_t* window_step, int64_t anomaly_padding, double min_percent, int lower_threshold, double* out,
                                 int* counts, int* status, int capacity, void* workspace, size_t workspace_bytes, hypad_stream_t stream) {
  size_t need = 0;
  const int rc = fa_check(n_signals, seg_off, window_size, window_step, lower_threshold, &need);
  if (rc) return rc;
  if (!scores || !out || !counts || !status || capacity < 1 || anomaly_padding < 0) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < need) return HYPAD_EWORKSPACE;
  const long long pad = std::min<int64_t>(anomaly_padding, INT_MAX);      // (no window is longer)
  const hipStream_t st = (hipStream_t)stream;
  int64_t wsb = 0;
  for (int c0 = 0; c0 < n_signals; c0 += FA_CHUNK) {                       // four launches per FA_CHUNK signals, five with lower_threshold
    FaTable t{};
    t.n = std::min(FA_CHUNK, n_signals - c0); t.seg0 = c0; t.passes = lower_threshold ? 2 : 1;
    int nch = 1;
    for (int i = 0; i < t.n; ++i) {
      const int64_t n = seg_off[c0 + i + 1] - seg_off[c0 + i];
      t.off[i] = seg_off[c0 + i];
      t.size[i] = (int)std::min(window_size[c0 + i], n); t.step[i] = (int)std::min(window_step[c0 + i], n);
      const int nw = (int)fa_windows(n, t.size[i], t.step[i]);
      t.woff[i + 1] = t.woff[i] + nw;
      const FaLayout l = fa_layout(t.size[i], nw, t.passes);
      t.wsb[i] = wsb; wsb += l.bytes;
      nch = std::max(nch, l.nch);
    }
    t.off[t.n] = seg_off[c0 + t.n];
    const dim3 gr((unsigned)t.woff[t.n], (unsigned)nch);
    char* ws = (char*)workspace;
    hipLaunchKernelGGL(fa_reduce_kernel<0>, gr, dim3(RED_T), 0, st, scores, ws, t);
    HYPAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(fa_reduce_kernel<1>, gr, dim3(RED_T), 0, st, scores, ws, t);
    HYPAD_CHECK_LAUNCH();
    if (lower_threshold) {
      hipLaunchKernelGGL(fa_reduce_kernel<2>, gr, dim3(RED_T), 0, st, scores, ws, t);
      HYPAD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(fa_window_kernel, dim3((unsigned)(t.woff[t.n] * t.passes)), dim3(BT), 0, st, scores, ws, t, pad, min_percent);
    HYPAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(fa_merge_kernel, dim3((unsigned)t.n), dim3(BT), 0, st, ws, t, out, counts, status, capacity);
    HYPAD_CHECK_LAUNCH();
  }
  return HYPAD_OK;
}

}  // extern "C"
