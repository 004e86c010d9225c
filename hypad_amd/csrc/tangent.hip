// The tangent maps at a point of the Poincare ball at k = -1: expmap (math_.py:1097-1102), logmap (:1226-1230), geodesic (:1042-1049),
// gyration (:657-675), parallel_transport (:1739-1746), parallel_transport0 (:1776-1779) and parallel_transport0back (:1810-1813).
// Every operand, result and gradient is (rows, dim) fp32, dim <= 256; t of geodesic holds one value, or one per row.
//
// One forward and one backward kernel per function in the launch form of dist.hip's row kernels: a wave per row, the row in fp64
// registers (RowD<64, 4>, scalar loads: any storage offset gives the same bits), sums by rowd_dot, a grid-stride walk under wave_grid.
// The per-row maps are rowops.h's *_d functions.  A backward recomputes the forward's intermediates from the operands; a gradient that
// is not asked for (NULL) is not stored, which leaves the bits of the others as they are.  No atomics, no workspace: every sum has one
// owner and a fixed order.  The per-row dL/dt of a t shared by the rows is added by the caller (hypad_column_sum at dim = 1).
#include <hip/hip_runtime.h>

#include "../../include/hypad.h"
#include "rowops.h"

using namespace hypad;

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_D = 64 * MAX_EPL;
constexpr int64_t INT_LIMIT = 0x7fffffff;
using RW = RowD<64, MAX_EPL>;                           // a row per wave

// the functions of two rows and of three, by name
struct Expmap {
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& u) { return expmap_d(x, u); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& u, const RW& go, RW& dx, RW& du) { expmap_bwd_d(x, u, go, dx, du); }
};
struct Logmap {
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& y) { return logmap_d(x, y); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& y, const RW& go, RW& dx, RW& dy) { logmap_bwd_d(x, y, go, dx, dy); }
};
template <bool BACK>
struct Transport0 {
  static __device__ __forceinline__ RW fwd(const RW& p, const RW& v) { return transport0_d<BACK>(p, v); }
  static __device__ __forceinline__ void bwd(const RW& p, const RW& v, const RW& go, RW& dp, RW& dv) { transport0_bwd_d<BACK>(p, v, go, dp, dv); }
};
struct Gyration {
  static __device__ __forceinline__ RW fwd(const RW& a, const RW& b, const RW& u) { return gyration_d(a, b, u); }
  static __device__ __forceinline__ void bwd(const RW& a, const RW& b, const RW& u, const RW& go, RW& da, RW& db, RW& du) {
    gyration_bwd_d(a, b, u, go, da, db, du);
  }
};
struct Transport {
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& y, const RW& v) { return parallel_transport_d(x, y, v); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& y, const RW& v, const RW& go, RW& dx, RW& dy, RW& dv) {
    parallel_transport_bwd_d(x, y, v, go, dx, dy, dv);
  }
};
struct Geodesic {
  static __device__ __forceinline__ RW fwd(double t, const RW& x, const RW& y) { return geodesic_d(t, x, y); }
  static __device__ __forceinline__ double bwd(double t, const RW& x, const RW& y, const RW& go, RW& dx, RW& dy) { return geodesic_bwd_d(t, x, y, go, dx, dy); }
};
struct GeodesicUnit {
  static __device__ __forceinline__ RW fwd(double t, const RW& x, const RW& u) { return geodesic_unit_d(t, x, u); }
  static __device__ __forceinline__ double bwd(double t, const RW& x, const RW& u, const RW& go, RW& dx, RW& du) {
    return geodesic_unit_bwd_d(t, x, u, go, dx, du);
  }
};
struct MobiusSub {
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& y) { return mobius_sub_d(x, y); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& y, const RW& go, RW& dx, RW& dy) { mobius_sub_bwd_d(x, y, go, dx, dy); }
};
template <bool SUB>
struct MobiusCoadd {
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& y) { return mobius_coadd_d<SUB>(x, y); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& y, const RW& go, RW& dx, RW& dy) { mobius_coadd_bwd_d<SUB>(x, y, go, dx, dy); }
};
struct Egrad2Rgrad {
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& g) { return egrad2rgrad_d(x, g); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& g, const RW& go, RW& dx, RW& dg) { egrad2rgrad_bwd_d(x, g, go, dx, dg); }
};
// the functions of N rows with one value per row: r[] the operands, d[] their gradients
struct LambdaX {
  static constexpr int N = 1;
  static __device__ __forceinline__ double fwd(const RW* r) { return lambda_x_d(r[0]); }
  static __device__ __forceinline__ void bwd(const RW* r, double g, RW* d) { lambda_x_bwd_d(r[0], g, d[0]); }
};
struct TangentNorm {
  static constexpr int N = 2;
  static __device__ __forceinline__ double fwd(const RW* r) { return tangent_norm_d(r[0], r[1]); }
  static __device__ __forceinline__ void bwd(const RW* r, double g, RW* d) { tangent_norm_bwd_d(r[0], r[1], g, d[0], d[1]); }
};
struct Inner {
  static constexpr int N = 3;
  static __device__ __forceinline__ double fwd(const RW* r) { return inner_d(r[0], r[1], r[2]); }
  static __device__ __forceinline__ void bwd(const RW* r, double g, RW* d) { inner_bwd_d(r[0], r[1], r[2], g, d[0], d[1], d[2]); }
};
// the projections: IN and OUT columns more than the ball's `dim`
struct Sproj {
  static constexpr int IN = 1, OUT = 0;
  static __device__ __forceinline__ RW fwd(const RW& h, int dim, int lane) { return sproj_d(h, dim, lane); }
  static __device__ __forceinline__ RW bwd(const RW& h, const RW& go, int dim, int lane) { return sproj_bwd_d(h, go, dim, lane); }
};
struct InvSproj {
  static constexpr int IN = 0, OUT = 1;
  static __device__ __forceinline__ RW fwd(const RW& x, int dim, int lane) { return inv_sproj_d(x, dim, lane); }
  static __device__ __forceinline__ RW bwd(const RW& x, const RW& go, int dim, int lane) { return inv_sproj_bwd_d(x, go, dim, lane); }
};
template <int N> struct Ptrs { const float* p[N]; };
template <int N> struct MutPtrs { float* p[N]; };

template <class F>
__global__ __launch_bounds__(THREADS) void rows2_fwd(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t rows,
                                                     int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dim, F::fwd(rowd_load<RW>(a + r * dim, dim, lane), rowd_load<RW>(b + r * dim, dim, lane)), dim, lane);
}
template <class F>
__global__ __launch_bounds__(THREADS) void rows2_bwd(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ go,
                                                     float* __restrict__ ga, float* __restrict__ gb, int64_t rows, int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW da, db;
    F::bwd(rowd_load<RW>(a + r * dim, dim, lane), rowd_load<RW>(b + r * dim, dim, lane), rowd_load<RW>(go + r * dim, dim, lane), da, db);
    if (ga) rowd_store(ga + r * dim, da, dim, lane);
    if (gb) rowd_store(gb + r * dim, db, dim, lane);
  }
}
template <class F>
__global__ __launch_bounds__(THREADS) void rows3_fwd(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                     float* __restrict__ out, int64_t rows, int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dim, F::fwd(rowd_load<RW>(a + r * dim, dim, lane), rowd_load<RW>(b + r * dim, dim, lane), rowd_load<RW>(c + r * dim, dim, lane)),
               dim, lane);
}
template <class F>
__global__ __launch_bounds__(THREADS) void rows3_bwd(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                     const float* __restrict__ go, float* __restrict__ ga, float* __restrict__ gb,
                                                     float* __restrict__ gc, int64_t rows, int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW da, db, dc;
    F::bwd(rowd_load<RW>(a + r * dim, dim, lane), rowd_load<RW>(b + r * dim, dim, lane), rowd_load<RW>(c + r * dim, dim, lane),
           rowd_load<RW>(go + r * dim, dim, lane), da, db, dc);
    if (ga) rowd_store(ga + r * dim, da, dim, lane);
    if (gb) rowd_store(gb + r * dim, db, dim, lane);
    if (gc) rowd_store(gc + r * dim, dc, dim, lane);
  }
}
// a scalar t and two rows (geodesic, geodesic_unit): t of one value (tbc) or one per row
template <class F>
__global__ __launch_bounds__(THREADS) void rowst_fwd(const float* __restrict__ t, const float* __restrict__ x, const float* __restrict__ y,
                                                     float* __restrict__ out, int64_t rows, int dim, int tbc) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dim, F::fwd((double)t[tbc ? 0 : r], rowd_load<RW>(x + r * dim, dim, lane), rowd_load<RW>(y + r * dim, dim, lane)), dim, lane);
}
template <class F>
__global__ __launch_bounds__(THREADS) void rowst_bwd(const float* __restrict__ t, const float* __restrict__ x, const float* __restrict__ y,
                                                     const float* __restrict__ go, float* __restrict__ gt, float* __restrict__ gx,
                                                     float* __restrict__ gy, int64_t rows, int dim, int tbc) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW dx, dy;
    const double g = F::bwd((double)t[tbc ? 0 : r], rowd_load<RW>(x + r * dim, dim, lane), rowd_load<RW>(y + r * dim, dim, lane),
                            rowd_load<RW>(go + r * dim, dim, lane), dx, dy);
    if (gt && lane == 0) gt[r] = (float)g;
    if (gx) rowd_store(gx + r * dim, dx, dim, lane);
    if (gy) rowd_store(gy + r * dim, dy, dim, lane);
  }
}
// N rows to one value per row (lambda_x, norm, inner), the form of dist.hip's dist_rows / dist_rows_bwd
template <class F>
__global__ __launch_bounds__(THREADS) void rows_scalar_fwd(const Ptrs<F::N> ops, float* __restrict__ out, int64_t rows, int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW a[F::N];
#pragma unroll
    for (int i = 0; i < F::N; ++i) a[i] = rowd_load<RW>(ops.p[i] + r * dim, dim, lane);
    const double o = F::fwd(a);
    if (lane == 0) out[r] = (float)o;
  }
}
template <class F>
__global__ __launch_bounds__(THREADS) void rows_scalar_bwd(const Ptrs<F::N> ops, const float* __restrict__ go, const MutPtrs<F::N> grads, int64_t rows,
                                                           int dim) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW a[F::N], d[F::N];
#pragma unroll
    for (int i = 0; i < F::N; ++i) a[i] = rowd_load<RW>(ops.p[i] + r * dim, dim, lane);
    F::bwd(a, (double)go[r], d);
#pragma unroll
    for (int i = 0; i < F::N; ++i)
      if (grads.p[i]) rowd_store(grads.p[i] + r * dim, d[i], dim, lane);
  }
}
// a row of dim + F::IN elements to one of dim + F::OUT (sproj, inv_sproj)
template <class F>
__global__ __launch_bounds__(THREADS) void proj_fwd(const float* __restrict__ a, float* __restrict__ out, int64_t rows, int dim) {
  const int lane = threadIdx.x & 63, din = dim + F::IN, dout = dim + F::OUT;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dout, F::fwd(rowd_load<RW>(a + r * din, din, lane), dim, lane), dout, lane);
}
template <class F>
__global__ __launch_bounds__(THREADS) void proj_bwd(const float* __restrict__ a, const float* __restrict__ go, float* __restrict__ ga, int64_t rows,
                                                    int dim) {
  const int lane = threadIdx.x & 63, din = dim + F::IN, dout = dim + F::OUT;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(ga + r * din, F::bwd(rowd_load<RW>(a + r * din, din, lane), rowd_load<RW>(go + r * dout, dout, lane), dim, lane), din, lane);
}

inline int wave_grid(int64_t rows) {
  const int64_t b = (rows + WAVES - 1) / WAVES;
  return (int)(b > 4096 ? 4096 : b < 1 ? 1 : b);
}
// sizes first, then the operands: each of `n` pointers may be NULL only where there are no rows
inline int rows_check(int64_t rows, int dim, const void* const* ops, int n) {
  if (rows < 0 || dim <= 0) return HYPAD_EINVAL;
  if (dim > MAX_D || rows > INT_LIMIT / dim) return HYPAD_EUNSUPPORTED;
  for (int i = 0; i < n; ++i)
    if (!ops[i] && rows > 0) return HYPAD_EINVAL;
  return HYPAD_OK;
}

template <class F>
int launch2_fwd(const float* a, const float* b, float* out, int64_t rows, int dim, hypad_stream_t s) {
  const void* ops[] = {a, b, out};
  const int rc = rows_check(rows, dim, ops, 3);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(rows2_fwd<F>, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, b, out, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F>
int launch2_bwd(const float* a, const float* b, const float* go, float* ga, float* gb, int64_t rows, int dim, hypad_stream_t s) {
  const void* ops[] = {a, b, go};
  const int rc = rows_check(rows, dim, ops, 3);
  if (rc || rows == 0 || (!ga && !gb)) return rc;
  hipLaunchKernelGGL(rows2_bwd<F>, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, b, go, ga, gb, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F>
int launch3_fwd(const float* a, const float* b, const float* c, float* out, int64_t rows, int dim, hypad_stream_t s) {
  const void* ops[] = {a, b, c, out};
  const int rc = rows_check(rows, dim, ops, 4);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(rows3_fwd<F>, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, b, c, out, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F>
int launch3_bwd(const float* a, const float* b, const float* c, const float* go, float* ga, float* gb, float* gc, int64_t rows, int dim,
                hypad_stream_t s) {
  const void* ops[] = {a, b, c, go};
  const int rc = rows_check(rows, dim, ops, 4);
  if (rc || rows == 0 || (!ga && !gb && !gc)) return rc;
  hipLaunchKernelGGL(rows3_bwd<F>, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, b, c, go, ga, gb, gc, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
// t_count values of t: one, or one per row (one value even where there are no rows)
template <class F>
int launcht_fwd(const float* t, const float* x, const float* y, float* out, int64_t rows, int dim, int64_t t_count, hypad_stream_t s) {
  const void* ops[] = {t, x, y, out};
  const int rc = rows_check(rows, dim, ops, 4);
  if (rc) return rc;
  if (t_count != 1 && t_count != rows) return HYPAD_EINVAL;
  if (!t && t_count > 0) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  hipLaunchKernelGGL(rowst_fwd<F>, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, t, x, y, out, rows, dim, (int)(t_count == 1 && rows != 1));
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F>
int launcht_bwd(const float* t, const float* x, const float* y, const float* go, float* gt, float* gx, float* gy, int64_t rows, int dim,
                int64_t t_count, hypad_stream_t s) {
  const void* ops[] = {t, x, y, go};
  const int rc = rows_check(rows, dim, ops, 4);
  if (rc) return rc;
  if (t_count != 1 && t_count != rows) return HYPAD_EINVAL;
  if (!t && t_count > 0) return HYPAD_EINVAL;
  if (rows == 0 || (!gt && !gx && !gy)) return HYPAD_OK;
  hipLaunchKernelGGL(rowst_bwd<F>, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, t, x, y, go, gt, gx, gy, rows, dim,
                     (int)(t_count == 1 && rows != 1));
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F>
int launch_scalar_fwd(const Ptrs<F::N> in, float* out, int64_t rows, int dim, hypad_stream_t s) {
  const void* ops[F::N + 1];
  for (int i = 0; i < F::N; ++i) ops[i] = in.p[i];
  ops[F::N] = out;
  const int rc = rows_check(rows, dim, ops, F::N + 1);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(rows_scalar_fwd<F>, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, in, out, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F>
int launch_scalar_bwd(const Ptrs<F::N> in, const float* go, const MutPtrs<F::N> grads, int64_t rows, int dim, hypad_stream_t s) {
  const void* ops[F::N + 1];
  bool any = false;
  for (int i = 0; i < F::N; ++i) { ops[i] = in.p[i]; any = any || grads.p[i]; }
  ops[F::N] = go;
  const int rc = rows_check(rows, dim, ops, F::N + 1);
  if (rc || rows == 0 || !any) return rc;
  hipLaunchKernelGGL(rows_scalar_bwd<F>, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, in, go, grads, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
// the wider side, dim + 1, is held to the limits
template <class F>
int launch_proj_fwd(const float* a, float* out, int64_t rows, int dim, hypad_stream_t s) {
  const void* ops[] = {a, out};
  if (dim <= 0) return HYPAD_EINVAL;
  const int rc = rows_check(rows, dim + 1, ops, 2);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(proj_fwd<F>, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, out, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F>
int launch_proj_bwd(const float* a, const float* go, float* ga, int64_t rows, int dim, hypad_stream_t s) {
  const void* ops[] = {a, go};
  if (dim <= 0) return HYPAD_EINVAL;
  const int rc = rows_check(rows, dim + 1, ops, 2);
  if (rc || rows == 0 || !ga) return rc;
  hipLaunchKernelGGL(proj_bwd<F>, dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, go, ga, rows, dim);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

}  // namespace

extern "C" {

int hypad_expmap_fwd(const float* x, const float* u, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_fwd<Expmap>(x, u, out, rows, dim, s);
}
int hypad_expmap_bwd(const float* x, const float* u, const float* grad_out, float* grad_x, float* grad_u, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_bwd<Expmap>(x, u, grad_out, grad_x, grad_u, rows, dim, s);
}
int hypad_logmap_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_fwd<Logmap>(x, y, out, rows, dim, s);
}
int hypad_logmap_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_bwd<Logmap>(x, y, grad_out, grad_x, grad_y, rows, dim, s);
}
int hypad_geodesic_fwd(const float* t, const float* x, const float* y, float* out, int64_t rows, int dim, int64_t t_count, hypad_stream_t s) {
  return launcht_fwd<Geodesic>(t, x, y, out, rows, dim, t_count, s);
}
int hypad_geodesic_bwd(const float* t, const float* x, const float* y, const float* grad_out, float* grad_t, float* grad_x, float* grad_y,
                       int64_t rows, int dim, int64_t t_count, hypad_stream_t s) {
  return launcht_bwd<Geodesic>(t, x, y, grad_out, grad_t, grad_x, grad_y, rows, dim, t_count, s);
}
int hypad_gyration_fwd(const float* a, const float* b, const float* u, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch3_fwd<Gyration>(a, b, u, out, rows, dim, s);
}
int hypad_gyration_bwd(const float* a, const float* b, const float* u, const float* grad_out, float* grad_a, float* grad_b, float* grad_u,
                       int64_t rows, int dim, hypad_stream_t s) {
  return launch3_bwd<Gyration>(a, b, u, grad_out, grad_a, grad_b, grad_u, rows, dim, s);
}
int hypad_parallel_transport_fwd(const float* x, const float* y, const float* v, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch3_fwd<Transport>(x, y, v, out, rows, dim, s);
}
int hypad_parallel_transport_bwd(const float* x, const float* y, const float* v, const float* grad_out, float* grad_x, float* grad_y, float* grad_v,
                                 int64_t rows, int dim, hypad_stream_t s) {
  return launch3_bwd<Transport>(x, y, v, grad_out, grad_x, grad_y, grad_v, rows, dim, s);
}
int hypad_parallel_transport0_fwd(const float* y, const float* v, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_fwd<Transport0<false>>(y, v, out, rows, dim, s);
}
int hypad_parallel_transport0_bwd(const float* y, const float* v, const float* grad_out, float* grad_y, float* grad_v, int64_t rows, int dim,
                                  hypad_stream_t s) {
  return launch2_bwd<Transport0<false>>(y, v, grad_out, grad_y, grad_v, rows, dim, s);
}
int hypad_parallel_transport0back_fwd(const float* x, const float* v, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_fwd<Transport0<true>>(x, v, out, rows, dim, s);
}
int hypad_parallel_transport0back_bwd(const float* x, const float* v, const float* grad_out, float* grad_x, float* grad_v, int64_t rows, int dim,
                                      hypad_stream_t s) {
  return launch2_bwd<Transport0<true>>(x, v, grad_out, grad_x, grad_v, rows, dim, s);
}
int hypad_mobius_sub_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_fwd<MobiusSub>(x, y, out, rows, dim, s);
}
int hypad_mobius_sub_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_bwd<MobiusSub>(x, y, grad_out, grad_x, grad_y, rows, dim, s);
}
int hypad_mobius_coadd_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_fwd<MobiusCoadd<false>>(x, y, out, rows, dim, s);
}
int hypad_mobius_coadd_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                           hypad_stream_t s) {
  return launch2_bwd<MobiusCoadd<false>>(x, y, grad_out, grad_x, grad_y, rows, dim, s);
}
int hypad_mobius_cosub_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_fwd<MobiusCoadd<true>>(x, y, out, rows, dim, s);
}
int hypad_mobius_cosub_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                           hypad_stream_t s) {
  return launch2_bwd<MobiusCoadd<true>>(x, y, grad_out, grad_x, grad_y, rows, dim, s);
}
int hypad_geodesic_unit_fwd(const float* t, const float* x, const float* u, float* out, int64_t rows, int dim, int64_t t_count, hypad_stream_t s) {
  return launcht_fwd<GeodesicUnit>(t, x, u, out, rows, dim, t_count, s);
}
int hypad_geodesic_unit_bwd(const float* t, const float* x, const float* u, const float* grad_out, float* grad_t, float* grad_x, float* grad_u,
                            int64_t rows, int dim, int64_t t_count, hypad_stream_t s) {
  return launcht_bwd<GeodesicUnit>(t, x, u, grad_out, grad_t, grad_x, grad_u, rows, dim, t_count, s);
}
int hypad_lambda_x_fwd(const float* x, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch_scalar_fwd<LambdaX>({{x}}, out, rows, dim, s);
}
int hypad_lambda_x_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, hypad_stream_t s) {
  return launch_scalar_bwd<LambdaX>({{x}}, grad_out, {{grad_x}}, rows, dim, s);
}
int hypad_inner_fwd(const float* x, const float* u, const float* v, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch_scalar_fwd<Inner>({{x, u, v}}, out, rows, dim, s);
}
int hypad_inner_bwd(const float* x, const float* u, const float* v, const float* grad_out, float* grad_x, float* grad_u, float* grad_v,
                    int64_t rows, int dim, hypad_stream_t s) {
  return launch_scalar_bwd<Inner>({{x, u, v}}, grad_out, {{grad_x, grad_u, grad_v}}, rows, dim, s);
}
int hypad_norm_fwd(const float* x, const float* u, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch_scalar_fwd<TangentNorm>({{x, u}}, out, rows, dim, s);
}
int hypad_norm_bwd(const float* x, const float* u, const float* grad_out, float* grad_x, float* grad_u, int64_t rows, int dim, hypad_stream_t s) {
  return launch_scalar_bwd<TangentNorm>({{x, u}}, grad_out, {{grad_x, grad_u}}, rows, dim, s);
}
int hypad_egrad2rgrad_fwd(const float* x, const float* grad, float* out, int64_t rows, int dim, hypad_stream_t s) {
  return launch2_fwd<Egrad2Rgrad>(x, grad, out, rows, dim, s);
}
int hypad_egrad2rgrad_bwd(const float* x, const float* grad, const float* grad_out, float* grad_x, float* grad_grad, int64_t rows, int dim,
                          hypad_stream_t s) {
  return launch2_bwd<Egrad2Rgrad>(x, grad, grad_out, grad_x, grad_grad, rows, dim, s);
}
int hypad_sproj_fwd(const float* h, float* out, int64_t rows, int dim, hypad_stream_t s) { return launch_proj_fwd<Sproj>(h, out, rows, dim, s); }
int hypad_sproj_bwd(const float* h, const float* grad_out, float* grad_h, int64_t rows, int dim, hypad_stream_t s) {
  return launch_proj_bwd<Sproj>(h, grad_out, grad_h, rows, dim, s);
}
int hypad_inv_sproj_fwd(const float* x, float* out, int64_t rows, int dim, hypad_stream_t s) { return launch_proj_fwd<InvSproj>(x, out, rows, dim, s); }
int hypad_inv_sproj_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, hypad_stream_t s) {
  return launch_proj_bwd<InvSproj>(x, grad_out, grad_x, rows, dim, s);
}

}  // extern "C"
