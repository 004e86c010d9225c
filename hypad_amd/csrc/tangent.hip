// The tangent maps at a point of the Poincare ball at k = -1: expmap (math_.py:1097-1102), logmap (:1226-1230), geodesic (:1042-1049),
// gyration (:657-675), parallel_transport (:1739-1746), parallel_transport0 (:1776-1779) and parallel_transport0back (:1810-1813).
// Every operand, result and gradient is (rows, dim) fp32, dim <= 256; t of geodesic holds one value, or one per row.
//
// One forward and one backward kernel per function in the launch form of dist.hip's row kernels: a wave per row, the row in fp64
// registers (RowD<64, 4>, scalar loads: any storage offset gives the same bits), sums by rowd_dot, a grid-stride walk under wave_grid.
// The per-row maps are rowops.h's *_d functions.  A backward recomputes the forward's intermediates from the operands; a gradient that
// is not asked for (NULL) is not stored, which leaves the bits of the others as they are.  No atomics, no workspace: every sum has one
// owner and a fixed order.  The per-row dL/dt of a t shared by the rows is added by the caller (hypad_column_sum at dim = 1).
//
// Any negative curvature k = -c (the hypad_ball_* entry points, docs/history/curvature.md): with s = sqrt(c), x -> s x takes the ball of
// radius 1 / s onto the unit ball and carries every function of math_.py at -c onto itself at -1, clamps included.  So
// f_c(a_0, ...) = s^EO f_1(s^E[0] a_0, ...) with the exponents each functor names, and the chain rule through those factors is the
// backward: grad_out times s^EO going in, every operand's gradient times its s^E[i] coming out.  The kernels are the same templates: a
// k = -1 launch passes no curvature at all and gets the code it always had, a curved one passes Curved as one more kernel argument.
// These entry points also cover the row functions whose k = -1 kernels live elsewhere (project, expmap0, logmap0, mobius_add,
// mobius_pointwise_mul, mobius_scalar_mul, dist, dist0), in this launch form.
#include <hip/hip_runtime.h>

#include <cmath>
#include <utility>

#include "../../include/hypad.h"
#include "rowops.h"

using namespace hypad;

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_D = 64 * MAX_EPL;
constexpr int64_t INT_LIMIT = 0x7fffffff;
using RW = RowD<64, MAX_EPL>;                           // a row per wave

// The curvature of a launch: the kernels take it as a trailing pack that is empty at k = -1 (Unit: every scaling is the identity and
// leaves no instruction) and holds one Curved, sqrt(c) and its reciprocal, at k = -c.  sc<E> multiplies by s^E, E in {-1, 0, 1}.
struct Unit {};
struct Curved {
  double s, rs;
  explicit Curved(double c) : s(std::sqrt(c)), rs(1.0 / std::sqrt(c)) {}
};
__device__ __forceinline__ Unit curvature() { return {}; }
__device__ __forceinline__ Curved curvature(const Curved& c) { return c; }
template <int E> __device__ __forceinline__ double sc(Unit, double a) { return a; }
template <int E> __device__ __forceinline__ const RW& sc(Unit, const RW& a) { return a; }   // (the row itself: a copy here moved registers about)
template <int E> __device__ __forceinline__ double sc(const Curved& c, double a) { return E == 1 ? a * c.s : E == -1 ? a * c.rs : a; }
template <int E> __device__ __forceinline__ RW sc(const Curved& c, RW a) {
  if (E != 0) {
#pragma unroll
    for (int e = 0; e < RW::EPL; ++e) a.v[e] = sc<E>(c, a.v[e]);
  }
  return a;
}
// the rows a[i] of a functor, each times its s^F::E[i]
template <class F, class C, int... I>
__device__ __forceinline__ void scale_each(const C& cv, RW* a, std::integer_sequence<int, I...>) {
  ((a[I] = sc<F::E[I]>(cv, a[I])), ...);
}

// the functions of two rows and of three, by name; E[i] and EO: the exponents of s = sqrt(c) on operand i and on the result
struct Expmap {
  static constexpr int E[2] = {1, 1}, EO = -1;
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& u) { return expmap_d(x, u); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& u, const RW& go, RW& dx, RW& du) { expmap_bwd_d(x, u, go, dx, du); }
};
struct Logmap {
  static constexpr int E[2] = {1, 1}, EO = -1;
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& y) { return logmap_d(x, y); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& y, const RW& go, RW& dx, RW& dy) { logmap_bwd_d(x, y, go, dx, dy); }
};
template <bool BACK>
struct Transport0 {
  static constexpr int E[2] = {1, 0}, EO = 0;
  static __device__ __forceinline__ RW fwd(const RW& p, const RW& v) { return transport0_d<BACK>(p, v); }
  static __device__ __forceinline__ void bwd(const RW& p, const RW& v, const RW& go, RW& dp, RW& dv) { transport0_bwd_d<BACK>(p, v, go, dp, dv); }
};
struct Gyration {
  static constexpr int E[3] = {1, 1, 0}, EO = 0;
  static __device__ __forceinline__ RW fwd(const RW& a, const RW& b, const RW& u) { return gyration_d(a, b, u); }
  static __device__ __forceinline__ void bwd(const RW& a, const RW& b, const RW& u, const RW& go, RW& da, RW& db, RW& du) {
    gyration_bwd_d(a, b, u, go, da, db, du);
  }
};
struct Transport {
  static constexpr int E[3] = {1, 1, 0}, EO = 0;
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& y, const RW& v) { return parallel_transport_d(x, y, v); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& y, const RW& v, const RW& go, RW& dx, RW& dy, RW& dv) {
    parallel_transport_bwd_d(x, y, v, go, dx, dy, dv);
  }
};
struct Geodesic {
  static constexpr int E[3] = {0, 1, 1}, EO = -1;
  static __device__ __forceinline__ RW fwd(double t, const RW& x, const RW& y) { return geodesic_d(t, x, y); }
  static __device__ __forceinline__ double bwd(double t, const RW& x, const RW& y, const RW& go, RW& dx, RW& dy) { return geodesic_bwd_d(t, x, y, go, dx, dy); }
};
struct GeodesicUnit {
  static constexpr int E[3] = {1, 1, 0}, EO = -1;
  static __device__ __forceinline__ RW fwd(double t, const RW& x, const RW& u) { return geodesic_unit_d(t, x, u); }
  static __device__ __forceinline__ double bwd(double t, const RW& x, const RW& u, const RW& go, RW& dx, RW& du) {
    return geodesic_unit_bwd_d(t, x, u, go, dx, du);
  }
};
struct MobiusSub {
  static constexpr int E[2] = {1, 1}, EO = -1;
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& y) { return mobius_sub_d(x, y); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& y, const RW& go, RW& dx, RW& dy) { mobius_sub_bwd_d(x, y, go, dx, dy); }
};
template <bool SUB>
struct MobiusCoadd {
  static constexpr int E[2] = {1, 1}, EO = -1;
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& y) { return mobius_coadd_d<SUB>(x, y); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& y, const RW& go, RW& dx, RW& dy) { mobius_coadd_bwd_d<SUB>(x, y, go, dx, dy); }
};
struct MobiusAdd {
  static constexpr int E[2] = {1, 1}, EO = -1;
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& y) { return mobius_add_d(x, y); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& y, const RW& go, RW& dx, RW& dy) { mobius_add_bwd_d(x, y, go, dx, dy); }
};
struct MobiusPointwiseMul {
  static constexpr int E[2] = {0, 1}, EO = -1;
  static __device__ __forceinline__ RW fwd(const RW& w, const RW& x) { return mobius_pointwise_mul_d(w, x); }
  static __device__ __forceinline__ void bwd(const RW& w, const RW& x, const RW& go, RW& dw, RW& dx) { mobius_pointwise_mul_bwd_d(w, x, go, dw, dx); }
};
struct Egrad2Rgrad {
  static constexpr int E[2] = {1, 0}, EO = 0;
  static __device__ __forceinline__ RW fwd(const RW& x, const RW& g) { return egrad2rgrad_d(x, g); }
  static __device__ __forceinline__ void bwd(const RW& x, const RW& g, const RW& go, RW& dx, RW& dg) { egrad2rgrad_bwd_d(x, g, go, dx, dg); }
};
// the functions of one row
struct Project {
  static constexpr int E[1] = {1}, EO = -1;
  static __device__ __forceinline__ RW fwd(const RW& x) { return project_d(x); }
  static __device__ __forceinline__ RW bwd(const RW& x, const RW& go) { return project_bwd_d(x, go); }
};
template <bool EXP>
struct RadialMap {                                           // expmap0 (EXP) and logmap0
  static constexpr int E[1] = {1}, EO = -1;
  static __device__ __forceinline__ RW fwd(const RW& u) { return radial_map_d<EXP>(u); }
  static __device__ __forceinline__ RW bwd(const RW& u, const RW& go) { return radial_map_bwd_d<EXP>(u, go); }
};
// a scalar r and one row
struct MobiusScalarMul {
  static constexpr int E[2] = {0, 1}, EO = -1;
  static __device__ __forceinline__ RW fwd(double r, const RW& x) { return mobius_scalar_mul_d(r, x); }
  static __device__ __forceinline__ double bwd(double r, const RW& x, const RW& go, RW& dx) { return mobius_scalar_mul_bwd_d(r, x, go, dx); }
};
// the functions of N rows with one value per row: r[] the operands, d[] their gradients
struct LambdaX {
  static constexpr int E[1] = {1}, EO = 0;
  static constexpr int N = 1;
  static __device__ __forceinline__ double fwd(const RW* r) { return lambda_x_d(r[0]); }
  static __device__ __forceinline__ void bwd(const RW* r, double g, RW* d) { lambda_x_bwd_d(r[0], g, d[0]); }
};
struct TangentNorm {
  static constexpr int E[2] = {1, 0}, EO = 0;
  static constexpr int N = 2;
  static __device__ __forceinline__ double fwd(const RW* r) { return tangent_norm_d(r[0], r[1]); }
  static __device__ __forceinline__ void bwd(const RW* r, double g, RW* d) { tangent_norm_bwd_d(r[0], r[1], g, d[0], d[1]); }
};
struct Inner {
  static constexpr int E[3] = {1, 0, 0}, EO = 0;
  static constexpr int N = 3;
  static __device__ __forceinline__ double fwd(const RW* r) { return inner_d(r[0], r[1], r[2]); }
  static __device__ __forceinline__ void bwd(const RW* r, double g, RW* d) { inner_bwd_d(r[0], r[1], r[2], g, d[0], d[1], d[2]); }
};
struct Dist {
  static constexpr int N = 2;
  static constexpr int E[2] = {1, 1}, EO = -1;
  static __device__ __forceinline__ double fwd(const RW* r) { return dist_row_d(r[0], r[1]); }
  static __device__ __forceinline__ void bwd(const RW* r, double g, RW* d) { dist_row_bwd_d(r[0], r[1], g, d[0], d[1]); }
};
struct Dist0 {
  static constexpr int N = 1;
  static constexpr int E[1] = {1}, EO = -1;
  static __device__ __forceinline__ double fwd(const RW* r) { return dist0_row_d(r[0]); }
  static __device__ __forceinline__ void bwd(const RW* r, double g, RW* d) { d[0] = dist0_row_bwd_d(r[0], g); }
};
// the projections: IN and OUT columns more than the ball's `dim`
struct Sproj {
  static constexpr int IN = 1, OUT = 0, E[1] = {1}, EO = -1;
  static __device__ __forceinline__ RW fwd(const RW& h, int dim, int lane) { return sproj_d(h, dim, lane); }
  static __device__ __forceinline__ RW bwd(const RW& h, const RW& go, int dim, int lane) { return sproj_bwd_d(h, go, dim, lane); }
};
struct InvSproj {
  static constexpr int IN = 0, OUT = 1, E[1] = {1}, EO = -1;
  static __device__ __forceinline__ RW fwd(const RW& x, int dim, int lane) { return inv_sproj_d(x, dim, lane); }
  static __device__ __forceinline__ RW bwd(const RW& x, const RW& go, int dim, int lane) { return inv_sproj_bwd_d(x, go, dim, lane); }
};
template <int N> struct Ptrs { const float* p[N]; };
template <int N> struct MutPtrs { float* p[N]; };

// K... below: the launch's curvature -- nothing at k = -1, one Curved at k = -c
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rows1_fwd(const float* __restrict__ a, float* __restrict__ out, int64_t rows, int dim, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dim, sc<F::EO>(cv, F::fwd(sc<F::E[0]>(cv, rowd_load<RW>(a + r * dim, dim, lane)))), dim, lane);
}
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rows1_bwd(const float* __restrict__ a, const float* __restrict__ go, float* __restrict__ ga, int64_t rows,
                                                     int dim, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(ga + r * dim,
               sc<F::E[0]>(cv, F::bwd(sc<F::E[0]>(cv, rowd_load<RW>(a + r * dim, dim, lane)), sc<F::EO>(cv, rowd_load<RW>(go + r * dim, dim, lane)))),
               dim, lane);
}
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rows2_fwd(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t rows,
                                                     int dim, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dim,
               sc<F::EO>(cv, F::fwd(sc<F::E[0]>(cv, rowd_load<RW>(a + r * dim, dim, lane)), sc<F::E[1]>(cv, rowd_load<RW>(b + r * dim, dim, lane)))), dim,
               lane);
}
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rows2_bwd(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ go,
                                                     float* __restrict__ ga, float* __restrict__ gb, int64_t rows, int dim, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW da, db;
    F::bwd(sc<F::E[0]>(cv, rowd_load<RW>(a + r * dim, dim, lane)), sc<F::E[1]>(cv, rowd_load<RW>(b + r * dim, dim, lane)),
           sc<F::EO>(cv, rowd_load<RW>(go + r * dim, dim, lane)), da, db);
    if (ga) rowd_store(ga + r * dim, sc<F::E[0]>(cv, da), dim, lane);
    if (gb) rowd_store(gb + r * dim, sc<F::E[1]>(cv, db), dim, lane);
  }
}
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rows3_fwd(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                     float* __restrict__ out, int64_t rows, int dim, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dim,
               sc<F::EO>(cv, F::fwd(sc<F::E[0]>(cv, rowd_load<RW>(a + r * dim, dim, lane)), sc<F::E[1]>(cv, rowd_load<RW>(b + r * dim, dim, lane)),
                                    sc<F::E[2]>(cv, rowd_load<RW>(c + r * dim, dim, lane)))),
               dim, lane);
}
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rows3_bwd(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                     const float* __restrict__ go, float* __restrict__ ga, float* __restrict__ gb,
                                                     float* __restrict__ gc, int64_t rows, int dim, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW da, db, dc;
    F::bwd(sc<F::E[0]>(cv, rowd_load<RW>(a + r * dim, dim, lane)), sc<F::E[1]>(cv, rowd_load<RW>(b + r * dim, dim, lane)),
           sc<F::E[2]>(cv, rowd_load<RW>(c + r * dim, dim, lane)), sc<F::EO>(cv, rowd_load<RW>(go + r * dim, dim, lane)), da, db, dc);
    if (ga) rowd_store(ga + r * dim, sc<F::E[0]>(cv, da), dim, lane);
    if (gb) rowd_store(gb + r * dim, sc<F::E[1]>(cv, db), dim, lane);
    if (gc) rowd_store(gc + r * dim, sc<F::E[2]>(cv, dc), dim, lane);
  }
}
// a scalar t and two rows (geodesic, geodesic_unit): t of one value (tbc) or one per row
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rowst_fwd(const float* __restrict__ t, const float* __restrict__ x, const float* __restrict__ y,
                                                     float* __restrict__ out, int64_t rows, int dim, int tbc, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dim,
               sc<F::EO>(cv, F::fwd(sc<F::E[0]>(cv, (double)t[tbc ? 0 : r]), sc<F::E[1]>(cv, rowd_load<RW>(x + r * dim, dim, lane)),
                                    sc<F::E[2]>(cv, rowd_load<RW>(y + r * dim, dim, lane)))),
               dim, lane);
}
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rowst_bwd(const float* __restrict__ t, const float* __restrict__ x, const float* __restrict__ y,
                                                     const float* __restrict__ go, float* __restrict__ gt, float* __restrict__ gx,
                                                     float* __restrict__ gy, int64_t rows, int dim, int tbc, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW dx, dy;
    const double g = F::bwd(sc<F::E[0]>(cv, (double)t[tbc ? 0 : r]), sc<F::E[1]>(cv, rowd_load<RW>(x + r * dim, dim, lane)),
                            sc<F::E[2]>(cv, rowd_load<RW>(y + r * dim, dim, lane)), sc<F::EO>(cv, rowd_load<RW>(go + r * dim, dim, lane)), dx, dy);
    if (gt && lane == 0) gt[r] = (float)sc<F::E[0]>(cv, g);
    if (gx) rowd_store(gx + r * dim, sc<F::E[1]>(cv, dx), dim, lane);
    if (gy) rowd_store(gy + r * dim, sc<F::E[2]>(cv, dy), dim, lane);
  }
}
// a scalar r and one row (mobius_scalar_mul): r of one value (rbc) or one per row
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rowsr_fwd(const float* __restrict__ rs, const float* __restrict__ x, float* __restrict__ out, int64_t rows,
                                                     int dim, int rbc, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dim, sc<F::EO>(cv, F::fwd(sc<F::E[0]>(cv, (double)rs[rbc ? 0 : r]), sc<F::E[1]>(cv, rowd_load<RW>(x + r * dim, dim, lane)))),
               dim, lane);
}
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rowsr_bwd(const float* __restrict__ rs, const float* __restrict__ x, const float* __restrict__ go,
                                                     float* __restrict__ gr, float* __restrict__ gx, int64_t rows, int dim, int rbc, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW dx;
    const double g = F::bwd(sc<F::E[0]>(cv, (double)rs[rbc ? 0 : r]), sc<F::E[1]>(cv, rowd_load<RW>(x + r * dim, dim, lane)),
                            sc<F::EO>(cv, rowd_load<RW>(go + r * dim, dim, lane)), dx);
    if (gr && lane == 0) gr[r] = (float)sc<F::E[0]>(cv, g);
    if (gx) rowd_store(gx + r * dim, sc<F::E[1]>(cv, dx), dim, lane);
  }
}
// N rows to one value per row (lambda_x, norm, inner, dist, dist0), the form of dist.hip's dist_rows / dist_rows_bwd
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rows_scalar_fwd(const Ptrs<F::N> ops, float* __restrict__ out, int64_t rows, int dim, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW a[F::N];
#pragma unroll
    for (int i = 0; i < F::N; ++i) a[i] = rowd_load<RW>(ops.p[i] + r * dim, dim, lane);
    scale_each<F>(cv, a, std::make_integer_sequence<int, F::N>{});
    const double o = sc<F::EO>(cv, F::fwd(a));
    if (lane == 0) out[r] = (float)o;
  }
}
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void rows_scalar_bwd(const Ptrs<F::N> ops, const float* __restrict__ go, const MutPtrs<F::N> grads, int64_t rows,
                                                           int dim, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW a[F::N], d[F::N];
#pragma unroll
    for (int i = 0; i < F::N; ++i) a[i] = rowd_load<RW>(ops.p[i] + r * dim, dim, lane);
    scale_each<F>(cv, a, std::make_integer_sequence<int, F::N>{});
    F::bwd(a, sc<F::EO>(cv, (double)go[r]), d);
    scale_each<F>(cv, d, std::make_integer_sequence<int, F::N>{});
#pragma unroll
    for (int i = 0; i < F::N; ++i)
      if (grads.p[i]) rowd_store(grads.p[i] + r * dim, d[i], dim, lane);
  }
}
// a row of dim + F::IN elements to one of dim + F::OUT (sproj, inv_sproj)
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void proj_fwd(const float* __restrict__ a, float* __restrict__ out, int64_t rows, int dim, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63, din = dim + F::IN, dout = dim + F::OUT;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(out + r * dout, sc<F::EO>(cv, F::fwd(sc<F::E[0]>(cv, rowd_load<RW>(a + r * din, din, lane)), dim, lane)), dout, lane);
}
template <class F, class... K>
__global__ __launch_bounds__(THREADS) void proj_bwd(const float* __restrict__ a, const float* __restrict__ go, float* __restrict__ ga, int64_t rows,
                                                    int dim, K... k) {
  const auto cv = curvature(k...);
  const int lane = threadIdx.x & 63, din = dim + F::IN, dout = dim + F::OUT;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES)
    rowd_store(ga + r * din,
               sc<F::E[0]>(cv, F::bwd(sc<F::E[0]>(cv, rowd_load<RW>(a + r * din, din, lane)), sc<F::EO>(cv, rowd_load<RW>(go + r * dout, dout, lane)), dim,
                                      lane)),
               din, lane);
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
// the hypad_ball_* entry points: c finite and positive
inline bool bad_c(double c) { return !(c > 0.0) || !std::isfinite(c); }

template <class F, class... K>
int launch1_fwd(const float* a, float* out, int64_t rows, int dim, hypad_stream_t s, K... k) {
  const void* ops[] = {a, out};
  const int rc = rows_check(rows, dim, ops, 2);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rows1_fwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, out, rows, dim, k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F, class... K>
int launch1_bwd(const float* a, const float* go, float* ga, int64_t rows, int dim, hypad_stream_t s, K... k) {
  const void* ops[] = {a, go};
  const int rc = rows_check(rows, dim, ops, 2);
  if (rc || rows == 0 || !ga) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rows1_bwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, go, ga, rows, dim, k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F, class... K>
int launch2_fwd(const float* a, const float* b, float* out, int64_t rows, int dim, hypad_stream_t s, K... k) {
  const void* ops[] = {a, b, out};
  const int rc = rows_check(rows, dim, ops, 3);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rows2_fwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, b, out, rows, dim, k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F, class... K>
int launch2_bwd(const float* a, const float* b, const float* go, float* ga, float* gb, int64_t rows, int dim, hypad_stream_t s, K... k) {
  const void* ops[] = {a, b, go};
  const int rc = rows_check(rows, dim, ops, 3);
  if (rc || rows == 0 || (!ga && !gb)) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rows2_bwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, b, go, ga, gb, rows, dim, k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F, class... K>
int launch3_fwd(const float* a, const float* b, const float* c, float* out, int64_t rows, int dim, hypad_stream_t s, K... k) {
  const void* ops[] = {a, b, c, out};
  const int rc = rows_check(rows, dim, ops, 4);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rows3_fwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, b, c, out, rows, dim, k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F, class... K>
int launch3_bwd(const float* a, const float* b, const float* c, const float* go, float* ga, float* gb, float* gc, int64_t rows, int dim,
                hypad_stream_t s, K... k) {
  const void* ops[] = {a, b, c, go};
  const int rc = rows_check(rows, dim, ops, 4);
  if (rc || rows == 0 || (!ga && !gb && !gc)) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rows3_bwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, b, c, go, ga, gb, gc, rows, dim,
                     k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
// t_count values of t: one, or one per row (one value even where there are no rows)
template <class F, class... K>
int launcht_fwd(const float* t, const float* x, const float* y, float* out, int64_t rows, int dim, int64_t t_count, hypad_stream_t s, K... k) {
  const void* ops[] = {t, x, y, out};
  const int rc = rows_check(rows, dim, ops, 4);
  if (rc) return rc;
  if (t_count != 1 && t_count != rows) return HYPAD_EINVAL;
  if (!t && t_count > 0) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rowst_fwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, t, x, y, out, rows, dim,
                     (int)(t_count == 1 && rows != 1), k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F, class... K>
int launcht_bwd(const float* t, const float* x, const float* y, const float* go, float* gt, float* gx, float* gy, int64_t rows, int dim,
                int64_t t_count, hypad_stream_t s, K... k) {
  const void* ops[] = {t, x, y, go};
  const int rc = rows_check(rows, dim, ops, 4);
  if (rc) return rc;
  if (t_count != 1 && t_count != rows) return HYPAD_EINVAL;
  if (!t && t_count > 0) return HYPAD_EINVAL;
  if (rows == 0 || (!gt && !gx && !gy)) return HYPAD_OK;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rowst_bwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, t, x, y, go, gt, gx, gy, rows, dim,
                     (int)(t_count == 1 && rows != 1), k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
// r_count values of r, as t_count above
template <class F, class... K>
int launchr_fwd(const float* r, const float* x, float* out, int64_t rows, int dim, int64_t r_count, hypad_stream_t s, K... k) {
  const void* ops[] = {r, x, out};
  const int rc = rows_check(rows, dim, ops, 3);
  if (rc) return rc;
  if (r_count != 1 && r_count != rows) return HYPAD_EINVAL;
  if (!r && r_count > 0) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rowsr_fwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, r, x, out, rows, dim,
                     (int)(r_count == 1 && rows != 1), k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F, class... K>
int launchr_bwd(const float* r, const float* x, const float* go, float* gr, float* gx, int64_t rows, int dim, int64_t r_count, hypad_stream_t s,
                K... k) {
  const void* ops[] = {r, x, go};
  const int rc = rows_check(rows, dim, ops, 3);
  if (rc) return rc;
  if (r_count != 1 && r_count != rows) return HYPAD_EINVAL;
  if (!r && r_count > 0) return HYPAD_EINVAL;
  if (rows == 0 || (!gr && !gx)) return HYPAD_OK;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rowsr_bwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, r, x, go, gr, gx, rows, dim,
                     (int)(r_count == 1 && rows != 1), k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F, class... K>
int launch_scalar_fwd(const Ptrs<F::N> in, float* out, int64_t rows, int dim, hypad_stream_t s, K... k) {
  const void* ops[F::N + 1];
  for (int i = 0; i < F::N; ++i) ops[i] = in.p[i];
  ops[F::N] = out;
  const int rc = rows_check(rows, dim, ops, F::N + 1);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rows_scalar_fwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, in, out, rows, dim, k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F, class... K>
int launch_scalar_bwd(const Ptrs<F::N> in, const float* go, const MutPtrs<F::N> grads, int64_t rows, int dim, hypad_stream_t s, K... k) {
  const void* ops[F::N + 1];
  bool any = false;
  for (int i = 0; i < F::N; ++i) { ops[i] = in.p[i]; any = any || grads.p[i]; }
  ops[F::N] = go;
  const int rc = rows_check(rows, dim, ops, F::N + 1);
  if (rc || rows == 0 || !any) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(rows_scalar_bwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, in, go, grads, rows, dim,
                     k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
// the wider side, dim + 1, is held to the limits
template <class F, class... K>
int launch_proj_fwd(const float* a, float* out, int64_t rows, int dim, hypad_stream_t s, K... k) {
  const void* ops[] = {a, out};
  if (dim <= 0) return HYPAD_EINVAL;
  const int rc = rows_check(rows, dim + 1, ops, 2);
  if (rc || rows == 0) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(proj_fwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, out, rows, dim, k...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <class F, class... K>
int launch_proj_bwd(const float* a, const float* go, float* ga, int64_t rows, int dim, hypad_stream_t s, K... k) {
  const void* ops[] = {a, go};
  if (dim <= 0) return HYPAD_EINVAL;
  const int rc = rows_check(rows, dim + 1, ops, 2);
  if (rc || rows == 0 || !ga) return rc;
  hipLaunchKernelGGL(HIP_KERNEL_NAME(proj_bwd<F, K...>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, a, go, ga, rows, dim, k...);
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

// The same functions at k = -c (docs/history/curvature.md): the k = -1 argument list plus c, finite and positive (else HYPAD_EINVAL, before
// any other check).  c = 1 gives the bits of the entry point above.
int hypad_ball_expmap_fwd(const float* x, const float* u, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_fwd<Expmap>(x, u, out, rows, dim, s, Curved(c));
}
int hypad_ball_expmap_bwd(const float* x, const float* u, const float* grad_out, float* grad_x, float* grad_u, int64_t rows, int dim,
                          double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_bwd<Expmap>(x, u, grad_out, grad_x, grad_u, rows, dim, s, Curved(c));
}
int hypad_ball_logmap_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_fwd<Logmap>(x, y, out, rows, dim, s, Curved(c));
}
int hypad_ball_logmap_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                          double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_bwd<Logmap>(x, y, grad_out, grad_x, grad_y, rows, dim, s, Curved(c));
}
int hypad_ball_geodesic_fwd(const float* t, const float* x, const float* y, float* out, int64_t rows, int dim, int64_t t_count,
                            double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launcht_fwd<Geodesic>(t, x, y, out, rows, dim, t_count, s, Curved(c));
}
int hypad_ball_geodesic_bwd(const float* t, const float* x, const float* y, const float* grad_out, float* grad_t, float* grad_x, float* grad_y,
                            int64_t rows, int dim, int64_t t_count, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launcht_bwd<Geodesic>(t, x, y, grad_out, grad_t, grad_x, grad_y, rows, dim, t_count, s, Curved(c));
}
int hypad_ball_gyration_fwd(const float* a, const float* b, const float* u, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch3_fwd<Gyration>(a, b, u, out, rows, dim, s, Curved(c));
}
int hypad_ball_gyration_bwd(const float* a, const float* b, const float* u, const float* grad_out, float* grad_a, float* grad_b, float* grad_u,
                            int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch3_bwd<Gyration>(a, b, u, grad_out, grad_a, grad_b, grad_u, rows, dim, s, Curved(c));
}
int hypad_ball_parallel_transport_fwd(const float* x, const float* y, const float* v, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch3_fwd<Transport>(x, y, v, out, rows, dim, s, Curved(c));
}
int hypad_ball_parallel_transport_bwd(const float* x, const float* y, const float* v, const float* grad_out, float* grad_x, float* grad_y, float* grad_v,
                                      int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch3_bwd<Transport>(x, y, v, grad_out, grad_x, grad_y, grad_v, rows, dim, s, Curved(c));
}
int hypad_ball_parallel_transport0_fwd(const float* y, const float* v, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_fwd<Transport0<false>>(y, v, out, rows, dim, s, Curved(c));
}
int hypad_ball_parallel_transport0_bwd(const float* y, const float* v, const float* grad_out, float* grad_y, float* grad_v, int64_t rows, int dim,
                                  double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_bwd<Transport0<false>>(y, v, grad_out, grad_y, grad_v, rows, dim, s, Curved(c));
}
int hypad_ball_parallel_transport0back_fwd(const float* x, const float* v, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_fwd<Transport0<true>>(x, v, out, rows, dim, s, Curved(c));
}
int hypad_ball_parallel_transport0back_bwd(const float* x, const float* v, const float* grad_out, float* grad_x, float* grad_v, int64_t rows, int dim,
                                      double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_bwd<Transport0<true>>(x, v, grad_out, grad_x, grad_v, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_sub_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_fwd<MobiusSub>(x, y, out, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_sub_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                              double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_bwd<MobiusSub>(x, y, grad_out, grad_x, grad_y, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_coadd_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_fwd<MobiusCoadd<false>>(x, y, out, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_coadd_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                           double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_bwd<MobiusCoadd<false>>(x, y, grad_out, grad_x, grad_y, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_cosub_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_fwd<MobiusCoadd<true>>(x, y, out, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_cosub_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                           double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_bwd<MobiusCoadd<true>>(x, y, grad_out, grad_x, grad_y, rows, dim, s, Curved(c));
}
int hypad_ball_geodesic_unit_fwd(const float* t, const float* x, const float* u, float* out, int64_t rows, int dim, int64_t t_count,
                                 double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launcht_fwd<GeodesicUnit>(t, x, u, out, rows, dim, t_count, s, Curved(c));
}
int hypad_ball_geodesic_unit_bwd(const float* t, const float* x, const float* u, const float* grad_out, float* grad_t, float* grad_x, float* grad_u,
                                 int64_t rows, int dim, int64_t t_count, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launcht_bwd<GeodesicUnit>(t, x, u, grad_out, grad_t, grad_x, grad_u, rows, dim, t_count, s, Curved(c));
}
int hypad_ball_lambda_x_fwd(const float* x, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_scalar_fwd<LambdaX>({{x}}, out, rows, dim, s, Curved(c));
}
int hypad_ball_lambda_x_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_scalar_bwd<LambdaX>({{x}}, grad_out, {{grad_x}}, rows, dim, s, Curved(c));
}
int hypad_ball_inner_fwd(const float* x, const float* u, const float* v, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_scalar_fwd<Inner>({{x, u, v}}, out, rows, dim, s, Curved(c));
}
int hypad_ball_inner_bwd(const float* x, const float* u, const float* v, const float* grad_out, float* grad_x, float* grad_u, float* grad_v,
                         int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_scalar_bwd<Inner>({{x, u, v}}, grad_out, {{grad_x, grad_u, grad_v}}, rows, dim, s, Curved(c));
}
int hypad_ball_norm_fwd(const float* x, const float* u, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_scalar_fwd<TangentNorm>({{x, u}}, out, rows, dim, s, Curved(c));
}
int hypad_ball_norm_bwd(const float* x, const float* u, const float* grad_out, float* grad_x, float* grad_u, int64_t rows, int dim,
                        double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_scalar_bwd<TangentNorm>({{x, u}}, grad_out, {{grad_x, grad_u}}, rows, dim, s, Curved(c));
}
int hypad_ball_egrad2rgrad_fwd(const float* x, const float* grad, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_fwd<Egrad2Rgrad>(x, grad, out, rows, dim, s, Curved(c));
}
int hypad_ball_egrad2rgrad_bwd(const float* x, const float* grad, const float* grad_out, float* grad_x, float* grad_grad, int64_t rows, int dim,
                          double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_bwd<Egrad2Rgrad>(x, grad, grad_out, grad_x, grad_grad, rows, dim, s, Curved(c));
}
int hypad_ball_sproj_fwd(const float* h, float* out, int64_t rows, int dim,
                         double c, hypad_stream_t s) { return bad_c(c) ? HYPAD_EINVAL : launch_proj_fwd<Sproj>(h, out, rows, dim, s, Curved(c)); }
int hypad_ball_sproj_bwd(const float* h, const float* grad_out, float* grad_h, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_proj_bwd<Sproj>(h, grad_out, grad_h, rows, dim, s, Curved(c));
}
int hypad_ball_inv_sproj_fwd(const float* x, float* out, int64_t rows, int dim,
                             double c, hypad_stream_t s) { return bad_c(c) ? HYPAD_EINVAL : launch_proj_fwd<InvSproj>(x, out, rows, dim, s, Curved(c)); }
int hypad_ball_inv_sproj_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_proj_bwd<InvSproj>(x, grad_out, grad_x, rows, dim, s, Curved(c));
}
// The row functions whose k = -1 kernels are the first-generation ones of ops_hyper.hip and dist.hip, here in the launch form of this
// file and without their one-row broadcast (the caller expands): every row operand is (rows, dim); r holds r_rows values, 1 or one per row.
int hypad_ball_project_fwd(const float* x, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch1_fwd<Project>(x, out, rows, dim, s, Curved(c));
}
int hypad_ball_project_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch1_bwd<Project>(x, grad_out, grad_x, rows, dim, s, Curved(c));
}
int hypad_ball_expmap0_fwd(const float* u, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch1_fwd<RadialMap<true>>(u, out, rows, dim, s, Curved(c));
}
int hypad_ball_expmap0_bwd(const float* u, const float* grad_out, float* grad_u, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch1_bwd<RadialMap<true>>(u, grad_out, grad_u, rows, dim, s, Curved(c));
}
int hypad_ball_logmap0_fwd(const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch1_fwd<RadialMap<false>>(y, out, rows, dim, s, Curved(c));
}
int hypad_ball_logmap0_bwd(const float* y, const float* grad_out, float* grad_y, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch1_bwd<RadialMap<false>>(y, grad_out, grad_y, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_add_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_fwd<MobiusAdd>(x, y, out, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_add_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, double c,
                              hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_bwd<MobiusAdd>(x, y, grad_out, grad_x, grad_y, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_pointwise_mul_fwd(const float* w, const float* x, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_fwd<MobiusPointwiseMul>(w, x, out, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_pointwise_mul_bwd(const float* w, const float* x, const float* grad_out, float* grad_w, float* grad_x, int64_t rows, int dim,
                                        double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch2_bwd<MobiusPointwiseMul>(w, x, grad_out, grad_w, grad_x, rows, dim, s, Curved(c));
}
int hypad_ball_mobius_scalar_mul_fwd(const float* r, const float* x, float* out, int64_t rows, int dim, int64_t r_rows, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launchr_fwd<MobiusScalarMul>(r, x, out, rows, dim, r_rows, s, Curved(c));
}
int hypad_ball_mobius_scalar_mul_bwd(const float* r, const float* x, const float* grad_out, float* grad_r, float* grad_x, int64_t rows, int dim,
                                     int64_t r_rows, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launchr_bwd<MobiusScalarMul>(r, x, grad_out, grad_r, grad_x, rows, dim, r_rows, s, Curved(c));
}
int hypad_ball_dist_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_scalar_fwd<Dist>({{x, y}}, out, rows, dim, s, Curved(c));
}
int hypad_ball_dist_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, double c,
                        hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_scalar_bwd<Dist>({{x, y}}, grad_out, {{grad_x, grad_y}}, rows, dim, s, Curved(c));
}
int hypad_ball_dist0_fwd(const float* x, float* out, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_scalar_fwd<Dist0>({{x}}, out, rows, dim, s, Curved(c));
}
int hypad_ball_dist0_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, double c, hypad_stream_t s) {
  return bad_c(c) ? HYPAD_EINVAL : launch_scalar_bwd<Dist0>({{x}}, grad_out, {{grad_x}}, rows, dim, s, Curved(c));
}

}  // extern "C"
