// Row-wise Riemannian optimiser steps: geoopt.optim.RiemannianAdam and RiemannianSGD (geoopt 0.5.0, restated: docs/history/riemannian_rows.md)
// for a parameter whose rows are points of the Poincare ball at k = -1 or unit vectors, and SGD's rule on plain rows.  The parameter,
// its gradient and every state tensor are (rows, dim) fp32, dim <= 256.
//
// One kernel body for manifold x rule in the launch form of tangent.hip: a wave per row, the row in fp64 registers (RowD<64, 4>, scalar
// loads: any storage offset gives the same bits), sums by rowd_dot, a grid-stride walk under wave_grid.  A launch loads the rows of x, g
// and the state, does the whole rule -- weight decay, Riemannian gradient, moments, retraction, transport of the first moment or the
// momentum buffer, stabilisation -- and stores x and the state in place.  No atomics, no workspace, no LDS: a row's bits do not depend on
// the rows around it.  The ball's maps are rowops.h's *_d functions of the tangent kernels; the sphere's are sphere_proju_d / sphere_projx_d.
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

// A manifold: rgrad, the Riemannian gradient of the Euclidean one; inner, the number the second moment takes for it; retr, the step from
// x along u; transp, a tangent vector of x carried to y; stabilise, the point put back on the manifold and the vector on its tangent space
struct Ball {
  static __device__ __forceinline__ RW rgrad(const RW& x, const RW& g) { return egrad2rgrad_d(x, g); }
  static __device__ __forceinline__ double inner(const RW& x, const RW& r) { return inner_d(x, r, r); }
  static __device__ __forceinline__ RW retr(const RW& x, const RW& u) {
    RW y;
#pragma unroll
    for (int e = 0; e < RW::EPL; ++e) y.v[e] = x.v[e] + u.v[e];
    return project_d(y);
  }
  static __device__ __forceinline__ RW transp(const RW& x, const RW& y, const RW& w) { return parallel_transport_d(x, y, w); }
  static __device__ __forceinline__ void stabilise(RW& x, RW&) { x = project_d(x); }
};
struct SphereM {
  static __device__ __forceinline__ RW rgrad(const RW& x, const RW& g) { return sphere_proju_d(x, g); }
  static __device__ __forceinline__ double inner(const RW&, const RW& r) { return rowd_dot(r, r); }
  static __device__ __forceinline__ RW retr(const RW& x, const RW& u) {
    RW y;
#pragma unroll
    for (int e = 0; e < RW::EPL; ++e) y.v[e] = x.v[e] + u.v[e];
    return sphere_projx_d(y);
  }
  static __device__ __forceinline__ RW transp(const RW&, const RW& y, const RW& w) { return sphere_proju_d(y, w); }
  static __device__ __forceinline__ void stabilise(RW& x, RW& w) { x = sphere_projx_d(x); w = sphere_proju_d(x, w); }
};
struct Euclid {                                         // RiemannianSGD on an untagged parameter: the identity maps
  static __device__ __forceinline__ RW rgrad(const RW&, const RW& g) { return g; }
  static __device__ __forceinline__ RW retr(const RW& x, const RW& u) {
    RW y;
#pragma unroll
    for (int e = 0; e < RW::EPL; ++e) y.v[e] = x.v[e] + u.v[e];
    return y;
  }
  static __device__ __forceinline__ RW transp(const RW&, const RW&, const RW& w) { return w; }
  static __device__ __forceinline__ void stabilise(RW&, RW&) {}
};

// A rule: the hyper-parameters of a launch as the entry point got them, the number of state rows it keeps, and the step of one row.  x
// and the state rows st[] are updated in place; g comes in with the weight decay added; st[0] is the tangent vector the step carries along.
struct AdamRule {
  static constexpr int STATES = 2;                      // st[0] exp_avg, st[1] exp_avg_sq
  float lr, b1, b2, eps, wd;
  int step, stabilize;
  struct Coef { double lr, b1, b2, eps, bc1, bc2; };
  // the bias corrections in fp64 from the step number, as train::adam_coef takes them
  __device__ __forceinline__ Coef coef() const {
    return {(double)lr, (double)b1, (double)b2, (double)eps, 1.0 - pow((double)b1, (double)step), 1.0 - pow((double)b2, (double)step)};
  }
  template <class M>
  static __device__ __forceinline__ void row(const Coef& c, RW& x, const RW& g, RW* st, bool) {
    RW &m = st[0], &v = st[1];
    const RW r = M::rgrad(x, g);
    // the second moment takes ONE number per row, kept once per element (geoopt's zeros_like(p) state): every element goes through the
    // same explicit fma, so a row that came in as one value repeated leaves as one value repeated (train_common.h, radam_ball_wave's vin)
    const double vin = (1.0 - c.b2) * M::inner(x, r);
    RW u;
#pragma unroll
    for (int e = 0; e < RW::EPL; ++e) {
      m.v[e] = c.b1 * m.v[e] + (1.0 - c.b1) * r.v[e];
      v.v[e] = fma(c.b2, v.v[e], vin);
      u.v[e] = -c.lr * ((m.v[e] / c.bc1) / (sqrt(v.v[e] / c.bc2) + c.eps));
    }
    const RW y = M::retr(x, u);
    m = M::transp(x, y, m);
    x = y;
  }
};
struct SgdRule {
  static constexpr int STATES = 1;                      // st[0] momentum_buffer, absent where momentum == 0
  float lr, momentum, dampening, wd;
  int nesterov, step, stabilize;
  struct Coef { double lr, mu, keep; bool nesterov; };
  __device__ __forceinline__ Coef coef() const { return {(double)lr, (double)momentum, 1.0 - (double)dampening, nesterov != 0}; }
  template <class M>
  static __device__ __forceinline__ void row(const Coef& c, RW& x, const RW& g, RW* st, bool has_buf) {
    RW& b = st[0];
    const RW r = M::rgrad(x, g);
    RW u;
#pragma unroll
    for (int e = 0; e < RW::EPL; ++e) {
      if (has_buf) {
        b.v[e] = c.mu * b.v[e] + c.keep * r.v[e];
        u.v[e] = -c.lr * (c.nesterov ? r.v[e] + c.mu * b.v[e] : b.v[e]);
      } else {
        u.v[e] = -c.lr * r.v[e];
      }
    }
    const RW y = M::retr(x, u);
    if (has_buf) b = M::transp(x, y, b);
    x = y;
  }
};

// s0, s1: the rule's state tensors (Adam: exp_avg, exp_avg_sq; SGD: the momentum buffer or NULL, and NULL)
template <class M, class R>
__global__ __launch_bounds__(THREADS) void riemann_rows_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                               float* __restrict__ s1, int64_t rows, int dim, const R h) {
  const int lane = threadIdx.x & 63;
  const typename R::Coef c = h.coef();
  const bool stab = h.stabilize > 0 && h.step % h.stabilize == 0;
  for (int64_t r = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * WAVES) {
    RW x = rowd_load<RW>(p + r * dim, dim, lane), gr = rowd_load<RW>(g + r * dim, dim, lane), st[R::STATES] = {};
    if (s0) st[0] = rowd_load<RW>(s0 + r * dim, dim, lane);
    if (R::STATES == 2) st[R::STATES - 1] = rowd_load<RW>(s1 + r * dim, dim, lane);
#pragma unroll
    for (int e = 0; e < RW::EPL; ++e) gr.v[e] += (double)h.wd * x.v[e];
    R::template row<M>(c, x, gr, st, s0 != nullptr);
    if (stab) M::stabilise(x, st[0]);
    rowd_store(p + r * dim, x, dim, lane);
    if (s0) rowd_store(s0 + r * dim, st[0], dim, lane);
    if (R::STATES == 2) rowd_store(s1 + r * dim, st[R::STATES - 1], dim, lane);
  }
}

inline int wave_grid(int64_t rows) {
  const int64_t b = (rows + WAVES - 1) / WAVES;
  return (int)(b > 4096 ? 4096 : b < 1 ? 1 : b);
}
// sizes, step and manifold first, then the limits, then the operands: each of `n` pointers may be NULL only where there are no rows
inline int step_check(int64_t rows, int dim, int step, bool manifold_known, const void* const* ops, int n) {
  if (rows < 0 || dim <= 0 || step < 1 || !manifold_known) return HYPAD_EINVAL;
  if (dim > MAX_D || rows > INT_LIMIT / dim) return HYPAD_EUNSUPPORTED;
  for (int i = 0; i < n; ++i)
    if (!ops[i] && rows > 0) return HYPAD_EINVAL;
  return HYPAD_OK;
}

template <class M, class R>
void launch(float* p, const float* g, float* s0, float* s1, int64_t rows, int dim, const R& h, hypad_stream_t s) {
  hipLaunchKernelGGL((riemann_rows_kernel<M, R>), dim3(wave_grid(rows)), dim3(THREADS), 0, (hipStream_t)s, p, g, s0, s1, rows, dim, h);
}

}  // namespace

extern "C" {

int hypad_radam_rows_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t rows, int dim, int manifold, int step, float lr,
                          float b1, float b2, float eps, float wd, int stabilize, hypad_stream_t s) {
  const void* ops[] = {p, g, exp_avg, exp_avg_sq};
  const int rc = step_check(rows, dim, step, manifold == HYPAD_MANIFOLD_BALL || manifold == HYPAD_MANIFOLD_SPHERE, ops, 4);
  if (rc || rows == 0) return rc;
  const AdamRule h = {lr, b1, b2, eps, wd, step, stabilize};
  if (manifold == HYPAD_MANIFOLD_BALL) launch<Ball>(p, g, exp_avg, exp_avg_sq, rows, dim, h, s);
  else launch<SphereM>(p, g, exp_avg, exp_avg_sq, rows, dim, h, s);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad_rsgd_rows_step(float* p, const float* g, float* momentum_buf, int64_t rows, int dim, int manifold, int step, float lr, float momentum,
                         float dampening, float wd, int nesterov, int stabilize, hypad_stream_t s) {
  const void* ops[] = {p, g};
  const bool known = manifold == HYPAD_MANIFOLD_EUCLIDEAN || manifold == HYPAD_MANIFOLD_BALL || manifold == HYPAD_MANIFOLD_SPHERE;
  const int rc = step_check(rows, dim, step, known, ops, 2);
  if (rc) return rc;
  if ((momentum_buf != nullptr) != (momentum != 0.f)) return HYPAD_EINVAL;       // a buffer exactly where the rule has momentum
  if (rows == 0) return HYPAD_OK;
  const SgdRule h = {lr, momentum, dampening, wd, nesterov, step, stabilize};
  if (manifold == HYPAD_MANIFOLD_BALL) launch<Ball>(p, g, momentum_buf, nullptr, rows, dim, h, s);
  else if (manifold == HYPAD_MANIFOLD_SPHERE) launch<SphereM>(p, g, momentum_buf, nullptr, rows, dim, h, s);
  else launch<Euclid>(p, g, momentum_buf, nullptr, rows, dim, h, s);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

}  // extern "C"
