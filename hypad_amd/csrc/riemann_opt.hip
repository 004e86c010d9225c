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
#include "riemann_rules.h"

using namespace hypad;
using namespace hypad::riemann;

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_D = 64 * MAX_EPL;
constexpr int64_t INT_LIMIT = 0x7fffffff;

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
