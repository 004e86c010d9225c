// The manifolds and rules of the row-wise optimiser steps, shared by riemann_opt.hip (one parameter per launch) and optim_group.hip (a
// group of parameters per launch): both inline the same row functions, so a row takes the same arithmetic in either kernel.  A row is
// RowD<64, MAX_EPL>: a wave per row in fp64 registers; the ball's maps are rowops.h's *_d functions, the sphere's sphere_proju_d /
// sphere_projx_d.
#pragma once
#include "rowops.h"

namespace hypad {
namespace riemann {

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

}  // namespace riemann
}  // namespace hypad
