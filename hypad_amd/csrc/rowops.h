// Row-wise Poincare-ball math (k = -1).  A row of `dim` <= 256 floats lives in the registers of a group of G lanes,
// EPL elements per lane at columns (lane mod G) + G*e; reductions are DPP butterflies.  Two layouts:
//   RowVec   = RowT<64, 4>: one row per wave -- the fused training kernels, whose rows sit in LDS tiles;
//   RowT<16, EPL>         : four rows per wave, one per DPP row of 16 lanes -- the stand-alone HBM-bound kernels: every
//                           per-row scalar (norm, tanh, artanh, acosh, divisions) is then computed for four rows by one
//                           instruction, and a row sum needs no cross-row step at all.
// Formulas and clamp constants: /root/reference/math_.py (see oracle/gmath.py, oracle/manual.py which these
// transcribe line by line).
#pragma once
#include <cmath>
#include <type_traits>

#include "device_utils.h"

namespace hypad {

constexpr int MAX_EPL = 4;  // dim <= 256 at 64 lanes per row

template <int G_, int EPL_>
struct RowT {
  static constexpr int G = G_, EPL = EPL_;
  float v[EPL_];
};
using RowVec = RowT<64, MAX_EPL>;

template <class R = RowVec>
__device__ __forceinline__ R row_load(const float* p, int dim, int lane) {
  R r;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) {
    int c = (lane & (R::G - 1)) + R::G * e;
    r.v[e] = c < dim ? p[c] : 0.f;
  }
  return r;
}
template <class R>
__device__ __forceinline__ void row_store(float* p, const R& r, int dim, int lane) {
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) {
    int c = (lane & (R::G - 1)) + R::G * e;
    if (c < dim) p[c] = r.v[e];
  }
}
template <class R>
__device__ __forceinline__ float row_dot(const R& a, const R& b) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) s += a.v[e] * b.v[e];
  return R::G == 64 ? wave_sum(s) : row16_sum(s);
}

// ---- expmap0 (math_.py:1132-1136)
template <class R>
__device__ __forceinline__ R expmap0_row(const R& u) {
  float n = fmaxf(sqrtf(row_dot(u, u)), MIN_NORM);
  float f = tanhf(fminf(n, TANH_CLAMP)) / n;
  R p;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) p.v[e] = f * u.v[e];
  return p;
}
template <class R>
__device__ __forceinline__ R expmap0_row_bwd(const R& u, const R& dp) {
  float raw = sqrtf(row_dot(u, u));
  float n = fmaxf(raw, MIN_NORM);
  float t = tanhf(fminf(n, TANH_CLAMP));
  float f = t / n;
  float tp = n <= TANH_CLAMP ? 1.f - t * t : 0.f;
  float dfdn = (tp * n - t) / (n * n);
  float s = raw >= MIN_NORM ? row_dot(dp, u) * dfdn / n : 0.f;
  R du;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) du.v[e] = f * dp.v[e] + s * u.v[e];
  return du;
}

// ---- logmap0 (math_.py:1267-1270)
__device__ __forceinline__ float artanh_clamped(float x) {
  x = fminf(fmaxf(x, -1.f + ARTANH_EPS), 1.f - ARTANH_EPS);
  return 0.5f * (logf(1.f + x) - logf(1.f - x));
}
template <class R>
__device__ __forceinline__ R logmap0_row(const R& y) {
  float n = fmaxf(sqrtf(row_dot(y, y)), MIN_NORM);
  float f = artanh_clamped(n) / n;
  R o;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) o.v[e] = f * y.v[e];
  return o;
}
template <class R>
__device__ __forceinline__ R logmap0_row_bwd(const R& y, const R& go) {
  float raw = sqrtf(row_dot(y, y));
  float n = fmaxf(raw, MIN_NORM);
  float a = artanh_clamped(n);
  float f = a / n;
  // d artanh(clamp(n)) / dn: 1/(1-n^2) inside the clamp, 0 outside
  float ap = (n >= -1.f + ARTANH_EPS && n <= 1.f - ARTANH_EPS) ? 1.f / (1.f - n * n) : 0.f;
  float dfdn = (ap * n - a) / (n * n);
  float s = raw >= MIN_NORM ? row_dot(go, y) * dfdn / n : 0.f;
  R gy;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) gy.v[e] = f * go.v[e] + s * y.v[e];
  return gy;
}

// ---- mobius_add (math_.py:536-555)
template <class R>
__device__ __forceinline__ R mobius_add_row(const R& x, const R& y) {
  float x2 = row_dot(x, x), y2 = row_dot(y, y), xy = row_dot(x, y);
  float A = 1.f + 2.f * xy + y2, Bc = 1.f - x2;
  float D = fmaxf(1.f + 2.f * xy + x2 * y2, MIN_NORM);
  const float rD = 1.f / D;              // one division per row; an IEEE division per element is ~12 instructions each
  R m;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) m.v[e] = (A * x.v[e] + Bc * y.v[e]) * rD;
  return m;
}
template <class R>
__device__ __forceinline__ void mobius_add_row_bwd(const R& x, const R& y, const R& dm, R& dx, R& dy) {
  float x2 = row_dot(x, x), y2 = row_dot(y, y), xy = row_dot(x, y);
  float A = 1.f + 2.f * xy + y2, Bc = 1.f - x2;
  float Draw = 1.f + 2.f * xy + x2 * y2;
  float D = fmaxf(Draw, MIN_NORM);
  const float rD = 1.f / D;
  R m, dN;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) {
    m.v[e] = (A * x.v[e] + Bc * y.v[e]) * rD;
    dN.v[e] = dm.v[e] * rD;
  }
  float dD = Draw >= MIN_NORM ? -row_dot(dm, m) * rD : 0.f;
  float dA = row_dot(dN, x), dBc = row_dot(dN, y);
  float dxy = 2.f * dA + 2.f * dD, dx2 = -dBc + y2 * dD, dy2 = dA + x2 * dD;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) {
    dx.v[e] = A * dN.v[e] + 2.f * dx2 * x.v[e] + dxy * y.v[e];
    dy.v[e] = Bc * dN.v[e] + 2.f * dy2 * y.v[e] + dxy * x.v[e];
  }
}

// ---- project (math_.py:340-352)
template <class R>
__device__ __forceinline__ R project_row(const R& x) {
  float n = fmaxf(sqrtf(row_dot(x, x)), MIN_NORM);
  R o = x;
  if (n > BALL_MAXNORM) {
    const float sc = BALL_MAXNORM / n;
#pragma unroll
    for (int e = 0; e < R::EPL; ++e) o.v[e] = x.v[e] * sc;
  }
  return o;
}
template <class R>
__device__ __forceinline__ R project_row_bwd(const R& x, const R& go) {
  float raw = sqrtf(row_dot(x, x));
  float n = fmaxf(raw, MIN_NORM);
  if (!(n > BALL_MAXNORM)) return go;
  float s = raw >= MIN_NORM ? row_dot(x, go) / (n * n) : 0.f;
  R gx;
  const float sc = BALL_MAXNORM / n;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) gx.v[e] = sc * (go.v[e] - x.v[e] * s);
  return gx;
}

// ---- fused Moebius head epilogue (hyrnn_nets.py:27-34)
template <class R>
__device__ __forceinline__ R head_row(const R& u, const R& bias) {
  return project_row(mobius_add_row(expmap0_row(u), bias));
}
template <class R>
__device__ __forceinline__ void head_row_bwd(const R& u, const R& bias, const R& dr, R& du, R& db) {
  R p = expmap0_row(u);
  R m = mobius_add_row(p, bias);
  R dm = project_row_bwd(m, dr);
  R dp;
  mobius_add_row_bwd(p, bias, dm, dp, db);
  du = expmap0_row_bwd(u, dp);
}

// ---- mobius_linear in any configuration (hyrnn_nets.py:13-58): the row chain after mx = x W^T, carried in fp64 registers.
// Why fp64: the matvec scaling leaves a row at norm tanh(|mx| / |x| artanh |x|) -- 1 - 1e-5 for an input a layer before this one
// projected to the rim -- and whatever follows (logmap0 of the non-linearity, the Moebius add) takes 1 - norm from that row again.
// In fp32 the last bit of the row's sum of squares decides three digits of 1 - norm: out moves by 1e-5 and grad_x by 1e-3 of its
// size with nothing but the order of a sum (docs/history/mobius_modes.md).  The chain lives in registers from the load of mx to
// the store of the result, so carrying it in fp64 costs no memory traffic; mx, the bias, the results and every buffer stay fp32.
// Same formulas and clamps as the fp32 row functions above (MIN_NORM under a norm, TANH_CLAMP, 1 - ARTANH_EPS, BALL_MAXNORM);
// on a clamp nothing flows back through the clamped quantity, as autograd gives the reference.
template <int G_, int EPL_>
struct RowD {
  static constexpr int G = G_, EPL = EPL_;
  double v[EPL_];
};
#define HYPAD_ROW_EACH for (int e = 0; e < R::EPL; ++e)
template <class R>
__device__ __forceinline__ R rowd_load(const float* p, int dim, int lane) {
  R r;
#pragma unroll
  HYPAD_ROW_EACH { int c = (lane & (R::G - 1)) + R::G * e; r.v[e] = c < dim ? (double)p[c] : 0.0; }
  return r;
}
template <class R>
__device__ __forceinline__ void rowd_store(float* p, const R& r, int dim, int lane) {
#pragma unroll
  HYPAD_ROW_EACH { int c = (lane & (R::G - 1)) + R::G * e; if (c < dim) p[c] = (float)r.v[e]; }
}
template <int G>
__device__ __forceinline__ double groupd_sum(double s) {
#pragma unroll
  for (int off = G >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, WAVE);
  return s;
}
template <class R>
__device__ __forceinline__ double rowd_dot(const R& a, const R& b) {
  double s = 0.0;
#pragma unroll
  HYPAD_ROW_EACH s += a.v[e] * b.v[e];
  return groupd_sum<R::G>(s);
}
__device__ __forceinline__ double tanh_clamped_d(double x) { return tanh(fmin(x, (double)TANH_CLAMP)); }
__device__ __forceinline__ double tanh_prime_d(double x, double t) { return x <= (double)TANH_CLAMP ? 1.0 - t * t : 0.0; }
constexpr double ARTANH_TOP = 1.0 - 1e-7;                       // math_.py:58
__device__ __forceinline__ double artanh_clamped_d(double x) { x = fmin(x, ARTANH_TOP); return 0.5 * (log1p(x) - log1p(-x)); }
__device__ __forceinline__ double artanh_prime_d(double x) { return x <= ARTANH_TOP ? 1.0 / ((1.0 - x) * (1.0 + x)) : 0.0; }

// y = f(|u|) u with f(n) = g(n) / n: expmap0 (g = tanh) and logmap0 (g = artanh) and their common backward
template <bool EXP, class R>
__device__ __forceinline__ R radial_map_d(const R& u) {
  const double n = fmax(sqrt(rowd_dot(u, u)), (double)MIN_NORM);
  const double f = (EXP ? tanh_clamped_d(n) : artanh_clamped_d(n)) / n;
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = f * u.v[e];
  return o;
}
template <bool EXP, class R>
__device__ __forceinline__ R radial_map_bwd_d(const R& u, const R& go) {
  const double raw = sqrt(rowd_dot(u, u));
  const double n = fmax(raw, (double)MIN_NORM);
  const double g = EXP ? tanh_clamped_d(n) : artanh_clamped_d(n);
  const double gp = EXP ? tanh_prime_d(n, g) : artanh_prime_d(n);
  const double f = g / n, dfdn = (gp * n - g) / (n * n);
  const double s = raw >= (double)MIN_NORM ? rowd_dot(go, u) * dfdn / n : 0.0;
  R du;
#pragma unroll
  HYPAD_ROW_EACH du.v[e] = f * go.v[e] + s * u.v[e];
  return du;
}
// mobius_add (math_.py:536-555)
template <class R>
__device__ __forceinline__ R mobius_add_d(const R& x, const R& y) {
  const double x2 = rowd_dot(x, x), y2 = rowd_dot(y, y), xy = rowd_dot(x, y);
  const double A = 1.0 + 2.0 * xy + y2, Bc = 1.0 - x2, rD = 1.0 / fmax(1.0 + 2.0 * xy + x2 * y2, (double)MIN_NORM);
  R m;
#pragma unroll
  HYPAD_ROW_EACH m.v[e] = (A * x.v[e] + Bc * y.v[e]) * rD;
  return m;
}
template <class R>
__device__ __forceinline__ void mobius_add_bwd_d(const R& x, const R& y, const R& dm, R& dx, R& dy) {
  const double x2 = rowd_dot(x, x), y2 = rowd_dot(y, y), xy = rowd_dot(x, y);
  const double A = 1.0 + 2.0 * xy + y2, Bc = 1.0 - x2, Draw = 1.0 + 2.0 * xy + x2 * y2;
  const double rD = 1.0 / fmax(Draw, (double)MIN_NORM);
  R m, dN;
#pragma unroll
  HYPAD_ROW_EACH { m.v[e] = (A * x.v[e] + Bc * y.v[e]) * rD; dN.v[e] = dm.v[e] * rD; }
  const double dD = Draw >= (double)MIN_NORM ? -rowd_dot(dm, m) * rD : 0.0;
  const double dA = rowd_dot(dN, x), dBc = rowd_dot(dN, y);
  const double dxy = 2.0 * dA + 2.0 * dD, dx2 = -dBc + y2 * dD, dy2 = dA + x2 * dD;
#pragma unroll
  HYPAD_ROW_EACH {
    dx.v[e] = A * dN.v[e] + 2.0 * dx2 * x.v[e] + dxy * y.v[e];
    dy.v[e] = Bc * dN.v[e] + 2.0 * dy2 * y.v[e] + dxy * x.v[e];
  }
}
// project (math_.py:340-352), the fp32 eps
template <class R>
__device__ __forceinline__ R project_d(const R& x) {
  const double n = fmax(sqrt(rowd_dot(x, x)), (double)MIN_NORM);
  R o = x;
  if (n > (double)BALL_MAXNORM) {
    const double sc = (double)BALL_MAXNORM / n;
#pragma unroll
    HYPAD_ROW_EACH o.v[e] = x.v[e] * sc;
  }
  return o;
}
template <class R>
__device__ __forceinline__ R project_bwd_d(const R& x, const R& go) {
  const double raw = sqrt(rowd_dot(x, x));
  const double n = fmax(raw, (double)MIN_NORM);
  if (!(n > (double)BALL_MAXNORM)) return go;
  const double s = raw >= (double)MIN_NORM ? rowd_dot(x, go) / (n * n) : 0.0, sc = (double)BALL_MAXNORM / n;
  R gx;
#pragma unroll
  HYPAD_ROW_EACH gx.v[e] = sc * (go.v[e] - x.v[e] * s);
  return gx;
}

// Moebius matrix-vector product, the part after mx = x W^T (hyrnn_nets.py:42-58; math_.py:1308-1323): tanh(|mx| / |x| artanh |x|)
// mx / |mx|.  xraw = |x| of the row the product came from, before its clamp.  A row of mx that is exactly zero gives the zero row
// (the reference's `cond`) and gets zero gradients.
template <class R>
__device__ __forceinline__ bool rowd_all_zero(const R& a) {
  double nz = 0.0;
#pragma unroll
  HYPAD_ROW_EACH nz += a.v[e] != 0.0 ? 1.0 : 0.0;
  return groupd_sum<R::G>(nz) == 0.0;
}
// The scaling the matvec and the point-wise product share: tanh(|m| / |x| artanh |x|) m / |m|; `zero` = the reference's `cond`.
template <class R>
__device__ __forceinline__ R mobius_scaled_row(const R& mx, double xraw, bool zero) {
  const double xn = fmax(xraw, (double)MIN_NORM);
  const double mn = fmax(sqrt(rowd_dot(mx, mx)), (double)MIN_NORM);
  const double s = zero ? 0.0 : tanh_clamped_d(mn / xn * artanh_clamped_d(xn)) / mn;
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = s * mx.v[e];
  return o;
}
// d mx and (returned) dL/d|x|
template <class R>
__device__ __forceinline__ double mobius_scaled_row_bwd(const R& mx, double xraw, bool cond, const R& go, R& dmx) {
  const double xn = fmax(xraw, (double)MIN_NORM);
  const double mraw = sqrt(rowd_dot(mx, mx));
  const double mn = fmax(mraw, (double)MIN_NORM);
  const double a = artanh_clamped_d(xn), q = a / xn, arg = mn / xn * a;
  const double t = tanh_clamped_d(arg), tp = tanh_prime_d(arg, t);
  const double s = cond ? 0.0 : t / mn;
  const double gm = cond ? 0.0 : rowd_dot(go, mx);             // d L / d s
  const double dsdmn = (tp * q * mn - t) / (mn * mn);
  const double c = mraw >= (double)MIN_NORM ? gm * dsdmn / mn : 0.0;
#pragma unroll
  HYPAD_ROW_EACH dmx.v[e] = s * go.v[e] + c * mx.v[e];
  const double dqdxn = (artanh_prime_d(xn) * xn - a) / (xn * xn);
  return xraw >= (double)MIN_NORM ? gm * tp * dqdxn : 0.0;     // (d s / d q = tp)
}
template <class R>
__device__ __forceinline__ R mobius_matvec_row(const R& mx, double xraw) { return mobius_scaled_row(mx, xraw, rowd_all_zero(mx)); }
template <class R>
__device__ __forceinline__ double mobius_matvec_row_bwd(const R& mx, double xraw, const R& go, R& dmx) {
  return mobius_scaled_row_bwd(mx, xraw, rowd_all_zero(mx), go, dmx);
}

// mobius_pointwise_mul (math_.py:1361-1371): the same scaling of wx = w * x, the zero row where every |w_e x_e| <= 1e-8 (the
// reference's `isclose` against zero).  The backward sends dL/d|x| back into x itself.
template <class R>
__device__ __forceinline__ bool rowd_all_close_to_zero(const R& a) {
  double nz = 0.0;
#pragma unroll
  HYPAD_ROW_EACH nz += fabs(a.v[e]) > 1e-8 ? 1.0 : 0.0;
  return groupd_sum<R::G>(nz) == 0.0;
}
template <class R>
__device__ __forceinline__ R mobius_pointwise_mul_d(const R& w, const R& x) {
  R wx;
#pragma unroll
  HYPAD_ROW_EACH wx.v[e] = w.v[e] * x.v[e];
  return mobius_scaled_row(wx, sqrt(rowd_dot(x, x)), rowd_all_close_to_zero(wx));
}
template <class R>
__device__ __forceinline__ void mobius_pointwise_mul_bwd_d(const R& w, const R& x, const R& go, R& dw, R& dx) {
  R wx, dwx;
#pragma unroll
  HYPAD_ROW_EACH wx.v[e] = w.v[e] * x.v[e];
  const double xraw = sqrt(rowd_dot(x, x));
  const double c = mobius_scaled_row_bwd(wx, xraw, rowd_all_close_to_zero(wx), go, dwx) / fmax(xraw, (double)MIN_NORM);
#pragma unroll
  HYPAD_ROW_EACH { dw.v[e] = dwx.v[e] * x.v[e]; dx.v[e] = dwx.v[e] * w.v[e] + c * x.v[e]; }
}

// mobius_scalar_mul (math_.py:853-858): tanh(r artanh |x|) x / |x| -- mobius_scaled_row's scaling with the scalar r in place of
// |m| / |x|, built from the same clamped maps; r may be negative, so the tanh clamp is two-sided here.  The backward returns dL/dr.
__device__ __forceinline__ double tanh_clamped2_d(double x) { return tanh(fmax(fmin(x, (double)TANH_CLAMP), -(double)TANH_CLAMP)); }
__device__ __forceinline__ double tanh_prime2_d(double x, double t) { return fabs(x) <= (double)TANH_CLAMP ? 1.0 - t * t : 0.0; }
template <class R>
__device__ __forceinline__ R mobius_scalar_mul_d(double r, const R& x) {
  const double n = fmax(sqrt(rowd_dot(x, x)), (double)MIN_NORM);
  const double s = tanh_clamped2_d(r * artanh_clamped_d(n)) / n;
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = s * x.v[e];
  return o;
}
template <class R>
__device__ __forceinline__ double mobius_scalar_mul_bwd_d(double r, const R& x, const R& go, R& dx) {
  const double raw = sqrt(rowd_dot(x, x));
  const double n = fmax(raw, (double)MIN_NORM);
  const double a = artanh_clamped_d(n), u = r * a;
  const double t = tanh_clamped2_d(u), tp = tanh_prime2_d(u, t);
  const double s = t / n, gs = rowd_dot(go, x);                  // d L / d s
  const double dsdn = (tp * r * artanh_prime_d(n) * n - t) / (n * n);
  const double c = raw >= (double)MIN_NORM ? gs * dsdn / n : 0.0;
#pragma unroll
  HYPAD_ROW_EACH dx.v[e] = s * go.v[e] + c * x.v[e];
  return gs * tp * a / n;
}

// The weighted gyromidpoint after its sums (math_.py:2051-2061,2084 and :2114-2122): t = nom / den', the halving
// t / (1 + sqrt(1 - |t|^2)), mobius_scalar_mul by r (lincomb), project.  den' = max(den, 1e-10) in the bmm form, clamp_abs(den, 1e-10)
// = den + 1e-10 (den is a sum of non-negative terms) in the reduce form.  Backward: g_nom = g_t / den', dL/d den (0 where the clamp or
// the zero of |.| holds it) and dL/dr.
struct MidpointCfg { bool halve, lincomb, project, clamp_abs; };
constexpr double MIDPOINT_DEN_EPS = 1e-10;
__device__ __forceinline__ double midpoint_den(double den, bool clamp_abs) {
  return clamp_abs ? den + MIDPOINT_DEN_EPS : fmax(den, MIDPOINT_DEN_EPS);
}
template <class R>
__device__ __forceinline__ R midpoint_tail_d(const R& nom, double den, double r, const MidpointCfg c) {
  const double rd = 1.0 / midpoint_den(den, c.clamp_abs);
  R a;
#pragma unroll
  HYPAD_ROW_EACH a.v[e] = nom.v[e] * rd;
  if (c.halve) {
    const double f = 1.0 / (1.0 + sqrt(1.0 - rowd_dot(a, a)));
#pragma unroll
    HYPAD_ROW_EACH a.v[e] *= f;
  }
  if (c.lincomb) a = mobius_scalar_mul_d(r, a);
  return c.project ? project_d(a) : a;
}
template <class R>
__device__ __forceinline__ void midpoint_tail_bwd_d(const R& nom, double den, double r, const MidpointCfg c, const R& go, R& gnom, double& gden,
                                                    double& gr) {
  const double rd = 1.0 / midpoint_den(den, c.clamp_abs);
  R t, a;
#pragma unroll
  HYPAD_ROW_EACH t.v[e] = nom.v[e] * rd;
  double f = 1.0, root = 1.0;
  if (c.halve) { root = sqrt(1.0 - rowd_dot(t, t)); f = 1.0 / (1.0 + root); }
#pragma unroll
  HYPAD_ROW_EACH a.v[e] = t.v[e] * f;
  R g = go;
  gr = 0.0;
  if (c.project) g = project_bwd_d(c.lincomb ? mobius_scalar_mul_d(r, a) : a, g);
  if (c.lincomb) { R ga; gr = mobius_scalar_mul_bwd_d(r, a, g, ga); g = ga; }
  if (c.halve) {                                                 // a = t f(|t|^2), f' = f^2 / (2 root)
    const double s = rowd_dot(g, t) * f * f / root;              // 2 g_s2
#pragma unroll
    HYPAD_ROW_EACH g.v[e] = f * g.v[e] + s * t.v[e];
  }
#pragma unroll
  HYPAD_ROW_EACH gnom.v[e] = g.v[e] * rd;
  const bool flows = c.clamp_abs ? den > 0.0 : den >= MIDPOINT_DEN_EPS;
  gden = flows ? -rowd_dot(g, t) * rd : 0.0;
}

// The geodesic distance (math_.py:861-975).  The pair map of dist_matmul (:942-947) from the three inner products:
//   num = x2 - 2 xy + y2    den = max(1 - 2 xy + x2 y2, 1e-15)    u = num / den    s = sqrt(max(u, 1e-15))    out = 2 artanh(s)
// Backward: a = dL/dnum and b = dL/dden of one pair under the incoming gradient g; g_u = g / (s (1 - s^2)), and nothing flows through
// a clamp that holds (u below 1e-15, s above 1 - 1e-7, den below 1e-15).
constexpr double DIST_EPS = 1e-15;
__device__ __forceinline__ double dist_pair_d(double x2, double y2, double xy) {
  const double num = x2 - 2.0 * xy + y2, den = fmax(1.0 - 2.0 * xy + x2 * y2, DIST_EPS);
  return 2.0 * artanh_clamped_d(sqrt(fmax(num / den, DIST_EPS)));
}
__device__ __forceinline__ void dist_pair_bwd_d(double x2, double y2, double xy, double g, double& a, double& b) {
  const double num = x2 - 2.0 * xy + y2, draw = 1.0 - 2.0 * xy + x2 * y2;
  const double rden = 1.0 / fmax(draw, DIST_EPS);
  const double u = num * rden, s = sqrt(fmax(u, DIST_EPS));
  const double gu = (u >= DIST_EPS && s <= ARTANH_TOP) ? g / (s * (1.0 - s) * (1.0 + s)) : 0.0;
  a = gu * rden;
  b = draw >= DIST_EPS ? -gu * u * rden : 0.0;
}
// The same maps at any negative curvature k = -c (docs/history/curvature_matmul.md): the reference's formulas with its k, not the k = -1
// maps on scaled operands -- the floors under u, under a length and under den sit on the unscaled quantities.  The kernels of dist.hip,
// midpoint.hip and attention.hip take the curvature as a trailing pack: empty at k = -1, where every call below resolves to the
// function above it and curv_mul is the identity, one Curv at k = -c.  With s = sqrt(c):
//   den = max(1 - 2 c xy + c^2 x2 y2, 1e-15)    u = max(num / den, 1e-15)    out = (2 / s) artanh(min(s sqrt(u), 1 - 1e-7))
// The backward returns a = dL/dnum and b = c dL/dden, so that dL/dxy = -2 (a + b) as at k = -1 and dL/dx2 = a + b (c y2).
struct Curv {
  double c, s, rs;                                               // c, sqrt(c), 1 / sqrt(c)
};
// the entry points' rule for c, and the Curv of a valid one (host side)
inline bool curv_invalid(double c) { return !(c > 0.0) || !std::isfinite(c); }
inline Curv curv_of(double c) { return Curv{c, std::sqrt(c), 1.0 / std::sqrt(c)}; }
__device__ __forceinline__ double curv_mul(double v) { return v; }
__device__ __forceinline__ double curv_mul(double v, const Curv& k) { return k.c * v; }
__device__ __forceinline__ double dist_pair_d(double x2, double y2, double xy, const Curv& k) {
  const double cxy = k.c * xy;
  const double num = x2 - 2.0 * xy + y2, den = fmax(1.0 - 2.0 * cxy + (k.c * x2) * (k.c * y2), DIST_EPS);
  return 2.0 * k.rs * artanh_clamped_d(k.s * sqrt(fmax(num / den, DIST_EPS)));
}
__device__ __forceinline__ void dist_pair_bwd_d(double x2, double y2, double xy, double g, double& a, double& b, const Curv& k) {
  const double num = x2 - 2.0 * xy + y2, draw = 1.0 - 2.0 * (k.c * xy) + (k.c * x2) * (k.c * y2);
  const double rden = 1.0 / fmax(draw, DIST_EPS);
  const double u = num * rden, r = sqrt(fmax(u, DIST_EPS)), z = k.s * r;
  const double gu = (u >= DIST_EPS && z <= ARTANH_TOP) ? g / (r * (1.0 - z) * (1.0 + z)) : 0.0;
  a = gu * rden;
  b = draw >= DIST_EPS ? -k.c * gu * u * rden : 0.0;
}
// mobius_scalar_mul: tanh(r artanh(s n)) x / (s n), n = max(|x|, 1e-15); project: onto the radius (1 - 4e-3) / s
template <class R>
__device__ __forceinline__ R mobius_scalar_mul_d(double r, const R& x, const Curv& k) {
  const double sn = k.s * fmax(sqrt(rowd_dot(x, x)), (double)MIN_NORM);
  const double f = tanh_clamped2_d(r * artanh_clamped_d(sn)) / sn;
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = f * x.v[e];
  return o;
}
template <class R>
__device__ __forceinline__ double mobius_scalar_mul_bwd_d(double r, const R& x, const R& go, R& dx, const Curv& k) {
  const double raw = sqrt(rowd_dot(x, x));
  const double n = fmax(raw, (double)MIN_NORM), sn = k.s * n;
  const double a = artanh_clamped_d(sn), u = r * a;
  const double t = tanh_clamped2_d(u), tp = tanh_prime2_d(u, t);
  const double f = t / sn, gs = rowd_dot(go, x);                 // d L / d f
  const double dfdn = k.s * (tp * r * artanh_prime_d(sn) * sn - t) / (sn * sn);
  const double c = raw >= (double)MIN_NORM ? gs * dfdn / n : 0.0;
#pragma unroll
  HYPAD_ROW_EACH dx.v[e] = f * go.v[e] + c * x.v[e];
  return gs * tp * a / sn;
}
template <class R>
__device__ __forceinline__ R project_d(const R& x, const Curv& k) {
  const double n = fmax(sqrt(rowd_dot(x, x)), (double)MIN_NORM), top = (double)BALL_MAXNORM * k.rs;
  R o = x;
  if (n > top) {
    const double sc = top / n;
#pragma unroll
    HYPAD_ROW_EACH o.v[e] = x.v[e] * sc;
  }
  return o;
}
template <class R>
__device__ __forceinline__ R project_bwd_d(const R& x, const R& go, const Curv& k) {
  const double raw = sqrt(rowd_dot(x, x));
  const double n = fmax(raw, (double)MIN_NORM), top = (double)BALL_MAXNORM * k.rs;
  if (!(n > top)) return go;
  const double s = raw >= (double)MIN_NORM ? rowd_dot(x, go) / (n * n) : 0.0, sc = top / n;
  R gx;
#pragma unroll
  HYPAD_ROW_EACH gx.v[e] = sc * (go.v[e] - x.v[e] * s);
  return gx;
}
// the midpoint's tail: the halving is t / (1 + sqrt(1 - c |t|^2)), f' = c f^2 / (2 root); den' and its rule are those of k = -1
template <class R>
__device__ __forceinline__ R midpoint_tail_d(const R& nom, double den, double r, const MidpointCfg c, const Curv& k) {
  const double rd = 1.0 / midpoint_den(den, c.clamp_abs);
  R a;
#pragma unroll
  HYPAD_ROW_EACH a.v[e] = nom.v[e] * rd;
  if (c.halve) {
    const double f = 1.0 / (1.0 + sqrt(1.0 - k.c * rowd_dot(a, a)));
#pragma unroll
    HYPAD_ROW_EACH a.v[e] *= f;
  }
  if (c.lincomb) a = mobius_scalar_mul_d(r, a, k);
  return c.project ? project_d(a, k) : a;
}
template <class R>
__device__ __forceinline__ void midpoint_tail_bwd_d(const R& nom, double den, double r, const MidpointCfg c, const R& go, R& gnom, double& gden,
                                                    double& gr, const Curv& k) {
  const double rd = 1.0 / midpoint_den(den, c.clamp_abs);
  R t, a;
#pragma unroll
  HYPAD_ROW_EACH t.v[e] = nom.v[e] * rd;
  double f = 1.0, root = 1.0;
  if (c.halve) { root = sqrt(1.0 - k.c * rowd_dot(t, t)); f = 1.0 / (1.0 + root); }
#pragma unroll
  HYPAD_ROW_EACH a.v[e] = t.v[e] * f;
  R g = go;
  gr = 0.0;
  if (c.project) g = project_bwd_d(c.lincomb ? mobius_scalar_mul_d(r, a, k) : a, g, k);
  if (c.lincomb) { R ga; gr = mobius_scalar_mul_bwd_d(r, a, g, ga, k); g = ga; }
  if (c.halve) {
    const double s = k.c * rowd_dot(g, t) * f * f / root;
#pragma unroll
    HYPAD_ROW_EACH g.v[e] = f * g.v[e] + s * t.v[e];
  }
#pragma unroll
  HYPAD_ROW_EACH gnom.v[e] = g.v[e] * rd;
  const bool flows = c.clamp_abs ? den > 0.0 : den >= MIDPOINT_DEN_EPS;
  gden = flows ? -rowd_dot(g, t) * rd : 0.0;
}
// dist (:893-902): 2 artanh(|(-x) (+) y|), the norm without a clamp.  Two rows that are equal element by element are at distance 0
// with gradient 0 (the norm's backward at 0, as torch defines it): decided from the rows themselves, because (-x) (+) x is only zero
// up to the rounding of 1 - 2 |x|^2 + |x|^2 against 1 - |x|^2, and a gradient of size g through a norm of 1e-16 is noise.
template <class R>
__device__ __forceinline__ R rowd_neg(const R& x) {
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = -x.v[e];
  return o;
}
template <class R>
__device__ __forceinline__ bool rowd_equal(const R& x, const R& y) {
  double ne = 0.0;
#pragma unroll
  HYPAD_ROW_EACH ne += x.v[e] != y.v[e] ? 1.0 : 0.0;
  return groupd_sum<R::G>(ne) == 0.0;
}
template <class R>
__device__ __forceinline__ double dist_row_d(const R& x, const R& y) {
  if (rowd_equal(x, y)) return 0.0;
  const R m = mobius_add_d(rowd_neg(x), y);
  return 2.0 * artanh_clamped_d(sqrt(rowd_dot(m, m)));
}
template <class R>
__device__ __forceinline__ void dist_row_bwd_d(const R& x, const R& y, double g, R& dx, R& dy) {
  const R nx = rowd_neg(x);
  const R m = mobius_add_d(nx, y);
  const double n = sqrt(rowd_dot(m, m));
  const double c = (n > 0.0 && !rowd_equal(x, y)) ? 2.0 * g * artanh_prime_d(n) / n : 0.0;
  R dm, dnx;
#pragma unroll
  HYPAD_ROW_EACH dm.v[e] = c * m.v[e];
  mobius_add_bwd_d(nx, y, dm, dnx, dy);
#pragma unroll
  HYPAD_ROW_EACH dx.v[e] = -dnx.v[e];
}
// dist0 (:973-975): 2 artanh(|x|); the all-zero row gets gradient 0
template <class R>
__device__ __forceinline__ double dist0_row_d(const R& x) { return 2.0 * artanh_clamped_d(sqrt(rowd_dot(x, x))); }
template <class R>
__device__ __forceinline__ R dist0_row_bwd_d(const R& x, double g) {
  const double n = sqrt(rowd_dot(x, x));
  const double c = n > 0.0 ? 2.0 * g * artanh_prime_d(n) / n : 0.0;
  R dx;
#pragma unroll
  HYPAD_ROW_EACH dx.v[e] = c * x.v[e];
  return dx;
}

// The tangent maps at a point of the ball (math_.py:1097-1102 expmap, :1226-1230 logmap, :1042-1049 geodesic, :657-675 gyration,
// :1739-1746 parallel_transport, :1776-1779 and :1810-1813 the two transports of the origin).  c(x) = max(1 - |x|^2, 1e-15) = 2 / lambda_x;
// nothing flows back through it where the clamp holds.  artanh is the log1p form above, so at coincident points logmap and geodesic
// follow artanh(n) / n -> 1 (the reference's fp32 difference of two logarithms returns 0 there).
__device__ __forceinline__ double conformal_d(double x2) { return fmax(1.0 - x2, DIST_EPS); }
__device__ __forceinline__ double conformal_prime_d(double x2) { return 1.0 - x2 >= DIST_EPS ? -1.0 : 0.0; }
// expmap: x (+) (tanh(min(n / c(x), 15)) u / n), n = max(|u|, 1e-15)
template <class R>
__device__ __forceinline__ R expmap_d(const R& x, const R& u) {
  const double n = fmax(sqrt(rowd_dot(u, u)), (double)MIN_NORM);
  const double f = tanh_clamped_d(n / conformal_d(rowd_dot(x, x))) / n;
  R s;
#pragma unroll
  HYPAD_ROW_EACH s.v[e] = f * u.v[e];
  return mobius_add_d(x, s);
}
template <class R>
__device__ __forceinline__ void expmap_bwd_d(const R& x, const R& u, const R& go, R& dx, R& du) {
  const double raw = sqrt(rowd_dot(u, u)), x2 = rowd_dot(x, x);
  const double n = fmax(raw, (double)MIN_NORM), c = conformal_d(x2), arg = n / c;
  const double t = tanh_clamped_d(arg), tp = tanh_prime_d(arg, t), f = t / n;
  R s, ds;
#pragma unroll
  HYPAD_ROW_EACH s.v[e] = f * u.v[e];
  mobius_add_bwd_d(x, s, go, dx, ds);
  const double gf = rowd_dot(ds, u);                             // d L / d f;  f = tanh(n / c) / n
  const double cu = raw >= (double)MIN_NORM ? gf * (tp * arg - t) / (n * n * n) : 0.0;
  const double cx = -2.0 * gf * tp / (c * c) * conformal_prime_d(x2);      // 2 dL/d|x|^2
#pragma unroll
  HYPAD_ROW_EACH { du.v[e] = f * ds.v[e] + cu * u.v[e]; dx.v[e] += cx * x.v[e]; }
}
// logmap: artanh(min(n, 1 - 1e-7)) c(x) w / n, w = (-x) (+) y, n = max(|w|, 1e-15)
template <class R>
__device__ __forceinline__ R logmap_d(const R& x, const R& y) {
  const R w = mobius_add_d(rowd_neg(x), y);
  const double n = fmax(sqrt(rowd_dot(w, w)), (double)MIN_NORM);
  const double f = artanh_clamped_d(n) * conformal_d(rowd_dot(x, x)) / n;
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = f * w.v[e];
  return o;
}
template <class R>
__device__ __forceinline__ void logmap_bwd_d(const R& x, const R& y, const R& go, R& dx, R& dy) {
  const R nx = rowd_neg(x);
  const R w = mobius_add_d(nx, y);
  const double raw = sqrt(rowd_dot(w, w)), x2 = rowd_dot(x, x);
  const double n = fmax(raw, (double)MIN_NORM), c = conformal_d(x2), a = artanh_clamped_d(n);
  const double f = a * c / n, gf = rowd_dot(go, w);              // d L / d f
  const double cw = raw >= (double)MIN_NORM ? gf * c * (artanh_prime_d(n) * n - a) / (n * n * n) : 0.0;
  const double cx = 2.0 * gf * a / n * conformal_prime_d(x2);
  R dw, dnx;
#pragma unroll
  HYPAD_ROW_EACH dw.v[e] = f * go.v[e] + cw * w.v[e];
  mobius_add_bwd_d(nx, y, dw, dnx, dy);
#pragma unroll
  HYPAD_ROW_EACH dx.v[e] = cx * x.v[e] - dnx.v[e];
}
// geodesic: x (+) (t (x) ((-x) (+) y)); the backward returns dL/dt
template <class R>
__device__ __forceinline__ R geodesic_d(double t, const R& x, const R& y) {
  return mobius_add_d(x, mobius_scalar_mul_d(t, mobius_add_d(rowd_neg(x), y)));
}
template <class R>
__device__ __forceinline__ double geodesic_bwd_d(double t, const R& x, const R& y, const R& go, R& dx, R& dy) {
  const R nx = rowd_neg(x);
  const R v = mobius_add_d(nx, y);
  R dtv, dv, dnx;
  mobius_add_bwd_d(x, mobius_scalar_mul_d(t, v), go, dx, dtv);
  const double gt = mobius_scalar_mul_bwd_d(t, v, dtv, dv);
  mobius_add_bwd_d(nx, y, dv, dnx, dy);
#pragma unroll
  HYPAD_ROW_EACH dx.v[e] -= dnx.v[e];
  return gt;
}
// gyration gyr[a, b] u = u + 2 (A a + B b) / d:  A = -<a,u> |b|^2 + <b,u> + 2 <a,b> <b,u>,  B = -<b,u> |a|^2 - <a,u>,
// d = max(1 + 2 <a,b> + |a|^2 |b|^2, 1e-15)
template <class R>
__device__ __forceinline__ R gyration_d(const R& a, const R& b, const R& u) {
  const double a2 = rowd_dot(a, a), b2 = rowd_dot(b, b), ab = rowd_dot(a, b), au = rowd_dot(a, u), bu = rowd_dot(b, u);
  const double q = 2.0 / fmax(1.0 + 2.0 * ab + a2 * b2, DIST_EPS);
  const double A = q * (-au * b2 + bu + 2.0 * ab * bu), B = q * (-bu * a2 - au);
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = u.v[e] + A * a.v[e] + B * b.v[e];
  return o;
}
template <class R>
__device__ __forceinline__ void gyration_bwd_d(const R& a, const R& b, const R& u, const R& go, R& da, R& db, R& du) {
  const double a2 = rowd_dot(a, a), b2 = rowd_dot(b, b), ab = rowd_dot(a, b), au = rowd_dot(a, u), bu = rowd_dot(b, u);
  const double draw = 1.0 + 2.0 * ab + a2 * b2, q = 2.0 / fmax(draw, DIST_EPS);
  const double A = -au * b2 + bu + 2.0 * ab * bu, B = -bu * a2 - au;
  const double gA = q * rowd_dot(go, a), gB = q * rowd_dot(go, b);           // d L / d A, d L / d B
  const double gd = draw >= DIST_EPS ? -0.5 * q * (A * gA + B * gB) : 0.0;
  const double gau = -b2 * gA - gB, gbu = (1.0 + 2.0 * ab) * gA - a2 * gB, gab = 2.0 * (bu * gA + gd);
  const double ga2 = -bu * gB + b2 * gd, gb2 = -au * gA + a2 * gd;
#pragma unroll
  HYPAD_ROW_EACH {
    da.v[e] = q * A * go.v[e] + gau * u.v[e] + gab * b.v[e] + 2.0 * ga2 * a.v[e];
    db.v[e] = q * B * go.v[e] + gbu * u.v[e] + gab * a.v[e] + 2.0 * gb2 * b.v[e];
    du.v[e] = go.v[e] + gau * a.v[e] + gbu * b.v[e];
  }
}
// parallel_transport: gyr[y, -x] v c(y) / c(x)
template <class R>
__device__ __forceinline__ R parallel_transport_d(const R& x, const R& y, const R& v) {
  const double s = conformal_d(rowd_dot(y, y)) / conformal_d(rowd_dot(x, x));
  R o = gyration_d(y, rowd_neg(x), v);
#pragma unroll
  HYPAD_ROW_EACH o.v[e] *= s;
  return o;
}
template <class R>
__device__ __forceinline__ void parallel_transport_bwd_d(const R& x, const R& y, const R& v, const R& go, R& dx, R& dy, R& dv) {
  const R nx = rowd_neg(x);
  const double x2 = rowd_dot(x, x), y2 = rowd_dot(y, y), cx = conformal_d(x2), cy = conformal_d(y2), s = cy / cx;
  const double gs = rowd_dot(go, gyration_d(y, nx, v));          // d L / d s
  R gg, dnx;
#pragma unroll
  HYPAD_ROW_EACH gg.v[e] = s * go.v[e];
  gyration_bwd_d(y, nx, v, gg, dy, dnx, dv);
  const double ky = 2.0 * gs / cx * conformal_prime_d(y2), kx = -2.0 * gs * s / cx * conformal_prime_d(x2);
#pragma unroll
  HYPAD_ROW_EACH { dy.v[e] += ky * y.v[e]; dx.v[e] = kx * x.v[e] - dnx.v[e]; }
}
// parallel_transport0: v c(y);  parallel_transport0back (BACK): v / c(x)
template <bool BACK, class R>
__device__ __forceinline__ R transport0_d(const R& p, const R& v) {
  const double c = conformal_d(rowd_dot(p, p)), s = BACK ? 1.0 / c : c;
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = s * v.v[e];
  return o;
}
template <bool BACK, class R>
__device__ __forceinline__ void transport0_bwd_d(const R& p, const R& v, const R& go, R& dp, R& dv) {
  const double p2 = rowd_dot(p, p), c = conformal_d(p2), s = BACK ? 1.0 / c : c;
  const double k = 2.0 * rowd_dot(go, v) * (BACK ? -s * s : 1.0) * conformal_prime_d(p2);
#pragma unroll
  HYPAD_ROW_EACH { dp.v[e] = k * p.v[e]; dv.v[e] = s * go.v[e]; }
}

// The rest of the gyrogroup and the metric (math_.py:558-589 mobius_sub, :678-744 mobius_coadd, :747-779 mobius_cosub, :1139-1185
// geodesic_unit, :355-383 lambda_x, :386-430 inner, :433-472 norm, :1816-1845 egrad2rgrad, :1848-1874 sproj, :1877-1905 inv_sproj).
// mobius_sub: x (+) (-y)
template <class R>
__device__ __forceinline__ R mobius_sub_d(const R& x, const R& y) { return mobius_add_d(x, rowd_neg(y)); }
template <class R>
__device__ __forceinline__ void mobius_sub_bwd_d(const R& x, const R& y, const R& go, R& dx, R& dy) {
  R dny;
  mobius_add_bwd_d(x, rowd_neg(y), go, dx, dny);
  dy = rowd_neg(dny);
}
// mobius_coadd: ((1 - |y|^2) x + (1 - |x|^2) y) / max(1 - |x|^2 |y|^2, 1e-15);  mobius_cosub (SUB): the same of x and -y
template <bool SUB, class R>
__device__ __forceinline__ R mobius_coadd_d(const R& x, const R& ys) {
  const R y = SUB ? rowd_neg(ys) : ys;
  const double x2 = rowd_dot(x, x), y2 = rowd_dot(y, y);
  const double A = 1.0 - y2, B = 1.0 - x2, rD = 1.0 / fmax(1.0 - x2 * y2, DIST_EPS);
  R m;
#pragma unroll
  HYPAD_ROW_EACH m.v[e] = (A * x.v[e] + B * y.v[e]) * rD;
  return m;
}
template <bool SUB, class R>
__device__ __forceinline__ void mobius_coadd_bwd_d(const R& x, const R& ys, const R& go, R& dx, R& dy) {
  const R y = SUB ? rowd_neg(ys) : ys;
  const double x2 = rowd_dot(x, x), y2 = rowd_dot(y, y);
  const double A = 1.0 - y2, B = 1.0 - x2, draw = 1.0 - x2 * y2, rD = 1.0 / fmax(draw, DIST_EPS);
  R m, dN;
#pragma unroll
  HYPAD_ROW_EACH { m.v[e] = (A * x.v[e] + B * y.v[e]) * rD; dN.v[e] = go.v[e] * rD; }
  const double dD = draw >= DIST_EPS ? -rowd_dot(go, m) * rD : 0.0;
  const double dA = rowd_dot(dN, x), dB = rowd_dot(dN, y);
  const double dx2 = -dB - y2 * dD, dy2 = -dA - x2 * dD, sy = SUB ? -1.0 : 1.0;
#pragma unroll
  HYPAD_ROW_EACH { dx.v[e] = A * dN.v[e] + 2.0 * dx2 * x.v[e]; dy.v[e] = sy * (B * dN.v[e] + 2.0 * dy2 * y.v[e]); }
}
// geodesic_unit: x (+) (tanh(clamp(t / 2, +-15)) u / n), n = max(|u|, 1e-15); the backward returns dL/dt
template <class R>
__device__ __forceinline__ R geodesic_unit_d(double t, const R& x, const R& u) {
  const double f = tanh_clamped2_d(0.5 * t) / fmax(sqrt(rowd_dot(u, u)), (double)MIN_NORM);
  R s;
#pragma unroll
  HYPAD_ROW_EACH s.v[e] = f * u.v[e];
  return mobius_add_d(x, s);
}
template <class R>
__device__ __forceinline__ double geodesic_unit_bwd_d(double t, const R& x, const R& u, const R& go, R& dx, R& du) {
  const double raw = sqrt(rowd_dot(u, u)), n = fmax(raw, (double)MIN_NORM);
  const double th = tanh_clamped2_d(0.5 * t), tp = tanh_prime2_d(0.5 * t, th), f = th / n;
  R s, ds;
#pragma unroll
  HYPAD_ROW_EACH s.v[e] = f * u.v[e];
  mobius_add_bwd_d(x, s, go, dx, ds);
  const double gf = rowd_dot(ds, u);                             // d L / d f;  f = tanh(t / 2) / n
  const double cu = raw >= (double)MIN_NORM ? -gf * th / (n * n * n) : 0.0;
#pragma unroll
  HYPAD_ROW_EACH du.v[e] = f * ds.v[e] + cu * u.v[e];
  return 0.5 * gf * tp / n;
}
// lambda_x = 2 / c(x), one value per row
template <class R>
__device__ __forceinline__ double lambda_x_d(const R& x) { return 2.0 / conformal_d(rowd_dot(x, x)); }
template <class R>
__device__ __forceinline__ void lambda_x_bwd_d(const R& x, double g, R& dx) {
  const double x2 = rowd_dot(x, x), c = conformal_d(x2);
  const double k = -4.0 * g / (c * c) * conformal_prime_d(x2);    // 2 dL/d|x|^2
#pragma unroll
  HYPAD_ROW_EACH dx.v[e] = k * x.v[e];
}
// inner: lambda_x^2 <u, v>
template <class R>
__device__ __forceinline__ double inner_d(const R& x, const R& u, const R& v) {
  const double c = conformal_d(rowd_dot(x, x));
  return 4.0 / (c * c) * rowd_dot(u, v);
}
template <class R>
__device__ __forceinline__ void inner_bwd_d(const R& x, const R& u, const R& v, double g, R& dx, R& du, R& dv) {
  const double x2 = rowd_dot(x, x), c = conformal_d(x2), l2 = 4.0 / (c * c);
  const double k = -16.0 * g * rowd_dot(u, v) / (c * c * c) * conformal_prime_d(x2), s = g * l2;
#pragma unroll
  HYPAD_ROW_EACH { dx.v[e] = k * x.v[e]; du.v[e] = s * v.v[e]; dv.v[e] = s * u.v[e]; }
}
// norm: lambda_x |u|, the Euclidean norm without a clamp; a zero tangent gets gradient 0
template <class R>
__device__ __forceinline__ double tangent_norm_d(const R& x, const R& u) { return 2.0 / conformal_d(rowd_dot(x, x)) * sqrt(rowd_dot(u, u)); }
template <class R>
__device__ __forceinline__ void tangent_norm_bwd_d(const R& x, const R& u, double g, R& dx, R& du) {
  const double x2 = rowd_dot(x, x), c = conformal_d(x2), n = sqrt(rowd_dot(u, u));
  const double k = -4.0 * g * n / (c * c) * conformal_prime_d(x2), s = n > 0.0 ? 2.0 * g / (c * n) : 0.0;
#pragma unroll
  HYPAD_ROW_EACH { dx.v[e] = k * x.v[e]; du.v[e] = s * u.v[e]; }
}
// egrad2rgrad: grad / lambda_x^2 = grad c(x)^2 / 4
template <class R>
__device__ __forceinline__ R egrad2rgrad_d(const R& x, const R& g) {
  const double c = conformal_d(rowd_dot(x, x)), s = 0.25 * c * c;
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = s * g.v[e];
  return o;
}
template <class R>
__device__ __forceinline__ void egrad2rgrad_bwd_d(const R& x, const R& g, const R& go, R& dx, R& dg) {
  const double x2 = rowd_dot(x, x), c = conformal_d(x2), s = 0.25 * c * c;
  const double k = rowd_dot(go, g) * c * conformal_prime_d(x2);   // 2 dL/d|x|^2
#pragma unroll
  HYPAD_ROW_EACH { dx.v[e] = k * x.v[e]; dg.v[e] = s * go.v[e]; }
}
// The unit sphere's maps for the row-wise optimiser steps (riemann_opt.hip; geoopt.manifolds.Sphere, restated): the projection of u on the
// tangent space at x, u - <x, u> x, which is also its egrad2rgrad and, taken at the end point, its vector transport; and the projection
// of a row on the sphere, which after x + u is its retraction.  The floor under the norm is this library's (DIST_EPS; geoopt divides
// unguarded): a row shorter than that stays as short instead of turning into NaN.
template <class R>
__device__ __forceinline__ R sphere_proju_d(const R& x, const R& u) {
  const double xu = rowd_dot(x, u);
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = u.v[e] - xu * x.v[e];
  return o;
}
template <class R>
__device__ __forceinline__ R sphere_projx_d(const R& x) {
  const double n = fmax(sqrt(rowd_dot(x, x)), DIST_EPS);
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = x.v[e] / n;
  return o;
}
// The two projections between the ball (D columns) and the hyperboloid (D + 1, the time-like coordinate last).  The element at one
// column of a row, for every lane: a masked sum.
template <class R>
__device__ __forceinline__ double rowd_at(const R& a, int col, int lane) {
  double s = 0.0;
#pragma unroll
  HYPAD_ROW_EACH s += (lane & (R::G - 1)) + R::G * e == col ? a.v[e] : 0.0;
  return groupd_sum<R::G>(s);
}
template <class R>
__device__ __forceinline__ void rowd_set(R& a, int col, int lane, double val) {
#pragma unroll
  HYPAD_ROW_EACH if ((lane & (R::G - 1)) + R::G * e == col) a.v[e] = val;
}
// sproj: h[:D] / (1 + h[D]), no clamp.  The result's column D is left as it comes: the store ends before it.
template <class R>
__device__ __forceinline__ R sproj_d(const R& h, int D, int lane) {
  const double f = 1.0 / (1.0 + rowd_at(h, D, lane));
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = f * h.v[e];
  return o;
}
// go holds D columns (column D zero, as rowd_load leaves it)
template <class R>
__device__ __forceinline__ R sproj_bwd_d(const R& h, const R& go, int D, int lane) {
  const double hD = rowd_at(h, D, lane), f = 1.0 / (1.0 + hD);
  const double gD = -f * f * (rowd_dot(go, h));                   // (go's column D is zero: the sum runs over the D space-like columns)
  R dh;
#pragma unroll
  HYPAD_ROW_EACH dh.v[e] = f * go.v[e];
  rowd_set(dh, D, lane, gD);
  return dh;
}
// inv_sproj: cat(lambda_x x, lambda_x - 1)
template <class R>
__device__ __forceinline__ R inv_sproj_d(const R& x, int D, int lane) {
  const double lam = 2.0 / conformal_d(rowd_dot(x, x));
  R o;
#pragma unroll
  HYPAD_ROW_EACH o.v[e] = lam * x.v[e];
  rowd_set(o, D, lane, lam - 1.0);
  return o;
}
// go holds D + 1 columns, x D (column D zero)
template <class R>
__device__ __forceinline__ R inv_sproj_bwd_d(const R& x, const R& go, int D, int lane) {
  const double x2 = rowd_dot(x, x), c = conformal_d(x2), lam = 2.0 / c;
  const double glam = rowd_dot(go, x) + rowd_at(go, D, lane);     // d L / d lambda
  const double k = -4.0 * glam / (c * c) * conformal_prime_d(x2);
  R dx;
#pragma unroll
  HYPAD_ROW_EACH dx.v[e] = lam * go.v[e] + k * x.v[e];
  return dx;
}

// The GRU gate sigmoid(logmap0(y)) (hyrnn_nets.py:81-82).  (Columns past the row's end come out as 0.5: every use multiplies them
// with a zero of the other operand before a sum is taken.)
template <class R>
__device__ __forceinline__ R sigmoid_logmap0_d(const R& y) {
  R g = radial_map_d<false>(y);
#pragma unroll
  HYPAD_ROW_EACH g.v[e] = 1.0 / (1.0 + exp(-g.v[e]));
  return g;
}
template <class R>
__device__ __forceinline__ R sigmoid_logmap0_bwd_d(const R& y, const R& dg) {
  const R g = sigmoid_logmap0_d(y);
  R dl;
#pragma unroll
  HYPAD_ROW_EACH dl.v[e] = dg.v[e] * g.v[e] * (1.0 - g.v[e]);
  return radial_map_bwd_d<false>(y, dl);
}

// one_rnn_transform (hyrnn_nets.py:61-65) after the two products: ((W (x) h) (+) (U (x) x)) (+) b, and its backward -- the product
// gradients, the bias gradient and dL/d|h|, dL/d|x|.
template <class R>
__device__ __forceinline__ R rnn_transform_row(const R& mh, double hraw, const R& mx, double xraw, const R& b) {
  return mobius_add_d(mobius_add_d(mobius_matvec_row(mh, hraw), mobius_matvec_row(mx, xraw)), b);
}
template <class R>
__device__ __forceinline__ void rnn_transform_row_bwd(const R& mh, double hraw, const R& mx, double xraw, const R& b, const R& dy, R& dmh,
                                                      R& dmx, R& db, double& ghn, double& gxn) {
  const R wh = mobius_matvec_row(mh, hraw), ux = mobius_matvec_row(mx, xraw);
  R ds, dwh, dux;
  mobius_add_bwd_d(mobius_add_d(wh, ux), b, dy, ds, db);
  mobius_add_bwd_d(wh, ux, ds, dwh, dux);
  ghn = mobius_matvec_row_bwd(mh, hraw, dwh, dmh);
  gxn = mobius_matvec_row_bwd(mx, xraw, dux, dmx);
}

// mobius_fn_apply (math_.py:1431-1469): expmap0(f(logmap0(x))) for the two functions the layer takes
enum { NONLIN_NONE = 0, NONLIN_TANH = 1, NONLIN_RELU = 2 };
template <int NONLIN, class R>
__device__ __forceinline__ R mobius_fn_row(const R& x) {
  R l = radial_map_d<false>(x);
#pragma unroll
  HYPAD_ROW_EACH l.v[e] = NONLIN == NONLIN_TANH ? tanh(l.v[e]) : fmax(l.v[e], 0.0);
  return radial_map_d<true>(l);
}
template <int NONLIN, class R>
__device__ __forceinline__ R mobius_fn_row_bwd(const R& x, const R& go) {
  const R l = radial_map_d<false>(x);
  R f;
#pragma unroll
  HYPAD_ROW_EACH f.v[e] = NONLIN == NONLIN_TANH ? tanh(l.v[e]) : fmax(l.v[e], 0.0);
  R df = radial_map_bwd_d<true>(f, go);
#pragma unroll
  HYPAD_ROW_EACH df.v[e] *= NONLIN == NONLIN_TANH ? 1.0 - f.v[e] * f.v[e] : (l.v[e] > 0.0 ? 1.0 : 0.0);
  return radial_map_bwd_d<false>(x, df);
}

// The chain (hyrnn_nets.py:23-35): matvec scaling or expmap0, the optional Moebius bias add, the optional non-linearity, project.
// `b` is the bias ON THE BALL (a Euclidean bias is mapped by the caller, once).
struct MobiusCfg { bool hyper_in, has_bias, project; int nonlin; };
template <class R>
__device__ __forceinline__ R mobius_chain_row(const R& mx, double xraw, const R& b, const MobiusCfg c) {
  R o = c.hyper_in ? mobius_matvec_row(mx, xraw) : radial_map_d<true>(mx);
  if (c.has_bias) o = mobius_add_d(o, b);
  if (c.nonlin == NONLIN_TANH) o = mobius_fn_row<NONLIN_TANH>(o);
  else if (c.nonlin == NONLIN_RELU) o = mobius_fn_row<NONLIN_RELU>(o);
  return c.project ? project_d(o) : o;
}
// everything but mx is recomputed (as head_row_bwd does); returns dL/d|x| (0 for a Euclidean input)
template <class R>
__device__ __forceinline__ double mobius_chain_row_bwd(const R& mx, double xraw, const R& b, const MobiusCfg c, const R& go, R& dmx, R& db) {
  const R p = c.hyper_in ? mobius_matvec_row(mx, xraw) : radial_map_d<true>(mx);
  const R m = c.has_bias ? mobius_add_d(p, b) : p;
  R d = go;
  if (c.project) {
    R f = m;
    if (c.nonlin == NONLIN_TANH) f = mobius_fn_row<NONLIN_TANH>(m);
    else if (c.nonlin == NONLIN_RELU) f = mobius_fn_row<NONLIN_RELU>(m);
    d = project_bwd_d(f, d);
  }
  if (c.nonlin == NONLIN_TANH) d = mobius_fn_row_bwd<NONLIN_TANH>(m, d);
  else if (c.nonlin == NONLIN_RELU) d = mobius_fn_row_bwd<NONLIN_RELU>(m, d);
  if (c.has_bias) {
    R dp;
    mobius_add_bwd_d(p, b, d, dp, db);
    d = dp;
  }
  if (c.hyper_in) return mobius_matvec_row_bwd(mx, xraw, d, dmx);
  dmx = radial_map_bwd_d<true>(mx, d);
  return 0.0;
}
#undef HYPAD_ROW_EACH

// ---- row-wise Poincare distance (train.py:226-230)
template <class R>
__device__ __forceinline__ float rowdist_row(const R& u, const R& v) {
  R d;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) d.v[e] = u.v[e] - v.v[e];
  float sq = row_dot(d, d), un = row_dot(u, u), vn = row_dot(v, v);
  return acoshf(1.f + 2.f * sq / ((1.f - un) * (1.f - vn)) + 1e-7f);
}
template <class R>
__device__ __forceinline__ float rowdist_row_bwd(const R& u, const R& v, float gd, R& du, R& dv) {
  R d;
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) d.v[e] = u.v[e] - v.v[e];
  float sq = row_dot(d, d), un = row_dot(u, u), vn = row_dot(v, v);
  float den = (1.f - un) * (1.f - vn);
  float xt = 1.f + 2.f * sq / den + 1e-7f;
  float gx = gd / sqrtf(xt * xt - 1.f);
  float dsq = gx * 2.f / den;
  float dden = -gx * 2.f * sq / (den * den);
  float dun = -dden * (1.f - vn), dvn = -dden * (1.f - un);
#pragma unroll
  for (int e = 0; e < R::EPL; ++e) {
    du.v[e] = dsq * 2.f * d.v[e] + dun * 2.f * u.v[e];
    dv.v[e] = -dsq * 2.f * d.v[e] + dvn * 2.f * v.v[e];
  }
  return acoshf(xt);
}

// Host launchers of ops_hyper.hip that the layer entry points of ops_dense.hip call (not exported; arguments checked by the caller):
// the row backward of mobius_chain_row -- g_mx (rows, N), the per-row bias gradients and dL/d|x| per row (either may be null) -- and
// grad_x += dL/d|x| x / |x|.
int mobius_chain_bwd_launch(const float* x, const float* mx, const float* bias, const float* go, float* gmx, float* gb_rows, float* gxn,
                            int64_t rows, int K, int N, bool hyper_in, bool hyper_bias, int nonlin, int project, void* stream);
int norm_grad_add_launch(const float* x, const float* gxn, float* gx, int64_t rows, int K, void* stream);
// lstm_t1_lds.hip, for hypad_lstm_bidir_fwd (the same arguments, checked by the caller): the weights-stationary forwards of the T = 1
// bidirectional LSTM layer.  An error code; or HYPAD_OK with *launched true: the layer ran; or HYPAD_OK with *launched false: not a
// shape of these kernels (fewer than 2 048 rows, hidden > 64, input > 128), nothing was launched and the caller runs the streamed form.
int lstm_t1_lds_launch(const float* x, const float* wf, const float* bif, const float* bhf, const float* wr, const float* bir,
                       const float* bhr, float* out, float* gates_save, int64_t rows, int K, int H, void* stream, bool* launched);

// f(integral_constant<int, EPL>) with the 16-lanes-per-row EPL that fits `dim` (wave-uniform branch)
template <class F>
__device__ __forceinline__ void epl16_dispatch(int dim, F f) {
  if (dim <= 64) f(std::integral_constant<int, 4>{});
  else if (dim <= 112) f(std::integral_constant<int, 7>{});      // window 100: 7 elements per lane instead of 8 (the row chains are VALU-bound)
  else if (dim <= 128) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

}  // namespace hypad
