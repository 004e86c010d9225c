/*
 * hypad.h -- C ABI of libhypad_hip.so: the HypAD / TadGAN train + score hot path on MI355X (gfx950).
 *
 * The reference (aleflabo/HypAD, pure Python) has no FFI: its hot path sits behind Python callables.
 * Each entry point below names the reference code it replaces (file:line under /root/reference), so a
 * maintainer can bind it (ctypes stub in INTEGRATION.md) where that code runs today.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  Every data pointer is a DEVICE pointer owned by the caller.
 *   - `stream` is a hipStream_t passed as void*.  All work is enqueued on it; nothing synchronises,
 *     allocates or frees, so every call may be captured into a hipGraph.
 *   - return 0 on success, a negative HYPAD_E* code for argument errors, a positive hipError_t otherwise.
 *   - fp32 arithmetic throughout unless a function says fp64 (scoring post-processing follows NumPy's fp64).
 *   - matrices are dense row-major; weights keep PyTorch's (out_features, in_features) layout.
 *   - curvature is fixed at k = -1 (the only value the reference uses: hyperspace/hyrnn_nets.py:20,166).
 */
#ifndef HYPAD_H_
#define HYPAD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the declarations below are its whole dynamic symbol table. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define HYPAD_ABI_VERSION 7

enum {
  HYPAD_OK = 0,
  HYPAD_EINVAL = -1,       /* bad argument (null pointer, non-positive size, unsupported shape) */
  HYPAD_EWORKSPACE = -2,   /* workspace missing or too small */
  HYPAD_EUNSUPPORTED = -3  /* shape outside the fused path's limits (see hypad_limits) */
};

typedef void* hypad_stream_t; /* hipStream_t */

int hypad_abi_version(void);
const char* hypad_error_string(int code);
/* signal_shape <= max_signal_shape, latent_dim <= max_latent for the fused network kernels.  The training calls (hypad_dims) also
 * refuse latent 29..32 with windows above 240 (HYPAD_EUNSUPPORTED): their stand-alone critic launches would need more LDS than a CU has. */
void hypad_limits(int* max_signal_shape, int* max_latent);

/* ------------------------------------------------------------------------------------------------
 * Parameter arenas.  One flat fp32 buffer per network; tensors sit at fixed, 16-byte aligned offsets
 * and carry the reference's state_dict names and shapes (models/tadgan.py:11-21,31-56,71-89,110-121;
 * SURVEY.md A.1).  The host side builds its torch views from these queries.
 * ---------------------------------------------------------------------------------------------- */
enum { HYPAD_NET_ENCODER = 0, HYPAD_NET_DECODER = 1, HYPAD_NET_CRITIC_X = 2, HYPAD_NET_CRITIC_Z = 3 };

int hypad_param_count(int net, int signal_shape, int latent_dim, int hyperbolic);   /* floats, padded */
int hypad_param_tensors(int net, int hyperbolic);
int hypad_param_info(int net, int signal_shape, int latent_dim, int hyperbolic, int index,
                     char* name, int name_cap, int* offset, int* rows, int* cols);   /* cols = 0 for 1-D */

/* ------------------------------------------------------------------------------------------------
 * Poincare-ball ops (geoopt.manifolds.stereographic.math, vendored as /root/reference/math_.py).
 * Row-wise over (rows, dim) matrices.
 * ---------------------------------------------------------------------------------------------- */
/* gmath.expmap0  math_.py:1132-1136 (+ tan_k :217-238, tanh :51-53) */
int hypad_expmap0_fwd(const float* u, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_expmap0_bwd(const float* u, const float* grad_out, float* grad_u, int64_t rows, int dim, hypad_stream_t stream);
/* gmath.logmap0  math_.py:1267-1270 (+ artan_k :241-262, artanh :56-59) */
int hypad_logmap0_fwd(const float* y, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_logmap0_bwd(const float* y, const float* grad_out, float* grad_y, int64_t rows, int dim, hypad_stream_t stream);
/* gmath.mobius_add  math_.py:536-555.  y_rows == 1 broadcasts y over the rows of x (hyrnn_nets.py:31);
 * then grad_y is the (rows, dim) matrix of per-row contributions, to be column-summed by the caller
 * (hypad_column_sum). */
int hypad_mobius_add_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, int64_t y_rows, hypad_stream_t stream);
int hypad_mobius_add_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y,
                         int64_t rows, int dim, int64_t y_rows, hypad_stream_t stream);
/* gmath.project  math_.py:340-352 (fp32 eps 4e-3) */
int hypad_project_fwd(const float* x, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_project_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, hypad_stream_t stream);
/* fused expmap0 -> mobius_add(bias) -> project: the tail of mobius_linear, hyperspace/hyrnn_nets.py:27-34 */
int hypad_mobius_head_fwd(const float* u, const float* bias, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_mobius_head_bwd(const float* u, const float* bias, const float* grad_out, float* grad_u,
                          float* grad_bias_rows, int64_t rows, int dim, hypad_stream_t stream);
/* MobiusLinear.forward / mobius_linear  hyperspace/hyrnn_nets.py:186-200, :13-35
 * (hyperbolic_input=False, hyperbolic_bias=True, nonlin=None).  weight (out_dim, in_dim), bias (out_dim).
 * workspace: hypad_mobius_linear_workspace_bytes(rows, out_dim) -- holds u = x W^T for the backward.
 * rows == 0 (the row buffers and the workspace may then be NULL): the backward writes zeros to grad_weight and grad_bias. */
size_t hypad_mobius_linear_workspace_bytes(int64_t rows, int out_dim);
int hypad_mobius_linear_fwd(const float* x, const float* weight, const float* bias, float* out, float* u_save,
                            int64_t rows, int in_dim, int out_dim, hypad_stream_t stream);
int hypad_mobius_linear_bwd(const float* x, const float* weight, const float* bias, const float* u_saved,
                            const float* grad_out, float* grad_x, float* grad_weight, float* grad_bias,
                            void* workspace, size_t workspace_bytes,
                            int64_t rows, int in_dim, int out_dim, hypad_stream_t stream);
/* mobius_matvec  hyperspace/hyrnn_nets.py:38-58 (math_.py:1308-1323): out = M (x) x for ball-valued rows x (rows, in_dim) and
 * weight M (out_dim, in_dim) -- tanh(|mx| / |x| artanh |x|) mx / |mx| with mx = x M^T, the zero row where mx is exactly zero.
 * No bias, no non-linearity, no project.  mx_save (rows, out_dim) receives mx for the backward (may be NULL).
 * bwd: grad_x and grad_weight may each be NULL; workspace: hypad_mobius_linear_ex_workspace_bytes(rows, out_dim).  rows == 0 as
 * hypad_mobius_linear_bwd. */
int hypad_mobius_matvec_fwd(const float* x, const float* weight, float* out, float* mx_save,
                            int64_t rows, int in_dim, int out_dim, hypad_stream_t stream);
int hypad_mobius_matvec_bwd(const float* x, const float* weight, const float* mx_saved, const float* grad_out,
                            float* grad_x, float* grad_weight, void* workspace, size_t workspace_bytes,
                            int64_t rows, int in_dim, int out_dim, hypad_stream_t stream);
/* mobius_linear in every configuration  hyperspace/hyrnn_nets.py:13-35 (+ mobius_fn_apply math_.py:1431-1469):
 *   flags & HYPAD_ML_HYPER_INPUT  x lies on the ball: mobius_matvec(weight, x) (:23-24); otherwise expmap0(x W^T) (:26-27)
 *   bias (out_dim), NULL = none   on the ball with HYPAD_ML_HYPER_BIAS, otherwise Euclidean and mapped with expmap0 (:28-31)
 *   nonlin                        expmap0(f(logmap0(.))) for f = tanh / relu (:32-33)
 * then project (:34).  One forward launch; mx_save (rows, out_dim) = x W^T is all the backward keeps (may be NULL).
 * The row chain after x W^T runs in fp64 registers (a row the matvec scaling leaves at 1 - 1e-5 has no digits of 1 - norm to
 * spare in fp32); every buffer is fp32.  The same holds for hypad_mobius_matvec_*.
 * bwd: grad_x, grad_weight and grad_bias may each be NULL (grad_bias must be NULL without a bias); every argument is validated
 * before anything is launched.  rows == 0 as hypad_mobius_linear_bwd.  The same limits as hypad_mobius_linear_*. */
enum { HYPAD_ML_HYPER_INPUT = 1, HYPAD_ML_HYPER_BIAS = 2 };
enum { HYPAD_NONLIN_NONE = 0, HYPAD_NONLIN_TANH = 1, HYPAD_NONLIN_RELU = 2 };
size_t hypad_mobius_linear_ex_workspace_bytes(int64_t rows, int out_dim);
int hypad_mobius_linear_ex_fwd(const float* x, const float* weight, const float* bias, float* out, float* mx_save,
                               int64_t rows, int in_dim, int out_dim, int flags, int nonlin, hypad_stream_t stream);
int hypad_mobius_linear_ex_bwd(const float* x, const float* weight, const float* bias, const float* mx_saved,
                               const float* grad_out, float* grad_x, float* grad_weight, float* grad_bias,
                               void* workspace, size_t workspace_bytes,
                               int64_t rows, int in_dim, int out_dim, int flags, int nonlin, hypad_stream_t stream);
/* MobiusDist2Hyperplane / dist2plane  hyperspace/hyrnn_nets.py:210-245, math_.py:1645-1666 (_mobius_add :537-555, arsin_k :266-290)
 * at k = -1: out (rows, out_dim) = the geodesic distance of every ball-valued row of x (rows, in_dim) to the out_dim hyperplanes of
 * the ball through the points p (out_dim, in_dim) with the normals a (out_dim, in_dim),
 *   asinh(2 s' / clamp_abs((1 - |(-p) (+) x|^2) |a|)),  s' = <(-p) (+) x, a> with HYPAD_D2P_SIGNED, its absolute value without,
 * times |a| with HYPAD_D2P_SCALED, times exp(log_scale[n]) where log_scale (out_dim) is given (NULL: none; the layer's `scale`,
 * hyrnn_nets.py:237).  One launch; nothing is saved for the backward.
 * bwd: `out` is the forward's result (may be NULL: the backward recomputes what it needs); grad_x, grad_p, grad_a and grad_log_scale
 * may each be NULL (grad_log_scale must be NULL without a log_scale).  Sums over rows are added in a fixed order: two runs give the
 * same bits.  rows == 0 writes zero parameter gradients.  Every argument is validated before anything is launched: HYPAD_EINVAL for
 * a NULL operand, a non-positive size or an unknown flag, HYPAD_EUNSUPPORTED for in_dim > 256 (bwd: also where
 * hypad_linear_act_bwd refuses out_dim' = 2 out_dim), HYPAD_EWORKSPACE below hypad_dist2plane_workspace_bytes. */
enum { HYPAD_D2P_SIGNED = 1, HYPAD_D2P_SCALED = 2 };
size_t hypad_dist2plane_workspace_bytes(int64_t rows, int in_dim, int out_dim);
int hypad_dist2plane_fwd(const float* x, const float* p, const float* a, const float* log_scale /* NULL: none */, float* out,
                         int64_t rows, int in_dim, int out_dim, int flags, hypad_stream_t stream);
int hypad_dist2plane_bwd(const float* x, const float* p, const float* a, const float* log_scale, const float* out,
                         const float* grad_out, float* grad_x, float* grad_p, float* grad_a, float* grad_log_scale,
                         void* workspace, size_t workspace_bytes,
                         int64_t rows, int in_dim, int out_dim, int flags, hypad_stream_t stream);
/* gmath.mobius_pointwise_mul  math_.py:1361-1371 at k = -1: tanh(|w x| / |x| artanh |x|) w x / |w x| for ball-valued rows x, the
 * zero row where every |w_e x_e| <= 1e-8 (the reference's isclose against zero); evaluated in fp64 registers, buffers fp32.
 * w_rows == 1 broadcasts w over the rows of x; then grad_w is the (rows, dim) matrix of per-row contributions, to be column-summed
 * by the caller (hypad_column_sum), as hypad_mobius_add_bwd's grad_y.  dim <= 256. */
int hypad_mobius_pointwise_mul_fwd(const float* w, const float* x, float* out, int64_t rows, int dim, int64_t w_rows, hypad_stream_t stream);
int hypad_mobius_pointwise_mul_bwd(const float* w, const float* x, const float* grad_out, float* grad_w, float* grad_x,
                                   int64_t rows, int dim, int64_t w_rows, hypad_stream_t stream);
/* gmath.mobius_scalar_mul  math_.py:788-858 (_mobius_scalar_mul :853-858; tan_k, artan_k with the clamps of :51-59) at k = -1:
 * tanh(r artanh |x|) x / |x| for ball-valued rows x, |x| clamped at 1e-15; evaluated in fp64 registers, buffers fp32.  r holds one
 * value per row (r_rows == rows) or one value for every row (r_rows == 1).  bwd: grad_r (rows) receives the per-row dL/dr -- with
 * r_rows == 1 the contributions to be summed by the caller (hypad_column_sum at dim = 1), as hypad_mobius_pointwise_mul_bwd's grad_w;
 * grad_r and grad_x may each be NULL.  dim <= 256. */
int hypad_mobius_scalar_mul_fwd(const float* r, const float* x, float* out, int64_t rows, int dim, int64_t r_rows, hypad_stream_t stream);
int hypad_mobius_scalar_mul_bwd(const float* r, const float* x, const float* grad_out, float* grad_r, float* grad_x,
                                int64_t rows, int dim, int64_t r_rows, hypad_stream_t stream);
/* gmath.weighted_midpoint_bmm  math_.py:2090-2122 (_weighted_midpoint_bmm :2104-2122, _lambda_x :382-383, _project :340-352) at
 * k = -1: the weighted Moebius gyromidpoint in its attention / aggregation form.  xs (batch, M, D) on the ball, weights
 * (batch, N, M) of any sign, out (batch, N, D):
 *   gamma_j = 2 / max(1 - |x_j|^2, 1e-15)    t_i = sum_j w_ij gamma_j x_j / max(sum_j |w_ij| (gamma_j - 1), 1e-10)
 *   out_i = project(t_i / (1 + sqrt(1 - |t_i|^2))), with HYPAD_MID_LINCOMB project(mobius_scalar_mul(sum_j |w_ij|, .)).
 * One launch: fp32 MFMA products from an xs chunk staged and scaled in LDS (1 - |x_j|^2 from an fp64 sum), the epilogue in fp64
 * registers.  saved (batch, N, D + 2) receives [nom | den | alpha] for the backward (NULL: inference, the same bits in out).
 * bwd: a row pass over the batch N output rows, then grad_weights (contraction over D) and grad_xs (contraction over N) in one launch
 * each; either may be NULL and the other keeps its bits.  No atomics: two runs give the same bits.  N == 0 launches no row kernel and
 * writes zeros to grad_xs.  workspace (bwd only): hypad_weighted_midpoint_bmm_workspace_bytes = 4 batch N (D + 2) bytes.
 * Every argument is validated before anything is launched: HYPAD_EINVAL for a NULL operand, a non-positive size or an unknown flag;
 * HYPAD_EUNSUPPORTED for D > 256, an element count of 2^31 or more, or LDS that does not fit; HYPAD_EWORKSPACE below the workspace size. */
enum { HYPAD_MID_LINCOMB = 1, HYPAD_MID_POSWEIGHT = 2, HYPAD_MID_COADD = 4 };
size_t hypad_weighted_midpoint_bmm_workspace_bytes(int64_t batch, int64_t N, int64_t M, int D);
int hypad_weighted_midpoint_bmm_fwd(const float* xs, const float* weights, float* out, float* saved /* NULL: inference */,
                                    int64_t batch, int64_t N, int64_t M, int D, int flags, hypad_stream_t stream);
int hypad_weighted_midpoint_bmm_bwd(const float* xs, const float* weights, const float* saved, const float* grad_out,
                                    float* grad_xs, float* grad_weights, void* workspace, size_t workspace_bytes,
                                    int64_t batch, int64_t N, int64_t M, int D, int flags, hypad_stream_t stream);
/* gmath.weighted_midpoint  math_.py:1953-2087 (_weighted_midpoint :2027-2087, _antipode :1940-1950, clamp_abs of geoopt.utils) at
 * k = -1: the weighted Moebius gyromidpoint in its pooling form.  The host presents xs as (M, R, D): M reduced positions of R kept
 * rows; weights (M, R) (w_count = M R), one value (w_count = 1), or NULL (w_count = 0: every weight 1); out (R, D):
 *   t = sum_m w_m gamma_m x_m / (sum_m |w_m| (gamma_m - 1) + 1e-10)    out = t / (1 + sqrt(1 - |t|^2))
 * HYPAD_MID_COADD skips the halving; HYPAD_MID_LINCOMB skips it and applies mobius_scalar_mul(alpha / 2, .) with alpha = sum_m w_m;
 * HYPAD_MID_POSWEIGHT weighs the antipode -x_m with |w_m| where w_m < 0, which leaves t as it is and makes alpha = sum_m |w_m|.  No
 * project.  A wave per kept row adds up the positions in fp64 registers; where R alone leaves the device idle, M is cut into slices
 * -- their number a function of (M, R) alone -- whose partial sums a second launch adds in slice order.  saved (R, D + 2), fp64,
 * receives [nom | den | alpha] (NULL: inference, the same bits in out): with one point carrying a row, grad_weights is the small
 * difference of two large terms, which fp32 sums would leave no digits.
 * bwd: a pass over the R kept rows, then one element-wise launch over the M R rows writes grad_xs (M, R, D) and grad_weights -- (M, R),
 * or for a single weight the sum of the M R summands in a fixed order; either may be NULL (grad_weights must be NULL without
 * weights).  No atomics: two runs give the same bits.  R == 0 launches no row kernel and writes a zero to a single weight's gradient.
 * workspace: hypad_weighted_midpoint_workspace_bytes(M, R, D) at an 8-byte aligned address, for both calls (the forward touches it
 * only when it slices).
 * Every argument is validated before anything is launched: HYPAD_EINVAL for a NULL operand, a non-positive size, a w_count that is
 * none of the three or an unknown flag; HYPAD_EUNSUPPORTED for D > 256 or M R (D + 2) >= 2^31; HYPAD_EWORKSPACE below the workspace
 * size or off that alignment. */
size_t hypad_weighted_midpoint_workspace_bytes(int64_t M, int64_t R, int D);
int hypad_weighted_midpoint_fwd(const float* xs, const float* weights /* NULL: none */, int64_t w_count, float* out,
                                double* saved /* NULL: inference */, void* workspace, size_t workspace_bytes,
                                int64_t M, int64_t R, int D, int flags, hypad_stream_t stream);
int hypad_weighted_midpoint_bwd(const float* xs, const float* weights, int64_t w_count, const double* saved, const float* grad_out,
                                float* grad_xs, float* grad_weights, void* workspace, size_t workspace_bytes,
                                int64_t M, int64_t R, int D, int flags, hypad_stream_t stream);
/* gmath.dist_matmul  math_.py:905-947 (_dist_matmul :937-947; artan_k with the clamp of :57-59) at k = -1: the geodesic distance of
 * every x_i from every y_j, the score of a hyperbolic attention layer.  x (batch, N, D), y (batch, M, D) -- row-major points: the
 * caller transposes the reference's (batch, D, M) --, out and grad_out (batch, N, M):
 *   num = |x|^2 - 2 <x, y> + |y|^2    den = max(1 - 2 <x, y> + |x|^2 |y|^2, 1e-15)    out = 2 artanh(min(sqrt(max(num / den, 1e-15)), 1 - 1e-7))
 * One launch: <x, y> on fp32 MFMA from tiles staged in LDS, the norms as fp64 sums of the staged values, the epilogue in fp64
 * registers.  bwd: one fused launch per gradient (the pair terms are recomputed tile by tile: no N x M intermediate, no workspace);
 * grad_x or grad_y may be NULL and the other keeps its bits.  Nothing flows through a clamp that holds.  No atomics: two runs give the
 * same bits.  batch, N or M == 0 launches nothing and writes zeros to the gradients.
 * Every argument is validated before anything is launched: HYPAD_EINVAL for a NULL operand (x, y, out / grad_out) that has elements,
 * a negative batch, N or M, or D <= 0; HYPAD_EUNSUPPORTED for D > 256, an element count of 2^31 or more, or LDS that does not fit. */
int hypad_dist_matmul_fwd(const float* x, const float* y, float* out, int64_t batch, int64_t N, int64_t M, int D, hypad_stream_t stream);
int hypad_dist_matmul_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y,
                          int64_t batch, int64_t N, int64_t M, int D, hypad_stream_t stream);
/* gmath.dist2plane_matmul  math_.py:2125-2159 (_dist2plane_matmul :2136-2159) at k = -1: the reference's batched hyperplane read-out
 * in the operand layout of dist_matmul.  x (batch, N, D) on the ball, the planes' points p and normals z (batch, M, D) -- row-major:
 * the caller transposes the reference's (batch, D, M) --, out and grad_out (batch, N, M).  With zh = z / max(|z|, 1e-15),
 * bx = max(1 - |x|^2, 1e-15), bp = max(1 - |p|^2, 1e-15), alpha = 1 - 2 <x, p> + |x|^2:
 *   t = (2 / bp) (<x, zh> - (alpha / bx) <p, zh>)    out = 2 asinh(t) |z|
 * -- not 2 hypad_dist2plane(signed, scaled) of the same operands: the two agree only at x = 0.
 * One launch: <x, p> and <x, z> on fp32 MFMA from one staged x tile, the norms and <p, z> as fp64 sums of the staged values (1 - |x|^2
 * and 1 - |p|^2 come from those sums), the epilogue in fp64 registers.  bwd: one fused launch for grad_x, one for grad_p and grad_z
 * together (the pair terms are recomputed tile by tile: no N x M intermediate, no workspace); each gradient may be NULL and the others
 * keep their bits.  Nothing flows through a clamp that holds; a zero normal gives out = 0 and adds nothing to any gradient.  No
 * atomics: two runs give the same bits.  batch, N or M == 0 launches nothing and writes zeros to the gradients.
 * Every argument is validated before anything is launched: HYPAD_EINVAL for a NULL operand (x, p, z, out / grad_out) that has
 * elements, a negative batch, N or M, or D <= 0; HYPAD_EUNSUPPORTED for D > 256, an element count of 2^31 or more, or LDS that does
 * not fit. */
int hypad_dist2plane_matmul_fwd(const float* x, const float* p, const float* z, float* out, int64_t batch, int64_t N, int64_t M, int D,
                                hypad_stream_t stream);
int hypad_dist2plane_matmul_bwd(const float* x, const float* p, const float* z, const float* grad_out, float* grad_x, float* grad_p,
                                float* grad_z, int64_t batch, int64_t N, int64_t M, int D, hypad_stream_t stream);
/* gmath.dist  math_.py:861-902 (_dist :893-902, _mobius_add :536-555) at k = -1: 2 artanh(|(-x) (+) y|) of the rows of x and y
 * (rows, dim), out and grad_out (rows); the norm has no clamp, artanh clamps at 1 - 1e-7.  A wave per row in fp64 registers.  Two
 * rows that are equal element by element give distance 0 and gradient 0.  bwd: grad_x or grad_y may be NULL.
 * gmath.dist0  math_.py:950-975 (_dist0 :973-975): 2 artanh(|x|), the distance from the origin; an all-zero row gets gradient 0.
 * HYPAD_EINVAL for a NULL operand with rows > 0, rows < 0 or dim <= 0; HYPAD_EUNSUPPORTED for dim > 256; rows == 0 launches nothing. */
int hypad_dist_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_dist_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                   hypad_stream_t stream);
int hypad_dist0_fwd(const float* x, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_dist0_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, hypad_stream_t stream);
/* The tangent maps at a point of the ball, at k = -1, on rows (rows, dim) of fp32; c(x) = max(1 - |x|^2, 1e-15) = 2 / lambda_x:
 *   gmath.expmap  math_.py:1052-1102 (_expmap :1097-1102):  x (+) (tanh(min(n / c(x), 15)) u / n),  n = max(|u|, 1e-15)
 *   gmath.logmap  math_.py:1188-1230 (_logmap :1226-1230):  artanh(min(n, 1 - 1e-7)) c(x) w / n,  w = (-x) (+) y,  n = max(|w|, 1e-15)
 *   gmath.geodesic  math_.py:978-1049 (_geodesic :1042-1049):  x (+) (t (x) ((-x) (+) y)), (x) as hypad_mobius_scalar_mul_fwd;
 *     t holds t_count values: 1, or one per row
 *   gmath.gyration  math_.py:592-675 (_gyration :657-675):  u + 2 (A a + B b) / max(1 + 2 <a,b> + |a|^2 |b|^2, 1e-15),
 *     A = -<a,u> |b|^2 + <b,u> + 2 <a,b> <b,u>,  B = -<b,u> |a|^2 - <a,u>
 *   gmath.parallel_transport  math_.py:1669-1746 (_parallel_transport :1739-1746):  gyration(y, -x, v) c(y) / c(x)
 *   gmath.parallel_transport0  math_.py:1749-1779 (_parallel_transport0 :1776-1779):  v c(y)
 *   gmath.parallel_transport0back  math_.py:1782-1813 (_parallel_transport0back :1810-1813):  v / c(x)
 * One launch forward and one backward each, a wave per row in fp64 registers; the backward recomputes everything from the operands.
 * artanh is 0.5 (log1p(n) - log1p(-n)): at coincident points logmap and geodesic follow artanh(n) / n -> 1, where the reference's fp32
 * difference of two logarithms returns 0.  Nothing flows back through a clamp that holds; the norm's gradient at 0 is 0.
 * bwd: every gradient may be NULL and the others keep their bits.  grad_t (rows) receives the per-row dL/dt -- with t_count == 1 the
 * contributions to be summed by the caller (hypad_column_sum at dim = 1), as hypad_mobius_scalar_mul_bwd's grad_r.  No atomics, no
 * workspace: two runs give the same bits.
 * Every argument is validated before anything is launched: HYPAD_EINVAL for a NULL operand that has elements, rows < 0, dim <= 0 or a
 * t_count that is neither 1 nor rows; HYPAD_EUNSUPPORTED for dim > 256 or rows dim >= 2^31; rows == 0 launches nothing. */
int hypad_expmap_fwd(const float* x, const float* u, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_expmap_bwd(const float* x, const float* u, const float* grad_out, float* grad_x, float* grad_u, int64_t rows, int dim,
                     hypad_stream_t stream);
int hypad_logmap_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_logmap_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                     hypad_stream_t stream);
int hypad_geodesic_fwd(const float* t, const float* x, const float* y, float* out, int64_t rows, int dim, int64_t t_count,
                       hypad_stream_t stream);
int hypad_geodesic_bwd(const float* t, const float* x, const float* y, const float* grad_out, float* grad_t, float* grad_x, float* grad_y,
                       int64_t rows, int dim, int64_t t_count, hypad_stream_t stream);
int hypad_gyration_fwd(const float* a, const float* b, const float* u, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_gyration_bwd(const float* a, const float* b, const float* u, const float* grad_out, float* grad_a, float* grad_b, float* grad_u,
                       int64_t rows, int dim, hypad_stream_t stream);
int hypad_parallel_transport_fwd(const float* x, const float* y, const float* v, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_parallel_transport_bwd(const float* x, const float* y, const float* v, const float* grad_out, float* grad_x, float* grad_y,
                                 float* grad_v, int64_t rows, int dim, hypad_stream_t stream);
int hypad_parallel_transport0_fwd(const float* y, const float* v, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_parallel_transport0_bwd(const float* y, const float* v, const float* grad_out, float* grad_y, float* grad_v, int64_t rows, int dim,
                                  hypad_stream_t stream);
int hypad_parallel_transport0back_fwd(const float* x, const float* v, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_parallel_transport0back_bwd(const float* x, const float* v, const float* grad_out, float* grad_x, float* grad_v, int64_t rows,
                                      int dim, hypad_stream_t stream);
/* The rest of the gyrogroup and the Riemannian metric, at k = -1, on rows (rows, dim) of fp32, in the launch form of the tangent maps;
 * (+) is hypad_mobius_add_fwd's, c(x) = max(1 - |x|^2, 1e-15), lambda_x = 2 / c(x):
 *   gmath.mobius_sub  math_.py:558-589 (_mobius_sub :588-589):  x (+) (-y)
 *   gmath.mobius_coadd  math_.py:678-744 (_mobius_coadd :731-744):  ((1 - |y|^2) x + (1 - |x|^2) y) / max(1 - |x|^2 |y|^2, 1e-15)
 *   gmath.mobius_cosub  math_.py:747-779 (_mobius_cosub :778-779):  mobius_coadd(x, -y)
 *   gmath.geodesic_unit  math_.py:1139-1185 (_geodesic_unit :1175-1185):  x (+) (tanh(clamp(t / 2, +-15)) u / max(|u|, 1e-15));
 *     t holds t_count values: 1, or one per row
 *   gmath.egrad2rgrad  math_.py:1816-1845 (_egrad2rgrad :1844-1845):  grad / lambda_x^2
 * with one value per row for out and grad_out, (rows):
 *   gmath.lambda_x  math_.py:355-383 (_lambda_x :382-383):  lambda_x
 *   gmath.inner  math_.py:386-430 (_inner :420-430):  lambda_x^2 <u, v>
 *   gmath.norm  math_.py:433-472 (_norm :463-472):  lambda_x |u|, the Euclidean norm without a clamp
 * and between the ball, rows of dim elements, and the hyperboloid, rows of dim + 1 with the time-like coordinate last:
 *   gmath.sproj  math_.py:1848-1874 (_sproj :1870-1874):  h (rows, dim + 1) -> h[:dim] / (1 + h[dim]) (rows, dim), no clamp
 *   gmath.inv_sproj  math_.py:1877-1905 (_inv_sproj :1899-1905):  x (rows, dim) -> cat(lambda_x x, lambda_x - 1) (rows, dim + 1)
 * One launch forward and one backward each, a wave per row in fp64 registers; the backward recomputes everything from the operands.
 * Nothing flows back through a clamp that holds; the gradient of a Euclidean norm at 0 is 0.  bwd: every gradient may be NULL and the
 * others keep their bits.  grad_t (rows) receives the per-row dL/dt, as hypad_geodesic_bwd's.  No atomics, no workspace: two runs
 * give the same bits.
 * Every argument is validated before anything is launched: HYPAD_EINVAL for a NULL operand that has elements, rows < 0, dim <= 0 or a
 * t_count that is neither 1 nor rows; HYPAD_EUNSUPPORTED for dim > 256 (the projections: dim + 1 > 256) or rows dim >= 2^31 (the
 * projections: rows (dim + 1)); rows == 0 launches nothing. */
int hypad_mobius_sub_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_mobius_sub_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                         hypad_stream_t stream);
int hypad_mobius_coadd_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_mobius_coadd_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                           hypad_stream_t stream);
int hypad_mobius_cosub_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_mobius_cosub_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim,
                           hypad_stream_t stream);
int hypad_geodesic_unit_fwd(const float* t, const float* x, const float* u, float* out, int64_t rows, int dim, int64_t t_count,
                            hypad_stream_t stream);
int hypad_geodesic_unit_bwd(const float* t, const float* x, const float* u, const float* grad_out, float* grad_t, float* grad_x,
                            float* grad_u, int64_t rows, int dim, int64_t t_count, hypad_stream_t stream);
int hypad_lambda_x_fwd(const float* x, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_lambda_x_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, hypad_stream_t stream);
int hypad_inner_fwd(const float* x, const float* u, const float* v, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_inner_bwd(const float* x, const float* u, const float* v, const float* grad_out, float* grad_x, float* grad_u, float* grad_v,
                    int64_t rows, int dim, hypad_stream_t stream);
int hypad_norm_fwd(const float* x, const float* u, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_norm_bwd(const float* x, const float* u, const float* grad_out, float* grad_x, float* grad_u, int64_t rows, int dim,
                   hypad_stream_t stream);
int hypad_egrad2rgrad_fwd(const float* x, const float* grad, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_egrad2rgrad_bwd(const float* x, const float* grad, const float* grad_out, float* grad_x, float* grad_grad, int64_t rows, int dim,
                          hypad_stream_t stream);
int hypad_sproj_fwd(const float* h, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_sproj_bwd(const float* h, const float* grad_out, float* grad_h, int64_t rows, int dim, hypad_stream_t stream);
int hypad_inv_sproj_fwd(const float* x, float* out, int64_t rows, int dim, hypad_stream_t stream);
int hypad_inv_sproj_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, hypad_stream_t stream);
/* The 25 row-wise functions at any negative curvature k = -c, c finite and positive, on rows (rows, dim) of fp32 -- what
 * hyrnn_nets.PoincareBall(c) calls for c != 1 (docs/history/curvature.md).  Each hypad_ball_<name>_fwd / _bwd has the argument list of
 * hypad_<name>_fwd / _bwd plus `double c` before the stream, and computes math_.py's function of that name with k = -c:
 *   project :340-352, lambda_x :355-383, inner :386-430, norm :433-472, mobius_add :536-555, mobius_sub :558-589, gyration :592-675,
 *   mobius_coadd :678-744, mobius_cosub :747-779, mobius_scalar_mul :788-858, dist :861-902, dist0 :950-975, geodesic :978-1049,
 *   expmap :1052-1102, expmap0 :1105-1136, geodesic_unit :1139-1185, logmap :1188-1230, logmap0 :1233-1270, mobius_pointwise_mul
 *   :1328-1371, parallel_transport :1669-1746, parallel_transport0 :1749-1779, parallel_transport0back :1782-1813, egrad2rgrad
 *   :1816-1845, sproj :1848-1874, inv_sproj :1877-1905.
 * With s = sqrt(c), x -> s x takes the ball of radius 1 / s onto the unit ball and every one of these functions at -c onto itself at
 * -1, clamps included (artanh at 1 - 1e-7, tanh at 15, max(1 + k |x|^2, 1e-15), project's radius (1 - 4e-3) / s):
 *   f_c(a_0, a_1, ...) = s^eo f_1(s^e0 a_0, s^e1 a_1, ...)
 * with exponents (e0, e1, ... -> eo):
 *   project, expmap0, logmap0, dist0, sproj, inv_sproj                                  1 -> -1
 *   mobius_add, mobius_sub, mobius_coadd, mobius_cosub, dist, logmap, expmap            1, 1 -> -1
 *   mobius_scalar_mul (r, x), mobius_pointwise_mul (w, x)                               0, 1 -> -1
 *   geodesic (t, x, y)                                                                  0, 1, 1 -> -1
 *   geodesic_unit (t, x, u)                                                             1, 1, 0 -> -1
 *   gyration (a, b, u), parallel_transport (x, y, v)                                    1, 1, 0 -> 0
 *   parallel_transport0 (y, v), parallel_transport0back (x, v), norm (x, u), egrad2rgrad (x, grad)   1, 0 -> 0
 *   lambda_x (x)  1 -> 0;   inner (x, u, v)  1, 0, 0 -> 0
 * and f_1 the k = -1 function documented above (sproj and inv_sproj with inv_r = sqrt(c) for the reference's sqrt(|k| + 1e-15)).  The
 * backward is the chain rule through the factors: grad_out times s^eo going in, each operand's gradient times its s^e coming out.
 * The kernels are those of the k = -1 entry points -- a wave per row in fp64 registers, operands scaled after the load and the result
 * before the store, the backward recomputed from the operands, no atomics, no workspace --, so c = 1.0 returns the bits of
 * hypad_<name>_*.  project, expmap0, logmap0, mobius_add, mobius_pointwise_mul, mobius_scalar_mul, dist and dist0, whose k = -1 entry
 * points are older kernels, run in this launch form too: within rounding of those at c = 1.0, and without their one-row broadcast
 * (every row operand is (rows, dim); r of mobius_scalar_mul holds r_rows values, 1 or one per row, as t_count).
 * Validation and return codes as hypad_<name>_*'s, after HYPAD_EINVAL for a c that is not finite and positive.  bwd: every gradient may
 * be NULL and the others keep their bits. */
int hypad_ball_expmap_fwd(const float* x, const float* u, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_expmap_bwd(const float* x, const float* u, const float* grad_out, float* grad_x, float* grad_u, int64_t rows, int dim, double c,
                          hypad_stream_t stream);
int hypad_ball_logmap_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_logmap_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, double c,
                          hypad_stream_t stream);
int hypad_ball_geodesic_fwd(const float* t, const float* x, const float* y, float* out, int64_t rows, int dim, int64_t t_count, double c,
                            hypad_stream_t stream);
int hypad_ball_geodesic_bwd(const float* t, const float* x, const float* y, const float* grad_out, float* grad_t, float* grad_x, float* grad_y,
                            int64_t rows, int dim, int64_t t_count, double c, hypad_stream_t stream);
int hypad_ball_gyration_fwd(const float* a, const float* b, const float* u, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_gyration_bwd(const float* a, const float* b, const float* u, const float* grad_out, float* grad_a, float* grad_b, float* grad_u,
                            int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_parallel_transport_fwd(const float* x, const float* y, const float* v, float* out, int64_t rows, int dim, double c,
                                      hypad_stream_t stream);
int hypad_ball_parallel_transport_bwd(const float* x, const float* y, const float* v, const float* grad_out, float* grad_x, float* grad_y,
                                      float* grad_v, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_parallel_transport0_fwd(const float* y, const float* v, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_parallel_transport0_bwd(const float* y, const float* v, const float* grad_out, float* grad_y, float* grad_v, int64_t rows, int dim,
                                       double c, hypad_stream_t stream);
int hypad_ball_parallel_transport0back_fwd(const float* x, const float* v, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_parallel_transport0back_bwd(const float* x, const float* v, const float* grad_out, float* grad_x, float* grad_v, int64_t rows,
                                           int dim, double c, hypad_stream_t stream);
int hypad_ball_mobius_sub_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_mobius_sub_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, double c,
                              hypad_stream_t stream);
int hypad_ball_mobius_coadd_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_mobius_coadd_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, double c,
                                hypad_stream_t stream);
int hypad_ball_mobius_cosub_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_mobius_cosub_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, double c,
                                hypad_stream_t stream);
int hypad_ball_geodesic_unit_fwd(const float* t, const float* x, const float* u, float* out, int64_t rows, int dim, int64_t t_count, double c,
                                 hypad_stream_t stream);
int hypad_ball_geodesic_unit_bwd(const float* t, const float* x, const float* u, const float* grad_out, float* grad_t, float* grad_x, float* grad_u,
                                 int64_t rows, int dim, int64_t t_count, double c, hypad_stream_t stream);
int hypad_ball_lambda_x_fwd(const float* x, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_lambda_x_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_inner_fwd(const float* x, const float* u, const float* v, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_inner_bwd(const float* x, const float* u, const float* v, const float* grad_out, float* grad_x, float* grad_u, float* grad_v,
                         int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_norm_fwd(const float* x, const float* u, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_norm_bwd(const float* x, const float* u, const float* grad_out, float* grad_x, float* grad_u, int64_t rows, int dim, double c,
                        hypad_stream_t stream);
int hypad_ball_egrad2rgrad_fwd(const float* x, const float* grad, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_egrad2rgrad_bwd(const float* x, const float* grad, const float* grad_out, float* grad_x, float* grad_grad, int64_t rows, int dim,
                               double c, hypad_stream_t stream);
int hypad_ball_sproj_fwd(const float* h, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_sproj_bwd(const float* h, const float* grad_out, float* grad_h, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_inv_sproj_fwd(const float* x, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_inv_sproj_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_project_fwd(const float* x, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_project_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_expmap0_fwd(const float* u, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_expmap0_bwd(const float* u, const float* grad_out, float* grad_u, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_logmap0_fwd(const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_logmap0_bwd(const float* y, const float* grad_out, float* grad_y, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_mobius_add_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_mobius_add_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, double c,
                              hypad_stream_t stream);
int hypad_ball_mobius_pointwise_mul_fwd(const float* w, const float* x, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_mobius_pointwise_mul_bwd(const float* w, const float* x, const float* grad_out, float* grad_w, float* grad_x, int64_t rows, int dim,
                                        double c, hypad_stream_t stream);
int hypad_ball_mobius_scalar_mul_fwd(const float* r, const float* x, float* out, int64_t rows, int dim, int64_t r_rows, double c,
                                     hypad_stream_t stream);
int hypad_ball_mobius_scalar_mul_bwd(const float* r, const float* x, const float* grad_out, float* grad_r, float* grad_x, int64_t rows, int dim,
                                     int64_t r_rows, double c, hypad_stream_t stream);
int hypad_ball_dist_fwd(const float* x, const float* y, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_dist_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t rows, int dim, double c,
                        hypad_stream_t stream);
int hypad_ball_dist0_fwd(const float* x, float* out, int64_t rows, int dim, double c, hypad_stream_t stream);
int hypad_ball_dist0_bwd(const float* x, const float* grad_out, float* grad_x, int64_t rows, int dim, double c, hypad_stream_t stream);
/* gmath.hyperbolic_attention: the composition of dist_matmul (math_.py:905-947), a softmax over the keys and weighted_midpoint_bmm
 * without lincomb (math_.py:2090-2122) at k = -1, with no N x M tensor in memory.  q (batch, N, D), keys (batch, M, D), values
 * (batch, M, E) on the ball, out and grad_out (batch, N, E); bias NULL or fp32 (N, M) per batch element at bias_batch_stride elements
 * (N M, or 0: one bias shared by every batch element), -inf masks a pair; beta by value:
 *   s_ij = -beta d(q_i, keys_j) + bias_ij    p_ij = softmax_j s_ij    out_i = the gyromidpoint of the values under p_i.
 * A row whose every s_ij is -inf gives out_i = 0 and adds nothing to any gradient (the composition gives NaN).
 * fwd: one launch, a workgroup per 16 query rows walks keys and values in chunks of 64 (16 a wave) with a running maximum; products on
 * fp32 MFMA, distances, exponentials and the epilogue in fp64 registers.  saved (batch, N, E + 1) = [nom | den] and lse (batch, N) = L are written
 * for the backward; both NULL: inference, the same bits in out.
 * bwd: a row pass into the workspace (hypad_hyp_attention_workspace_bytes = 4 batch N (E + 2) bytes), one launch for grad_q, one for
 * grad_keys and grad_values; p is recomputed from L.  Each gradient may be NULL and the others keep their bits.  No atomics: two runs give
 * the same bits.  batch == 0 or N == 0 launches nothing; the backward then writes zeros to grad_keys and grad_values.
 * Every argument is validated before anything is launched: HYPAD_EINVAL for a NULL operand that has elements, a negative size, D or
 * E <= 0, M == 0 with N > 0, a bias stride that is neither, saved without lse, or a beta that is not finite; HYPAD_EUNSUPPORTED for D or
 * E > 128, 2^31 or more pairs, or LDS that does not fit; HYPAD_EWORKSPACE below the workspace size. */
size_t hypad_hyp_attention_workspace_bytes(int64_t batch, int64_t N, int64_t M, int D, int E);
int hypad_hyp_attention_fwd(const float* q, const float* keys, const float* values, const float* bias /* NULL: none */,
                            int64_t bias_batch_stride, double beta, float* out, float* saved /* NULL: inference */, float* lse,
                            int64_t batch, int64_t N, int64_t M, int D, int E, hypad_stream_t stream);
int hypad_hyp_attention_bwd(const float* q, const float* keys, const float* values, const float* bias, int64_t bias_batch_stride,
                            double beta, const float* saved, const float* lse, const float* grad_out, float* grad_q, float* grad_keys,
                            float* grad_values, void* workspace, size_t workspace_bytes, int64_t batch, int64_t N, int64_t M, int D, int E,
                            hypad_stream_t stream);
/* dist_matmul, weighted_midpoint_bmm, weighted_midpoint and the attention above at any negative curvature k = -c, c > 0 and finite: what
 * the matmul methods of hyrnn_nets.PoincareBall(c) run (docs/history/curvature_matmul.md).  Each has the arguments of the entry point
 * hypad_<name>_* plus `c` before the stream, the same kernels with c in their fp64 stages only (no operand tile is scaled), the same
 * validation and return codes after HYPAD_EINVAL for a c that is not finite and positive -- c is checked first --, and the same
 * workspace: the hypad_*_workspace_bytes functions above serve both.  With s = sqrt(c), the reference's formulas at k = -c:
 *   dist_matmul   num = x2 - 2 xy + y2    den = max(1 - 2 c xy + c^2 x2 y2, 1e-15)    u = max(num / den, 1e-15)
 *                 out = (2 / s) artanh(min(s sqrt(u), 1 - 1e-7))
 *   midpoints     gamma_j = 2 / max(1 - c |x_j|^2, 1e-15);  nom, den, alpha and den' (its 1e-10) as at k = -1;  t = nom / den'
 *                 a = t / (1 + sqrt(1 - c |t|^2))    lincomb: a = tanh(r artanh(s |a|)) a / (s |a|), r = alpha (bmm), alpha / 2 (reduce)
 *                 bmm and attention: project onto the radius (1 - 4e-3) / s;  the reduce form does not project
 *   attention     softmax_j(-beta d_c(q_i, keys_j) + bias_ij), then the bmm midpoint of the values without lincomb; a fully masked row
 *                 gives the origin and adds nothing to any gradient
 * The floors 1e-15 under u, under a length and under 1 - c |x|^2 sit on the unscaled quantities, so these are not everywhere the k = -1
 * functions on operands times s: a coincident pair is at distance (2 / s) artanh(s sqrt(1e-15)) = 6.3e-8 for every c.  Where a clamp holds
 * nothing flows back through it, as at k = -1.  c = 1.0 is within rounding of hypad_<name>_*, not its bits. */
int hypad_ball_dist_matmul_fwd(const float* x, const float* y, float* out, int64_t batch, int64_t N, int64_t M, int D, double c,
                               hypad_stream_t stream);
int hypad_ball_dist_matmul_bwd(const float* x, const float* y, const float* grad_out, float* grad_x, float* grad_y, int64_t batch, int64_t N,
                               int64_t M, int D, double c, hypad_stream_t stream);
int hypad_ball_weighted_midpoint_bmm_fwd(const float* xs, const float* weights, float* out, float* saved /* NULL: inference */, int64_t batch,
                                         int64_t N, int64_t M, int D, int flags, double c, hypad_stream_t stream);
int hypad_ball_weighted_midpoint_bmm_bwd(const float* xs, const float* weights, const float* saved, const float* grad_out, float* grad_xs,
                                         float* grad_weights, void* workspace, size_t workspace_bytes, int64_t batch, int64_t N, int64_t M,
                                         int D, int flags, double c, hypad_stream_t stream);
int hypad_ball_weighted_midpoint_fwd(const float* xs, const float* weights /* NULL: none */, int64_t w_count, float* out,
                                     double* saved /* NULL: inference */, void* workspace, size_t workspace_bytes, int64_t M, int64_t R, int D,
                                     int flags, double c, hypad_stream_t stream);
int hypad_ball_weighted_midpoint_bwd(const float* xs, const float* weights, int64_t w_count, const double* saved, const float* grad_out,
                                     float* grad_xs, float* grad_weights, void* workspace, size_t workspace_bytes, int64_t M, int64_t R, int D,
                                     int flags, double c, hypad_stream_t stream);
int hypad_ball_hyp_attention_fwd(const float* q, const float* keys, const float* values, const float* bias /* NULL: none */,
                                 int64_t bias_batch_stride, double beta, float* out, float* saved /* NULL: inference */, float* lse,
                                 int64_t batch, int64_t N, int64_t M, int D, int E, double c, hypad_stream_t stream);
int hypad_ball_hyp_attention_bwd(const float* q, const float* keys, const float* values, const float* bias, int64_t bias_batch_stride,
                                 double beta, const float* saved, const float* lse, const float* grad_out, float* grad_q, float* grad_keys,
                                 float* grad_values, void* workspace, size_t workspace_bytes, int64_t batch, int64_t N, int64_t M, int D, int E,
                                 double c, hypad_stream_t stream);
/* The Moebius GRU hyperspace/hyrnn_nets.py:61-151 (one_rnn_transform :61-65, mobius_gru_cell :68-91, the equal-length branch of
 * mobius_gru_loop :113-127) at k = -1.  x (steps, rows, in_dim) and h0 (rows, hidden) on the ball, w_ih (3 hidden, in_dim),
 * w_hh (3 hidden, hidden), bias (3, hidden) on the ball, chunk order r, h, z; out (steps, rows, hidden) = the hidden state after
 * every step (the last one is h_last); no project anywhere, as in the reference.  steps = 1 is the cell.  nonlin: HYPAD_NONLIN_*
 * on h~ (:87-88).  Forward: one GEMM for x W_ih^T of all steps and ONE launch for the recurrence; the row chains run in fp64
 * registers, every buffer and every MFMA product is fp32.  saved (steps, rows, 6 hidden) receives the products
 * [mx_r | mx_h | mx_z | mh_r | mh_z | m_rh] for the backward (NULL: inference).
 * bwd: one persistent launch walks the steps in reverse, then dense contractions over steps * rows rows.  grad_out
 * (steps, rows, hidden); grad_h_last (rows, hidden) is added to the last step's (NULL: none); grad_x, grad_h0, grad_w_ih, grad_w_hh
 * and grad_bias may each be NULL.  No atomics: two runs give the same bits.  rows == 0 launches no row kernel and writes zero
 * parameter gradients (the row buffers and the workspace may then be NULL).
 * workspace: hypad_mobius_gru_workspace_bytes(steps, rows, in_dim, hidden) = 4 steps rows (14 hidden + 1) bytes, for both calls.
 * Every argument is validated before anything is launched: HYPAD_EINVAL for a NULL operand, a non-positive size or an unknown
 * nonlin; HYPAD_EUNSUPPORTED for in_dim or hidden > 256, steps * rows >= 2^31, or LDS that does not fit (also where
 * hypad_linear_act_fwd / _bwd refuse 3 hidden outputs); HYPAD_EWORKSPACE below the workspace size. */
size_t hypad_mobius_gru_workspace_bytes(int steps, int64_t rows, int in_dim, int hidden);
int hypad_mobius_gru_fwd(const float* x, const float* h0, const float* w_ih, const float* w_hh, const float* bias, float* out,
                         float* saved /* NULL: inference */, void* workspace, size_t workspace_bytes,
                         int steps, int64_t rows, int in_dim, int hidden, int nonlin, hypad_stream_t stream);
int hypad_mobius_gru_bwd(const float* x, const float* h0, const float* w_ih, const float* w_hh, const float* bias, const float* out,
                         const float* saved, const float* grad_out, const float* grad_h_last /* NULL: none */,
                         float* grad_x, float* grad_h0, float* grad_w_ih, float* grad_w_hh, float* grad_bias,
                         void* workspace, size_t workspace_bytes,
                         int steps, int64_t rows, int in_dim, int hidden, int nonlin, hypad_stream_t stream);
/* inline row-wise Poincare distance  train.py:226-230; utils/anomaly_detection_utils.py:58-66,167-175 */
int hypad_poincare_rowdist_fwd(const float* u, const float* v, float* dist, int64_t rows, int dim, hypad_stream_t stream);
int hypad_poincare_rowdist_bwd(const float* u, const float* v, const float* grad_dist, float* grad_u, float* grad_v,
                               int64_t rows, int dim, hypad_stream_t stream);
/* hyperbolic reconstruction loss  train.py:226-232: loss[0] = sum_r dist(u_r, v_r) / batch.
 * bwd: gradients of (grad_loss * loss) w.r.t. u and v. */
int hypad_hyper_loss_fwd(const float* u, const float* v, float* loss, int64_t rows, int dim, int batch, hypad_stream_t stream);
int hypad_hyper_loss_bwd(const float* u, const float* v, float grad_loss, float* grad_u, float* grad_v,
                         int64_t rows, int dim, int batch, hypad_stream_t stream);
/* pair-wise distance  hyperspace/poincare_distance.py:5-16 (+ :19-25, :28-48): out (n, m) */
int hypad_poincare_pairdist_fwd(const float* pred, const float* gt, float* out, int n, int m, int dim, hypad_stream_t stream);
/* out[c] = sum_r in[r][c] */
int hypad_column_sum(const float* in, float* out, int64_t rows, int dim, hypad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dense building blocks (torch ATen calls of the reference: F.linear, nn.LSTM at T=1).
 * ---------------------------------------------------------------------------------------------- */
enum { HYPAD_ACT_NONE = 0, HYPAD_ACT_TANH = 1, HYPAD_ACT_LEAKY02 = 2 };
/* y = act(x W^T + b): nn.Linear + nn.Tanh / nn.LeakyReLU(0.2)  models/tadgan.py:21,34,39,40,77-89.  rows == 0 launches nothing (x and y
 * may then be NULL). */
int hypad_linear_act_fwd(const float* x, const float* weight, const float* bias, float* y,
                         int64_t rows, int in_dim, int out_dim, int act, hypad_stream_t stream);
/* grad_x = (grad_y * act'(y)) W ; grad_w = (grad_y * act')^T x ; grad_b = colsum(grad_y * act').  y = forward output.
 * grad_x, grad_weight, grad_bias and grad_pre_scratch may each be NULL (not computed); grad_weight needs x and grad_pre_scratch, and
 * grad_bias needs grad_weight: every argument is validated before anything is launched or written.  rows == 0 (the row buffers may
 * then be NULL) writes zeros to grad_weight and grad_bias on `stream`. */
int hypad_linear_act_bwd(const float* x, const float* weight, const float* y, const float* grad_y,
                         float* grad_x, float* grad_weight, float* grad_bias, float* grad_pre_scratch,
                         int64_t rows, int in_dim, int out_dim, int act, hypad_stream_t stream);
/* One bidirectional LSTM layer at seq_len 1 with h0 = c0 = 0 (models/tadgan.py:15-20,35-37 as driven by
 * :24-25,59-60): out (rows, 2*hidden) = [h_fwd | h_rev].  w_ih_* (4*hidden, in_dim) with
 * PyTorch gate order [i,f,g,o]; W_hh cannot influence the result and is not read.
 * gates_save (rows, 2, 4, hidden) receives (i, g, o, tanh(c)) for the backward (may be NULL).  rows == 0 launches nothing (x and out
 * may then be NULL). */
int hypad_lstm_bidir_fwd(const float* x, const float* w_ih_f, const float* b_ih_f, const float* b_hh_f,
                         const float* w_ih_r, const float* b_ih_r, const float* b_hh_r,
                         float* out, float* gates_save, int64_t rows, int in_dim, int hidden, hypad_stream_t stream);
/* grad_gates (rows, 2, 4*hidden) pre-activation gradients in PyTorch gate order (f block zero);
 * grad_x (rows, in_dim); parameter gradients follow as grad_gates^T x (hypad_linear weight rule).  rows == 0 launches nothing (the
 * row buffers may then be NULL). */
int hypad_lstm_bidir_bwd(const float* w_ih_f, const float* w_ih_r, const float* gates_saved, const float* grad_out,
                         float* grad_gates, float* grad_x, int64_t rows, int in_dim, int hidden, hypad_stream_t stream);

/* The same layer over seq_len time steps -- torch.nn.LSTM(in_dim, hidden, num_layers=1, bidirectional=True) on a (seq_len, rows,
 * in_dim) input, with W_hh and optional initial states (the module models/tadgan.py:15-20, :35-38 builds; the reference itself
 * always feeds it seq_len = 1, where hypad_lstm_bidir_fwd is the faster form).  x (seq_len, rows, in_dim); w_ih_* (4*hidden,
 * in_dim), w_hh_* (4*hidden, hidden), biases (4*hidden), PyTorch gate order [i,f,g,o]; h0 / c0 (2, rows, hidden) or NULL = zeros;
 * out (seq_len, rows, 2*hidden) = [h_fwd(t) | h_rev(t)]; hn / cn (2, rows, hidden) final states, may be NULL.  The input
 * projections of all steps run as one MFMA GEMM; the recurrence is a persistent kernel per (16-row tile, direction): W_hh in
 * LDS, h_t in LDS, c_t in registers, the four gates of a unit on one lane, one barrier per step.  hidden <= 64.
 * workspace: hypad_lstm_seq_workspace_bytes(seq_len, rows, hidden).  rows == 0 launches nothing: the row buffers and the
 * (zero-byte) workspace may then be NULL. */
size_t hypad_lstm_seq_workspace_bytes(int seq_len, int64_t rows, int hidden);
int hypad_lstm_bidir_seq_fwd(const float* x, const float* w_ih_f, const float* w_hh_f, const float* b_ih_f, const float* b_hh_f,
                             const float* w_ih_r, const float* w_hh_r, const float* b_ih_r, const float* b_hh_r,
                             const float* h0, const float* c0, float* out, float* hn, float* cn, int seq_len, int64_t rows,
                             int in_dim, int hidden, void* workspace, size_t workspace_bytes, hypad_stream_t stream);
/* The training form and its back-propagation through time (ABI 7) -- what autograd gives the nn.LSTM modules of
 * models/tadgan.py:15-27, 35-38 at any seq_len.  fwd_train = the forward above that also fills
 *   saved (seq_len, rows, 2, 5, hidden) = per (step, row, direction) [i | f | g | o | c]: gate activations and cell state.
 * bwd: grad_out (seq_len, rows, 2*hidden), grad_hn / grad_cn (2, rows, hidden) -- any of the three may be NULL (= zeros), not all;
 *   grad_x (seq_len, rows, in_dim); grad_w_ih_* (4*hidden, in_dim); grad_w_hh_* (4*hidden, hidden); grad_b_* (4*hidden) = the
 *   gradient of b_ih_* AND of b_hh_* (they enter as a sum); grad_h0 / grad_c0 (2, rows, hidden) may be NULL.  h0 / c0 / out as
 *   the forward took / returned them.  A persistent kernel per (16-row tile, direction) walks the steps in reverse (W_hh^T in
 *   LDS, carried dh / dc in registers, one barrier per step) and writes the pre-activation gradients of every step; the
 *   parameter / input gradients are dense contractions over seq_len * rows rows (hypad_linear_act_bwd).  hidden <= 64.
 * workspace: hypad_lstm_seq_bwd_workspace_bytes(seq_len, rows, in_dim, hidden).  rows == 0: fwd_train writes nothing, bwd writes
 *   zeros to the six parameter gradients on the caller's stream; row buffers and workspace may be NULL. */
int hypad_lstm_bidir_seq_fwd_train(const float* x, const float* w_ih_f, const float* w_hh_f, const float* b_ih_f, const float* b_hh_f,
                                   const float* w_ih_r, const float* w_hh_r, const float* b_ih_r, const float* b_hh_r,
                                   const float* h0, const float* c0, float* out, float* hn, float* cn, float* saved, int seq_len,
                                   int64_t rows, int in_dim, int hidden, void* workspace, size_t workspace_bytes, hypad_stream_t stream);
size_t hypad_lstm_seq_bwd_workspace_bytes(int seq_len, int64_t rows, int in_dim, int hidden);
int hypad_lstm_bidir_seq_bwd(const float* x, const float* w_ih_f, const float* w_hh_f, const float* w_ih_r, const float* w_hh_r,
                             const float* h0, const float* c0, const float* out, const float* saved, const float* grad_out,
                             const float* grad_hn, const float* grad_cn, float* grad_x, float* grad_w_ih_f, float* grad_w_hh_f,
                             float* grad_b_f, float* grad_w_ih_r, float* grad_w_hh_r, float* grad_b_r, float* grad_h0, float* grad_c0,
                             int seq_len, int64_t rows, int in_dim, int hidden, void* workspace, size_t workspace_bytes,
                             hypad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Networks, forward (eval or train-mode dropout).  `params` = arena of that network.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hypad_dropout {
  int train_mode;        /* 0: eval (no dropout).  1: dropout active as after .train() */
  const float* masks;    /* optional injected masks holding 0 or 1/(1-p); layout stated per function */
  uint64_t seed;         /* used when train_mode && !masks: device Philox4x32-10 */
  uint64_t offset;       /* Philox stream offset (e.g. an iteration counter) */
} hypad_dropout;

/* Encoder.forward  models/tadgan.py:23-27: x (rows, S) -> (rows, L) */
int hypad_encoder_fwd(const float* params, const float* x, float* out, int64_t rows, int signal_shape,
                      int latent_dim, hypad_stream_t stream);
/* Decoder.forward  models/tadgan.py:58-67: z (rows, L) -> eucl (rows, S) and, if hyperbolic, hyper (rows, S).
 * dropout mask layout: (rows, 128) inter-layer LSTM mask (p = 0.2). */
int hypad_decoder_fwd(const float* params, const float* z, float* hyper_out, float* eucl_out, int64_t rows,
                      int signal_shape, int latent_dim, int hyperbolic, const hypad_dropout* drop, hypad_stream_t stream);
/* CriticX.forward  models/tadgan.py:91-106: x (rows, S) -> (rows,).  masks: 4 x (rows, L), p = 0.25 */
int hypad_critic_x_fwd(const float* params, const float* x, float* out, int64_t rows, int signal_shape,
                       int latent_dim, const hypad_dropout* drop, hypad_stream_t stream);
/* CriticZ.forward  models/tadgan.py:123-132: z (rows, L) -> (rows,).  masks: 2 x (rows, L), p = 0.2 */
int hypad_critic_z_fwd(const float* params, const float* z, float* out, int64_t rows, int latent_dim,
                       const hypad_dropout* drop, hypad_stream_t stream);
/* test_tadgan batch body  anomaly_detection.py:67-113 (eval mode), fused: for every window row
 *   lat = Encoder(x); (hyper, eucl) = Decoder(lat); hyper_real = hyperbolic_linear(x); critic = CriticX(x);
 *   rowdist = poincare distance(hyper_real, hyper)  (utils/anomaly_detection_utils.py:58-66).
 * Any output pointer may be NULL (that output is then not written).  Euclidean mode: recon = eucl only. */
/* The same on the training kernels' machinery (MFMA-native packed weights built into `workspace` by the call, LSTM cells in
 * the gate products' epilogues, 512 threads per 16 windows): ~4x the rate of hypad_score_forward at large `rows`.
 * x_row_stride: 0 / S = window matrix, 1 = x is the scaled series and window n is x[n .. n+S) (no matrix at all); any other
 *   stride in floats up to 2^24 (a tile's rows are addressed with 32-bit byte offsets: 16 rows x 2^24 floats x 4 bytes): a larger
 *   one returns HYPAD_EUNSUPPORTED (hypad_score_forward takes contiguous rows only; gather such rows first).
 * Which tile form runs (16 or 32 windows per workgroup; the latter from 65 536 windows on, window 100 / latent 20 only) depends on
 *   the arguments alone and changes no result bit.
 * workspace: hypad_score_workspace_bytes(S, L, hyperbolic). */
size_t hypad_score_workspace_bytes(int signal_shape, int latent_dim, int hyperbolic);
int hypad_score_forward_packed(const float* enc, const float* dec, const float* cx, const float* x, int64_t x_row_stride,
                               float* hyper, float* eucl, float* hyper_real, float* critic, float* rowdist, int64_t rows,
                               int signal_shape, int latent_dim, int hyperbolic, void* workspace, size_t workspace_bytes,
                               hypad_stream_t stream);
int hypad_score_forward(const float* enc, const float* dec, const float* cx, const float* x,
                        float* hyper, float* eucl, float* hyper_real, float* critic, float* rowdist,
                        int64_t rows, int signal_shape, int latent_dim, int hyperbolic, hypad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Training iterations (train.py:18-104, :107-186, :189-249) with the optimizer step fused in
 * (torch.optim.Adam train.py:274-281; geoopt RiemannianAdam train.py:282-288).
 * ---------------------------------------------------------------------------------------------- */
typedef struct hypad_dims {
  int signal_shape;  /* params.signal_shape */
  int latent_dim;    /* params.latent_space_dim (train.py:413) */
  int batch;         /* params.batch_size; multiple of 16 */
  int hyperbolic;    /* params.hyperbolic */
  int n_signals;     /* independent models trained side by side (one per signal); >= 1 */
  int first_signal;  /* ABI 5: model s of this call draws its device random streams (latent vectors, interpolation weights, dropout)
                        as stream first_signal + s.  A signal's training then does not depend on which models share its launches:
                        model k of a group whose first_signal is f == a single model trained with first_signal = f + k, bit for bit
                        (hypad_amd.train.train_signals_resident: one model per signal, train.py:428-437).  0 = streams 0 .. n_signals-1 */
} hypad_dims;

typedef struct hypad_nets { float *enc, *dec, *cx, *cz; } hypad_nets;

typedef struct hypad_train_state {
  hypad_nets params;       /* signal s of a net at base + s * hypad_param_count(net) */
  hypad_nets exp_avg;      /* Adam first moment, same layout */
  hypad_nets exp_avg_sq;   /* Adam second moment */
  int32_t* counters;       /* device int32[8]: [0..2] optimizer steps taken by {critic_x, critic_z, generator}, [3] rng ticks,
                              [4] STATUS of hypad_train_epoch's resident critic launch (0 = fine; otherwise the code of the first
                              bounded wait that gave up, see hypad_epoch_status), [5] how many critics of the last hypad_train_epoch's resident
                              launch had all their chunk workgroups on one XCD (a speed matter only), [6..7] reserved (zero) */
  float lr, beta1, beta2, eps;
  float gen_weight_decay;  /* hyperbolic generator optimizer: 1e-5 (train.py:286); ignored otherwise */
  int gen_stabilize;       /* 10 (train.py:287) */
} hypad_train_state;

typedef struct hypad_iter_io {
  const float* x;            /* window matrix resident in HBM: (n_signals, n_windows, S) fp32 */
  int64_t x_signal_stride;   /* floats between signals */
  int64_t x_row_stride;      /* floats between consecutive window rows of x: 0 or signal_shape = a dense (n_windows,
                                signal_shape) matrix; 1 = x is the scaled series itself and window n is x[n .. n + signal_shape)
                                (utils/dataloader.py:139-222 materialises exactly that sliding view) */
  const int32_t* row_index;  /* (batch) rows of x forming this minibatch (shared by all signals); NULL = 0..batch-1 */
  const float* z;            /* injected N(0,1) latent draw (n_signals, batch, L) or NULL = device Philox (train.py:24,118,205) */
  const float* alpha;        /* injected U(0,1) interpolation weights (n_signals, batch, S or L) or NULL (train.py:64,149) */
  hypad_dropout drop;        /* masks layout per signal:  critic_x_iteration: valid 4x(B,L) | fake 4x(B,L) | interpolated 4x(B,L) | decoder (B,128)
                                                          critic_z_iteration: fake 2x(B,L) | valid 2x(B,L) | interpolated 2x(B,L)
                                                          decoder_iteration : critic_z 2x(B,L) | critic_x 4x(B,L) | decoder(z) (B,128) | decoder(enc(x)) (B,128) */
  float* losses;             /* device out (n_signals, 4): [loss, aux (hyper_loss or mse), mean critic term a, mean critic term b] */
  void* workspace;
  size_t workspace_bytes;    /* >= hypad_train_workspace_bytes(dims) */
} hypad_iter_io;

size_t hypad_train_workspace_bytes(const hypad_dims* dims);
/* The training workspace also holds MFMA-native packed copies of the generator's weights (blocks of 16 output rows x 16
 * reduction columns laid out as the matrix cores consume them; forward and transposed).  The library builds them itself
 * (every hypad_decoder_iteration call; once per hypad_train_epoch, whose dW + Adam kernel then keeps them current), so
 * callers never need these two: hypad_pack_generator rebuilds the copies of every signal from the parameter arenas,
 * hypad_packed_region reports where they are (floats from the start of a signal's workspace slice, slice stride and
 * count) -- for tests and tools. */
int hypad_pack_generator(const hypad_dims* dims, const hypad_train_state* st, void* workspace, size_t workspace_bytes,
                         hypad_stream_t stream);
int hypad_packed_region(const hypad_dims* dims, int64_t* offset_floats, int64_t* signal_stride_floats, int64_t* count_floats);
/* critic_x_iteration train.py:18-104 / critic_z_iteration :107-186 / decoder_iteration :189-249 -- one optimizer step each.
 * The two critic entry points have two forms with the same results up to floating-point summation order (and the device dropout
 * streams, where the masks are not injected): three stand-alone launches (pass, gradient penalty, dW + Adam), or -- when
 * io->workspace_bytes >= hypad_epoch_workspace_bytes(dims, 1, 1) and the shape fits the epoch's critic kernels -- a one-iteration
 * phase of the epoch's hoisted form (pack of the frozen generator half, record precompute, iteration launch, finalising launch,
 * counter advance): 45 / 29 us of GPU time per call instead of 66 / 39 at the reference configuration, five launches instead of
 * three.  HYPAD_ITER_PHASE=0 in the environment keeps the stand-alone launches whatever the workspace. */
int hypad_critic_x_iteration(const hypad_dims* dims, const hypad_train_state* st, const hypad_iter_io* io, hypad_stream_t stream);
int hypad_critic_z_iteration(const hypad_dims* dims, const hypad_train_state* st, const hypad_iter_io* io, hypad_stream_t stream);
int hypad_decoder_iteration(const hypad_dims* dims, const hypad_train_state* st, const hypad_iter_io* io, hypad_stream_t stream);

/* One epoch of train_tadgan's loops (train.py:299-356): n_critics passes of (critic_x, critic_z) over every
 * minibatch, then one generator pass.  row_index: ((n_critics + 1), n_batches * batch) int32 window rows (the
 * DataLoader's shuffles); noise and dropout come from device Philox (seed).  losses: (n_signals,
 * (2 * n_critics + 1) * n_batches, 4) in launch order. */
/* Optional injected randomness of a whole epoch (parity runs; a NULL plane = device Philox keyed by `seed`).  Planes are
 * iteration-major, so one iteration's slice has exactly the layout hypad_iter_io states for that iteration:
 * critic iteration it = pass * n_batches + batch (launch order), generator iteration b = batch. */
typedef struct hypad_epoch_noise {
  const float* z_cx;      /* (n_critics * n_batches, n_signals, batch, L)  N(0,1), decoder input of critic_x_iteration  train.py:24 */
  const float* alpha_cx;  /* (n_critics * n_batches, n_signals, batch, S)  U[0,1)                                        train.py:64 */
  const float* z_cz;      /* (n_critics * n_batches, n_signals, batch, L)  N(0,1), `valid` latent of critic_z_iteration   train.py:118 */
  const float* alpha_cz;  /* (n_critics * n_batches, n_signals, batch, L)                                                train.py:149 */
  const float* z_gen;     /* (n_batches, n_signals, batch, L)              decoder_iteration                              train.py:205 */
  /* dropout keep-scales (0 or 1/(1-p)), read when train_mode != 0: all three planes or none.  Per (iteration, signal)
   * the layouts of hypad_iter_io.drop for critic_x_iteration / critic_z_iteration / decoder_iteration. */
  const float* masks_cx;
  const float* masks_cz;
  const float* masks_gen;
} hypad_epoch_noise;

typedef struct hypad_epoch_io {
  const float* x; int64_t x_signal_stride;
  int64_t x_row_stride;      /* as in hypad_iter_io */
  const int32_t* row_index;  /* (n_critics + 1, n_batches * batch): the passes' shuffles */
  int n_batches, n_critics;
  int train_mode; uint64_t seed;
  float* losses;
  void* workspace; size_t workspace_bytes;   /* >= hypad_train_workspace_bytes(dims); with >= hypad_epoch_workspace_bytes(...)
                                                the critic phase runs in its hoisted form (see below) */
  const hypad_epoch_noise* noise;            /* NULL: all randomness from device Philox(seed) */
  int flags;                                 /* HYPAD_EPOCH_* bits, 0 = defaults */
  /* ABI 4.  Optional: n_aux_streams (<= 7) further streams of the same device.  With more than one signal (model) per call the
   * generator phase (train.py:347-352: 29 x [decoder_iteration, its optimizer step] per model, the models independent of each other)
   * then runs the models in n_aux_streams + 1 groups, each group's chain of launches on a stream of its own -- forked from `stream`
   * by an event after the critic phase, joined into it before the call returns its last launches -- so one group's optimizer
   * launch overlaps another group's generator launch.  Results are the same bits with any number of streams (the step number and
   * rng tick of every launch are its own arguments; the counters advance once, after the join).  Capturable like everything else:
   * the groups become parallel branches of the captured graph.  NULL / 0: everything on `stream`.  Calls that pass auxiliary streams
   * share one process-wide set of fork / join events: issue them from one host thread at a time. */
  hypad_stream_t const* aux_streams; int n_aux_streams;
  /* ABI 5.  int32 elements between the row_index planes of consecutive signals: 0 = ONE plane shared by all signals (every model sees
   * the same shuffles); (n_critics + 1) * n_batches * batch or more = a plane per signal -- signals of different lengths (each with
   * permutations of its OWN window count, hypad_epoch_shuffles_signals) trained by the same launches. */
  int64_t row_index_signal_stride;
  /* ABI 6.  Optional scratch, n_signals x enc_table_rows x latent_dim floats, enc_table_rows = number of window rows of `x` a row
   * index may name (every model: rows 0 .. enc_table_rows - 1 of its x must be readable).  The encoder is frozen through the critic
   * phase (train.py:306-309) and every pass shuffles the same windows, so encoder(x) -- critic_z's fake input, train.py:111-116 --
   * is then evaluated ONCE per window row in front of the phase (one launch) and gathered by the record producers, instead of once
   * per pass (n_critics times): worth it from 14 models per call on, where the producers bound the phase (16 models: 4.25 -> 3.97 ms
   * per epoch, 32: 5.99 -> 5.76); the same bits either way (the encoder output of a row does not depend on the other rows of its tile).  NULL: off. */
  float* enc_table; int64_t enc_table_rows;
} hypad_epoch_io;
enum {
  HYPAD_EPOCH_PER_ITERATION = 1,             /* run the critic phase as one launch per iteration even where the resident form fits */
  /* A/B switches (tests, timing).  The library reads NO environment variable: which kernels a call launches depends on its
   * arguments alone.  Every combination gives the same results bit for bit, except PER_ITERATION / PER_MINIBATCH (another
   * summation order of the critics' gradient shares). */
  HYPAD_EPOCH_NO_PRODUCERS = 2,              /* resident critic launch behind a precompute launch instead of with its own record producers */
  HYPAD_EPOCH_ID_ORDER = 4,                  /* resident critic workgroups in id order (no per-XCD placement: shares go through memory) */
  HYPAD_EPOCH_CLEAR_TILES = 8,               /* sweep the activation / delta tiles after every resident iteration (round-2 behaviour) */
  HYPAD_EPOCH_PER_MINIBATCH = 16,            /* no hoisting at all: one launch group per minibatch (critic_x || critic_z pass, penalty, dW) */
  HYPAD_EPOCH_DW_COLOC = 32,                 /* dW + Adam workgroups co-located per model and XCD (the default from 8 models per call on) */
  HYPAD_EPOCH_DW_SPREAD = 64,                /* ... spread over the chip (the default below 8 models) */
  HYPAD_EPOCH_TEST_GIVE_UP_SHIFT = 8         /* tests only: bits 8..15 = k > 0 makes the resident launch behave as if its wait for the
                                                siblings' shares had timed out at critic iteration k (signal 0, critic_x) */
};
/* The DataLoader's shuffles of one epoch (main.py:38: shuffle=True, drop_last=True; train.py:315-351 iterates the loader once per
 * pass) drawn on the device: row_index (n_passes, take) int32 <- for every pass the first `take` = n_batches * batch entries of an
 * independent uniform random permutation of [0, n_windows) (argsort of Philox keys, keyed by seed, pass and the rng tick
 * counters[3] -- NULL: tick 0 -- so every epoch of a replayed graph is shuffled afresh).  Capturable: an epoch including its
 * shuffles is then a fixed launch sequence with no host work at all.  n_windows <= 4096 (one workgroup sorts a pass in LDS);
 * HYPAD_EUNSUPPORTED beyond: draw the permutations with any other generator and pass them to hypad_train_epoch as before. */
int hypad_epoch_shuffles(int32_t* row_index, int n_passes, int take, int n_windows, uint64_t seed, const int32_t* counters,
                         hypad_stream_t stream);
/* The same for n_signals models of different lengths in one launch: signal s gets its own plane row_index + s * signal_stride
 * (n_passes, take) of permutations of [0, n_windows[s]) (n_windows: DEVICE int32[n_signals], each in [take, 4096]), keyed by
 * (seed, first_signal + s, pass, tick): the plane of signal s == hypad_epoch_shuffles' for one model with that seed and
 * first_signal + s (the key folds the stream number in; stream 0 is the key of hypad_epoch_shuffles itself). */
int hypad_epoch_shuffles_signals(int32_t* row_index, int64_t signal_stride, int n_signals, int first_signal, const int32_t* n_windows,
                                 int n_passes, int take, uint64_t seed, const int32_t* counters, hypad_stream_t stream);

/* HOST helper (the one entry point whose pointers are host pointers; no device work, no stream): the latent draws of a whole epoch
 * of the reference's loop -- np.random.normal(size=(1, batch, L)) on NumPy's GLOBAL generator, once per iteration, train.py:24,118,205
 * -- continued from that generator's state (np.random.get_state(): MT19937 key[624], pos, has_gauss, cached_gaussian; all updated in
 * place: hand them back with np.random.set_state()) and written as float32 (torch.Tensor(float64 array), train.py:24) into the pinned
 * planes hypad_epoch_noise is uploaded from.  Draw order: for r in [0, rounds): for k in [0, n_outs): `chunk` values -> outs[k] + r*chunk
 * (critic phase: outs = {z_cx, z_cz}, chunk = batch * L, rounds = n_critics * n_batches: critic_x_iteration draws before
 * critic_z_iteration, train.py:320-327; generator pass: outs = {z_gen}).  NumPy's legacy polar Box-Muller bit for bit
 * (tests/test_host_rng.py); unlike np.random.normal the call does not hold the interpreter lock. */
int hypad_host_mt19937_normal(uint32_t* key, int* pos, int* has_gauss, double* cached_gaussian, float* const* outs, int n_outs,
                              int64_t chunk, int64_t rounds);
/* hypad_host_mt19937_normal with `threads` helper threads: the calling thread runs the generator and the polar method's rejection test
 * (sequential), the helpers take the accepted pairs' transforms -- sqrt(-2 log(r2) / r2), two products, the float32 stores; independent
 * per pair -- block by block as they become ready.  Same values, same final state; threads < 1 = hypad_host_mt19937_normal.  Worth it
 * from about a million values per call on (configs[3]: 4.1 M per epoch). */
int hypad_host_mt19937_normal_mt(uint32_t* key, int* pos, int* has_gauss, double* cached_gaussian, float* const* outs, int n_outs,
                                 int64_t chunk, int64_t rounds, int threads);
/* The interpolation weights of train.py:64,149 -- torch.rand(...) on torch's default CPU generator -- for a whole pass in one call:
 * `state` = the bytes of torch.get_rng_state() (5 056: at::CPUGeneratorImplState, an at::mt19937 inside), advanced in place as n draws
 * leave it; out[i] = the i-th float32 torch.rand would have returned.  HOST pointers, like hypad_host_mt19937_normal. */
int hypad_host_torch_mt19937_uniform(void* state, size_t state_bytes, float* out, int64_t n);

/* Workspace that lets hypad_train_epoch hoist the frozen generator's forwards (decoder(z_i), encoder(x_i) of every
 * critic iteration, train.py:306-328) out of the sequential critic chain: hypad_train_workspace_bytes plus room for up
 * to 512 iterations of precomputed rows (longer phases are processed in chunks).  Same random streams and the same
 * arithmetic per row as the per-iteration entry points; only floating-point summation order differs. */
size_t hypad_epoch_workspace_bytes(const hypad_dims* dims, int n_batches, int n_critics);
/* 1 when hypad_train_epoch (given that workspace) runs the critic phase of these dimensions as ONE resident launch -- every
 * (signal, critic, 16-row chunk) workgroup stays on its CU for all iterations, weights in LDS, Adam state in registers, gradient
 * shares exchanged through write-through stores and epoch words -- instead of one launch per iteration.  Needs
 * 2 * n_signals * batch / 16 <= CUs of the device; HYPAD_CRITIC_PERSISTENT=0 in the environment selects the launches. */
int hypad_critic_phase_persistent(const hypad_dims* dims);
/* 1 when that resident launch also produces the phase's records itself (extra workgroups behind the resident ones: no separate
 * precompute launch) for a phase of n_iters = n_critics * n_batches iterations: where the resident critics hold at most half of
 * the device's CUs (the producers need the others); hypad_epoch_io.flags & HYPAD_EPOCH_NO_PRODUCERS turns it off. */
int hypad_critic_phase_producers(const hypad_dims* dims, int n_iters);
int hypad_train_epoch(const hypad_dims* dims, const hypad_train_state* st, const hypad_epoch_io* io, hypad_stream_t stream);

/* Status channel of the resident critic launch.  That launch needs every one of its critic workgroups co-resident (one per CU:
 * the launcher checks the grid against the device's CU count and the kernel's occupancy, but a CU mask, a partitioned or shared
 * device can still withhold CUs) and all its waits are bounded: a wait that gives up stores its code -- 0x100 + it: a sibling's
 * gradient share of critic iteration `it` never arrived; 0x200 + it: a sibling's scalars; 0x300 + it: a record -- into
 * counters[4] (first code wins), writes NaN into that iteration's loss row, and the launch ends.  From then on every training
 * launch of hypad_train_epoch on this state is a no-op (fail-stop: the generator is never stepped against half-updated
 * critics, the snapshot below is never overwritten) until hypad_epoch_restore.
 *   hypad_epoch_status : copies counters[4] to *status_host and SYNCHRONISES the stream (not capturable).
 *   hypad_epoch_restore: puts both critics' parameters and moments and counters[0..3] back to what they were when the failed
 *                        hypad_train_epoch call began (it snapshots them into its workspace first: 50 KB per signal) and clears
 *                        counters[4]; the caller then repeats that epoch with HYPAD_EPOCH_PER_ITERATION -- same random streams:
 *                        bit for bit the epoch a healthy run in that form produces (the two forms differ only in floating-point
 *                        summation order).  Capturable; workspace = the failed call's. */
int hypad_epoch_status(const hypad_train_state* st, int* status_host, hypad_stream_t stream);
int hypad_epoch_restore(const hypad_dims* dims, const hypad_train_state* st, void* workspace, size_t workspace_bytes,
                        hypad_stream_t stream);

/* Where hypad_train_epoch's hoisted critic phase left its precomputed records (tests and tools; valid after a call with
 * n_critics * n_batches <= 512 iterations): records of critic `critic` (0 = critic_x, 1 = critic_z) start `offset_floats` floats
 * into the workspace and are indexed (signal, iteration, batch / 16 chunks); one record is `record_floats` floats:
 * [48][row_stride] input rows (16 real | 16 fake | 16 interpolated; the input, a constant-one column, zero padding) followed,
 * at `mask_offset_floats`, by the dropout keep-scales [n_layers][48][mask_row_stride] (pass order real, fake, interpolated) and
 * a tail of 32 floats (Adam's bias corrections of the step the next iteration applies, then zeros: records stay 128-byte
 * aligned).  With the resident form of the phase the records are written by producer workgroups of that launch itself
 * (HYPAD_CRITIC_PRODUCERS=0 in the environment: by a launch in front of it) -- same layout, same bits. */
typedef struct hypad_record_info {
  int64_t offset_floats;
  int record_floats, row_stride, mask_offset_floats, mask_row_stride, n_layers, in_dim;
} hypad_record_info;
int hypad_epoch_record_info(const hypad_dims* dims, int n_batches, int n_critics, int critic, hypad_record_info* out);

/* The device random streams the training kernels draw from when no plane is injected -- Philox4x32-10 keyed by (seed, tick,
 * stream, signal), element index = position in the (batch, width) matrix -- exported for distribution tests.
 * kind: 0 = N(0,1) (z), 1 = U[0,1) (alpha), 2 = dropout keep-scale 0 | 1/(1-p_drop).  tick = counters[3] at the iteration.
 * streams: HYPAD_STREAM_*; a critic's dropout stream is HYPAD_STREAM_DROP_CRITIC + 8 * pass + layer (pass: critic_x 0 valid,
 * 1 fake, 2 interpolated; critic_z 0 fake, 1 valid, 2 interpolated).  Inside hypad_train_epoch the critic_z side draws with
 * hypad_critic_z_seed(seed). */
enum { HYPAD_RNG_NORMAL = 0, HYPAD_RNG_UNIFORM = 1, HYPAD_RNG_DROPOUT = 2 };
enum { HYPAD_STREAM_Z = 1, HYPAD_STREAM_ALPHA = 2, HYPAD_STREAM_DROP_DEC0 = 3, HYPAD_STREAM_DROP_DEC1 = 4, HYPAD_STREAM_DROP_CRITIC = 16 };
int hypad_rng_fill(int kind, uint64_t seed, uint32_t tick, uint32_t rng_stream, uint32_t signal, float p_drop, float* out,
                   int64_t n, hypad_stream_t stream);
uint64_t hypad_critic_z_seed(uint64_t seed);

/* Measurement aid (bench.py): run ONE iteration (kind 0 = critic_x, 1 = critic_z, 2 = decoder, 3 = the critic_x ||
 * critic_z pair of the per-iteration path) or, kind 4, 145 iterations of the hoisted critic phase of hypad_train_epoch
 * over rows 0 .. batch-1 (row_index is ignored), with HIP events recorded on `stream` between the kernels; synchronise;
 * return the per-kernel durations in ms: critic iterations -> {pass kernel, gradient-penalty kernel, dW+Adam};
 * decoder -> {generator kernel, dW+Adam}; kind 4 -> {precompute kernel (the 145 iterations' records), X, mean time of one
 * critic_x || critic_z iteration}: when the phase runs as one resident launch (hypad_critic_phase_persistent) X is the
 * re-initialisation of its epoch words and the mean is that launch's duration / 145; otherwise X is the first iteration launch
 * (no Adam in its prologue) and the mean is over the 144 steady-state launches that follow back to back.  losses: room for
 * 2 * n_signals * 4 floats (kind 3) / 290 * n_signals * 4 floats (kind 4); workspace for kind 4:
 * hypad_epoch_workspace_bytes(dims, 145, 1).  kind 5 = the decoder iteration's two kernels as hypad_train_epoch launches them (the decay-only tensors left to the epoch's
 * decay launch), each launched 64 times back to back
 * between its events -> {mean generator kernel, mean dW+Adam}: an event pair around ONE launch of a 9 - 40 us kernel also measures
 * the event path (the sum of such figures exceeded the epoch they were taken from); the 64 dW+Adam launches are 64 optimizer steps
 * on the same gradient (the weights move: measure after, not inside, a run whose results matter).
 * Not capturable into a graph. */
int hypad_profile_iteration(int kind, const hypad_dims* dims, const hypad_train_state* st, const hypad_iter_io* io,
                            float* ms_out, int n_out, hypad_stream_t stream);

/* Stand-alone optimizer steps over a flat arena given its gradient arena.
 * torch.optim.Adam (train.py:274-281): step_index = 1-based step number. */
int hypad_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                    int step_index, float lr, float beta1, float beta2, float eps, float weight_decay,
                    hypad_stream_t stream);
/* geoopt.optim.RiemannianAdam (train.py:282-288; geoopt==0.5.0, restated -- see oracle/radam.py):
 * Euclidean rule on [0, n) except the ball-valued vector [ball_offset, ball_offset + ball_dim) (ball_dim = 0: none). */
int hypad_radam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                     int64_t ball_offset, int ball_dim, int step_index, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int stabilize, hypad_stream_t stream);
/* Row-wise Riemannian steps: a parameter (rows, dim) of fp32 whose every row is one point of its manifold -- the Poincare ball at
 * k = -1 (geoopt.PoincareBall) or the unit sphere (geoopt.manifolds.Sphere) -- with its gradient and state tensors of the same shape,
 * updated in place by ONE launch: a wave per row in fp64 registers, no atomics, no workspace, a row's bits independent of the rows around
 * it.  Per row x with gradient g, after g <- g + weight_decay x (the maps are listed in docs/history/riemannian_rows.md):
 *   ball:    r = g / lambda_x^2,  second-moment number lambda_x^2 <r, r>,  retr(x, u) = project(x + u) (hypad_project_fwd),
 *            transp = hypad_parallel_transport_fwd,  stabilise: x <- project(x)
 *   sphere:  r = g - <x, g> x,  second-moment number <r, r>,  retr(x, u) = (x + u) / max(|x + u|, 1e-15),  transp(x, y, w) = w - <y, w> y,
 *            stabilise: x <- x / max(|x|, 1e-15), then w <- w - <x, w> x for the first moment / momentum buffer
 * hypad_radam_rows_step -- geoopt.optim.RiemannianAdam.step for such a parameter (train.py:282-288 hands the reference's tagged
 * parameters, hyrnn_nets.py:216-225, to it; geoopt==0.5.0 restated, oracle/radam.py); replaces the ~10 launches of the rule composed from
 * egrad2rgrad, inner, project, parallel_transport and elementwise ops, and extends hypad_radam_step's single ball vector to rows:
 *   m <- b1 m + (1 - b1) r;  v <- b2 v + (1 - b2) number, on every element of the row (a row of exp_avg_sq that holds one value
 *   repeated keeps doing so, bit for bit);  y = retr(x, -lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps));  m <- transp(x, y, m);  x <- y.
 * hypad_rsgd_rows_step -- geoopt.optim.RiemannianSGD.step, also for HYPAD_MANIFOLD_EUCLIDEAN rows (r = g, retr(x, u) = x + u, no
 * transport): without momentum x <- retr(x, -lr r) and momentum_buf is NULL; with momentum b <- momentum b + (1 - dampening) r,
 * d = r + momentum b (nesterov) or b, y = retr(x, -lr d), b <- transp(x, y, b), x <- y.  The caller creates the buffer (geoopt: a
 * clone of the first gradient).
 * Both stabilise when stabilize > 0 and step_index % stabilize == 0.  step_index is the 1-based step number, by value: not for graph
 * capture.  Every argument is validated before anything is launched: HYPAD_EINVAL for rows < 0, dim <= 0, step_index < 1, an unknown
 * manifold (hypad_radam_rows_step: also HYPAD_MANIFOLD_EUCLIDEAN), a NULL operand with rows > 0, or a momentum_buf that is not NULL
 * exactly where momentum == 0; HYPAD_EUNSUPPORTED for dim > 256 or rows dim >= 2^31; rows == 0 launches nothing. */
enum { HYPAD_MANIFOLD_EUCLIDEAN = 0, HYPAD_MANIFOLD_BALL = 1, HYPAD_MANIFOLD_SPHERE = 2 };
int hypad_radam_rows_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t rows, int dim, int manifold,
                          int step_index, float lr, float beta1, float beta2, float eps, float weight_decay, int stabilize,
                          hypad_stream_t stream);
int hypad_rsgd_rows_step(float* params, const float* grads, float* momentum_buf, int64_t rows, int dim, int manifold, int step_index,
                         float lr, float momentum, float dampening, float weight_decay, int nesterov, int stabilize,
                         hypad_stream_t stream);

/* Grouped, capturable steps (csrc/optim_group.hip, docs/history/capturable_optim.md): ONE launch updates up to HYPAD_OPTIM_GROUP_MAX
 * tensors of one rule, each described by a hypad_optim_tensor, and may take its step number and learning rate from device memory, so
 * that a step captured into a graph advances with every replay.  The descriptors travel by value in the kernel's argument: the array
 * may be freed when the call returns, and a captured kernel node owns its copy.
 *   rows, dim   a wave per row of `dim` <= 256 elements, as above
 *   manifold    HYPAD_MANIFOLD_BALL / _SPHERE: rows dim == numel, the rules and maps of the row-wise steps above.
 *               HYPAD_MANIFOLD_EUCLIDEAN: a flat tensor of numel elements cut into rows of `dim` with a short last row
 *               ((rows - 1) dim < numel <= rows dim); SGD's rule with the identity maps, and under Adam the ELEMENT-WISE rule of
 *               torch.optim.Adam: g += wd p, m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, p -= lr (m / bc1) / (sqrt(v / bc2) + eps),
 *               in fp64 registers, rounded once.
 *   state0/1    Adam: exp_avg, exp_avg_sq.  SGD: the momentum buffer (NULL exactly where momentum == 0), and NULL.
 * step_dev: the 1-based step number in device memory, read by the kernel (NULL: `step_index`, by value); lr_dev likewise (NULL: `lr`).
 * hypad_optim_step_advance adds one to a device step counter: a step is "advance, then the grouped launches" in stream order, and no
 * kernel both reads and writes the counter.  Every argument is validated before anything is launched: HYPAD_EINVAL for n < 1,
 * n > HYPAD_OPTIM_GROUP_MAX, a NULL list, step_index < 1 where step_dev is NULL, rows < 0, dim <= 0, an unknown manifold, a numel that
 * disagrees with rows and dim, a NULL operand on a tensor with rows, or a momentum buffer that is not NULL exactly where
 * momentum == 0; HYPAD_EUNSUPPORTED for dim > 256 or rows dim >= 2^31.  A tensor with rows == 0 is skipped; a call whose tensors are all
 * empty launches nothing. */
#define HYPAD_OPTIM_GROUP_MAX 32
typedef struct hypad_optim_tensor {
  float* param;
  const float* grad;
  float* state0;
  float* state1;
  int64_t rows;
  int64_t numel;
  int dim;
  int manifold;
} hypad_optim_tensor;
int hypad_optim_step_advance(int32_t* step, hypad_stream_t stream);
int hypad_optim_group_adam(const hypad_optim_tensor* tensors, int n, const int32_t* step_dev, int step_index, const float* lr_dev, float lr,
                           float beta1, float beta2, float eps, float weight_decay, int stabilize, hypad_stream_t stream);
int hypad_optim_group_sgd(const hypad_optim_tensor* tensors, int n, const int32_t* step_dev, int step_index, const float* lr_dev, float lr,
                          float momentum, float dampening, float weight_decay, int nesterov, int stabilize, hypad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Window scoring (utils/anomaly_detection_utils.py).  fp64 where NumPy computes in fp64.
 * ---------------------------------------------------------------------------------------------- */
/* reconstruction_errors un-roll, :918-935: for t in [0, n + S - 1) gather y_hat[t - j, j] over valid j;
 * median (T,) in the input precision (np.median of float32) and, if summary != NULL, (T, 5) fp64
 * [min, p25, p50, p75, max] with NumPy's linear-interpolated percentiles. */
int hypad_unroll_median(const float* y_hat, float* median, double* summary, int64_t n, int window, hypad_stream_t stream);
/* :908-910 -- true[t] = y[t][0] (t < n), y[n-1][t-n+1] otherwise; y (n, S) fp64 */
int hypad_unroll_true(const double* y, double* out, int64_t n, int window, hypad_stream_t stream);
/* the same from the fp32 window matrix the forward reads (row n at y + n * row_stride: row_stride = S for a matrix, 1 for the
 * scaled series itself) -- no fp64 copy of the (n, S) matrix for the sake of n + S - 1 of its values */
int hypad_unroll_true_f32(const float* y, int64_t row_stride, double* out, int64_t n, int window, hypad_stream_t stream);
/* _point_wise_error :761-777 */
int hypad_point_error(const double* y, const float* y_hat, double* out, int64_t t, hypad_stream_t stream);
/* _area_error :780-812 (centred rolling trapezoid, window score_window, min_periods score_window/2) */
int hypad_area_error(const double* y, const float* y_hat, double* out, int64_t t, int score_window, hypad_stream_t stream);
/* _dtw_error :815-863 (pyts.metrics.dtw classic, squared cost, sqrt of the accumulated cost) */
int hypad_dtw_error(const double* y, const float* y_hat, double* out, int64_t t, int score_window, hypad_stream_t stream);
/* pandas rolling(window, center=True, min_periods=window/2).mean()  :953-961, :325-330 -- of in[], or, with sub != NULL, of the
 * point-wise error |in[i] - sub[i]| (:761-777 fused).  Windows wider than 32 are summed from two levels of pre-summed chunks
 * (16 and 256 elements) aligned to the absolute index origin + i, in one canonical order: O(60 + window / 256) additions per
 * output instead of O(window), and a caller that smooths a slice [origin, origin + t) of a longer series gets, for every
 * timestep whose window lies inside the slice, the bits the whole series gives (sharded scoring).
 * workspace: hypad_rolling_workspace_bytes(t) (may be NULL for window <= 32). */
size_t hypad_rolling_workspace_bytes(int64_t t);
int hypad_rolling_mean(const double* in, const float* sub, double* out, int64_t t, int window, int64_t origin, void* workspace,
                       size_t workspace_bytes, hypad_stream_t stream);
/* workspace of hypad_zscore_clip / hypad_critic_zscore: the per-slice partial statistics of their first launch */
#define HYPAD_STATS_WORKSPACE_BYTES (256 * 5 * 8)
/* stats.zscore -> clip(min=0) + 1  :523-524,542-543.  workspace: HYPAD_STATS_WORKSPACE_BYTES */
int hypad_zscore_clip(const double* in, double* out, int64_t t, void* workspace, size_t workspace_bytes, hypad_stream_t stream);
/* final_critic_scores :365-404 (also :470-504), KDE step: modes (n + window - 1) fp64 -- for every un-rolled timestep
 * the window-critic value at which scipy.stats.gaussian_kde of the covering windows' values peaks (median fallback). */
int hypad_kde_mode(const float* critic, double* modes, int64_t n, int window, hypad_stream_t stream);
/* _compute_critic_score :307-322: out = |x - mean(x within [q25, q75])| / std(x) + 1 (quantiles supplied by the caller;
 * the rolling mean of :325-330 is hypad_rolling_mean).  workspace: HYPAD_STATS_WORKSPACE_BYTES */
int hypad_critic_zscore(const double* in, double q25, double q75, double* out, int64_t t, void* workspace,
                        size_t workspace_bytes, hypad_stream_t stream);
/* np.quantile(in, q) (method "linear") for nq <= 2 quantiles of n fp64 values, out (nq) fp64 ON THE DEVICE: exact order
 * statistics by radix selection on the keys (no sort, no host round trip), numpy's interpolation; any NaN -> NaN.
 * :319-320 (`np.quantile(critics, 0.25)`, `np.quantile(critics, 0.75)`).  workspace: hypad_quantile_workspace_bytes() */
size_t hypad_quantile_workspace_bytes(void);
int hypad_quantiles(const double* in, int64_t n, const double* q, int nq, double* out, void* workspace, size_t workspace_bytes,
                    hypad_stream_t stream);
/* _compute_critic_score :307-322 with the two quantiles taken on the device (hypad_quantiles), then as hypad_critic_zscore.
 * workspace: hypad_critic_score_workspace_bytes() */
size_t hypad_critic_score_workspace_bytes(void);
int hypad_critic_score(const double* in, double* out, int64_t t, void* workspace, size_t workspace_bytes, hypad_stream_t stream);
/* np.linalg.norm(recons, axis=1)  :341,347,350,359 */
int hypad_row_norms(const float* x, double* out, int64_t rows, int dim, hypad_stream_t stream);
/* np.linalg.norm(true - recons, axis=1) with the fp32 difference formed as the two matrices are read -- the Euclidean reconstruction
 * score of multivariate_anomaly_detection, utils/anomaly_detection_utils.py:157 (`true_signal - recons_signal`, then the norm of
 * :160-161).  a, b (rows, dim) fp32; out (rows) fp64, the bits of hypad_row_norms on the fp32 matrix a - b.  One launch; rows of a
 * signal group need no offsets.  NULL pointer, rows <= 0 or dim <= 0: HYPAD_EINVAL without a launch. */
int hypad_row_diff_norms(const float* a, const float* b, double* out, int64_t rows, int dim, hypad_stream_t stream);
/* combine_scores :336-362 */
enum { HYPAD_COMB_SUM = 0, HYPAD_COMB_MULT = 1, HYPAD_COMB_UNCERTAINTY = 2, HYPAD_COMB_CRITIC = 3,
       HYPAD_COMB_CRITIC_UNCERTAINTY = 4, HYPAD_COMB_SUM_UNCERTAINTY = 5, HYPAD_COMB_REC = 6,
       HYPAD_COMB_REC_UNCERTAINTY = 7,
       /* score_anomalies tail :553-570 */
       HYPAD_COMB_EUCL_MULT = 8, HYPAD_COMB_EUCL_SUM = 9 };
int hypad_combine_scores(int combination, const double* critic_scores, const double* rec_scores,
                         const double* uncertainty, double* out, int64_t n, hypad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Signal groups: the test loop and the critic-score chain of many trained models at once (the per-signal
 * anomaly_detection.py:20-155 + utils/anomaly_detection_utils.py:54-86, :336-404 of a dataset run, one model per signal).
 * row_off (n_signals + 1) and x_off (n_signals) are HOST int64 arrays: the launch plan is taken from them and they travel in the
 * kernel arguments.  row_off[0] = 0 and every signal has at least one window, else HYPAD_EINVAL without any launch.
 * TIMESTEP LAYOUT: a vector with one entry per un-rolled timestep of every signal -- signal s, n_s = row_off[s + 1] - row_off[s]
 * windows, owns the n_s + window - 1 entries from row_off[s] + s (window - 1) on; row_off[n_signals] + n_signals (window - 1) in all.
 * ---------------------------------------------------------------------------------------------- */
/* hypad_score_forward_packed for n_signals models: enc / dec / cx are stacked arenas, (n_signals, hypad_param_count(net, ...))
 * each (hypad_amd Engine.params).  Signal s has windows row_off[s] .. row_off[s + 1]; its window n is x[x_off[s] + n * x_row_stride ..]
 * (x_row_stride 0 / S: window matrix, 1: the signal's scaled series).  Outputs as hypad_score_forward_packed's, concatenated in row
 * order, each optional.  One pack launch for all signals, then per 64 signals one critic launch and one forward launch whose tiles
 * never straddle two signals.  The tile form (16 or 32 windows) follows from row_off[n_signals] as hypad_score_forward_packed's
 * from its `rows`; every signal's rows equal a hypad_score_forward_packed call on that signal alone, bit for bit.
 * workspace: hypad_score_signals_workspace_bytes(S, L, hyperbolic, n_signals). */
size_t hypad_score_signals_workspace_bytes(int signal_shape, int latent_dim, int hyperbolic, int n_signals);
int hypad_score_forward_signals(const float* enc, const float* dec, const float* cx, int n_signals, const int64_t* row_off,
                                const int64_t* x_off, const float* x, int64_t x_row_stride, float* hyper, float* eucl,
                                float* hyper_real, float* critic, float* rowdist, int signal_shape, int latent_dim, int hyperbolic,
                                void* workspace, size_t workspace_bytes, hypad_stream_t stream);
/* The forward launch's plan for such a group: windows per tile (16 or 32) and the number of tiles. */
int hypad_score_signals_tiles(int signal_shape, int latent_dim, int n_signals, const int64_t* row_off, int* rows_per_tile, int64_t* tiles);
/* final_critic_scores :365-404 per signal, KDE step: segment s of `modes` (row_off[s] + s (window - 1), n_s + window - 1 fp64)
 * is hypad_kde_mode of critic[row_off[s] .. row_off[s + 1]). */
int hypad_kde_mode_signals(const float* critic, double* modes, int n_signals, const int64_t* row_off, int window, hypad_stream_t stream);
/* final_critic_scores :365-404 per signal, the rest (_compute_critic_score :307-333): per segment of `modes` (layout as above)
 * hypad_critic_score, then the centred rolling mean with the signal's own window trunc(n_s * 0.01) -- all NaN where that is 0, as
 * pandas gives.  Each segment is reduced with the single-signal partition: the same bits as the per-signal calls.
 * workspace: hypad_critic_score_signals_workspace_bytes(n_signals, row_off, window). */
size_t hypad_critic_score_signals_workspace_bytes(int n_signals, const int64_t* row_off, int window);
int hypad_critic_score_signals(const double* modes, double* out, int n_signals, const int64_t* row_off, int window, void* workspace,
                               size_t workspace_bytes, hypad_stream_t stream);
/* combine_scores :336-362 per signal: out[row_off[s] + i] from critic_scores[row_off[s] + s (window - 1) + i] (the first n_s of the
 * signal's final_critic_scores), rec_scores[row_off[s] + i] and uncertainty[row_off[s] + i]; any input may be NULL as for
 * hypad_combine_scores.  One launch per 64 signals. */
int hypad_combine_scores_signals(int combination, const double* critic_scores, const double* rec_scores, const double* uncertainty,
                                 double* out, int n_signals, const int64_t* row_off, int window, hypad_stream_t stream);
/* stats.zscore -> clip(min=0) + 1 of every segment [seg_off[s], seg_off[s + 1]) of a plain segmented fp64 vector -- WINDOW LAYOUT, one
 * entry per window: the multivariate detector's reconstruction scores, utils/anomaly_detection_utils.py:160-161 (Euclidean) and
 * :177-178 (hyperbolic), for a group.  Segment s of `out` equals hypad_zscore_clip on that segment alone, bit for bit (the same slices,
 * the same merge tree; no floating-point atomics, so it does not depend on the group either); in == out is allowed.  seg_off
 * (n_signals + 1, HOST): checked like row_off.  Two launches per 64 signals, whatever the segment lengths.  No launch when an
 * argument check fails.  workspace: hypad_zscore_clip_signals_workspace_bytes(n_signals) (0 for n_signals < 1). */
size_t hypad_zscore_clip_signals_workspace_bytes(int n_signals);
int hypad_zscore_clip_signals(const double* in, double* out, int n_signals, const int64_t* seg_off, void* workspace,
                              size_t workspace_bytes, hypad_stream_t stream);
/* The Euclidean (TadGAN) branch of a group, score_anomalies :407-576 per signal.  Un-roll (reconstruction_errors :918-935): segment s
 * of `median` (timestep layout, fp32) is hypad_unroll_median(y_hat + row_off[s] * window, ., NULL, n_s, window) -- the median of every
 * anti-diagonal of the signal's own rows, no summary.  One launch per 64 signals; a tile never straddles two signals. */
int hypad_unroll_median_signals(const float* y_hat, float* median, int n_signals, const int64_t* row_off, int window, hypad_stream_t stream);
/* Reconstruction scores (reconstruction_errors :937-961, then stats.zscore -> clip(min=0) + 1 :523-524) of the kinds in `kinds`
 * (HYPAD_REC_* bits) from the un-rolled truth (fp64) and median (fp32), all vectors in timestep layout; out_* of a kind not asked for
 * may be NULL.  Per segment: hypad_point_error (inside the smoothing) / hypad_area_error / hypad_dtw_error(score_window), then
 * hypad_rolling_mean with the signal's own window trunc(n_s * 0.01) at origin 0 (all NaN where that is 0) and hypad_zscore_clip,
 * every edge taken against the segment's own ends: the same bits as those calls on the segment alone.  Launches per 64 signals: one
 * per error kernel, four for smoothing and z-score of all kinds together.
 * workspace: hypad_rec_scores_signals_workspace_bytes(n_signals, row_off, window). */
#define HYPAD_REC_POINT 1
#define HYPAD_REC_AREA 2
#define HYPAD_REC_DTW 4
size_t hypad_rec_scores_signals_workspace_bytes(int n_signals, const int64_t* row_off, int window);
int hypad_rec_scores_signals(int kinds, const double* true_unrolled, const float* median, double* out_point, double* out_area,
                             double* out_dtw, int n_signals, const int64_t* row_off, int window, int score_window, void* workspace,
                             size_t workspace_bytes, hypad_stream_t stream);
/* np.quantile(., q) (method "linear", nq <= 2) of every segment of `in` (fp64, timestep layout) at once: :319-320
 * (`np.quantile(critics, 0.25)`, `np.quantile(critics, 0.75)`) for a group.  out: (n_signals, nq) fp64 ON THE DEVICE; segment s's row
 * equals hypad_quantiles on that segment alone (exact order statistics; a NaN in a segment makes that segment's row NaN, no other's).
 * Six launches per 64 signals.  Argument checks as hypad_quantiles', plus the offsets'.
 * workspace: hypad_quantiles_signals_workspace_bytes(n_signals). */
size_t hypad_quantiles_signals_workspace_bytes(int n_signals);
int hypad_quantiles_signals(const double* in, int n_signals, const int64_t* row_off, int window, const double* q, int nq, double* out,
                            void* workspace, size_t workspace_bytes, hypad_stream_t stream);
/* final_critic_scores :365-404 per signal, whole (KDE step :374-400, _compute_critic_score :307-333): segment s of `out` (timestep
 * layout, fp64) equals hypad_kde_mode -> hypad_critic_score -> hypad_rolling_mean with the signal's own window trunc(n_s * 0.01) (all
 * NaN where that is 0) on critic[row_off[s] .. row_off[s + 1]) alone, bit for bit -- what hypad_kde_mode_signals followed by
 * hypad_critic_score_signals give, in at most eleven launches per 64 signals instead of about eleven per signal.  modes_out: NULL, or
 * the KDE modes (timestep layout, fp64; what hypad_kde_mode_signals writes).  No launch when an argument check fails.
 * workspace: hypad_critic_chain_signals_workspace_bytes(n_signals, row_off, window). */
size_t hypad_critic_chain_signals_workspace_bytes(int n_signals, const int64_t* row_off, int window);
int hypad_critic_chain_signals(const float* critic, double* modes_out, double* out, int n_signals, const int64_t* row_off, int window,
                               void* workspace, size_t workspace_bytes, hypad_stream_t stream);
/* find_anomalies :1363-1472 with fixed_threshold=True (_fixed_threshold :1098-1114, _find_sequences / _get_max_errors /
 * _prune_anomalies / _compute_scores / _merge_sequences :1117-1313) of every segment of `scores` (fp64, on the device) at once.
 * seg_off (n_signals + 1, HOST): any ascending offsets from 0 -- row_off for window-layout scores, the timestep-layout offsets for
 * Euclidean ones.  window_size / window_step (n_signals, HOST): each signal's integer window and step, as the caller's
 * int(np.ceil(n * portion)) gives them; window k of a signal is [k step, min(k step + size, n)) while the previous window ended before n.
 * Per window: mean and population standard deviation by two-pass fp64 reductions (a constant window has std 0), threshold
 * mean + 4 std, the runs of `x > threshold` dilated by anomaly_padding, each run's maximum and the maximum outside the runs, the
 * prune by min_percent (a NaN ratio keeps), the scores (max - threshold) / (mean + std); with lower_threshold the same again on
 * 2 mean - x.  A window that holds a NaN yields nothing.  Per signal the kept runs are merged by start (touching or overlapping
 * runs join; score = sum w s / sum w, w = stop - start).
 * out: (n_signals, capacity, 3) fp64 rows (start, stop, score), positions relative to the segment; counts[s]: the signal's merged
 * intervals (all of them, also beyond capacity); status[s]: HYPAD_FA_* bits.  Rows from min(counts[s], capacity) on are not written.
 * All three ON THE DEVICE.  No floating-point atomics; a signal's rows do not depend on the group it is scored in.  Four launches
 * per 64 signals (five with lower_threshold), whatever the number of windows.  No launch when an argument check fails.
 * workspace: hypad_find_anomalies_signals_workspace_bytes(n_signals, seg_off, window_size, window_step, lower_threshold) (0: bad arguments). */
#define HYPAD_FA_ZERO_WEIGHT 1   /* a merged group's first two weights are 0: np.average raises ZeroDivisionError there (:1302) */
#define HYPAD_FA_OVERFLOW 2      /* counts[s] > capacity */
#define HYPAD_FA_INTERNAL 4      /* more values above mean + 4 std than window / 16 + 2 (impossible by Chebyshev's bound) */
size_t hypad_find_anomalies_signals_workspace_bytes(int n_signals, const int64_t* seg_off, const int64_t* window_size,
                                                    const int64_t* window_step, int lower_threshold);
int hypad_find_anomalies_signals(const double* scores, int n_signals, const int64_t* seg_off, const int64_t* window_size,
                                 const int64_t* window_step, int64_t anomaly_padding, double min_percent, int lower_threshold, double* out,
                                 int* counts, int* status, int capacity, void* workspace, size_t workspace_bytes, hypad_stream_t stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* HYPAD_H_ */
