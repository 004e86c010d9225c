// Grouped optimiser steps (docs/history/capturable_optim.md): one launch updates up to HYPAD_OPTIM_GROUP_MAX tensors of one rule -- Adam
// or SGD in the forms of riemann_opt.hip -- and may read its step number and its learning rate from device memory, so that a step
// captured into a graph takes another bias correction and another `step % stabilize` with every replay.
//
// The launch form is riemann_rows_kernel's: a wave per row in RowD<64, 4> fp64 registers, scalar loads, rowd_dot sums, a grid-stride
// walk under the same cap on the blocks; no atomics, no LDS, no workspace.  The rows of all tensors are numbered through; a wave finds
// the tensor of its row by a wave-uniform search of the prefix sums and branches wave-uniformly on that tensor's manifold, so the waves
// of one block may sit in tensors of different manifold and dim.  Ball and sphere rows go through riemann_rules.h, the structs
// riemann_opt.hip instantiates.  A plain tensor is a flat run of numel elements cut into rows with a short last row: SGD's rule with the
// identity maps, and under Adam the element-wise rule of torch.optim.Adam (AdamRule keeps ONE second-moment number per row, which is a
// manifold's rule, not a plain tensor's).
//
// The descriptors travel in the kernel argument, by value: a captured kernel node owns them, nothing is copied to the device and no
// host memory has to outlive the call.
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
constexpr int GROUP_MAX = HYPAD_OPTIM_GROUP_MAX;
constexpr size_t KERNARG_LIMIT = 4096;                  // bytes of arguments a kernel launch takes

struct Group {
  hypad_optim_tensor t[GROUP_MAX];
  int64_t end[GROUP_MAX];                               // end[i]: rows of t[0..i]; entries past the list's length repeat the total
};
// the step number and the learning rate: from the device where the pointer is given, else the value of the entry point's argument
struct Clock {
  const int32_t* step_dev;
  const float* lr_dev;
};

// torch.optim.Adam's rule on the elements of a plain row (g comes in with the weight decay added); lanes past the row's end compute on
// zeros and are not stored
__device__ __forceinline__ void adam_elementwise(const AdamRule::Coef& c, RW& x, const RW& g, RW* st) {
  RW &m = st[0], &v = st[1];
#pragma unroll
  for (int e = 0; e < RW::EPL; ++e) {
    m.v[e] = c.b1 * m.v[e] + (1.0 - c.b1) * g.v[e];
    v.v[e] = c.b2 * v.v[e] + (1.0 - c.b2) * (g.v[e] * g.v[e]);
    x.v[e] -= c.lr * ((m.v[e] / c.bc1) / (sqrt(v.v[e] / c.bc2) + c.eps));
  }
}

// rowd_load's values through loads that do not each sit under a branch of their own: a lane past the row's end reads the row's first
// element (dim >= 1: in bounds) and drops it.  The loads of a row's tensors are then in flight together instead of one after the other
__device__ __forceinline__ RW load_row(const float* p, int dim, int lane) {
  RW r;
#pragma unroll
  for (int e = 0; e < RW::EPL; ++e) {
    const int c = lane + 64 * e;
    const float v = p[c < dim ? c : 0];
    r.v[e] = c < dim ? (double)v : 0.0;
  }
  return r;
}

template <class M, class R>
__device__ __forceinline__ void manifold_row(const typename R::Coef& c, RW& x, const RW& g, RW* st, bool has_s0, bool stab) {
  R::template row<M>(c, x, g, st, has_s0);
  if (stab) M::stabilise(x, st[0]);
}

template <class R>
__global__ __launch_bounds__(THREADS) void optim_group_kernel(const Group grp, const Clock clk, R h) {
  const int lane = threadIdx.x & 63;
  // (the wave's number within the block through a scalar register: the search and the descriptor loads below are then scalar too)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (clk.step_dev) h.step = *clk.step_dev;
  if (clk.lr_dev) h.lr = *clk.lr_dev;
  const typename R::Coef c = h.coef();
  const bool stab = h.stabilize > 0 && h.step % h.stabilize == 0;
  const int64_t total = grp.end[GROUP_MAX - 1];
  // the wave's rows only go up, so its tensor only goes forward: tensor i holds the rows [begin, end), and its descriptor stays in scalar
  // registers until the walk leaves it
  int i = -1;
  int64_t begin = 0, end = 0;
  hypad_optim_tensor t = {};
  for (int64_t r = (int64_t)blockIdx.x * WAVES + wave; r < total; r += (int64_t)gridDim.x * WAVES) {
    if (r >= end) {
      do {                                              // r < total = grp.end[GROUP_MAX - 1]: ends with i < GROUP_MAX, on the row's tensor
        ++i;
        begin = end;
        end = grp.end[i];
      } while (r >= end && i < GROUP_MAX - 1);
      t = grp.t[i];
    }
    const int64_t off = (r - begin) * t.dim, left = t.numel - off;
    const int dim = left < t.dim ? (int)left : t.dim;   // the short last row of a plain tensor
    float *p = t.param + off, *s0 = t.state0 ? t.state0 + off : nullptr, *s1 = t.state1 ? t.state1 + off : nullptr;
    RW x = load_row(p, dim, lane), gr = load_row(t.grad + off, dim, lane), st[R::STATES] = {};
    if (s0) st[0] = load_row(s0, dim, lane);
    if (R::STATES == 2) st[R::STATES - 1] = load_row(s1, dim, lane);
#pragma unroll
    for (int e = 0; e < RW::EPL; ++e) gr.v[e] += (double)h.wd * x.v[e];
    if (t.manifold == HYPAD_MANIFOLD_BALL) manifold_row<Ball, R>(c, x, gr, st, s0 != nullptr, stab);
    else if (t.manifold == HYPAD_MANIFOLD_SPHERE) manifold_row<SphereM, R>(c, x, gr, st, s0 != nullptr, stab);
    else if constexpr (R::STATES == 2) adam_elementwise(c, x, gr, st);
    else manifold_row<Euclid, R>(c, x, gr, st, s0 != nullptr, stab);
    rowd_store(p, x, dim, lane);
    if (s0) rowd_store(s0, st[0], dim, lane);
    if (R::STATES == 2) rowd_store(s1, st[R::STATES - 1], dim, lane);
  }
}
static_assert(sizeof(Group) + sizeof(Clock) + sizeof(AdamRule) <= KERNARG_LIMIT && sizeof(Group) + sizeof(Clock) + sizeof(SgdRule) <= KERNARG_LIMIT,
              "the descriptors of a group travel in the kernel argument");

__global__ void advance_kernel(int32_t* step) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *step += 1;
}

inline int wave_grid(int64_t rows) {
  const int64_t b = (rows + WAVES - 1) / WAVES;
  return (int)(b > 4096 ? 4096 : b < 1 ? 1 : b);
}

// sizes, step and manifolds first, then the limits, then the operands of the tensors that have rows: Adam's two moments, SGD's one
// buffer exactly where the rule has momentum
int group_check(const hypad_optim_tensor* t, int n, const int32_t* step_dev, int step, bool sgd, bool has_momentum) {
  if (n < 1 || n > GROUP_MAX || !t || (!step_dev && step < 1)) return HYPAD_EINVAL;
  for (int i = 0; i < n; ++i) {
    const int m = t[i].manifold;
    if (t[i].rows < 0 || t[i].dim <= 0 || (m != HYPAD_MANIFOLD_EUCLIDEAN && m != HYPAD_MANIFOLD_BALL && m != HYPAD_MANIFOLD_SPHERE)) return HYPAD_EINVAL;
  }
  for (int i = 0; i < n; ++i)
    if (t[i].dim > MAX_D || t[i].rows > INT_LIMIT / t[i].dim) return HYPAD_EUNSUPPORTED;
  for (int i = 0; i < n; ++i) {
    if (t[i].rows == 0) continue;
    const int64_t full = t[i].rows * t[i].dim;
    if (t[i].manifold == HYPAD_MANIFOLD_EUCLIDEAN ? (t[i].numel > full || t[i].numel <= full - t[i].dim) : t[i].numel != full) return HYPAD_EINVAL;
    if (!t[i].param || !t[i].grad) return HYPAD_EINVAL;
    if (sgd ? (t[i].state0 != nullptr) != has_momentum : (!t[i].state0 || !t[i].state1)) return HYPAD_EINVAL;
  }
  return HYPAD_OK;
}

template <class R>
int launch(const hypad_optim_tensor* t, int n, const int32_t* step_dev, const float* lr_dev, const R& h, hypad_stream_t s) {
  Group grp = {};
  int64_t total = 0;
  for (int i = 0; i < GROUP_MAX; ++i) {
    if (i < n) {
      grp.t[i] = t[i];
      total += t[i].rows;
    }
    grp.end[i] = total;
  }
  if (total == 0) return HYPAD_OK;
  const Clock clk = {step_dev, lr_dev};
  hipLaunchKernelGGL((optim_group_kernel<R>), dim3(wave_grid(total)), dim3(THREADS), 0, (hipStream_t)s, grp, clk, h);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

}  // namespace

extern "C" {

int hypad_optim_step_advance(int32_t* step, hypad_stream_t s) {
  if (!step) return HYPAD_EINVAL;
  hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, step);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad_optim_group_adam(const hypad_optim_tensor* t, int n, const int32_t* step_dev, int step, const float* lr_dev, float lr, float b1,
                           float b2, float eps, float wd, int stabilize, hypad_stream_t s) {
  const int rc = group_check(t, n, step_dev, step, false, false);
  if (rc) return rc;
  const AdamRule h = {lr, b1, b2, eps, wd, step, stabilize};
  return launch(t, n, step_dev, lr_dev, h, s);
}

int hypad_optim_group_sgd(const hypad_optim_tensor* t, int n, const int32_t* step_dev, int step, const float* lr_dev, float lr, float momentum,
                          float dampening, float wd, int nesterov, int stabilize, hypad_stream_t s) {
  const int rc = group_check(t, n, step_dev, step, true, momentum != 0.f);
  if (rc) return rc;
  const SgdRule h = {lr, momentum, dampening, wd, nesterov, step, stabilize};
  return launch(t, n, step_dev, lr_dev, h, s);
}

}  // extern "C"
