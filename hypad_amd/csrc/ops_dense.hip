// Network forwards and the dense building blocks, as row-tile kernels:
// one workgroup = 16 (or 32) window rows carried through every layer with activations in LDS.
// Also the stand-alone optimiser steps (hypad_adam_step, hypad_radam_step).
// The T = 1 bidirectional LSTM layer: its streamed forward (lstm_fwd_kernel) and its backward are here; the weights-stationary
// forwards that take over from 2 048 rows on, with their launch rule, are in lstm_t1_lds.hip (hypad_lstm_bidir_fwd asks it first).
#include <hip/hip_runtime.h>

#include "../../include/hypad.h"
#include "nets.h"
#include "train_common.h"

using namespace hypad;

namespace {

constexpr int THREADS = 256;
constexpr int WST = (THREADS / 64) * WSTAGE_FLOATS;     // wave-private weight slabs of gemm_nt

__host__ __device__ inline int ld_of(int n) { return pad4(n) + 4; }

__device__ __forceinline__ DropSrc make_drop(const hypad_dropout& d, int batch, uint32_t stream, float p) {
  DropSrc s;
  s.mode = d.train_mode ? (d.masks ? 1 : 2) : 0;
  s.ptr = d.masks; s.batch = batch; s.seed = d.seed; s.tick = (uint32_t)d.offset; s.stream = stream; s.sig = 0; s.p = p;
  return s;
}

// ------------------------------------------------------------------------------------------ generic linear
__global__ __launch_bounds__(THREADS) void linear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ b, float* __restrict__ y,
                                                              int64_t rows, int K, int N, int act) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldx = ld_of(K), ldy = ld_of(N);
  float* xs = smem;
  float* ys = xs + 16 * ldx;
  float* wst = ys + 16 * ldy;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, rows - r0);
  tile_load(xs, ldx, x + r0 * K, K, 16, K, valid);
  __syncthreads();
  gemm_nt<1, true>(xs, ldx, w, K, K, N, identity_map(), b, nullptr, ys, ldy, 0, wst);
  __syncthreads();
  for (int i = threadIdx.x; i < valid * N; i += THREADS) {
    int r = i / N, c = i - r * N;
    float v = ys[r * ldy + c];
    if (act == HYPAD_ACT_TANH) v = tanhf(v);
    else if (act == HYPAD_ACT_LEAKY02) v = v > 0.f ? v : LEAK * v;
    y[(r0 + r) * N + c] = v;
  }
}

// grad_pre = grad_y * act'(y) -> scratch (rows, N) ; grad_x = grad_pre W
__global__ __launch_bounds__(THREADS) void linear_bwd_data_kernel(const float* __restrict__ w, const float* __restrict__ y,
                                                                   const float* __restrict__ gy, float* __restrict__ gpre,
                                                                   float* __restrict__ gx, int64_t rows, int K, int N, int act) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldd = ld_of(N), ldx = ld_of(K);
  float* ds = smem;
  float* xs = ds + 16 * ldd;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, rows - r0);
  for (int i = threadIdx.x; i < 16 * N; i += THREADS) {
    int r = i / N, c = i - r * N;
    float v = 0.f;
    if (r < valid) {
      v = gy[(r0 + r) * N + c];
      float o = y ? y[(r0 + r) * N + c] : 0.f;
      if (act == HYPAD_ACT_TANH) v *= 1.f - o * o;
      else if (act == HYPAD_ACT_LEAKY02) v *= o > 0.f ? 1.f : LEAK;
      if (gpre) gpre[(r0 + r) * N + c] = v;
    }
    ds[r * ldd + c] = v;
  }
  __syncthreads();
  if (gx) {
    gemm_nn<1>(ds, ldd, 0, w, K, N, identity_map(), K, xs, ldx, false);
    __syncthreads();
    tile_store(gx + r0 * K, K, xs, ldx, 16, K, valid);
  }
}

// grad_w[n][k] = sum_r left[r][n] * right[r][k]; 16x16 tile per wave on MFMA; optional bias column sums.
__global__ __launch_bounds__(THREADS) void outer_sum_kernel(const float* __restrict__ left, int ldl, const float* __restrict__ right,
                                                             int ldr, float* __restrict__ gw, float* __restrict__ gb,
                                                             int64_t rows, int N, int K) {
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int j = lane & 15, q = lane >> 4;
  const int tk = (K + 15) >> 4, tn = (N + 15) >> 4;
  const int tile = blockIdx.x * 4 + wave;
  if (tile < tn * tk) {
    const int n0 = (tile / tk) * 16, k0 = (tile % tk) * 16;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t rr = 0; rr < rows; rr += 4) {
      const int64_t r = rr + q;
      const float a = (r < rows && n0 + j < N) ? left[r * ldl + n0 + j] : 0.f;
      const float b = (r < rows && k0 + j < K) ? right[r * ldr + k0 + j] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int n = n0 + 4 * q + r, k = k0 + j;
      if (n < N && k < K) gw[(size_t)n * K + k] = acc[r];
    }
  }
  if (gb) {
    int n = blockIdx.x * THREADS + threadIdx.x;
    if (n < N) {
      float s = 0.f;
      for (int64_t r = 0; r < rows; ++r) s += left[r * ldl + n];
      gb[n] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------ generic BiLSTM (T=1)
__global__ __launch_bounds__(THREADS) void lstm_fwd_kernel(const float* __restrict__ x, const float* wf, const float* bif,
                                                            const float* bhf, const float* wr, const float* bir,
                                                            const float* bhr, float* __restrict__ out,
                                                            float* __restrict__ gates_save, int64_t rows, int K, int H) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldx = ld_of(K), ldg = ld_of(6 * H), ldh = ld_of(2 * H);
  float* xs = smem;
  float* gs = xs + 16 * ldx;
  float* hs = gs + 16 * ldg;
  float* wst = hs + 16 * ldh;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, rows - r0);
  tile_load(xs, ldx, x + r0 * K, K, 16, K, valid);
  __syncthreads();
  gemm_nt<1, true>(xs, ldx, wf, K, K, 3 * H, lstm_gate_map(H), bif, bhf, gs, ldg, 0, wst);
  gemm_nt<1, true>(xs, ldx, wr, K, K, 3 * H, lstm_gate_map(H), bir, bhr, gs, ldg, 3 * H, wst);
  __syncthreads();
  lstm_cell_tile(gs, ldg, H, 16, hs, ldh, gates_save ? gates_save + r0 * 8 * H : nullptr, valid);
  __syncthreads();
  tile_store(out + r0 * 2 * H, 2 * H, hs, ldh, 16, 2 * H, valid);
}

__global__ __launch_bounds__(THREADS) void lstm_bwd_kernel(const float* wf, const float* wr, const float* __restrict__ gates_saved,
                                                            const float* __restrict__ gout, float* __restrict__ ggates,
                                                            float* __restrict__ gx, int64_t rows, int K, int H) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldx = ld_of(K), ldg = ld_of(6 * H), ldh = ld_of(2 * H);
  float* dhs = smem;
  float* dgs = dhs + 16 * ldh;
  float* xs = dgs + 16 * ldg;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, rows - r0);
  tile_load(dhs, ldh, gout + r0 * 2 * H, 2 * H, 16, 2 * H, valid);
  __syncthreads();
  lstm_cell_bwd_tile(dhs, ldh, gates_saved + r0 * 8 * H, H, 16, dgs, ldg, valid);
  __syncthreads();
  if (ggates) {   // (rows, 2, 4H) in PyTorch gate order, f block zero
    for (int i = threadIdx.x; i < valid * 8 * H; i += THREADS) {
      int r = i / (8 * H), c = i - r * 8 * H;
      int d = c / (4 * H), g = (c - d * 4 * H) / H, jj = c - d * 4 * H - g * H;
      float v = 0.f;
      if (g != 1) v = dgs[r * ldg + d * 3 * H + (g == 0 ? 0 : g - 1) * H + jj];
      ggates[(r0 + r) * 8 * H + c] = v;
    }
  }
  if (gx) {
    gemm_nn<1>(dgs, ldg, 0, wf, K, 3 * H, lstm_gate_map(H), K, xs, ldx, false);
    gemm_nn<1>(dgs, ldg, 3 * H, wr, K, 3 * H, lstm_gate_map(H), K, xs, ldx, true);
    __syncthreads();
    tile_store(gx + r0 * K, K, xs, ldx, 16, K, valid);
  }
}

// ------------------------------------------------------------------------------------------ networks
struct NetLds {          // float offsets into dynamic LDS for the network kernels
  int xs, zs, bufA, bufB, crit, wst, total;
  int ldS, bufFloats;
};
__host__ __device__ inline NetLds net_lds(int S, int MT) {
  NetLds n;
  n.ldS = lds_stride(S);
  int rows = MT * 16;
  int per_row = n.ldS > 6 * DEC_H + 4 ? n.ldS : 6 * DEC_H + 4;
  n.bufFloats = rows * per_row;
  int o = 0;
  n.xs = o; o += 16 * n.ldS;
  n.zs = o; o += rows * LP;
  n.bufA = o; o += n.bufFloats;
  n.bufB = o; o += n.bufFloats;
  n.crit = o; o += CRITIC_LDS_FLOATS;
  n.wst = o; o += WST;
  n.total = o;
  return n;
}

__global__ __launch_bounds__(THREADS) void encoder_fwd_kernel(const float* __restrict__ P, const float* __restrict__ x,
                                                               float* __restrict__ out, int64_t rows, int S, int L) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const NetLds nl = net_lds(S, 1);
  const EncLayout el = enc_layout(S, L);
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, rows - r0);
  tile_load(smem + nl.xs, nl.ldS, x + r0 * S, S, 16, S, valid);
  __syncthreads();
  encoder_fwd_tile(smem + nl.xs, nl.ldS, S, L, P, el, smem + nl.bufA, ENC_LDG, smem + nl.bufB, ENC_LDH,
                   smem + nl.zs, nullptr, nullptr, valid, smem + nl.wst);
  tile_store(out + r0 * L, L, smem + nl.zs, LP, 16, L, valid);
}

template <int MT>
__global__ __launch_bounds__(THREADS) void decoder_fwd_kernel(const float* __restrict__ P, const float* __restrict__ z,
                                                               float* __restrict__ hyper, float* __restrict__ eucl,
                                                               int64_t rows, int S, int L, int hyperbolic, hypad_dropout dp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = MT * 16;
  const NetLds nl = net_lds(S, MT);
  const DecLayout dl = dec_layout(S, L, hyperbolic);
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int valid = (int)min((int64_t)R, rows - r0);
  float* zs = smem + nl.zs; float* bufA = smem + nl.bufA; float* bufB = smem + nl.bufB;
  tile_load(zs, LP, z + r0 * L, L, R, L, valid);
  __syncthreads();
  DropSrc drop = make_drop(dp, (int)rows, RS_DROP_DEC0, 0.2f);
  DecSave none{16, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const int base_row = (int)r0;
  decoder_trunk_fwd_tile<MT>(zs, L, S, P, dl, bufA, bufB, nl.ldS, drop, [base_row](int r) { return base_row + r; }, none, valid,
                             smem + nl.wst);
  if (eucl) tile_store(eucl + r0 * S, S, bufA, nl.ldS, R, S, valid);
  if (hyperbolic && hyper) {
    gemm_nt<MT>(bufA, nl.ldS, P + dl.head_w, S, S, S, identity_map(), nullptr, nullptr, bufB, nl.ldS, 0, smem + nl.wst);
    __syncthreads();
    head_rows_tile(bufB, nl.ldS, R, S, P + dl.head_b);
    __syncthreads();
    tile_store(hyper + r0 * S, S, bufB, nl.ldS, R, S, valid);
  }
}

__global__ __launch_bounds__(THREADS) void critic_fwd_kernel(const float* __restrict__ P, const float* __restrict__ x,
                                                              float* __restrict__ out, int64_t rows, int in_dim, int L,
                                                              int nh, float p, hypad_dropout dp) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldx = pad4(in_dim) + 4;
  float* xs = smem;
  CriticLds cs = critic_lds(smem + 16 * ldx);
  float* wst = smem + 16 * ldx + CRITIC_LDS_FLOATS;
  // (only the scalar fields: critic_fwd_tile takes its offsets from the closed forms wof / bof -- filling the w[] / b[] tables with a
  // run-time layer count put the struct into 64 bytes of scratch per lane)
  CriticLayout cl; cl.nh = nh; cl.in_dim = in_dim; cl.L = L; cl.p_drop = p; cl.total = 0;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, rows - r0);
  tile_load(xs, ldx, x + r0 * in_dim, in_dim, 16, in_dim, valid);
  __syncthreads();
  DropSrc drop = make_drop(dp, (int)rows, RS_DROP_CRITIC, p);
  critic_fwd_tile(xs, ldx, P, cl, L, cs, drop, (int)r0, wst);
  if (threadIdx.x < valid) out[r0 + threadIdx.x] = cs.out[threadIdx.x];
}

// mobius_linear forward: u = x W^T (saved) ; out = head(u)
__global__ __launch_bounds__(THREADS) void mobius_linear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, float* __restrict__ out,
                                                                     float* __restrict__ u_save, int64_t rows, int K, int N) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldx = ld_of(K), ldy = ld_of(N);
  float* xs = smem;
  float* ys = xs + 16 * ldx;
  float* wst = ys + 16 * ldy;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, rows - r0);
  tile_load(xs, ldx, x + r0 * K, K, 16, K, valid);
  __syncthreads();
  gemm_nt<1, true>(xs, ldx, w, K, K, N, identity_map(), nullptr, nullptr, ys, ldy, 0, wst);
  __syncthreads();
  if (u_save) tile_store(u_save + r0 * N, N, ys, ldy, 16, N, valid);
  __syncthreads();
  head_rows_tile(ys, ldy, 16, N, bias);
  __syncthreads();
  tile_store(out + r0 * N, N, ys, ldy, 16, N, valid);
}

// mobius_linear in every configuration (hyrnn_nets.py:13-35), and the bare Moebius matvec (project = 0, no bias, no non-linearity):
// mx = x W^T (saved) ; out = chain(mx, |x|) -- rowops.h: mobius_chain_row.  Ys[16][ldy] holds mx and is rewritten in place; the
// row norms of x come from its LDS tile.  Four rows per wave, one per group of 16 lanes, as head_rows_tile, in fp64 registers (rowops.h); a Euclidean bias is
// mapped onto the ball once per wave, in registers, before the rows.
__device__ __forceinline__ void mobius_chain_rows_tile(float* Ys, int ldy, const float* Xs, int ldx, int K, int N, const float* bias_g,
                                                       int flags, int nonlin, int project) {
  const int lane = threadIdx.x & 63, wave = wave_id(), nw = blockDim.x >> 6, sub = lane >> 4;
  const MobiusCfg cfg{(flags & HYPAD_ML_HYPER_INPUT) != 0, bias_g != nullptr, project != 0, nonlin};
  epl16_dispatch(N, [&](auto tag) {
    using R = RowD<16, decltype(tag)::value>;
    R b = {};
    if (cfg.has_bias) {
      b = rowd_load<R>(bias_g, N, lane);
      if (!(flags & HYPAD_ML_HYPER_BIAS)) b = radial_map_d<true>(b);
    }
    for (int r0 = wave * 4; r0 < 16; r0 += nw * 4) {
      const int r = r0 + sub;
      double xraw = 0.0;
      if (cfg.hyper_in) {
        double s = 0.0;
        for (int c = lane & 15; c < K; c += 16) { const double v = Xs[r * ldx + c]; s += v * v; }
        xraw = sqrt(groupd_sum<16>(s));
      }
      const R o = mobius_chain_row(rowd_load<R>(Ys + r * ldy, N, lane), xraw, b, cfg);
      rowd_store(Ys + r * ldy, o, N, lane);
    }
  });
}
__global__ __launch_bounds__(THREADS) void mobius_linear_ex_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                        const float* __restrict__ bias, float* __restrict__ out,
                                                                        float* __restrict__ mx_save, int64_t rows, int K, int N,
                                                                        int flags, int nonlin, int project) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ldx = ld_of(K), ldy = ld_of(N);
  float* xs = smem;
  float* ys = xs + 16 * ldx;
  float* wst = ys + 16 * ldy;
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, rows - r0);
  tile_load(xs, ldx, x + r0 * K, K, 16, K, valid);
  __syncthreads();
  gemm_nt<1, true>(xs, ldx, w, K, K, N, identity_map(), nullptr, nullptr, ys, ldy, 0, wst);
  __syncthreads();
  if (mx_save) tile_store(mx_save + r0 * N, N, ys, ldy, 16, N, valid);
  __syncthreads();
  mobius_chain_rows_tile(ys, ldy, xs, ldx, K, N, bias, flags, nonlin, project);
  __syncthreads();
  tile_store(out + r0 * N, N, ys, ldy, 16, N, valid);
}

// fused scoring forward (anomaly_detection.py:67-113 + utils/anomaly_detection_utils.py:58-66)
__global__ __launch_bounds__(THREADS) void score_forward_kernel(const float* __restrict__ PE, const float* __restrict__ PD,
                                                                 const float* __restrict__ PC, const float* __restrict__ x,
                                                                 float* __restrict__ hyper, float* __restrict__ eucl,
                                                                 float* __restrict__ hyper_real, float* __restrict__ critic,
                                                                 float* __restrict__ rowdist, int64_t rows, int S, int L,
                                                                 int hyperbolic) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const NetLds nl = net_lds(S, 2);      // bufA/bufB sized for 32 rows: decoder rows 0..15, head(x) rows 16..31
  const EncLayout el = enc_layout(S, L);
  const DecLayout dl = dec_layout(S, L, hyperbolic);
  const CriticLayout cl = cx_layout(S, L);
  const int64_t r0 = (int64_t)blockIdx.x * 16;
  const int valid = (int)min((int64_t)16, rows - r0);
  float* xs = smem + nl.xs; float* zs = smem + nl.zs; float* bufA = smem + nl.bufA; float* bufB = smem + nl.bufB;
  CriticLds cs = critic_lds(smem + nl.crit);
  tile_load(xs, nl.ldS, x + r0 * S, S, 16, S, valid);
  __syncthreads();
  if (critic) {
    critic_fwd_tile(xs, nl.ldS, PC, cl, L, cs, no_drop(), 0, smem + nl.wst);
    if (threadIdx.x < valid) critic[r0 + threadIdx.x] = cs.out[threadIdx.x];
  }
  encoder_fwd_tile(xs, nl.ldS, S, L, PE, el, bufA, ENC_LDG, bufB, ENC_LDH, zs, nullptr, nullptr, valid, smem + nl.wst);
  DecSave none{16, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  decoder_trunk_fwd_tile<1>(zs, L, S, PD, dl, bufA, bufB, nl.ldS, no_drop(), [](int r) { return r; }, none, valid, smem + nl.wst);
  if (eucl) tile_store(eucl + r0 * S, S, bufA, nl.ldS, 16, S, valid);
  if (hyperbolic) {
    // rows 16..31 of bufA <- x: one head GEMM serves decoder output and the real window
    for (int i = threadIdx.x; i < 16 * nl.ldS; i += THREADS) bufA[16 * nl.ldS + i] = xs[i];
    __syncthreads();
    gemm_nt<2>(bufA, nl.ldS, PD + dl.head_w, S, S, S, identity_map(), nullptr, nullptr, bufB, nl.ldS, 0, smem + nl.wst);
    __syncthreads();
    head_rows_tile(bufB, nl.ldS, 32, S, PD + dl.head_b);
    __syncthreads();
    if (hyper) tile_store(hyper + r0 * S, S, bufB, nl.ldS, 16, S, valid);
    if (hyper_real) tile_store(hyper_real + r0 * S, S, bufB + 16 * nl.ldS, nl.ldS, 16, S, valid);
    if (rowdist) {
      const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      for (int r = wave; r < valid; r += 4) {
        // (pred = real window on the ball, true = reconstruction): anomaly_detection_utils.py:58-65
        float d = rowdist_row(row_load(bufB + (16 + r) * nl.ldS, S, lane), row_load(bufB + r * nl.ldS, S, lane));
        if (lane == 0) rowdist[r0 + r] = d;
      }
    }
  }
}

inline int tiles16(int64_t rows) { return (int)((rows + 15) / 16); }

// zeros on the caller's stream (a parameter gradient summed over no rows); p may be null
inline int zero_floats(float* p, size_t n, hypad_stream_t s) {
  if (!p) return HYPAD_OK;
  hipError_t e = hipMemsetAsync(p, 0, n * sizeof(float), (hipStream_t)s);
  return e == hipSuccess ? HYPAD_OK : (int)e;
}

// ---- stand-alone optimizers (the update rules of the training kernels: train_common.h)
using train::AdamCoef; using train::adam_coef; using train::adam_update; using train::radam_ball_wave;
__global__ __launch_bounds__(THREADS) void adam_flat_kernel(float* p, const float* g, float* m, float* v, int64_t n, int step,
                                                             float lr, float b1, float b2, float eps, float wd, int riem,
                                                             int64_t ball_off, int ball_dim) {
  const AdamCoef co = adam_coef(lr, b1, b2, eps, wd, riem, 0, step);
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
    if (ball_dim > 0 && i >= ball_off && i < ball_off + ball_dim) continue;
    float pp = p[i], mm = m[i], vv = v[i];
    float gg = g[i];
    if (!riem) gg += wd * pp;     // torch.optim.Adam weight_decay: L2 into the gradient
    adam_update(pp, mm, vv, gg, co);
    p[i] = pp; m[i] = mm; v[i] = vv;
  }
}
__global__ __launch_bounds__(64) void radam_ball_kernel(float* p, const float* g, float* m, float* v, int dim, int step, float lr,
                                                         float b1, float b2, float eps, float wd, int stabilize) {
  const AdamCoef co = adam_coef(lr, b1, b2, eps, wd, 1, stabilize, step);
  radam_ball_wave(p, m, v, row_load(g, dim, threadIdx.x), dim, threadIdx.x, co);
}

}  // namespace

extern "C" {

int hypad_linear_act_fwd(const float* x, const float* w, const float* b, float* y, int64_t rows, int K, int N, int act,
                         hypad_stream_t s) {
  if (!w || rows < 0 || K <= 0 || N <= 0) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;                          // (an empty batch has no rows to point at: x / y may be NULL)
  if (!x || !y) return HYPAD_EINVAL;
  size_t lds = (size_t)(16 * (ld_of(K) + ld_of(N)) + WST) * sizeof(float);
  if (lds > 150 * 1024) return HYPAD_EUNSUPPORTED;
  hipError_t e = allow_lds((const void*)linear_fwd_kernel, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(linear_fwd_kernel, dim3(tiles16(rows)), dim3(THREADS), lds, (hipStream_t)s, x, w, b, y, rows, K, N, act);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad_linear_act_bwd(const float* x, const float* w, const float* y, const float* gy, float* gx, float* gw, float* gb,
                         float* gpre, int64_t rows, int K, int N, int act, hypad_stream_t s) {
  if (!w || rows < 0 || K <= 0 || N <= 0) return HYPAD_EINVAL;
  if (gb && !gw) return HYPAD_EINVAL;                      // (the bias sums ride in the weight-gradient launch)
  if (rows == 0) {
    // an empty batch (its row buffers may be NULL): the sums over no rows are zeros, written like any other result
    int rc = zero_floats(gw, (size_t)N * K, s);
    return rc ? rc : zero_floats(gb, (size_t)N, s);
  }
  if (!gy) return HYPAD_EINVAL;
  if (act != HYPAD_ACT_NONE && !y) return HYPAD_EINVAL;
  if (gw && (!gpre || !x)) return HYPAD_EINVAL;
  size_t lds = (size_t)16 * (ld_of(K) + ld_of(N)) * sizeof(float);
  if (lds > 150 * 1024) return HYPAD_EUNSUPPORTED;
  hipError_t e = allow_lds((const void*)linear_bwd_data_kernel, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(linear_bwd_data_kernel, dim3(tiles16(rows)), dim3(THREADS), lds, (hipStream_t)s, w, y, gy, gpre, gx,
                     rows, K, N, act);
  HYPAD_CHECK_LAUNCH();
  if (gw) {
    int tiles = ((N + 15) / 16) * ((K + 15) / 16);
    int blocks = (tiles + 3) / 4;
    int bb = (N + THREADS - 1) / THREADS;
    if (bb > blocks) blocks = bb;
    hipLaunchKernelGGL(outer_sum_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)s, gpre, N, x, K, gw, gb, rows, N, K);
    HYPAD_CHECK_LAUNCH();
  }
  return HYPAD_OK;
}

int hypad_lstm_bidir_fwd(const float* x, const float* wf, const float* bif, const float* bhf, const float* wr,
                         const float* bir, const float* bhr, float* out, float* gates_save, int64_t rows, int K, int H,
                         hypad_stream_t s) {
  if (!wf || !bif || !bhf || !wr || !bir || !bhr || rows < 0 || K <= 0 || H <= 0) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  if (!x || !out) return HYPAD_EINVAL;
  // many rows: the weights-stationary forms (lstm_t1_lds.hip); any other shape: the streamed form
  bool launched = false;
  const int rc = lstm_t1_lds_launch(x, wf, bif, bhf, wr, bir, bhr, out, gates_save, rows, K, H, s, &launched);
  if (rc || launched) return rc;
  size_t lds = (size_t)(16 * (ld_of(K) + ld_of(6 * H) + ld_of(2 * H)) + WST) * sizeof(float);
  if (lds > 150 * 1024) return HYPAD_EUNSUPPORTED;
  hipError_t e = allow_lds((const void*)lstm_fwd_kernel, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(lstm_fwd_kernel, dim3(tiles16(rows)), dim3(THREADS), lds, (hipStream_t)s, x, wf, bif, bhf, wr, bir, bhr,
                     out, gates_save, rows, K, H);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad_lstm_bidir_bwd(const float* wf, const float* wr, const float* gates_saved, const float* gout, float* ggates,
                         float* gx, int64_t rows, int K, int H, hypad_stream_t s) {
  if (!wf || !wr || rows < 0 || K <= 0 || H <= 0) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  if (!gates_saved || !gout) return HYPAD_EINVAL;
  size_t lds = (size_t)16 * (ld_of(K) + ld_of(6 * H) + ld_of(2 * H)) * sizeof(float);
  if (lds > 150 * 1024) return HYPAD_EUNSUPPORTED;
  hipError_t e = allow_lds((const void*)lstm_bwd_kernel, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(lstm_bwd_kernel, dim3(tiles16(rows)), dim3(THREADS), lds, (hipStream_t)s, wf, wr, gates_saved, gout,
                     ggates, gx, rows, K, H);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

static int check_net(int S, int L) {
  if (S <= 0 || L <= 0) return HYPAD_EINVAL;
  if (S > MAX_S || L > MAX_L) return HYPAD_EUNSUPPORTED;
  return HYPAD_OK;
}

int hypad_encoder_fwd(const float* P, const float* x, float* out, int64_t rows, int S, int L, hypad_stream_t s) {
  int rc = check_net(S, L);
  if (rc) return rc;
  if (!P || !x || !out || rows < 0) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  size_t lds = (size_t)net_lds(S, 1).total * sizeof(float);
  hipError_t e = allow_lds((const void*)encoder_fwd_kernel, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(encoder_fwd_kernel, dim3(tiles16(rows)), dim3(THREADS), lds, (hipStream_t)s, P, x, out, rows, S, L);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad_decoder_fwd(const float* P, const float* z, float* hyper, float* eucl, int64_t rows, int S, int L, int hyperbolic,
                      const hypad_dropout* drop, hypad_stream_t s) {
  int rc = check_net(S, L);
  if (rc) return rc;
  if (!P || !z || rows < 0 || (!hyper && !eucl)) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  hypad_dropout dp = drop ? *drop : hypad_dropout{0, nullptr, 0, 0};
  if (rows >= 32 * 512) {
    size_t lds = (size_t)net_lds(S, 2).total * sizeof(float);
    hipError_t e = allow_lds((const void*)decoder_fwd_kernel<2>, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(decoder_fwd_kernel<2>, dim3((int)((rows + 31) / 32)), dim3(THREADS), lds, (hipStream_t)s, P, z, hyper,
                       eucl, rows, S, L, hyperbolic, dp);
  } else {
    size_t lds = (size_t)net_lds(S, 1).total * sizeof(float);
    hipError_t e = allow_lds((const void*)decoder_fwd_kernel<1>, lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(decoder_fwd_kernel<1>, dim3(tiles16(rows)), dim3(THREADS), lds, (hipStream_t)s, P, z, hyper, eucl,
                       rows, S, L, hyperbolic, dp);
  }
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

static int critic_fwd(const float* P, const float* x, float* out, int64_t rows, int in_dim, int L, int nh, float p,
                      const hypad_dropout* drop, hypad_stream_t s) {
  if (!P || !x || !out || rows < 0) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  hypad_dropout dp = drop ? *drop : hypad_dropout{0, nullptr, 0, 0};
  size_t lds = (size_t)(16 * (pad4(in_dim) + 4) + CRITIC_LDS_FLOATS + WST) * sizeof(float);
  hipLaunchKernelGGL(critic_fwd_kernel, dim3(tiles16(rows)), dim3(THREADS), lds, (hipStream_t)s, P, x, out, rows, in_dim, L,
                     nh, p, dp);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_critic_x_fwd(const float* P, const float* x, float* out, int64_t rows, int S, int L, const hypad_dropout* drop,
                       hypad_stream_t s) {
  int rc = check_net(S, L);
  if (rc) return rc;
  return critic_fwd(P, x, out, rows, S, L, 4, 0.25f, drop, s);
}
int hypad_critic_z_fwd(const float* P, const float* z, float* out, int64_t rows, int L, const hypad_dropout* drop,
                       hypad_stream_t s) {
  int rc = check_net(1, L);
  if (rc) return rc;
  return critic_fwd(P, z, out, rows, L, L, 2, 0.2f, drop, s);
}

size_t hypad_mobius_linear_workspace_bytes(int64_t rows, int out_dim) {
  return (size_t)rows * out_dim * 2 * sizeof(float);   // grad_u and per-row bias gradients
}
int hypad_mobius_linear_fwd(const float* x, const float* w, const float* bias, float* out, float* u_save, int64_t rows,
                            int K, int N, hypad_stream_t s) {
  if (!w || !bias || rows < 0 || K <= 0 || N <= 0) return HYPAD_EINVAL;
  if (N > 64 * MAX_EPL) return HYPAD_EUNSUPPORTED;
  if (rows == 0) return HYPAD_OK;
  if (!x || !out) return HYPAD_EINVAL;
  size_t lds = (size_t)(16 * (ld_of(K) + ld_of(N)) + WST) * sizeof(float);
  if (lds > 150 * 1024) return HYPAD_EUNSUPPORTED;
  hipError_t e = allow_lds((const void*)mobius_linear_fwd_kernel, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(mobius_linear_fwd_kernel, dim3(tiles16(rows)), dim3(THREADS), lds, (hipStream_t)s, x, w, bias, out,
                     u_save, rows, K, N);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_mobius_linear_bwd(const float* x, const float* w, const float* bias, const float* u_saved, const float* go,
                            float* gx, float* gw, float* gbias, void* workspace, size_t workspace_bytes, int64_t rows,
                            int K, int N, hypad_stream_t s) {
  if (!w || !bias || rows < 0 || K <= 0 || N <= 0) return HYPAD_EINVAL;
  if (N > 64 * MAX_EPL) return HYPAD_EUNSUPPORTED;
  if (rows == 0) {                                         // an empty batch: zeros for the parameter gradients (hypad_linear_act_bwd)
    int rc = zero_floats(gbias, (size_t)N, s);
    return rc ? rc : hypad_linear_act_bwd(nullptr, w, nullptr, nullptr, nullptr, gw, nullptr, nullptr, 0, K, N, HYPAD_ACT_NONE, s);
  }
  if (!x || !u_saved || !go) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < hypad_mobius_linear_workspace_bytes(rows, N)) return HYPAD_EWORKSPACE;
  float* gu = (float*)workspace;
  float* gb_rows = gu + (size_t)rows * N;
  int rc = hypad_mobius_head_bwd(u_saved, bias, go, gu, gb_rows, rows, N, s);
  if (rc) return rc;
  if (gbias) {
    rc = hypad_column_sum(gb_rows, gbias, rows, N, s);
    if (rc) return rc;
  }
  // grad_x = gu W ; grad_w = gu^T x
  return hypad_linear_act_bwd(x, w, nullptr, gu, gx, gw, nullptr, gw ? gb_rows /*scratch for grad_pre*/ : nullptr, rows, K, N,
                              HYPAD_ACT_NONE, s);
}

// ---- mobius_linear in every configuration; the bare matvec is the same pair of launches without bias, non-linearity and project
static int mobius_ex_check(const float* w, int64_t rows, int K, int N, int flags, int nonlin, bool fwd) {
  if (!w || rows < 0 || K <= 0 || N <= 0) return HYPAD_EINVAL;
  if ((flags & ~(HYPAD_ML_HYPER_INPUT | HYPAD_ML_HYPER_BIAS)) || nonlin < HYPAD_NONLIN_NONE || nonlin > HYPAD_NONLIN_RELU) return HYPAD_EINVAL;
  if (N > 64 * MAX_EPL) return HYPAD_EUNSUPPORTED;
  // (the backward's LDS is that of hypad_linear_act_bwd: refused here, before the row kernel has written anything)
  if ((size_t)(16 * (ld_of(K) + ld_of(N)) + (fwd ? WST : 0)) * sizeof(float) > 150 * 1024) return HYPAD_EUNSUPPORTED;
  return HYPAD_OK;
}
static int mobius_ex_fwd(const float* x, const float* w, const float* bias, float* out, float* mx_save, int64_t rows, int K, int N,
                         int flags, int nonlin, int project, hypad_stream_t s) {
  int rc = mobius_ex_check(w, rows, K, N, flags, nonlin, true);
  if (rc) return rc;
  if (rows == 0) return HYPAD_OK;
  if (!x || !out) return HYPAD_EINVAL;
  size_t lds = (size_t)(16 * (ld_of(K) + ld_of(N)) + WST) * sizeof(float);
  hipError_t e = allow_lds((const void*)mobius_linear_ex_fwd_kernel, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(mobius_linear_ex_fwd_kernel, dim3(tiles16(rows)), dim3(THREADS), lds, (hipStream_t)s, x, w, bias, out, mx_save,
                     rows, K, N, flags, nonlin, project);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
static int mobius_ex_bwd(const float* x, const float* w, const float* bias, const float* mx_saved, const float* go, float* gx,
                         float* gw, float* gbias, void* workspace, size_t workspace_bytes, int64_t rows, int K, int N, int flags,
                         int nonlin, int project, hypad_stream_t s) {
  int rc = mobius_ex_check(w, rows, K, N, flags, nonlin, false);
  if (rc) return rc;
  if (gbias && !bias) return HYPAD_EINVAL;
  if (rows == 0) {                                         // an empty batch: zeros for the parameter gradients (hypad_mobius_linear_bwd)
    rc = zero_floats(gbias, (size_t)N, s);
    return rc ? rc : zero_floats(gw, (size_t)N * K, s);
  }
  if (!x || !mx_saved || !go) return HYPAD_EINVAL;
  if (!workspace || workspace_bytes < hypad_mobius_linear_ex_workspace_bytes(rows, N)) return HYPAD_EWORKSPACE;
  const bool hyper_in = (flags & HYPAD_ML_HYPER_INPUT) != 0, hyper_bias = (flags & HYPAD_ML_HYPER_BIAS) != 0;
  float* gmx = (float*)workspace;                          // (rows, N)
  float* gb_rows = gmx + (size_t)rows * N;                 // (rows, N): per-row bias gradients, then grad_pre scratch
  float* gxn = gb_rows + (size_t)rows * N;                 // (rows): dL/d|x|
  float* gball = gxn + rows;                               // (N): the gradient of the mapped bias
  rc = mobius_chain_bwd_launch(x, mx_saved, bias, go, gmx, gbias ? gb_rows : nullptr, hyper_in ? gxn : nullptr, rows, K, N, hyper_in,
                               hyper_bias, nonlin, project, s);
  if (rc) return rc;
  if (gbias) {
    rc = hypad_column_sum(gb_rows, hyper_bias ? gbias : gball, rows, N, s);
    if (rc) return rc;
    if (!hyper_bias) {                                     // bias -> expmap0(bias), once
      rc = hypad_expmap0_bwd(bias, gball, gbias, 1, N, s);
      if (rc) return rc;
    }
  }
  // grad_x = gmx W ; grad_w = gmx^T x
  rc = hypad_linear_act_bwd(x, w, nullptr, gmx, gx, gw, nullptr, gw ? gb_rows : nullptr, rows, K, N, HYPAD_ACT_NONE, s);
  if (rc || !hyper_in || !gx) return rc;
  return norm_grad_add_launch(x, gxn, gx, rows, K, s);     // grad_x += dL/d|x| x / |x|
}

size_t hypad_mobius_linear_ex_workspace_bytes(int64_t rows, int out_dim) {
  return ((size_t)rows * out_dim * 2 + (size_t)rows + (size_t)out_dim) * sizeof(float);
}
int hypad_mobius_linear_ex_fwd(const float* x, const float* w, const float* bias, float* out, float* mx_save, int64_t rows, int K,
                               int N, int flags, int nonlin, hypad_stream_t s) {
  return mobius_ex_fwd(x, w, bias, out, mx_save, rows, K, N, flags, nonlin, 1, s);
}
int hypad_mobius_linear_ex_bwd(const float* x, const float* w, const float* bias, const float* mx_saved, const float* go,
                               float* gx, float* gw, float* gbias, void* workspace, size_t workspace_bytes, int64_t rows, int K,
                               int N, int flags, int nonlin, hypad_stream_t s) {
  return mobius_ex_bwd(x, w, bias, mx_saved, go, gx, gw, gbias, workspace, workspace_bytes, rows, K, N, flags, nonlin, 1, s);
}
int hypad_mobius_matvec_fwd(const float* x, const float* w, float* out, float* mx_save, int64_t rows, int K, int N,
                            hypad_stream_t s) {
  return mobius_ex_fwd(x, w, nullptr, out, mx_save, rows, K, N, HYPAD_ML_HYPER_INPUT, HYPAD_NONLIN_NONE, 0, s);
}
int hypad_mobius_matvec_bwd(const float* x, const float* w, const float* mx_saved, const float* go, float* gx, float* gw,
                            void* workspace, size_t workspace_bytes, int64_t rows, int K, int N, hypad_stream_t s) {
  return mobius_ex_bwd(x, w, nullptr, mx_saved, go, gx, gw, nullptr, workspace, workspace_bytes, rows, K, N, HYPAD_ML_HYPER_INPUT,
                       HYPAD_NONLIN_NONE, 0, s);
}

int hypad_score_forward(const float* enc, const float* dec, const float* cx, const float* x, float* hyper, float* eucl,
                        float* hyper_real, float* critic, float* rowdist, int64_t rows, int S, int L, int hyperbolic,
                        hypad_stream_t s) {
  int rc = check_net(S, L);
  if (rc) return rc;
  if (!enc || !dec || !x || rows < 0 || (critic && !cx)) return HYPAD_EINVAL;
  if (rows == 0) return HYPAD_OK;
  size_t lds = (size_t)net_lds(S, 2).total * sizeof(float);
  hipError_t e = allow_lds((const void*)score_forward_kernel, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(score_forward_kernel, dim3(tiles16(rows)), dim3(THREADS), lds, (hipStream_t)s, enc, dec, cx, x, hyper,
                     eucl, hyper_real, critic, rowdist, rows, S, L, hyperbolic);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}

int hypad_adam_step(float* p, const float* g, float* m, float* v, int64_t n, int step, float lr, float b1, float b2, float eps,
                    float wd, hypad_stream_t s) {
  if (!p || !g || !m || !v || n < 0 || step < 1) return HYPAD_EINVAL;
  if (n == 0) return HYPAD_OK;
  int blocks = (int)((n + THREADS - 1) / THREADS);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(adam_flat_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)s, p, g, m, v, n, step, lr, b1, b2, eps, wd, 0,
                     (int64_t)0, 0);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
int hypad_radam_step(float* p, const float* g, float* m, float* v, int64_t n, int64_t ball_off, int ball_dim, int step, float lr,
                     float b1, float b2, float eps, float wd, int stabilize, hypad_stream_t s) {
  if (!p || !g || !m || !v || n < 0 || step < 1 || ball_dim < 0 || ball_dim > 64 * MAX_EPL) return HYPAD_EINVAL;
  if (ball_dim > 0 && (ball_off < 0 || ball_off + ball_dim > n)) return HYPAD_EINVAL;
  if (n == 0) return HYPAD_OK;
  int blocks = (int)((n + THREADS - 1) / THREADS);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(adam_flat_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)s, p, g, m, v, n, step, lr, b1, b2, eps, wd, 1,
                     ball_off, ball_dim);
  HYPAD_CHECK_LAUNCH();
  if (ball_dim > 0) {
    hipLaunchKernelGGL(radam_ball_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, p + ball_off, g + ball_off, m + ball_off,
                       v + ball_off, ball_dim, step, lr, b1, b2, eps, wd, stabilize);
    HYPAD_CHECK_LAUNCH();
  }
  return HYPAD_OK;
}

}  // extern "C"
