// One bidirectional LSTM layer at T = 1 for MANY rows: the three weights-stationary forwards (lstm_fwd_lds_kernel, lstm_fwd_lds2_kernel,
// lstm_fwd_lds3_kernel) and the rule that picks one, lstm_t1_lds_launch (rowops.h), which hypad_lstm_bidir_fwd asks before it runs the
// streamed lstm_fwd_kernel of ops_dense.hip.  The layer's backward is lstm_bwd_kernel, also there.
#include <hip/hip_runtime.h>

#include "../../include/hypad.h"
#include "rowops.h"
#include "tile_gemm.h"

using namespace hypad;

namespace {

// Dynamic LDS of the three kernels, in floats: each formula once, for the kernel's carving and for the launch.
// lstm_fwd_lds_kernel: [gate i, g, o][Hp units][ld = 16 KG + 4]
__host__ __device__ constexpr int lstm_lds_floats(int KG, int Hp) { return 3 * Hp * (KG * 16 + 4); }
// lstm_fwd_lds2_kernel: [column tile][16][ld] -- three per full 16-unit block, one for the remainder -- then bias_s[3][H]
__host__ __device__ constexpr int lstm_lds2_floats(int K, int H) { return (3 * (H / 16) + (H % 16 ? 1 : 0)) * 16 * ((K + 15) / 16 * 16 + 4) + 3 * H; }
// lstm_fwd_lds3_kernel: the same, then per wave a slab of eight rows
__host__ __device__ constexpr int lstm_slab_row(int H) { return 3 * H + 2; }
__host__ __device__ constexpr int lstm_lds3_floats(int K, int H, int NW) { return lstm_lds2_floats(K, H) + NW * 8 * lstm_slab_row(H); }

// ---- the same layer for MANY rows (round 3): weights stationary in LDS.  lstm_fwd_kernel (ops_dense.hip) re-reads the layer's weights from L2
// for every 16-row tile and re-shapes them through a wave-private LDS slab (gemm_nt: 25-28 % of the SIMD-cycles are matrix-pipe
// cycles by counter, profiles/r03_mfma_util.json).  Here a 512-thread workgroup owns ONE direction: its three gate blocks of W_ih
// (i, g, o: the f gate meets c0 = 0) sit in LDS for the workgroup's lifetime -- [gate][unit][k], row stride kpad + 4 (= 4 x odd:
// the 16 lanes of a ds_read_b128 phase hit 16 different 4-bank groups) -- and every wave walks its own 16-row tiles: the tile's x
// rows go straight from global memory into the MFMA A layout (lane (row, kq) holds x[row][16 g + 4 kq .. + 3]; the four MFMAs of a
// k-group use the components in turn, so A and B agree on a permuted k order), one 16-unit block at a time takes its three
// accumulators through the whole K, and the cell runs on the accumulators (lane (unit, q), register r = row 4 q + r: the three
// gates of a unit on one lane).  No barrier after the weights are staged.
template <int KG, int NW>              // k-groups of 16: in_dim <= 16 KG; NW waves per workgroup (16 where the registers allow: more waves to put
                                       // under the layer's stores)
__global__ __launch_bounds__(64 * NW) void lstm_fwd_lds_kernel(const float* __restrict__ x, const float* wf, const float* bif, const float* bhf,
                                                            const float* wr, const float* bir, const float* bhr, float* __restrict__ out,
                                                            float* __restrict__ gates_save, int64_t rows, int K, int H) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int dir = blockIdx.x & 1, slice = blockIdx.x >> 1, nslices = gridDim.x >> 1;
  const float* __restrict__ w = dir ? wr : wf;
  const float* __restrict__ b1 = dir ? bir : bif;
  const float* __restrict__ b2 = dir ? bhr : bhf;
  const int Hp = (H + 15) & ~15, nub = Hp >> 4;
  constexpr int ld = KG * 16 + 4;
  for (int idx = threadIdx.x; idx < lstm_lds_floats(KG, Hp); idx += 64 * NW) {
    const int g3 = idx / (Hp * ld), rem = idx - g3 * Hp * ld, n = rem / ld, k = rem - n * ld;
    smem[idx] = (n < H && k < K) ? w[(int64_t)((g3 == 0 ? 0 : g3 + 1) * H + n) * K + k] : 0.f;      // PyTorch gate order i, f, g, o
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = wave_id(), j = lane & 15, q = lane >> 4;
  const int64_t ntiles = (rows + 15) >> 4;
  const bool vec = (K & 3) == 0 && ((uintptr_t)x & 15) == 0;
  const bool nt_ok = (H & 15) == 0 && gates_save && ((uintptr_t)gates_save & 63) == 0;
  // A tile: rows past the end repeat the last one (their results are not stored)
  auto load_a = [&](float4 (&a)[KG], int64_t tile) __attribute__((always_inline)) {
    const int64_t r0 = tile << 4;
    const int64_t row = r0 + j < rows ? r0 + j : rows - 1;
    const float* xr = x + row * K;
#pragma unroll
    for (int g = 0; g < KG; ++g) {
      const int k0 = 16 * g + 4 * q;
      if (vec && k0 + 3 < K) a[g] = *reinterpret_cast<const float4*>(xr + k0);
      else a[g] = make_float4(k0 < K ? xr[k0] : 0.f, k0 + 1 < K ? xr[k0 + 1] : 0.f, k0 + 2 < K ? xr[k0 + 2] : 0.f, k0 + 3 < K ? xr[k0 + 3] : 0.f);
    }
  };
  const int64_t tstep = (int64_t)nslices * NW;
  float4 a[KG], an[KG];
  int64_t tile = (int64_t)slice * NW + wave;
  if (tile < ntiles) load_a(a, tile);
  for (; tile < ntiles; tile += tstep) {
    const int64_t r0 = tile << 4;
    // the next tile's rows are requested before this tile's results are stored: memory operations of a wave return in order, so
    // loads issued behind the epilogue's ~80 stores would wait for all of them
    if (tile + tstep < ntiles) load_a(an, tile + tstep);
    // two 16-unit blocks at a time: their stores land next to each other in time, so the two 64-byte halves of a 128-byte line of the
    // saved gates meet in L2 instead of leaving it one by one (the output is 2 KB per row: the launch is bound by its writes)
    for (int ub = 0; ub < nub; ub += 2) {
      const bool two = ub + 1 < nub;
      f32x4 ai = {0.f, 0.f, 0.f, 0.f}, ag = ai, ao = ai, ci = ai, cg = ai, co = ai;
      const float* wb = smem + (ub * 16 + j) * ld + 4 * q;
      const float* wc = wb + (two ? 16 * ld : 0);
#pragma unroll
      for (int g = 0; g < KG; ++g) {
        const float4 bi = *reinterpret_cast<const float4*>(wb + 16 * g);
        const float4 bg = *reinterpret_cast<const float4*>(wb + Hp * ld + 16 * g);
        const float4 bo = *reinterpret_cast<const float4*>(wb + 2 * Hp * ld + 16 * g);
        const float4 di = *reinterpret_cast<const float4*>(wc + 16 * g);
        const float4 dg = *reinterpret_cast<const float4*>(wc + Hp * ld + 16 * g);
        const float4 dO = *reinterpret_cast<const float4*>(wc + 2 * Hp * ld + 16 * g);
#define HYPAD_LSTM_STEP(c)                                                   \
        ai = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].c, bi.c, ai, 0, 0, 0); \
        ag = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].c, bg.c, ag, 0, 0, 0); \
        ao = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].c, bo.c, ao, 0, 0, 0); \
        if (two) {                                                           \
          ci = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].c, di.c, ci, 0, 0, 0); \
          cg = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].c, dg.c, cg, 0, 0, 0); \
          co = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g].c, dO.c, co, 0, 0, 0); \
        }
        HYPAD_LSTM_STEP(x) HYPAD_LSTM_STEP(y) HYPAD_LSTM_STEP(z) HYPAD_LSTM_STEP(w)
#undef HYPAD_LSTM_STEP
      }
      // stores through buffer addressing: the tile's base in the descriptor, the lane's (row 4 q, unit) once as a 32-bit offset,
      // row and gate as scalar offsets -- per-element 64-bit address arithmetic was a third of this epilogue's instructions
      const GBuf ob(out + r0 * 2 * H), gb(gates_save ? gates_save + r0 * 8 * H : out);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int unit = (ub + half) * 16 + j;
        if (half == 1 && !two) break;
        if (unit >= H) continue;
        const f32x4 pi = half ? ci : ai, pg = half ? cg : ag, po = half ? co : ao;
        const float bsi = b1[unit] + b2[unit], bsg = b1[2 * H + unit] + b2[2 * H + unit], bso = b1[3 * H + unit] + b2[3 * H + unit];
        const int vo_h = (4 * q * 2 * H + dir * H + unit) * 4, vo_g = (4 * q * 8 * H + dir * 4 * H + unit) * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (r0 + 4 * q + r >= rows) continue;
          const float gi = sigmoidf_(pi[r] + bsi), gg = tanhf_(pg[r] + bsg), go = sigmoidf_(po[r] + bso);
          const float tc = tanhf_(gi * gg);
          ob.st(go * tc, vo_h, r * 2 * H * 4);
          if (gates_save) {
            // whole, aligned 64-byte segments (hidden a multiple of 16): past the caches (non-temporal) -- 323 -> 288 us at 128 -> 2 x 64;
            // with 200-byte gate rows (hidden 50) the same hint makes partial lines and costs 100 us, so it is not given there
            if (nt_ok) {
              auto nt = [&](float v, int so) __attribute__((always_inline)) { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), gb.rs, vo_g, so, 2); };
              nt(gi, r * 8 * H * 4); nt(gg, (r * 8 * H + H) * 4); nt(go, (r * 8 * H + 2 * H) * 4); nt(tc, (r * 8 * H + 3 * H) * 4);
            } else {
              gb.st(gi, vo_g, r * 8 * H * 4); gb.st(gg, vo_g, (r * 8 * H + H) * 4);
              gb.st(go, vo_g, (r * 8 * H + 2 * H) * 4); gb.st(tc, vo_g, (r * 8 * H + 3 * H) * 4);
            }
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < KG; ++g) a[g] = an[g];
  }
}

// ---- round 4: the same layer with the reference's shapes folded in.  What the kernel above loses (rocprofv3 + what-if builds, round 4:
// 349 us per 200 000 rows at 100 -> 2 x 50 with the gates saved, 217 us with every store removed, against 109 us of MFMA issue): its
// run-time "second unit block" branch splits the K loop into basic blocks, the compiler -- at the 128-register budget of four waves
// per SIMD -- reloads the second block's B operands dword by dword right in front of each MFMA (ds_read_b32, s_waitcnt lgkmcnt(0),
// v_mfma: the LDS latency exposed three times per k-step), and a quarter of its MFMAs multiply padding (hidden 50 in blocks of 64,
// K = 100 in groups of 16).  Here H and the k-groups are template arguments:
//  * column tiles: gate i / g / o of every FULL 16-unit block (H / 16 of them), then ONE remainder tile that holds the last H % 16
//    units of all three gates side by side (columns [i .. | g .. | o ..], H % 16 <= 5): 10 tiles at H = 50 instead of 12;
//  * K: full groups of 16 exactly as above (lane (row, q) holds x[row][16 g + 4 q ..+ 3], MFMA c takes component c), the last
//    partial group in the order k = 16 g + 4 c + q, so it costs ceil(rest / 4) MFMAs instead of four: 25 per tile at K = 100, not 28;
//  * two passes per row tile (two unit blocks = six accumulators; at H = 50 the second pass has four), every pass a straight-line K
//    loop; the NEXT tile's x rows are requested inside the last pass, group by group, into the registers the MFMAs have just read
//    (no second register set: the kernel stays below the budget without spilling);
//  * the summed biases sit in LDS.
// Any other shape keeps the kernel above.
template <int K, int H, int NW>
__global__ __launch_bounds__(64 * NW) void lstm_fwd_lds2_kernel(const float* __restrict__ x, const float* wf, const float* bif, const float* bhf,
                                                             const float* wr, const float* bir, const float* bhr, float* __restrict__ out,
                                                             float* __restrict__ gates_save, int64_t rows) {
  constexpr int NFB = H / 16, REM = H % 16;
  // column n of tile ct -> (gate 0 / 1 / 2 = i / g / o, unit): all the staging needs to know (the rest of it, and the row-tile
  // machinery, is text shared with lstm_fwd_lds3_kernel)
#define HYPAD_LSTM_COLUMN(ct, n, gate, unit)                                                                             \
    if (ct < 3 * NFB) { gate = ct % 3; unit = (ct / 3) * 16 + n; }                                                       \
    else { gate = REM ? n / (REM ? REM : 1) : 3; unit = NFB * 16 + (REM ? n % (REM ? REM : 1) : 0); }
#include "lstm_t1_tile_body.inc"
#undef HYPAD_LSTM_COLUMN
  for (; tile < ntiles; tile += tstep) {
    // (the weights in LDS are loop-invariant: without this the compiler hoists their reads out of the tile loop and spills 236 registers)
    asm volatile("" ::: "memory");
    const int64_t r0 = tile << 4;
    const int64_t next = tile + tstep < ntiles ? tile + tstep : tile;
    const GBuf ob(out + r0 * 2 * H), gb(gates_save ? gates_save + r0 * 8 * H : out);
    // the cell on one lane's (i, g, o) of unit `unit`, rows 4 q + r
    auto cell = [&](const f32x4& pi, const f32x4& pg, const f32x4& po, int unit) __attribute__((always_inline)) {
      const float bsi = bias_s[unit], bsg = bias_s[H + unit], bso = bias_s[2 * H + unit];
      constexpr int HS = H;
      const int vo_h = (4 * q * 2 * H + dir * H + unit) * 4, vo_g = (4 * q * 8 * HS + dir * 4 * HS + unit) * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (r0 + 4 * q + r >= rows) continue;
        const float gi = sigmoidf_(pi[r] + bsi), gg = tanhf_(pg[r] + bsg), go = sigmoidf_(po[r] + bso);
        const float tc = tanhf_(gi * gg);
        ob.st(go * tc, vo_h, r * 2 * H * 4);
        if (gates_save) {
          if (nt_ok) {
            auto nt = [&](float v, int so) __attribute__((always_inline)) { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), gb.rs, vo_g, so, 2); };
            nt(gi, r * 8 * HS * 4); nt(gg, (r * 8 * HS + HS) * 4); nt(go, (r * 8 * HS + 2 * HS) * 4); nt(tc, (r * 8 * HS + 3 * HS) * 4);
          } else {
            gb.st(gi, vo_g, r * 8 * HS * 4); gb.st(gg, vo_g, (r * 8 * HS + HS) * 4);
            gb.st(go, vo_g, (r * 8 * HS + 2 * HS) * 4); gb.st(tc, vo_g, (r * 8 * HS + 3 * HS) * 4);
          }
        }
      }
    };
    // the remainder tile: columns [i x REM | g x REM | o x REM]: g and o of a unit come from the lanes REM and 2 REM further on
    auto cell_rem = [&](const f32x4& p) __attribute__((always_inline)) {
      f32x4 pg, po;
#pragma unroll
      for (int r = 0; r < 4; ++r) { pg[r] = __shfl_down(p[r], REM ? REM : 1); po[r] = __shfl_down(p[r], REM ? 2 * REM : 1); }
      if (j < REM) cell(p, pg, po, NFB * 16 + j);
    };
    constexpr int FIRST = NFB >= 2 ? 6 : 3;                  // first pass: two full blocks (or the only one)
    constexpr int SECOND = NT - FIRST;                       // second pass: what is left (0 .. 6 tiles)
    f32x4 acc[6];
    pass(std::integral_constant<int, FIRST>{}, std::integral_constant<bool, SECOND == 0>{}, 0, acc, next);
    cell(acc[0], acc[1], acc[2], j);
    if constexpr (FIRST == 6) cell(acc[3], acc[4], acc[5], 16 + j);
    if constexpr (SECOND > 0) {
      pass(std::integral_constant<int, SECOND>{}, std::true_type{}, FIRST, acc, next);
      constexpr int fb2 = NFB - 2;                           // full blocks in the second pass (NFB >= 2 here)
      if constexpr (fb2 >= 1) cell(acc[0], acc[1], acc[2], 32 + j);
      if constexpr (fb2 >= 2) cell(acc[3], acc[4], acc[5], 48 + j);
      if constexpr (REM > 0) cell_rem(acc[3 * fb2]);
    }
  }
}

// ---- the same with the layer's stores staged through LDS (hidden not a multiple of 16: the reference's encoder, 2 x 50): see the
// comment at "pass A" below.  Column tiles in the order the passes take them.
template <int K, int H, int NW>
__global__ __launch_bounds__(64 * NW) void lstm_fwd_lds3_kernel(const float* __restrict__ x, const float* wf, const float* bif, const float* bhf,
                                                             const float* wr, const float* bir, const float* bhr, float* __restrict__ out,
                                                             float* __restrict__ gates_save, int64_t rows) {
  constexpr int NFB = H / 16, REM = H % 16;
  // column n of tile ct -> (gate 0 / 1 / 2 = i / g / o, unit).  Tile order: (i, ub), (g, ub) for every full block; the remainder tile; (o, ub)
#define HYPAD_LSTM_COLUMN(ct, n, gate, unit)                                                                             \
    if (ct < 2 * NFB) { gate = ct & 1; unit = (ct >> 1) * 16 + n; }                                                      \
    else if (REM && ct == 2 * NFB) { gate = n / (REM ? REM : 1); unit = NFB * 16 + n % (REM ? REM : 1); }                \
    else { gate = 2; unit = (ct - 2 * NFB - (REM ? 1 : 0)) * 16 + n; }
#include "lstm_t1_tile_body.inc"
#undef HYPAD_LSTM_COLUMN
  // ---- pass A: gates i and g of every unit (+ the remainder tile, which also carries o of the last H % 16 units); pass B: gate o
  // of the full blocks.  tc = tanh(sigma(i) tanh(g)) needs pass A only and waits in registers for o.  What a pass produces goes
  // through a wave-private LDS slab, eight rows at a time, and leaves as 16-byte stores of whole row pieces: [i | g] = floats
  // [0, 2 H) of the row's (direction) block after pass A, [o | tanh c] = floats [2 H, 4 H) and the h row after pass B.  With 4-byte
  // stores from the accumulator layout (16 units = 64 bytes per row and instruction, at 200-byte gate rows never sector-aligned)
  // nearly every sector was written in pieces: 305 us with the gates against 163 without, 238 with the gate rows padded to 64
  // floats (what-if, round 4); whole sectors also take the non-temporal hint.
  constexpr int NA = 2 * NFB + (REM ? 1 : 0), NB = NFB;       // column tiles of the two passes
  constexpr int SROW = lstm_slab_row(H);                      // slab row: [o | tc | h] (pass B) or [i | g] (pass A); even, not a multiple of 32
  float* slab = smem + lstm_lds2_floats(K, H) + wave * (8 * SROW);
  const bool g16 = gates_save && (((uintptr_t)gates_save | (uintptr_t)(4 * H * 4)) & 15) == 0;
  for (; tile < ntiles; tile += tstep) {
    // (the weights in LDS are loop-invariant: without this the compiler hoists their reads out of the tile loop and spills 236 registers)
    asm volatile("" ::: "memory");
    const int64_t r0 = tile << 4;
    const int64_t next = tile + tstep < ntiles ? tile + tstep : tile;
    const int nvalid = rows - r0 < 16 ? (int)(rows - r0) : 16;
    // buffer descriptors sized to the tile's valid rows: stores past the end are dropped by the hardware (no per-row branches)
    const __amdgpu_buffer_rsrc_t gsr = __builtin_amdgcn_make_buffer_rsrc(gates_save ? gates_save + (r0 * 2 + dir) * 4 * H : out, 0,
                                                                          gates_save ? (nvalid * 8 * H - dir * 4 * H) * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t osr = __builtin_amdgcn_make_buffer_rsrc(out + r0 * 2 * H + dir * H, 0, (nvalid * 2 * H - dir * H) * 4, 0x00020000);
    f32x4 acc[NA > NB ? NA : NB];
    float tck[NFB + 1][4], gok[4];                            // tanh(c) of every block's rows 4 q + r; sigma(o) of the remainder units
    const int lrow = 4 * (q & 1);                             // this lane's first row inside its half of the tile
    // ---- pass A
    pass(std::integral_constant<int, NA>{}, std::false_type{}, 0, acc, next);
    float gi_[NFB + 1][4], gg_[NFB + 1][4];
#pragma unroll
    for (int ub = 0; ub < NFB; ++ub) {
      const int unit = 16 * ub + j;
      const float bsi = bias_s[unit], bsg = bias_s[H + unit];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        gi_[ub][r] = sigmoidf_(acc[2 * ub][r] + bsi); gg_[ub][r] = tanhf_(acc[2 * ub + 1][r] + bsg);
        tck[ub][r] = tanhf_(gi_[ub][r] * gg_[ub][r]);
      }
    }
    if constexpr (REM > 0) {
      const int unit = 16 * NFB + (j < REM ? j : 0);
      const float bsi = bias_s[unit], bsg = bias_s[H + unit], bso = bias_s[2 * H + unit];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = acc[2 * NFB][r];
        const float pg = __shfl_down(p, REM), po = __shfl_down(p, 2 * REM);
        gi_[NFB][r] = sigmoidf_(p + bsi); gg_[NFB][r] = tanhf_(pg + bsg); gok[r] = sigmoidf_(po + bso);
        tck[NFB][r] = tanhf_(gi_[NFB][r] * gg_[NFB][r]);
      }
    }
    if (gates_save) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if ((q >> 1) == half) {
#pragma unroll
          for (int ub = 0; ub < NFB; ++ub)
#pragma unroll
            for (int r = 0; r < 4; ++r) { slab[(lrow + r) * SROW + 16 * ub + j] = gi_[ub][r]; slab[(lrow + r) * SROW + H + 16 * ub + j] = gg_[ub][r]; }
          if constexpr (REM > 0) {
            if (j < REM) {
#pragma unroll
              for (int r = 0; r < 4; ++r) { slab[(lrow + r) * SROW + 16 * NFB + j] = gi_[NFB][r]; slab[(lrow + r) * SROW + H + 16 * NFB + j] = gg_[NFB][r]; }
            }
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // rows 8 half .. + 7, floats [0, 2 H) of the (row, direction) block: 2 H / 4 pieces of 16 bytes per row
        constexpr int PPR = 2 * H / 4;
        for (int p = lane; p < 8 * PPR; p += 64) {
          const int rr = p / PPR, c4 = p - rr * PPR;
          const float* src = slab + rr * SROW + 4 * c4;
          const float4 v = make_float4(src[0], src[1], src[2], src[3]);
          const int off = ((8 * half + rr) * 8 * H + 4 * c4) * 4;
          if (g16) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(wl_u32x4, v), gsr, off, 0, 2);
          else { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v.x), gsr, off, 0, 0); __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v.y), gsr, off + 4, 0, 0);
                 __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v.z), gsr, off + 8, 0, 0); __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v.w), gsr, off + 12, 0, 0); }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (the slab is rewritten by the other half / by pass B)
      }
    }
    // ---- pass B: o of the full blocks; the next tile's x rows arrive under it
    pass(std::integral_constant<int, NB>{}, std::true_type{}, NA, acc, next);
    float go_[NFB + 1][4];
#pragma unroll
    for (int ub = 0; ub < NFB; ++ub) {
      const float bso = bias_s[2 * H + 16 * ub + j];
#pragma unroll
      for (int r = 0; r < 4; ++r) go_[ub][r] = sigmoidf_(acc[ub][r] + bso);
    }
    if constexpr (REM > 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) go_[NFB][r] = gok[r];
    }
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if ((q >> 1) == half) {
#pragma unroll
        for (int ub = 0; ub < NFB + (REM ? 1 : 0); ++ub) {
          if (ub < NFB || j < REM) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float* row = slab + (lrow + r) * SROW + 16 * ub + j;
              row[0] = go_[ub][r]; row[H] = tck[ub][r]; row[2 * H] = go_[ub][r] * tck[ub][r];
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (gates_save) {
        constexpr int PPR = 2 * H / 4;
        for (int p = lane; p < 8 * PPR; p += 64) {
          const int rr = p / PPR, c4 = p - rr * PPR;
          const float* src = slab + rr * SROW + 4 * c4;
          const float4 v = make_float4(src[0], src[1], src[2], src[3]);
          const int off = ((8 * half + rr) * 8 * H + 2 * H + 4 * c4) * 4;
          if (g16 && (H % 2) == 0 && ((2 * H * 4) & 15) == 0) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(wl_u32x4, v), gsr, off, 0, 2);
          else { __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v.x), gsr, off, 0, 0); __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v.y), gsr, off + 4, 0, 0);
                 __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v.z), gsr, off + 8, 0, 0); __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v.w), gsr, off + 12, 0, 0); }
        }
      }
      {                                                         // the h rows: H floats per (row, direction), pieces of 8 bytes
        constexpr int PPR2 = H / 2;
        for (int p = lane; p < 8 * PPR2; p += 64) {
          const int rr = p / PPR2, c2 = p - rr * PPR2;
          const float* src = slab + rr * SROW + 2 * H + 2 * c2;
          const int off = ((8 * half + rr) * 2 * H + 2 * c2) * 4;
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(wl_u32x2, make_float2(src[0], src[1])), osr, off, 0, 0);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
}

// ------------------------------------------------------------------------------------------ launch
struct LayerArgs {       // what hypad_lstm_bidir_fwd was given
  const float *x, *wf, *bif, *bhf, *wr, *bir, *bhr;
  float *out, *gates_save;
  int64_t rows;
  hipStream_t s;
};

// one workgroup per direction and slice of the row tiles, NW waves each: as many slices as give every wave a tile, at most 128 (one
// workgroup per CU and direction).  `shape`: the run-time K, H of lstm_fwd_lds_kernel.
template <int NW, class... S>
int launch_sliced(void (*kernel)(const float*, const float*, const float*, const float*, const float*, const float*, const float*, float*, float*,
                                 int64_t, S...), int lds_floats, const LayerArgs& a, S... shape) {
  const size_t lds = (size_t)lds_floats * sizeof(float);
  hipError_t e = allow_lds((const void*)kernel, lds);
  if (e != hipSuccess) return (int)e;
  const int64_t ntiles = (a.rows + 15) >> 4;
  int nslices = (int)((ntiles + NW - 1) / NW);
  if (nslices > 128) nslices = 128;
  hipLaunchKernelGGL(kernel, dim3(2 * nslices), dim3(64 * NW), lds, a.s, a.x, a.wf, a.bif, a.bhf, a.wr, a.bir, a.bhr, a.out, a.gates_save,
                     a.rows, shape...);
  HYPAD_CHECK_LAUNCH();
  return HYPAD_OK;
}
template <int K, int H, int NW> int launch_lds2(const LayerArgs& a) { return launch_sliced<NW>(lstm_fwd_lds2_kernel<K, H, NW>, lstm_lds2_floats(K, H), a); }
template <int K, int H, int NW> int launch_lds3(const LayerArgs& a) { return launch_sliced<NW>(lstm_fwd_lds3_kernel<K, H, NW>, lstm_lds3_floats(K, H, NW), a); }
template <int KG, int NW> int launch_lds(const LayerArgs& a, int K, int H) {
  return launch_sliced<NW>(lstm_fwd_lds_kernel<KG, NW>, lstm_lds_floats(KG, (H + 15) & ~15), a, K, H);
}

template <int N> using IntC = std::integral_constant<int, N>;
template <class F> int kgroups_dispatch(int K, F&& f) {            // (K <= 128; returns what f does)
  switch ((K + 15) >> 4) {
    case 1: return f(IntC<1>{});
    case 2: return f(IntC<2>{});
    case 3: return f(IntC<3>{});
    case 4: return f(IntC<4>{});
    case 5: return f(IntC<5>{});
    case 6: return f(IntC<6>{});
    case 7: return f(IntC<7>{});
    default: return f(IntC<8>{});
  }
}

}  // namespace

namespace hypad {

int lstm_t1_lds_launch(const float* x, const float* wf, const float* bif, const float* bhf, const float* wr, const float* bir,
                       const float* bhr, float* out, float* gates_save, int64_t rows, int K, int H, void* stream, bool* launched) {
  // many rows: the weights-stationary form (one direction's W_ih in LDS per workgroup); HYPAD_LSTM_LDS=0 keeps the streamed form
  static const int lds_form = HYPAD_TUNE_INT("HYPAD_LSTM_LDS", 1);
  *launched = lds_form && rows >= 2048 && H <= 64 && K <= 128;
  if (!*launched) return HYPAD_OK;
  const LayerArgs a{x, wf, bif, bhf, wr, bir, bhr, out, gates_save, rows, (hipStream_t)stream};
  // the reference's three layer shapes (encoder 100 -> 2 x 50; decoder 50 -> 2 x 64 and 128 -> 2 x 64): lstm_fwd_lds2_kernel, or
  // lstm_fwd_lds3_kernel where the gate rows are no multiple of 16 floats.  Sixteen waves, except 50 -> 2 x 64 with saved gates: eight
  // waves, 132 -> 117 us per 200 000 rows -- round 6 sweep of waves x slices, scripts/time_lstm.py; every other shape is fastest at sixteen
  if (H == 50 && K == 100) {
    if (!gates_save) return launch_lds2<100, 50, 16>(a);            // (forward only: 163 us per 200 000 rows, 171 through the slab)
    return launch_lds3<100, 50, 16>(a);
  }
  if (H == 64 && K == 128) return launch_lds2<128, 64, 16>(a);
  if (H == 64 && K == 50) return gates_save ? launch_lds2<50, 64, 8>(a) : launch_lds2<50, 64, 16>(a);
  // any other shape: lstm_fwd_lds_kernel
  static const int nw_env = HYPAD_TUNE_INT("HYPAD_LSTM_WAVES", 0);
  // (16 waves: 357 -> 349 us at 100 -> 2 x 50, 356 -> 321 at 128 -> 2 x 64, gates saved, 200 000 rows -- for inputs up to 96 wide: at seven and
  // eight k-groups the 128-register budget of sixteen waves spills 2 / 10 registers, so those widths run eight waves, spill-free)
  return kgroups_dispatch(K, [&](auto kg) {
    constexpr int KG = decltype(kg)::value;
    if constexpr (KG < 7) {
      if (nw_env != 8) return launch_lds<KG, 16>(a, K, H);
    }
    return launch_lds<KG, 8>(a, K, H);
  });
}

}  // namespace hypad
