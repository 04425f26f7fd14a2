// K2 of libptzba for gfx950: the reduced camera system of the Schur complement (SURVEY §8a row a4,
// the exact replacement of scipy's dense trf solve at bundle_adjustment.py:200-202).
// Compiled without SLP vectorisation: packing the per-lane FMA chains into v_pk_* operations with
// register shuffles serialises them (dependent pk_mul -> pk_fma -> pk_add chains with s_nop hazards).
#include <cstdlib>
#include <string>

#include "ptzba_common.h"
#include "ptzba_kernels.h"

namespace ptzba {

// ------------------------------------------------------------------------------------------------
// K2: reduced camera system  S = U - sum_l W_l V~_l^-1 W_l^T   (damping added after the exchange),
//                            b = -g_pose + sum_l W_l V~_l^-1 g_l
// Two launches:
//   k_schur        the coupling blocks, register-blocked with LDS-staged operands (below); chunk-0
//                  items also sum the diagonal terms (U, g_pose, W V~^-1 g) of their frames;
//   k_schur_reduce sums the split partials of each tile, adds U on the diagonal, writes S (lower
//                  triangle, system order) and b | g_pose | diag U.
// k_schur work item = (tile: block F1 of 32 consecutive free frames x chunk of 64 partner frames,
// split of the tile's landmark list).  Lane = partner frame f2; wave w owns the 4 frames f1 = f1b+4w..
// of F1, so a lane accumulates the four 3x3 blocks S_{f1,f2} in registers (no atomics, no scatter).
// W lives in the dense landmark x frame slot table (slot = toff_l + f - first_l, written by K1; slots
// of frames that do not see the landmark stay zero).  Per batch of SNB landmarks the workgroup stages
// in LDS, double-buffered with the next batch's loads in flight during the current batch's FMAs:
//   * the landmarks' W rows over the chunk's 64 frames (coalesced: consecutive slots) -- loaded once
//     and read by all 8 waves (32 frames of reuse per load);
//   * Y = W_{f1,l} V~_l^-1 for every (landmark, f1 in F1) pair (zero where f1 does not see l), so the
//     batch's FMAs run straight-line without branches.
// Products are accumulated in the record precision per batch and flushed to fp64 registers; each
// split writes its fp64 blocks to a partial buffer [item][32 f1][9][64 f2] (coalesced), reduced by
// k_schur_reduce in a fixed order (deterministic).
// ------------------------------------------------------------------------------------------------
#ifndef S2_DU
#define S2_DU 4  // diagonal-term loads in flight per thread (chunk-0 items)
#endif
constexpr int SF = SCHUR_F1;   // frames per F1 block
constexpr int SFW = SF / 8;    // f1 frames per wave (8 waves)

// Bijection block -> item that gives each XCD group (b mod 8) a contiguous run of items.
__device__ __forceinline__ int xcd_swizzle(int b, int nb) {
  const int c = b & 7, idx = b >> 3;
  int start = 0;
  for (int q = 0; q < c; ++q) start += (nb - q + 7) >> 3;
  return start + idx;
}

// chunk-0 items: diagonal terms of the F1 frames over this split's landmarks: U, g_pose and W V~^-1 g,
// read from the dense slots (thread = (landmark j0 + 16 k, frame i): consecutive threads, consecutive
// slots), reduced through `red` ([512][12] doubles of LDS that is free until staging) into part_diag.
template <typename real>
__device__ __forceinline__ void schur_diag_terms(const SchurArgs& a, const int4* sL, int nl, int f1b, int item,
                                                 bool alt, double* red) {
  const int t = threadIdx.x;
  const real* __restrict__ w_slot = (const real*)(alt ? a.w_slot1 : a.w_slot);
  const real* __restrict__ ug_slot = (const real*)(alt ? a.ug_slot1 : a.ug_slot);
  const int i = t & (SF - 1), f = f1b + i;
  double acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0;
  // DU landmarks per thread and step, all loads issued before any is consumed (clamped, branch-free)
  constexpr int DU = S2_DU, JS = 512 / SF;
  for (int j0 = t >> 5; j0 < nl; j0 += DU * JS) {
    real u[DU][9], w[DU][6];
    double vg[DU][2];
    bool in[DU];
#pragma unroll
    for (int d = 0; d < DU; ++d) {
      const int j = j0 + d * JS;
      const int4 m = sL[min(j, nl - 1)];
      in[d] = j < nl && f >= m.y && f <= m.z;
      const int64_t slot = m.w + min(max(f - m.y, 0), m.z - m.y);
      slot_load6(w[d], w_slot + slot * W_STRIDE);
      slot_load9(u[d], ug_slot + slot * UG_STRIDE);
      const double* vi = a.lm_aux + (int64_t)m.x * 8;
      vg[d][0] = vi[3];
      vg[d][1] = vi[4];
    }
#pragma unroll
    for (int d = 0; d < DU; ++d) {
      if (in[d]) {
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] += (double)u[d][k];
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[9 + q] += (double)w[d][2 * q] * vg[d][0] + (double)w[d][2 * q + 1] * vg[d][1];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) red[t * 12 + k] = acc[k];
  __syncthreads();
  if (t < SF * 12) {
    double v = 0;
    for (int j0 = 0; j0 < 512 / SF; ++j0) v += red[j0 * SF * 12 + t];
    a.part_diag[(int64_t)item * SF * 12 + t] = v;
  }
  __syncthreads();
}

#ifdef SK_TIMING
__device__ long long g_sk[16][16];
__device__ long long g_sk_items[4096][4];  // per item: start, end (s_memrealtime, 100 MHz), chunk, nl
#define SK_T(k) do { if (skrec) sk[k] = clock64(); } while (0)
#define SK_ACC(k, t0) do { if (skrec) sk[k] += clock64() - (t0); } while (0)
#define SK_NOW(t0) do { if (skrec) t0 = clock64(); } while (0)
#else
#define SK_T(k) do { } while (0)
#define SK_ACC(k, t0) do { } while (0)
#define SK_NOW(t0) do { } while (0)
#endif
template <typename real>
__global__ __launch_bounds__(512) void k_schur(SchurArgs a) {
  // fp64 (parity path) stages half as many landmarks per batch to stay inside 160 KiB of LDS
  constexpr int SNB = sizeof(real) == 4 ? 16 : 8;
  constexpr int WP = sizeof(real) == 4 ? 8 : 6;  // 16-B aligned row pitch for 6 values
  __shared__ real sW[2][SNB][6][WAVE];                             // W rows of the chunk's frames (SoA)
  // Y of (landmark, f1), 0 if unobserved.  fp32: frames (2p, 2p+1) interleaved per component, so one
  // 8-byte read gives the pair's value for the packed FMAs; fp64: one row of 6 per frame.
  __shared__ __attribute__((aligned(16))) real sY[2][SNB][SF][WP];
  __shared__ int4 sL[SCHUR_LMAX];                                    // the item's landmark list
  if (a.skip_if && *a.skip_if) return;
#ifdef SK_TIMING
  const bool skrec = threadIdx.x == 0 && blockIdx.x < 16;
  long long* sk = g_sk[blockIdx.x & 15];
  if (skrec)
    for (int k = 0; k < 16; ++k) sk[k] = 0;
#endif
  long long skt = 0;
  (void)skt;
  SK_T(0);
  const int item = xcd_swizzle(blockIdx.x, gridDim.x);
  const int4 it = a.items[item];
#ifdef SK_TIMING
  if (threadIdx.x == 0 && item < 4096) {
    g_sk_items[item][0] = __builtin_amdgcn_s_memrealtime();
    g_sk_items[item][2] = it.y;
    g_sk_items[item][3] = it.w - it.z;
  }
#endif
  const int f1b = it.x, chunk = it.y, lb = it.z, nl = it.w - it.z;
  const int t = threadIdx.x, lane = lane_id(), wv = t >> 6;
  const int f2base = f1b + WAVE * chunk;
  const bool alt = a.sel && *a.sel;  // device-chosen linearisation slot
  const real* __restrict__ w_slot = (const real*)(alt ? a.w_slot1 : a.w_slot);
  for (int k = t; k < nl; k += 512) sL[k] = a.item_lm[lb + k];
  __syncthreads();
  SK_T(1);

  if (chunk == 0) schur_diag_terms<real>(a, sL, nl, f1b, item, alt, reinterpret_cast<double*>(&sW[0][0][0][0]));
  SK_T(2);

  // ---- staging registers: W slots (e = t, t + 512 over [SNB][64]) and one Y pair (j = t / SF, i = t % SF;
  // fp64: threads >= SNB*SF repeat a pair and do not stage it).  Branch-free, so the loads stay in flight
  // until stage() consumes them after the current batch's FMAs.
  constexpr int NSL = SNB * WAVE / 512;  // W slots per thread per batch (2 fp32, 1 fp64)
  real rw[NSL][6];
  bool rwin[NSL];
  real ryw[6];
  double rvi[3];
  bool ryin;
  const int yj = (t / SF) & (SNB - 1), yi = t & (SF - 1);
  auto fetch = [&](int p) {  // landmarks [p, p + SNB) of the list
#pragma unroll
    for (int q = 0; q < NSL; ++q) {
      const int e = t + 512 * q, j = e >> 6, ln = e & 63;
      const int4 m = sL[min(p + j, nl - 1)];  // {landmark, first frame, last frame, slot offset}
      const int idx = f2base + ln - m.y;
      rwin[q] = (p + j < nl) && idx >= 0 && f2base + ln <= m.z;
      slot_load6(rw[q], w_slot + (int64_t)(m.w + min(max(idx, 0), m.z - m.y)) * W_STRIDE);
    }
    const int f = f1b + yi;
    const int4 m = sL[min(p + yj, nl - 1)];
    ryin = (p + yj < nl) && f >= m.y && f <= m.z;
    slot_load6(ryw, w_slot + (int64_t)(m.w + min(max(f - m.y, 0), m.z - m.y)) * W_STRIDE);
    const double* vi = a.lm_aux + (int64_t)m.x * 8;
    rvi[0] = vi[0]; rvi[1] = vi[1]; rvi[2] = vi[2];
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < NSL; ++q) {
      const int e = t + 512 * q, j = e >> 6, ln = e & 63;
      if constexpr (sizeof(real) == 4) {
        // fp32: W as component pairs (w_2r, w_2r+1) per lane, so the packed FMAs take one half of a
        // loaded pair for both result halves (op_sel) instead of building splat pairs with moves
        float2* w2p = reinterpret_cast<float2*>(&sW[0][0][0][0]) + ((buf * SNB + j) * 3) * WAVE + ln;
#pragma unroll
        for (int r = 0; r < 3; ++r)
          w2p[r * WAVE] = rwin[q] ? make_float2(rw[q][2 * r], rw[q][2 * r + 1]) : make_float2(0.f, 0.f);
      } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) sW[buf][j][k][ln] = rwin[q] ? rw[q][k] : (real)0;
      }
    }
    if (t < SNB * SF) {
      // pair layout (fp32): element (frame 2p + h, component k) at [2p][0] + 2 k + h of the pair's 16 reals
      real* y = sizeof(real) == 4 ? &sY[buf][yj][yi & ~1][0] + (yi & 1) : sY[buf][yj][yi];
      const int ks = sizeof(real) == 4 ? 2 : 1;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double W0 = ryin ? (double)ryw[2 * q] : 0.0, W1 = ryin ? (double)ryw[2 * q + 1] : 0.0;
        y[ks * (2 * q)] = (real)-(W0 * rvi[0] + W1 * rvi[1]);  // staged negated: the FMAs accumulate -Y W^T
        y[ks * (2 * q + 1)] = (real)-(W0 * rvi[1] + W1 * rvi[2]);
      }
    }
  };

  double acc[SFW][9];
#pragma unroll
  for (int i = 0; i < SFW; ++i)
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[i][k] = 0;

  if (nl > 0) {
    fetch(0);
    stage(0);
  }
  __syncthreads();
  SK_T(3);
#ifdef SK_TIMING
  if (skrec) {
    sk[8] = nl;
    sk[9] = chunk;
  }
#endif
  int buf = 0;
  for (int p = 0; p < nl; p += SNB) {
    const bool more = p + SNB < nl;  // block-uniform
    fetch(p + SNB);  // next batch's loads in flight during this batch's FMAs (unconditional: no phi
                     // at a join forces an early wait; past the list the lanes load clamped slots)
    real accr[SFW][9];
#pragma unroll
    for (int i = 0; i < SFW; ++i)
#pragma unroll
      for (int k = 0; k < 9; ++k) accr[i][k] = 0;
    SK_NOW(skt);
    // straight-line over the whole batch: slots past the list and unobserved (landmark, f1) pairs were
    // staged as zeros, so no branch (and no wait at a branch) interrupts the LDS reads and the FMAs
    if constexpr (sizeof(real) == 4) {
      // packed: one v_pk_fma_f32 updates the same block entry of two frames (2p, 2p+1)
      typedef float f2 __attribute__((ext_vector_type(2)));
      f2 accp[SFW / 2][9];
#pragma unroll
      for (int pp = 0; pp < SFW / 2; ++pp)
#pragma unroll
        for (int k = 0; k < 9; ++k) accp[pp][k] = f2{0.f, 0.f};
#pragma unroll 2
      for (int j = 0; j < SNB; ++j) {
        const f2* wsrc = reinterpret_cast<const f2*>(&sW[0][0][0][0]) + ((buf * SNB + j) * 3) * WAVE + lane;
        f2 wp[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) wp[r] = wsrc[r * WAVE];
#pragma unroll
        for (int pp = 0; pp < SFW / 2; ++pp) {
          const f2* ys = reinterpret_cast<const f2*>(&sY[buf][j][SFW * wv + 2 * pp][0]);
          f2 y[6];
#pragma unroll
          for (int k = 0; k < 6; ++k) y[k] = ys[k];
#pragma unroll
          for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
              accp[pp][3 * q + r] = __builtin_elementwise_fma(y[2 * q], __builtin_shufflevector(wp[r], wp[r], 0, 0),
                                                              accp[pp][3 * q + r]);
              accp[pp][3 * q + r] = __builtin_elementwise_fma(y[2 * q + 1], __builtin_shufflevector(wp[r], wp[r], 1, 1),
                                                              accp[pp][3 * q + r]);
            }
        }
      }
#pragma unroll
      for (int pp = 0; pp < SFW / 2; ++pp)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          acc[2 * pp][k] += (double)accp[pp][k].x;
          acc[2 * pp + 1][k] += (double)accp[pp][k].y;
        }
    } else {
#pragma unroll 2
      for (int j = 0; j < SNB; ++j) {
        real w2[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) w2[k] = sW[buf][j][k][lane];
#pragma unroll
        for (int i = 0; i < SFW; ++i) {
          const real* ys = sY[buf][j][SFW * wv + i];
          real y[6];
#pragma unroll
          for (int k = 0; k < 6; ++k) y[k] = ys[k];
#pragma unroll
          for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int r = 0; r < 3; ++r) {
              accr[i][3 * q + r] = fma(y[2 * q], w2[2 * r], accr[i][3 * q + r]);
              accr[i][3 * q + r] = fma(y[2 * q + 1], w2[2 * r + 1], accr[i][3 * q + r]);
            }
        }
      }
#pragma unroll
      for (int i = 0; i < SFW; ++i)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[i][k] += (double)accr[i][k];
    }
    SK_ACC(4, skt);  // compute
    SK_NOW(skt);
    if (more) stage(buf ^ 1);
    SK_ACC(5, skt);  // stage (waits for the prefetched loads)
    SK_NOW(skt);
    __syncthreads();
    SK_ACC(6, skt);  // barrier
    buf ^= 1;
  }
  SK_T(7);
  // partial blocks of this split: part[item][f1 local][k][f2 lane]
  // split partials in the record precision: half the bytes of fp64 for the fp32 path (each is a sum of
  // fp64-flushed batches, rounded once; the reduce sums them in fp64)
  real* out = (real*)a.part + (int64_t)item * (SF * 9 * WAVE);
#pragma unroll
  for (int i = 0; i < SFW; ++i)
#pragma unroll
    for (int k = 0; k < 9; ++k) out[((SFW * wv + i) * 9 + k) * WAVE + lane] = (real)acc[i][k];
  SK_T(10);
#ifdef SK_TIMING
  __syncthreads();
  if (threadIdx.x == 0 && item < 4096) g_sk_items[item][1] = __builtin_amdgcn_s_memrealtime();
#endif
}
// ------------------------------------------------------------------------------------------------
// K2 on the matrix cores (k_schur_mfp: the fp32 path): the same work items, split partials and diagonal terms as
// k_schur; each batch of 16 landmarks is one k-step (K = 16 landmarks x 2 ray dimensions) of
// v_mfma_f32_16x16x32_f16 over the item's 96 x 192 block S(F1 dofs, chunk dofs) -- 72 output blocks of 16 x 16.
// Zero products (a landmark covers ~19 % of a tile) cost matrix-core cycles instead of VALU issue.
// Precision: every operand is split x = hi + lo into two fp16 (22 significant bits) and a product is
// hi*hi + hi*lo + lo*hi (the dropped lo*lo is ~2^-22 of it), accumulated in fp32 over the item's batches
// and stored as the fp32 split partial (the reduce sums the splits in fp64).
// Range: W (~1e4 px^2) and Y = -W V~^-1 (~1) would not both fit fp16, so row k = (landmark, d) of W is scaled by
// g_l = 2^round(log2 sqrt(tr V~_l^-1)) and the same row of Y by 1 / g_l: the product Y^T W is unchanged (powers of
// two: exact), both factors ~ sqrt(|W| |Y|).
// The focal-length rows of both operands are ~2^8 below the pan / tilt rows (d x / d f = (x - u) / f ~ 0.1 against
// d x / d pan ~ f pi / 180 ~ 50 px / deg), so their lo halves fell below fp16's normal range (6e-5) and kept only a few
// bits -- at lambda = 0 the undamped step of tests/test_gpu_k1_paths.py was off by up to 8.6e-3 of its largest entry,
// reproduced to three digits by a CPU emulation of this split.  Those rows are staged times MF_FROW = 2^7 (still below
// the pan / tilt rows: no new overflow) and the accumulators of the f rows / columns scaled back: exact.
// Roles: the eight waves take fixed roles, so that the staging of one batch (loads, g_l scaling, fp16 splits, LDS
// writes: VALU + memory issue) runs beside the products of another (fragment reads + MFMAs) on every SIMD:
//   * waves 0-3 stage: per batch each thread loads four W slots of the chunk's frames and two (landmark, f1) pairs,
//     scales and splits them and writes the operand rows; V~^-1, g_l and V~^-1 g come from a per-landmark LDS table
//     built with the list.  On chunk-0 items the thread that stages Y of a pair also sums that pair's diagonal terms
//     (U, g_pose, W V~^-1 g; HBM-bound, ~100 MB per build), their loads issued with the pair's, under the MFMAs;
//   * waves 4-7 multiply: 18 output blocks each (3 row blocks x 6 column blocks), per block al*bh, ah*bl, ah*bh in
//     batch order, then the partial store.
// Hand-off: a ring of NR operand buffers and two LDS counter sets, one counter per wave and one writer per counter:
// s_ready[w] = b + 1 once staging wave w's part of batch b is in LDS (after lgkmcnt(0)), s_done[w] = b + 1 once
// product wave w holds batch b's fragments in registers (after lgkmcnt(0)).  A product wave starts batch b when all
// four s_ready >= b + 1; a staging wave re-fills the buffer of batch b - NR when all four s_done >= b - NR + 1.
// Why it cannot stall: the counters live in LDS and are zeroed before the one __syncthreads that precedes
// every wait; the skip_if exit is taken by whole workgroups before it; the batch count nb is block-uniform,
// so all eight waves run the same number of hand-offs; a counter only grows, and the wait of batch b on
// either side needs only signals of batches < b from the other side (s_ready of b needs s_done of
// b - NR, which needs s_ready of b - NR): the dependency chain ends at batch 0, which waits for
// nothing.  No wait looks at global memory or at another workgroup.
// Folded build prologue (SchurArgs::ztiles != nullptr: device-driven single-GPU builds, api.hip build_impl): the
// launch also does k_build_prologue's work, so that launch is not needed.  The list build forms V~^-1, g_l and
// V~^-1 g from K1's landmark row, D_ray and lambda (lm_damp: the prologue's fp64 expressions; it only reads), and the
// product waves, idle until the first batch is staged, zero the pattern tiles of S, b | g_pose | dU and info[0].
// A launch that leaves at skip_if zeroes nothing: the next solve's first build zeroes for itself.
// ------------------------------------------------------------------------------------------------
constexpr float MF_FROW = 128.f;
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));
constexpr int MKP = 40;  // k pitch of an operand row in halves: 80-B rows keep the 16-B fragment reads aligned

// (x0, x1) -> hi + lo, each a packed pair of fp16 (v_cvt_pkrtz: toward zero; x - hi is exact in fp32 and
// has at most 13 significant bits, of which lo keeps 11)
typedef __fp16 hp2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_pk(float x0, float x1, hp2v& h, hp2v& l) {
  h = __builtin_amdgcn_cvt_pkrtz(x0, x1);
  l = __builtin_amdgcn_cvt_pkrtz(x0 - (float)h[0], x1 - (float)h[1]);
}

__device__ __forceinline__ void k2_signal(int* p, int v) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS stores / fragment reads are done
  if (lane_id() == 0) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// all four counters of a set >= v (v <= 0: nothing to wait for)
__device__ __forceinline__ void k2_wait4(const int* p, int v) {
  if (v > 0) {
    for (;;) {
      const int c0 = __hip_atomic_load(p + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const int c1 = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const int c2 = __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const int c3 = __hip_atomic_load(p + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (__builtin_amdgcn_readfirstlane(min(min(c0, c1), min(c2, c3))) >= v) break;
      __builtin_amdgcn_s_sleep(1);
    }
  }
  asm volatile("" ::: "memory");
}

__global__ __launch_bounds__(512) void k_schur_mfp(SchurArgs a) {
  constexpr int SNB = 16;                // landmarks per batch
  constexpr int NR = 2;                  // operand buffers in the ring: 116 KB of LDS (a ring of 3, 159 KB, measured no faster)
  constexpr int NSL = SNB * WAVE / 256;  // W slots staged per staging thread per batch
  constexpr int NYP = SNB * SF / 256;    // (landmark, f1) pairs per staging thread per batch
  __shared__ __attribute__((aligned(16))) _Float16 sY[NR][2][3 * SF][MKP];     // [buf][hi|lo][q*32 + f1][2j + d]
  __shared__ __attribute__((aligned(16))) _Float16 sWt[NR][2][3 * WAVE][MKP];  // [buf][hi|lo][r*64 + f2][2j + d]
  __shared__ int4 sL[SCHUR_LMAX];
  // per landmark of the list, converted once instead of per (landmark, f1) pair: {V~^-1 (3, fp32), 1 / g_l} and
  // {g_l, V~^-1 g (2, fp32: the diagonal terms' factor), -}
  __shared__ float4 sV[SCHUR_LMAX], sD[SCHUR_LMAX];
  __shared__ int s_ready[4], s_done[4];
  static_assert(sizeof(sWt) >= 512 * 12 * sizeof(double), "the diagonal terms' reduction reuses sWt");
  if (a.skip_if && *a.skip_if) return;
  const int t = threadIdx.x, lane = lane_id(), wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const bool prod = wv < 4;  // producer of operands: waves 0-3 stage, waves 4-7 multiply
  const int rk = wv & 3;     // rank inside the role
#ifdef SK_TIMING
  const bool skrec = lane == 0 && rk == 0 && blockIdx.x < 16;  // first staging and first product wave
  long long* sk = g_sk[blockIdx.x & 15];
  if (skrec && prod)
    for (int k = 0; k < 16; ++k) sk[k] = 0;
  long long tk0 = 0, tk1 = 0, tk2 = 0;
#define SKP_ACC(v, t0) do { if (skrec) v += clock64() - (t0); } while (0)
#else
#define SKP_ACC(v, t0) do { } while (0)
#endif
  long long skt = 0;
  (void)skt;
  if (prod) SK_T(0);
  const int item = xcd_swizzle(blockIdx.x, gridDim.x);
  const int4 it = a.items[item];
#ifdef SK_TIMING
  if (threadIdx.x == 0 && item < 4096) {
    g_sk_items[item][0] = __builtin_amdgcn_s_memrealtime();
    g_sk_items[item][2] = it.y;
    g_sk_items[item][3] = it.w - it.z;
  }
#endif
  const int f1b = it.x, chunk = it.y, lb = it.z, nl = it.w - it.z;
  const int nb = (nl + SNB - 1) / SNB;  // batches (block-uniform)
  const int f2base = f1b + WAVE * chunk;
  const bool alt = a.sel && *a.sel;  // device-chosen linearisation slot
  const float* __restrict__ w_slot = (const float*)(alt ? a.w_slot1 : a.w_slot);
  // folded prologue (SchurArgs::ztiles): the damped landmark blocks are formed here from K1's rows, D_ray and lambda
  // (read-only: nothing of them is written by this launch) instead of being read from lm_aux -- lm_damp gives the
  // prologue's own bits
  const bool fold = a.ztiles != nullptr;  // (uniform over the launch)
  const double* __restrict__ lm_rows = alt ? a.lm_out1 : a.lm_out;
  const double lambda = fold ? (a.prep.lam_dev ? *a.prep.lam_dev : a.prep.lambda) : 0.0;
  for (int k = t; k < nl; k += 512) {
    const int4 m = a.item_lm[lb + k];
    sL[k] = m;
    double vi[5];
    if (fold) {
      const double* in = lm_rows + (int64_t)m.x * 8;
      const LmDamp d = lm_damp(in[0], in[1], in[2], in[3], in[4], a.D_ray[2 * (int64_t)m.x],
                               a.D_ray[2 * (int64_t)m.x + 1], lambda);
      vi[0] = d.i00; vi[1] = d.i01; vi[2] = d.i11; vi[3] = d.vg0; vi[4] = d.vg1;
    } else {
      const double* p = a.lm_aux + (int64_t)m.x * 8;
#pragma unroll
      for (int q = 0; q < 5; ++q) vi[q] = p[q];
    }
    int e = 0;
    (void)frexp(vi[0] + vi[2], &e);
    const float g = ldexpf(1.f, e / 2);
    sV[k] = make_float4((float)vi[0], (float)vi[1], (float)vi[2], 1.f / g);  // (1 / g: a power of two, exact)
    sD[k] = make_float4(g, (float)vi[3], (float)vi[4], 0.f);
  }
  if (t < 4) {
    s_ready[t] = 0;
    s_done[t] = 0;
  }
  __syncthreads();
  if (prod) SK_T(1);

  if (prod) {
    // ---- staging waves ----
    const int pt = rk * WAVE + lane;  // 0..255
    const bool diag = chunk == 0;
    const float* __restrict__ ug_slot = (const float*)(alt ? a.ug_slot1 : a.ug_slot);
    // staging registers of one batch (two sets: the loads of batch b + 2 are issued when batch b is staged)
    struct Pre {
      float rw[NSL][6], rgw[NSL], ryw[NYP][6];
      float4 rv[NYP];  // V~^-1 | 1 / g
      bool rwin[NSL], ryin[NYP];
      float du[NYP][9], dg[NYP][2];
    };
    // element map of a staging thread: W slot q -> (landmark j of the batch, frame ln of the chunk), pair u ->
    // (landmark yj, frame yi of F1).  Any bijection gives the same LDS contents and the same sums (one dacc set per
    // pair).  A wave takes 16 consecutive frames x 4 landmarks: its b32 LDS stores (rows 80 B apart: bank = 20 frame +
    // landmark mod 64) reach all 64 banks, where 64 consecutive frames of one landmark hit 16 banks four ways; a
    // landmark's loads still run over 16 consecutive slots (384 B).
    auto wj = [&](int) { return (lane >> 4) + 4 * rk; };
    auto wln = [&](int q) { return (lane & 15) + 16 * q; };
    auto pyj = [&](int) { return (lane >> 4) + 4 * rk; };
    auto pyi = [&](int u) { return (lane & 15) + 16 * u; };
    auto fetch = [&](Pre& P, int p) {  // landmarks [p, p + SNB) of the list (clamped, branch-free)
#pragma unroll
      for (int q = 0; q < NSL; ++q) {
        const int j = wj(q), ln = wln(q);
        const int jj = min(p + j, nl - 1);
        const int4 m = sL[jj];
        const int idx = f2base + ln - m.y;
        P.rwin[q] = (p + j < nl) && idx >= 0 && f2base + ln <= m.z;
        P.rgw[q] = sD[jj].x;
        slot_load6(P.rw[q], w_slot + (int64_t)(m.w + min(max(idx, 0), m.z - m.y)) * W_STRIDE);
      }
#pragma unroll
      for (int u = 0; u < NYP; ++u) {
        const int yj = pyj(u), yi = pyi(u);
        const int f = f1b + yi, jj = min(p + yj, nl - 1);
        const int4 m = sL[jj];
        P.ryin[u] = (p + yj < nl) && f >= m.y && f <= m.z;
        P.rv[u] = sV[jj];
        const int64_t slot = m.w + min(max(f - m.y, 0), m.z - m.y);
        slot_load6(P.ryw[u], w_slot + slot * W_STRIDE);
        if (diag && p < nl) {  // chunk-0 items: the pair's U | g_pose terms (block-uniform branch)
          slot_load9(P.du[u], ug_slot + slot * UG_STRIDE);
          P.dg[u][0] = sD[jj].y;
          P.dg[u][1] = sD[jj].z;
        }
      }
    };
    auto stage = [&](const Pre& P, int buf) {
#pragma unroll
      for (int q = 0; q < NSL; ++q) {
        const int j = wj(q), ln = wln(q);
        const float gq = P.rwin[q] ? P.rgw[q] : 0.f;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          hp2v h, l;
          const float gr = r == 2 ? gq * MF_FROW : gq;
          split_pk(P.rw[q][2 * r] * gr, P.rw[q][2 * r + 1] * gr, h, l);
          *reinterpret_cast<hp2v*>(&sWt[buf][0][r * WAVE + ln][2 * j]) = h;
          *reinterpret_cast<hp2v*>(&sWt[buf][1][r * WAVE + ln][2 * j]) = l;
        }
      }
      // Y / g = -(W / g) V~^-1, staged negated: the products accumulate -Y W^T (fp32 is exact enough: the operand
      // keeps 22 bits).  1 / g is a power of two: exact.
#pragma unroll
      for (int u = 0; u < NYP; ++u) {
        const int yj = pyj(u), yi = pyi(u);
        const float gi = P.ryin[u] ? P.rv[u].w : 0.f;
        const float v0 = P.rv[u].x * gi, v1 = P.rv[u].y * gi, v2 = P.rv[u].z * gi;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float W0 = P.ryw[u][2 * q], W1 = P.ryw[u][2 * q + 1];
          hp2v h, l;
          const float sq = q == 2 ? -MF_FROW : -1.f;
          split_pk(sq * fmaf(W0, v0, W1 * v1), sq * fmaf(W0, v1, W1 * v2), h, l);
          *reinterpret_cast<hp2v*>(&sY[buf][0][q * SF + yi][2 * yj]) = h;
          *reinterpret_cast<hp2v*>(&sY[buf][1][q * SF + yi][2 * yj]) = l;
        }
      }
    };
    float dacc[NYP][12];  // fp32 over the item's <= 32 batches, one term per batch and pair (the reduction below is fp64)
#pragma unroll
    for (int u = 0; u < NYP; ++u)
#pragma unroll
      for (int k = 0; k < 12; ++k) dacc[u][k] = 0.f;
    auto daccum = [&](const Pre& P) {
#pragma unroll
      for (int u = 0; u < NYP; ++u)
        if (P.ryin[u]) {
          const float g0 = P.dg[u][0], g1 = P.dg[u][1];
#pragma unroll
          for (int k = 0; k < 9; ++k) dacc[u][k] += P.du[u][k];
#pragma unroll
          for (int q = 0; q < 3; ++q) dacc[u][9 + q] += fmaf(P.ryw[u][2 * q], g0, P.ryw[u][2 * q + 1] * g1);
        }
    };
    Pre A, B;
    if (nb > 0) {
      fetch(A, 0);
      // (keeps set A's loads ahead of set B's in issue order, as in the loop: interleaved here, the loop's first
      // stage(A) would have to wait for B's loads too)
      __builtin_amdgcn_sched_barrier(0);
      fetch(B, SNB);
    }
    SK_T(2);
    SK_T(3);
#ifdef SK_TIMING
    if (skrec) {
      sk[8] = nl;
      sk[9] = chunk;
    }
#endif
    // batch b from set A (b even) or B (b odd) into buffer b % NR.  The loop always runs both halves and has one
    // exit (an odd last batch is staged after it): with a second exit between the halves the compiler's wait
    // counts at the loop head must allow for set A's loads being the newest, and stage(A) waits for set B's too.
    int buf = 0;
    auto half = [&](Pre& P, int b, bool again) {
      SK_NOW(skt);
      k2_wait4(s_done, b - NR + 1);
      SKP_ACC(tk0, skt);
      SK_NOW(skt);
      stage(P, buf);
      if (diag) daccum(P);
      k2_signal(&s_ready[rk], b + 1);
      SKP_ACC(tk1, skt);
      SK_NOW(skt);
      if (again) fetch(P, (b + 2) * SNB);
      SKP_ACC(tk2, skt);
      buf = buf + 1 == NR ? 0 : buf + 1;
    };
    int b = 0;
    for (; b + 1 < nb; b += 2) {
      half(A, b, true);
      half(B, b + 1, true);
    }
    if (b < nb) half(A, b, false);
    SK_T(7);
#ifdef SK_TIMING
    if (skrec) {
      sk[6] = tk0;
      sk[5] = tk1;
      sk[11] = tk2;
    }
#endif
    if (diag) {  // fixed-order reduction over the 16 landmark lanes of each frame (as schur_diag_terms)
      k2_wait4(s_done, nb);  // the last fragment reads of the ring have landed: sWt is free
      double* red = reinterpret_cast<double*>(&sWt[0][0][0][0]);
#pragma unroll
      for (int u = 0; u < NYP; ++u)
#pragma unroll
        for (int k = 0; k < 12; ++k) red[(pyj(u) * SF + pyi(u)) * 12 + k] = (double)dacc[u][k];
      k2_signal(&s_ready[rk], nb + 1);
      k2_wait4(s_ready, nb + 1);  // all four staging waves' terms are in `red`
      for (int e = pt; e < SF * 12; e += 256) {
        double v = 0;
        for (int j0 = 0; j0 < 512 / SF; ++j0) v += red[j0 * SF * 12 + e];
        a.part_diag[(int64_t)item * SF * 12 + e] = v;
      }
    }
    SK_T(10);
  } else {
    // ---- product waves: row blocks 3 rg.., column blocks 6 cg.. ----
    const int rg = rk >> 1, cg = rk & 1;
    const int fr = lane & 15, fk = (lane >> 4) * 8;  // fragment row / column and k offset of this lane
    if (fold) {
      // folded prologue: while the first batch is staged, these 256 threads zero the factor pattern's tiles item,
      // item + n_items, ... with k_build_prologue's stores (the fused prepare's constant diagonal entries included),
      // item 0 also b | g_pose | dU and info[0].  This launch touches S and the vectors nowhere else (the partials
      // go to part / part_diag; k_schur_reduce, the next launch, writes S), and the previous factor's last reader
      // finished before the launch started.
      const int pt = rk * WAVE + lane;
      for (int tz = item; tz < a.n_ztiles; tz += (int)gridDim.x) {
        const int2 tij = a.ztiles[tz];
        double* T = a.S + (int64_t)tij.x * CHOL_NB * a.ld + (int64_t)tij.y * CHOL_NB;
        const bool diag_tile = a.prep.pad && tij.x == tij.y;
        for (int e = pt; e < CHOL_NB * CHOL_NB / 2; e += 4 * WAVE) {
          const int row = e >> 4, c0 = 2 * (e & 15);
          double2 v = make_double2(0.0, 0.0);
          if (diag_tile && (row == c0 || row == c0 + 1)) {
            const int64_t r = (int64_t)tij.x * CHOL_NB + row;
            double dv;
            if (r < a.prep.n_aug) dv = a.prep.pad[r] ? 1.0 : 0.0;
            else dv = r == a.prep.n_aug ? 1e300 : 1.0;
            if (row == c0) v.x = dv; else v.y = dv;
          }
          *reinterpret_cast<double2*>(T + (int64_t)row * a.ld + c0) = v;
        }
      }
      if (item == 0) {
        for (int64_t e = pt; e < a.n_vec; e += 4 * WAVE) a.vec[e] = 0.0;
        if (a.prep.pad && pt == 0) a.prep.info[0] = 0;
      }
    }
    // the item's products accumulate in fp32 over all its batches (<= 32 of 16 landmarks); the split partial is
    // stored in fp32 anyway, and round 6 measured fp64 flushes every 4 batches (72 more VGPRs: spills, and an early
    // vmcnt(0) in the loop) as no more accurate: max |S32 - S64| / sqrt(S_ii S_jj) 2.87e-7 / 4.24e-7 at configs 2 / 3
    // against 2.90e-7 / 3.93e-7, 3 us faster per build (profiles/r06_k2_ab.json)
    f4v c[3][6];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = 0; y < 6; ++y) c[x][y] = f4v{0.f, 0.f, 0.f, 0.f};
    int buf = 0;
    for (int b = 0; b < nb; ++b) {
      SK_NOW(skt);
      k2_wait4(s_ready, b + 1);
      SKP_ACC(tk0, skt);
      SK_NOW(skt);
      h8v bh[6], bl[6], ah[3], al[3];
#pragma unroll
      for (int y = 0; y < 6; ++y) {
        const int col = 16 * (6 * cg + y) + fr;
        bh[y] = *reinterpret_cast<const h8v*>(&sWt[buf][0][col][fk]);
        bl[y] = *reinterpret_cast<const h8v*>(&sWt[buf][1][col][fk]);
      }
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const int row = 16 * (3 * rg + x) + fr;
        ah[x] = *reinterpret_cast<const h8v*>(&sY[buf][0][row][fk]);
        al[x] = *reinterpret_cast<const h8v*>(&sY[buf][1][row][fk]);
      }
      k2_signal(&s_done[rk], b + 1);  // the fragments are in registers: the buffer may be re-filled
#pragma unroll
      for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 6; ++y) {
          c[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[x], bh[y], c[x][y], 0, 0, 0);
          c[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[x], bl[y], c[x][y], 0, 0, 0);
          c[x][y] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[x], bh[y], c[x][y], 0, 0, 0);
        }
      SKP_ACC(tk1, skt);
      buf = buf + 1 == NR ? 0 : buf + 1;
    }
#ifdef SK_TIMING
    if (skrec) {
      sk[12] = tk0;
      sk[4] = tk1;
    }
#endif
    // partial blocks of this split: part[item][f1 local][3q + r][f2], as k_schur writes them
    float* out = (float*)a.part + (int64_t)item * (SF * 9 * WAVE);
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = 0; y < 6; ++y)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int row = 16 * (3 * rg + x) + (lane >> 4) * 4 + v, col = 16 * (6 * cg + y) + fr;
          const int q = row / SF, i = row % SF, r = col / WAVE, f2 = col % WAVE;
          const float back = (q == 2 ? 1.f / MF_FROW : 1.f) * (r == 2 ? 1.f / MF_FROW : 1.f);  // (exact: powers of two)
          out[(i * 9 + 3 * q + r) * WAVE + f2] = c[x][y][v] * back;
        }
  }
#ifdef SK_TIMING
  __syncthreads();
  if (threadIdx.x == 0 && item < 4096) g_sk_items[item][1] = __builtin_amdgcn_s_memrealtime();
#endif
}


#ifdef SK_TIMING
extern "C" int ptzba_debug_sk(long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sk), sizeof(g_sk)) == hipSuccess ? 0 : -1;
}
extern "C" int ptzba_debug_sk_items(long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sk_items), sizeof(g_sk_items)) == hipSuccess ? 0 : -1;
}
#endif

// The tile reduction is a launch of its own and reads the split partials with plain loads.  (Rounds 3-4 also reduced
// each tile in its last split, with agent-scope loads and a counter per tile: 258 us per build with an acq_rel
// counter, not faster with write-through partials; removed in round 5.)
// lane `lane`'s copy of v (wave-uniform lane index; reads the register whether or not that lane is still active)
__device__ __forceinline__ double lane_read(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
template <typename real>
__device__ __forceinline__ void schur_reduce_elem(const SchurArgs& a, const int4 g, int e) {
  constexpr int NE = SF * 9 * WAVE;
  const int f1b = g.x, chunk = g.y;
  const int ln = e & 63, ik = e >> 6, i = ik / 9, k = ik - 9 * i, q = k / 3, r = k - 3 * q;
  const int f1 = f1b + i, f2 = f1b + WAVE * chunk + ln;
  // the window bound and both frames' system positions in one round trip (clamped indices: a thread outside the
  // window reads a valid entry and leaves)
  const int f1c = min(f1, a.n_pose - 1), f2c = min(f2, a.n_pose - 1);
  const int whi = a.frame_win_hi[f1c];
  const int64_t col0 = a.frame_pos[f1c], pf2 = a.frame_pos[f2c];
  // chunk 0: the wave's one diagonal lane (f2 == f1; i, q, r are wave-uniform) adds U of the frame over the tile's
  // splits.  The wave requests them for it in the same round trip, lane u the value of split u (clamped), and the
  // diagonal lane takes them in item order by lane reads below: one load and two registers in place of one
  // dependent load per split in one lane.
  const int last = g.w - 1;  // (a group has at least one split)
  const int ui = q <= r ? (q == 0 ? r : (q == 1 ? 2 + r : 5)) : (r == 0 ? q : (r == 1 ? 2 + q : 5));
  const double* pd = a.part_diag + (int64_t)i * 12 + ui;
  const bool tile0 = chunk == 0 && f1 < a.n_pose;  // (wave-uniform)
  double uc = 0;
  if (tile0) uc = pd[(int64_t)min(g.z + ln, last) * (SF * 12)];
  // (the fused prepare's damping operands of the diagonal lane: with the same round trip)
  const bool damp = a.prep.pad && q == r && f2 == f1;
  double Dv = 0, lambda = 0;
  if (damp) {
    lambda = a.prep.lam_dev ? *a.prep.lam_dev : a.prep.lambda;
    Dv = a.prep.D_pose[3 * (int64_t)f1c + q];
  }
  const bool in = f1 < a.n_pose && f2 >= f1 && f2 <= whi;
  double v = 0;
  if (in) {
    // the splits' partials in batches of 8 with the next batch requested before this one is summed (a tile of up
    // to 16 splits: one round trip), branch-free: an index past the group reads the group's last split and is
    // dropped.  Summed in item order.
    const real* p = (const real*)a.part;  // (uniform split base + the thread's element)
    real x[8], y[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      x[u] = p[(int64_t)min(g.z + u, last) * NE + (unsigned)e];
      y[u] = 0;
    }
    if (g.z + 8 < g.w) {
#pragma unroll
      for (int u = 0; u < 8; ++u) y[u] = p[(int64_t)min(g.z + 8 + u, last) * NE + (unsigned)e];
    }
    for (int it = g.z;;) {
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (it + u < g.w) v += (double)x[u];
      it += 8;
      if (it >= g.w) break;
#pragma unroll
      for (int u = 0; u < 8; ++u) x[u] = y[u];
      if (it + 8 < g.w) {
#pragma unroll
        for (int u = 0; u < 8; ++u)
          y[u] = p[(int64_t)min(it + 8 + u, last) * NE + (unsigned)e];
      }
    }
  }
  if (tile0) {  // (the whole wave again: the lane reads see every lane's value)
    const bool diag = in && f2 == f1;
    double du = 0;  // diag U as the chunk-0 vector block sums it (fresh, item order): the damping's scale
    const int nw = min(g.w - g.z, WAVE);
    for (int u = 0; u < nw; ++u) {
      const double uu = lane_read(uc, u);
      if (diag) {
        v += uu;
        du += uu;
      }
    }
    if (diag)
      for (int it2 = g.z + WAVE; it2 < g.w; ++it2) {  // (a tile of more than 64 splits: the rest one by one)
        const double uu = pd[(int64_t)it2 * (SF * 12)];
        v += uu;
        du += uu;
      }
    if (diag && damp) {  // fused prepare: Marquardt damping of the pose row (k_chol_prepare's rule)
      const double d = fmax(Dv, fmax(du, 1e-12));
      a.prep.D_pose[3 * (int64_t)f1 + q] = d;
      const int64_t row = col0 + q;
      a.S[row * a.ld + row] = v;
      a.S[row * a.ld + row] += lambda * d;
      return;
    }
  }
  if (!in) return;
  const int64_t ld = a.ld;
  if (pf2 >= col0) a.S[(pf2 + r) * ld + col0 + q] = v;
  else a.S[(col0 + q) * ld + pf2 + r] = v;
}
__device__ __forceinline__ void schur_reduce_vec(const SchurArgs& a, const int4 g, int tid) {
  const int f1b = g.x;
  // threads [0, 3 SF): g_pose and sum W V~^-1 g of (frame, q2) -> b, g_pose; threads [3 SF, 6 SF): diag U -> dU.
  // Each of a frame's 12 values is a sum of its own (split by split in item order), so a thread reads only the
  // ones it writes: eight splits in flight with clamped indices, the system row with the first batch.
  const bool diag = tid >= SF * 3;
  const int t = diag ? tid - SF * 3 : tid;
  const int i2 = t / 3, q2 = t - 3 * i2, f = f1b + i2;
  if (f >= a.n_pose) return;
  const int c0 = a.frame_pos[f];
  const int last = g.w - 1;
  const int k0 = diag ? (q2 == 0 ? 0 : (q2 == 1 ? 3 : 5)) : 6 + q2;
  const double* pd = a.part_diag + (int64_t)i2 * 12 + k0;
  double d0 = 0, d1 = 0;  // value k0 and (g_pose threads) value k0 + 3
  for (int it2 = g.z; it2 < g.w; it2 += 8) {
    double x0[8], x1[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double* ps = pd + (int64_t)min(it2 + u, last) * (SF * 12);
      x0[u] = *ps;
      x1[u] = *(diag ? ps : ps + 3);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (it2 + u < g.w) {
        d0 += x0[u];
        d1 += x1[u];
      }
  }
  if (diag) {
    a.dU[c0 + q2] = d0;
    return;
  }
  const double bv = -d0 + d1;
  a.b[c0 + q2] = bv;
  a.g_pose[c0 + q2] = d0;
  if (a.prep.pad) a.S[a.prep.n_aug * a.ld + c0 + q2] = bv;  // fused prepare: the augmented row b^T
}

// (Four elements per reduce thread with 16-B partial loads, `SR_VEC`, and four independent elements with all their
// partials in flight, measured slower (r03v: 77-78 vs 71 us; r05ac: 93 vs 72 us per build), are gone since round 5.)

// tile reduction: fixed-order sum of the splits, U on the diagonal blocks, write the lower triangle in the
// system order (mirror when f2 precedes f1); chunk-0 tiles also write b | g_pose | diag U of their frames.
// fp32 partials: thread = four elements of a tile (grid: tile x 18 blocks of 256); fp64: one element
// (tile x 72 blocks).
template <typename real>
__global__ __launch_bounds__(256, sizeof(real) == 4 ? 8 : 6) void k_schur_reduce(SchurArgs a) {
  if (a.skip_if && *a.skip_if) return;
  const int4 g = a.groups[blockIdx.y];  // {f1b, chunk, first item, end item}
  schur_reduce_elem<real>(a, g, blockIdx.x * 256 + threadIdx.x);
  if (g.y == 0 && blockIdx.x == 0 && threadIdx.x < SF * 6) schur_reduce_vec(a, g, threadIdx.x);
}

template <typename real>
void launch_schur(const SchurArgs& a, int n_items, int n_groups, int n_fixed, hipStream_t st, bool valu32) {
  const int n_free = a.n_pose - n_fixed;
  if (n_free <= 0) return;
  // fp32: the matrix cores (fp16 hi/lo splits), or with valu32 the VALU kernel on the float32 slots -- float32
  // products, fp64 flush per batch -- for the covariance build, whose error the split-fp16 products would dominate;
  // fp64: the VALU kernel
  if (n_items > 0) {
    if (sizeof(real) == 4 && !valu32) hipLaunchKernelGGL(k_schur_mfp, dim3(n_items), dim3(512), 0, st, a);
    else hipLaunchKernelGGL(k_schur<real>, dim3(n_items), dim3(512), 0, st, a);
  }
  if (n_groups > 0)
    hipLaunchKernelGGL(k_schur_reduce<real>, dim3(SF * 9 * WAVE / 256, n_groups),
                       dim3(256), 0, st, a);
}

template void launch_schur<float>(const SchurArgs&, int, int, int, hipStream_t, bool);
template void launch_schur<double>(const SchurArgs&, int, int, int, hipStream_t, bool);

}  // namespace ptzba
