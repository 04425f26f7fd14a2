// The pieces K1's two kernels share (internal header).  k_linearize (ba_kernels.hip) and k_linearize_one
// (k1_one_kernel.hip) stay kernels of their own; written once here are the DPP shuffles and wave totals, the
// staging of the workgroup's frame tables, the fp64 projection, the landmark's output row and the launch dispatch.
// Device pieces are __device__ __forceinline__; barriers and early exits stay in the kernels.
// Not here, and still twins in the two kernels: the table fetches, the record's robust terms, the Jacobian call and the
// segment's blocks -- written as functions they compile to other code in k_linearize (other VGPR counts, in the fp32
// Huber forms too), so the merge and displacement tests still guard those by comparing bits.
#pragma once
#include <hip/hip_ext.h>

#include "ptzba_common.h"
#include "ptzba_kernels.h"
#include "robust_loss.h"

#include <type_traits>

namespace ptzba {

// ---- DPP lane shuffles (VALU, no LDS round trip).  Lanes whose source is out of range or whose row
// is masked off read 0 (bound_ctrl), which the segmented scan treats as "different segment".
template <int CTRL, int ROWMASK>
__device__ __forceinline__ int dpp_i(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, ROWMASK, 0xf, true);
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ float dpp_r(float x) {
  return __int_as_float(dpp_i<CTRL, ROWMASK>(__float_as_int(x)));
}
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_r(double x) {
  const int lo = dpp_i<CTRL, ROWMASK>(__double2loint(x)), hi = dpp_i<CTRL, ROWMASK>(__double2hiint(x));
  return __hiloint2double(hi, lo);
}
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;
constexpr int DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143, DPP_WAVE_SHL1 = 0x130;

// Wave total by a DPP inclusive scan (VALU only): the sum is valid in lane 63.  Needs every lane active.
// The butterfly of wave_sum costs one LDS round trip (ds_bpermute) per step and value: at the end of K1
// six fp64 butterflies took ~5K cycles per wave, 15 % of the wave's time (K1_TIMING build).
template <typename T>
__device__ __forceinline__ T wave_total(T v) {
  v += dpp_r<DPP_ROW_SHR1, 0xf>(v);
  v += dpp_r<DPP_ROW_SHR2, 0xf>(v);
  v += dpp_r<DPP_ROW_SHR4, 0xf>(v);
  v += dpp_r<DPP_ROW_SHR8, 0xf>(v);
  v += dpp_r<DPP_ROW_BCAST15, 0xa>(v);
  v += dpp_r<DPP_ROW_BCAST31, 0xc>(v);
  return v;
}

// Six wave totals at once, step by step across the values (round 6): each DPP step's six reads of the previous step's
// results are independent, so the DPP read-after-write wait states of one value are covered by the others' work
// instead of s_nop padding (six back-to-back wave_total calls serialised).  Same additions, same order per value.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void wave_total_step6(double (&v)[6]) {
  double t[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) t[k] = dpp_r<CTRL, ROWMASK>(v[k]);
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] += t[k];
}
__device__ __forceinline__ void wave_total6(double (&v)[6]) {
  wave_total_step6<DPP_ROW_SHR1, 0xf>(v);
  wave_total_step6<DPP_ROW_SHR2, 0xf>(v);
  wave_total_step6<DPP_ROW_SHR4, 0xf>(v);
  wave_total_step6<DPP_ROW_SHR8, 0xf>(v);
  wave_total_step6<DPP_ROW_BCAST15, 0xa>(v);
  wave_total_step6<DPP_ROW_BCAST31, 0xc>(v);
}
// the landmark's wave totals {V00, V01, V11, g0, g1, cost} into its row lm_out[l][8] (every lane active)
__device__ __forceinline__ void k1_store_landmark(double (&lm)[6], double* o) {
  wave_total6(lm);
  if (lane_id() == WAVE - 1) {
    o[0] = lm[0]; o[1] = lm[1]; o[2] = lm[2]; o[3] = lm[3]; o[4] = lm[4]; o[5] = 0.5 * lm[5]; o[6] = 0; o[7] = 0;
  }
}

// ---- the workgroup's frame tables.  s_ft[k][fs - fbase]: ca, sa, cb, sb, f per staged frame (fp64)
typedef double K1FrameLds[5][K1_FT_LDS];
// The frames the workgroup's landmarks see, [min first frame, max last frame] over its K1_WPB descriptors (scalar
// loads; the work order keeps a workgroup's landmarks close in frame order, so this is ~a coupling window, not the whole
// table), staged when they fit the LDS table: returns whether they do (else the workgroup reads the tables from global
// memory), fbase: the first staged frame.  The caller's __syncthreads() follows: the block's only barrier.
__device__ __forceinline__ bool k1_stage_frames(const LinArgs& a, K1FrameLds& s_ft, int& fbase) {
  int fmax = -1;
  fbase = a.n_pose;
#pragma unroll
  for (int q = 0; q < K1_WPB; ++q) {
    const int4 m = a.lm_work[2 * min((int)blockIdx.x * K1_WPB + q, a.n_work - 1) + 1];
    fbase = min(fbase, m.x);
    fmax = max(fmax, m.y);
  }
  const bool ftl_ok = k1_ftl_fits(fbase, fmax);
  if (ftl_ok)
    for (int e = fbase + (int)threadIdx.x; e <= fmax; e += blockDim.x) {
      const double4 t0 = reinterpret_cast<const double4*>(a.ft64)[2 * e];
      const double f = reinterpret_cast<const double*>(a.ft64)[8 * e + 4];
      const int el = e - fbase;
      s_ft[0][el] = t0.x; s_ft[1][el] = t0.y; s_ft[2][el] = t0.z; s_ft[3][el] = t0.w; s_ft[4][el] = f;
    }
  return ftl_ok;
}

// ---- the segment's fp64 projection.  DISP: the displaced camera model (ptzba_common.h ptz_project_disp; LinArgs::disp)
template <bool DISP>
__device__ __forceinline__ void k1_project64(const LinArgs& a, const FrameTab<double>& F, const RayTab<double>& R64,
                                             double& x, double& y) {
  if constexpr (DISP) {
    const double dc[3] = {a.disp[0], a.disp[1], a.disp[2]}, dk[3] = {a.disp[3], a.disp[4], a.disp[5]};
    ptz_project_disp<double>(F, R64, a.u, a.v, dc, dk, x, y);
  } else {
    ptz_project<double>(F, R64, a.u, a.v, x, y);
  }
}

// ---- launch dispatch (host): f(integral_constant<int, PTZBA_LOSS_*>) for a runtime loss id, f(bool_constant) for a flag
template <typename F>
inline void k1_with_loss(int loss, F&& f) {
  switch (loss) {
    case PTZBA_LOSS_LINEAR: f(std::integral_constant<int, PTZBA_LOSS_LINEAR>{}); break;
    case PTZBA_LOSS_HUBER: f(std::integral_constant<int, PTZBA_LOSS_HUBER>{}); break;
    case PTZBA_LOSS_SOFT_L1: f(std::integral_constant<int, PTZBA_LOSS_SOFT_L1>{}); break;
    case PTZBA_LOSS_CAUCHY: f(std::integral_constant<int, PTZBA_LOSS_CAUCHY>{}); break;
    default: f(std::integral_constant<int, PTZBA_LOSS_ARCTAN>{}); break;  // (ptzba_set_problem refuses other ids)
  }
}
template <typename F>
inline void k1_with_flag(bool on, F&& f) {
  on ? f(std::true_type{}) : f(std::false_type{});
}
// one wave per work item, K1_WPB per workgroup; ev0 / ev1: the kernel timer's events (ptzba_kernel_times)
template <typename K>
inline void k1_launch(K kern, const LinArgs& a, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  if (a.n_work <= 0) return;
  const dim3 grid((a.n_work + K1_WPB - 1) / K1_WPB);
  if (ev0) hipExtLaunchKernelGGL(kern, grid, dim3(64 * K1_WPB), 0, st, ev0, ev1, 0, a);
  else hipLaunchKernelGGL(kern, grid, dim3(64 * K1_WPB), 0, st, a);
}

}  // namespace ptzba
