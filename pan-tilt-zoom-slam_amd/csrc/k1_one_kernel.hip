// K1 on a merged record stream that holds exactly one record per segment (problem_layout.h: pair-form input whose
// repeats are all adjacent -- config 3, the reference's pipeline): `k_linearize_one`.
//
// Same work split, tables, outputs and arithmetic per record as k_linearize (ba_kernels.hip): one wave per landmark,
// K1_WPB landmarks per workgroup, the workgroup's frame range of the fp64 frame tables staged in LDS (a workgroup whose
// range exceeds K1_FT_LDS reads them from global memory).  What is gone is phase B: segment s of the landmark owns
// record r0 + (s - s0), so the lane that projects the segment loads that record, forms its residual, robust weights and
// cost term and goes straight on to the segment's Jacobian and normal-equation blocks -- no key stream, no 4-record
// groups, no segmented scan, no LDS sums, no CSR load for later windows.  A kernel of its own, in its own translation
// unit: as a further form of the k_linearize template it changed how hipcc compiled the other forms.  The
// frame staging, the fp64 projection, the wave totals and the launch dispatch are k_linearize's own (k1_device.h).
#include "../../include/ptzba.h"
#include "k1_device.h"

namespace ptzba {

namespace {

// DISP: the displaced camera model (ptzba_common.h; LinArgs::disp) in the fp64 projection and in the Jacobian
template <typename real, int LOSS, bool DISP>
__global__ __launch_bounds__(64 * K1_WPB, 4) void k_linearize_one(LinArgs a) {
  __shared__ K1FrameLds s_ft;
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int task = blockIdx.x * K1_WPB + wv;
  if (a.run_if && !*a.run_if) return;  // conditional re-linearisation (device-driven LM): the whole grid leaves
  const int tq = min(task, a.n_work - 1);
  const int4 wd = a.lm_work[2 * tq];      // {landmark, first segment, end segment, first record}
  const int4 wm = a.lm_work[2 * tq + 1];  // {first frame, last frame, slot offset, -}
  int fbase;                              // the first staged frame
  const bool ftl_ok = k1_stage_frames(a, s_ft, fbase);  // (else this workgroup reads the tables from global memory)
  __syncthreads();                                       // the block's only barrier
  if (task >= a.n_work) return;                          // whole wave leaves after the barrier

  const int l = wd.x, s0 = wd.y, s1 = wd.z;
  const RayTab<double> R64 = ((const RayTab<double>*)a.rt64)[l];
  RayTab<real> R;  // the record-precision table is the rounded fp64 one (k_tables)
  R.p0 = (real)R64.p0; R.p1 = (real)R64.p1; R.d0t = (real)R64.d0t; R.d1t = (real)R64.d1t; R.d1p = (real)R64.d1p;
  const real* __restrict__ rec_xy = (const real*)a.rec_xy;
  const real* __restrict__ rec_w = (const real*)a.rec_w;
  const bool alt = a.sel && ((*a.sel ^ a.sel_xor) & 1);  // device-chosen linearisation slot
  real* __restrict__ ug_slot = (real*)(alt ? a.ug_slot1 : a.ug_slot);
  real* __restrict__ w_slot = (real*)(alt ? a.w_slot1 : a.w_slot);
  const int64_t slot0 = (int64_t)wm.z - wm.x;
  const int64_t r0 = (int64_t)(uint32_t)wd.w - s0;  // record of segment s: r0 + s
  const real u = (real)a.u, v = (real)a.v;
  const real fs2 = (real)a.fs2, ifs2 = (real)a.inv_fs2;
  const real hc = (real)(a.hcurv_dev ? *a.hcurv_dev : a.hcurv);
  (void)fs2; (void)ifs2; (void)hc;

  double V00 = 0, V01 = 0, V11 = 0, g0 = 0, g1 = 0, cost = 0;
  for (int s = s0 + lane; s < s1; s += WAVE) {
    const int64_t r = r0 + s;
    real ox, oy;
    if constexpr (sizeof(real) == 4) {
      const float2 o = reinterpret_cast<const float2*>(rec_xy)[r];
      ox = o.x; oy = o.y;
    } else {
      const double2 o = reinterpret_cast<const double2*>(rec_xy)[r];
      ox = o.x; oy = o.y;
    }
    const real wt = rec_w[r];
    const int fs = a.seg_frame[s];
    // the segment's projection in fp64, as the offset from its base observation (O(residual) magnitudes in `real`)
    FrameTab<double> F64;
    if (ftl_ok) {
      const int fl = fs - fbase;
      F64.ca = s_ft[0][fl]; F64.sa = s_ft[1][fl]; F64.cb = s_ft[2][fl]; F64.sb = s_ft[3][fl]; F64.f = s_ft[4][fl];
      F64.pad0 = F64.pad1 = F64.pad2 = 0.0;
    } else {
      F64 = ((const FrameTab<double>*)a.ft64)[fs];
    }
    double x64, y64;
    k1_project64<DISP>(a, F64, R64, x64, y64);
    const double2 bs = a.seg_base[s];
    const real rx = (real)(x64 - bs.x) - ox, ry = (real)(y64 - bs.y) - oy;
    // the record's robust terms (k_linearize's consume_c): gradient weights wx, wy = w rho', Hessian weights hx, hy
    real wx, wy, c, hx, hy;
    if constexpr (LOSS == 0) {
      wx = wt; wy = wt;
      hx = wt; hy = wt;
      c = wt * (rx * rx + ry * ry);
    } else if constexpr (LOSS == 1) {
      real zx = rx * rx * ifs2, zy = ry * ry * ifs2;
      bool ix = zx <= (real)1, iy = zy <= (real)1;
      real sqx, sqy;
      if constexpr (sizeof(real) == 4) {
        const real rsx = __builtin_amdgcn_rsqf(ix ? (real)1 : zx), rsy = __builtin_amdgcn_rsqf(iy ? (real)1 : zy);
        sqx = zx * rsx; sqy = zy * rsy;
        wx = ix ? wt : wt * rsx;
        wy = iy ? wt : wt * rsy;
      } else {
        sqx = sqrt(zx); sqy = sqrt(zy);
        wx = ix ? wt : wt / sqx;
        wy = iy ? wt : wt / sqy;
      }
      c = wt * fs2 * ((ix ? zx : (real)2 * sqx - (real)1) + (iy ? zy : (real)2 * sqy - (real)1));
      hx = ix ? wx : wx * hc;
      hy = iy ? wy : wy * hc;
    } else {  // soft_l1 / cauchy / arctan (robust_loss.h)
      real rhx, rhy, w1x, w1y, wnx, wny;
      robust_eval<LOSS, real>(rx * rx * ifs2, rhx, w1x, wnx);
      robust_eval<LOSS, real>(ry * ry * ifs2, rhy, w1y, wny);
      wx = wt * w1x; wy = wt * w1y;
      hx = wt * robust_curv(w1x, wnx, hc);
      hy = wt * robust_curv(w1y, wny, hc);
      c = wt * fs2 * (rhx + rhy);
    }
    cost += (double)c;
    const real Sx = hx, Sy = hy, Srx = wx * rx, Sry = wy * ry;
    // the segment's Jacobian and blocks (k_linearize's phase C)
    real x, y, J[2][5];
    if constexpr (DISP) {
      real dc[3], dk[3];
      lin_disp<real>(a, dc, dk);
      FrameTab<real> F;
      if (ftl_ok) {
        F.ca = (real)F64.ca; F.sa = (real)F64.sa; F.cb = (real)F64.cb; F.sb = (real)F64.sb; F.f = (real)F64.f;
        F.pad0 = F.pad1 = F.pad2 = (real)0;
      } else {
        F = ((const FrameTab<real>*)a.ft)[fs];
      }
      ptz_project_jac_disp<real>(F, R, u, v, dc, dk, x, y, J);
    } else if (ftl_ok) {
      FrameTab<real> F;
      F.ca = (real)F64.ca; F.sa = (real)F64.sa; F.cb = (real)F64.cb; F.sb = (real)F64.sb; F.f = (real)F64.f;
      F.pad0 = F.pad1 = F.pad2 = (real)0;
      ptz_project_jac<real>(F, R, u, v, x, y, J);
    } else {
      ptz_project_jac<real>(((const FrameTab<real>*)a.ft)[fs], R, u, v, x, y, J);
    }
    real W[6];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      W[2 * p + 0] = Sx * J[0][p] * J[0][3] + Sy * J[1][p] * J[1][3];
      W[2 * p + 1] = Sx * J[0][p] * J[0][4] + Sy * J[1][p] * J[1][4];
    }
    slot_store6(w_slot + (slot0 + fs) * W_STRIDE, W);
    const real UG[9] = {Sx * J[0][0] * J[0][0] + Sy * J[1][0] * J[1][0], Sx * J[0][0] * J[0][1] + Sy * J[1][0] * J[1][1],
                        Sx * J[0][0] * J[0][2] + Sy * J[1][0] * J[1][2], Sx * J[0][1] * J[0][1] + Sy * J[1][1] * J[1][1],
                        Sx * J[0][1] * J[0][2] + Sy * J[1][1] * J[1][2], Sx * J[0][2] * J[0][2] + Sy * J[1][2] * J[1][2],
                        J[0][0] * Srx + J[1][0] * Sry, J[0][1] * Srx + J[1][1] * Sry, J[0][2] * Srx + J[1][2] * Sry};
    slot_store9(ug_slot + (slot0 + fs) * UG_STRIDE, UG);
    V00 += (double)(Sx * J[0][3] * J[0][3] + Sy * J[1][3] * J[1][3]);
    V01 += (double)(Sx * J[0][3] * J[0][4] + Sy * J[1][3] * J[1][4]);
    V11 += (double)(Sx * J[0][4] * J[0][4] + Sy * J[1][4] * J[1][4]);
    g0 += (double)(J[0][3] * Srx + J[1][3] * Sry);
    g1 += (double)(J[0][4] * Srx + J[1][4] * Sry);
  }
  // (the loop's trip count differs per lane: every lane is active again here, as the DPP totals need)
  double lm[6] = {V00, V01, V11, g0, g1, cost};
  k1_store_landmark(lm, (alt ? a.lm_out1 : a.lm_out) + (int64_t)l * 8);
}

}  // namespace

template <typename real>
void launch_linearize_one(const LinArgs& a, int loss, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  k1_with_loss(loss, [&](auto loss_c) {
    k1_with_flag(a.displaced, [&](auto disp_c) {
      k1_launch(k_linearize_one<real, decltype(loss_c)::value, decltype(disp_c)::value>, a, st, ev0, ev1);
    });
  });
}

template void launch_linearize_one<float>(const LinArgs&, int, hipStream_t, hipEvent_t, hipEvent_t);
template void launch_linearize_one<double>(const LinArgs&, int, hipStream_t, hipEvent_t, hipEvent_t);

}  // namespace ptzba
