// Pose-only refinement with the rays fixed (gfx950, fp64).
//
// relocalization.py:186 refines a lost camera's (pan, tilt, f) with
//   least_squares(_compute_residual, pose, x_scale='jac', ftol=1e-4, method='trf', args=(rays, points, u, v))
// over the from_ray_to_image residual (relocalization.py:22-40).  Here one 256-thread workgroup per
// hypothesis runs the whole Levenberg-Marquardt loop on the device: residual + 2x3 analytic pose
// Jacobian per correspondence (the BA projection of ptzba_common.h, |q2| in y), block reduction of
// J^T W J (6) / J^T W r (3) / cost, a 3x3 damped solve, trial evaluation, gain-ratio acceptance and
// scipy-style termination — with the same Marquardt scaling and lambda rule as ptzba.LMSolver.
// Hypotheses share the correspondence set or take CSR subsets of it (preemptive-RANSAC style batches,
// SURVEY §8f-3).
// The LM loop itself is the device function rf_lm of pose_lm.h (the pose RANSAC refits with it too).
// `ptz_refine_poses_disp` runs the same loop under the displaced camera K (R p + d(f)): the DISP
// instantiation of the kernel, with the six displacement values by value in RefineArgs.
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/ptzba.h"
#include "host_util.h"
#include "pose_lm.h"
#include "ptzba_common.h"
#include "ptzba_kernels.h"

namespace ptzba {

template <bool DISP>
__global__ __launch_bounds__(RF_THREADS) void k_refine_poses(RefineArgs a) {
  __shared__ RefineShared S;
  const int h = blockIdx.x;
  double p[3] = {a.ptz[3 * h], a.ptz[3 * h + 1], a.ptz[3 * h + 2]};
  double cost;
  int it, status;
  rf_lm<DISP>(a, h, p, cost, it, status, S);
  if (threadIdx.x == 0) {
    a.ptz[3 * h] = p[0];
    a.ptz[3 * h + 1] = p[1];
    a.ptz[3 * h + 2] = p[2];
    if (a.cost_out) a.cost_out[h] = cost;
    if (a.iters_out) a.iters_out[h] = it;
    if (a.status_out) a.status_out[h] = status;
  }
}

}  // namespace ptzba

using namespace ptzba;

// d6: the six displacement values, or nullptr for the displacement-free kernel
static int refine_poses(int device, int32_t n_hyp, double* ptz_inout, int64_t n_corr, const double* rays,
                        const double* points, double u, double v, const int64_t* subset_offsets,
                        const int32_t* subset_index, const ptz_refine_opts* opts, const double* d6, double* cost_out,
                        int32_t* iters_out, int32_t* status_out) {
  if (n_hyp < 0 || n_corr < 0) return fail("bad sizes");
  if (n_hyp == 0) return 0;
  if (!ptz_inout || (n_corr > 0 && (!rays || !points))) return fail("null argument");
  ptz_refine_opts o{100, PTZBA_LOSS_LINEAR, 1e-4, 1e-8, 1.0};
  if (opts) o = *opts;
  if (o.max_iter < 0 || !(o.ftol >= 0) || !(o.xtol >= 0)) return fail("bad options");
  if (!loss_is_known(o.loss)) return fail("bad loss %d", o.loss);
  if (o.loss != PTZBA_LOSS_LINEAR && !(o.f_scale > 0)) return fail("a robust loss needs f_scale > 0");
  int64_t n_sub = 0;
  if (subset_offsets) {
    if (subset_offsets[0] != 0) return fail("subset_offsets[0] must be 0");
    for (int h = 0; h < n_hyp; ++h)
      if (subset_offsets[h + 1] < subset_offsets[h]) return fail("subset_offsets not ascending");
    n_sub = subset_offsets[n_hyp];
    for (int64_t k = 0; k < n_sub; ++k)
      if (subset_index[k] < 0 || subset_index[k] >= n_corr) return fail("subset index %lld out of range", (long long)k);
  }
  if (select_device(device)) return -1;
  DBuf dptz, drays, dpts, doff, didx, dcost, dit, dst;
  if (dptz.alloc((size_t)n_hyp * 24) || drays.alloc((size_t)n_corr * 16) || dpts.alloc((size_t)n_corr * 16) ||
      dcost.alloc((size_t)n_hyp * 8) || dit.alloc((size_t)n_hyp * 4) || dst.alloc((size_t)n_hyp * 4))
    return -1;
  HIPCHK(hipMemcpy(dptz.p, ptz_inout, (size_t)n_hyp * 24, hipMemcpyHostToDevice));
  if (n_corr) {
    HIPCHK(hipMemcpy(drays.p, rays, (size_t)n_corr * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dpts.p, points, (size_t)n_corr * 16, hipMemcpyHostToDevice));
  }
  if (subset_offsets) {
    if (doff.alloc((size_t)(n_hyp + 1) * 8) || didx.alloc((size_t)n_sub * 4 + 4)) return -1;
    HIPCHK(hipMemcpy(doff.p, subset_offsets, (size_t)(n_hyp + 1) * 8, hipMemcpyHostToDevice));
    if (n_sub) HIPCHK(hipMemcpy(didx.p, subset_index, (size_t)n_sub * 4, hipMemcpyHostToDevice));
  }
  RefineArgs a;
  a.n_hyp = n_hyp;
  a.ptz = dptz.as<double>();
  a.sub_off = subset_offsets ? doff.as<int64_t>() : nullptr;
  a.sub_idx = subset_offsets ? didx.as<int32_t>() : nullptr;
  a.n_corr = n_corr;
  a.rays = drays.as<double>();
  a.pts = dpts.as<double>();
  a.u = u;
  a.v = v;
  a.max_iter = o.max_iter;
  a.loss = o.loss;
  a.ftol = o.ftol;
  a.xtol = o.xtol;
  a.fs2 = o.f_scale * o.f_scale;
  a.inv_fs2 = 1.0 / a.fs2;
  a.cost_out = dcost.as<double>();
  a.iters_out = dit.as<int>();
  a.status_out = dst.as<int>();
  for (int k = 0; k < 3; ++k) {
    a.dc[k] = d6 ? d6[k] : 0.0;
    a.dk[k] = d6 ? d6[3 + k] : 0.0;
  }
  if (d6) hipLaunchKernelGGL(k_refine_poses<true>, dim3(n_hyp), dim3(RF_THREADS), 0, nullptr, a);
  else hipLaunchKernelGGL(k_refine_poses<false>, dim3(n_hyp), dim3(RF_THREADS), 0, nullptr, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(ptz_inout, dptz.p, (size_t)n_hyp * 24, hipMemcpyDeviceToHost));
  if (cost_out) HIPCHK(hipMemcpy(cost_out, dcost.p, (size_t)n_hyp * 8, hipMemcpyDeviceToHost));
  if (iters_out) HIPCHK(hipMemcpy(iters_out, dit.p, (size_t)n_hyp * 4, hipMemcpyDeviceToHost));
  if (status_out) HIPCHK(hipMemcpy(status_out, dst.p, (size_t)n_hyp * 4, hipMemcpyDeviceToHost));
  return 0;
}

int ptz_refine_poses(int device, int32_t n_hyp, double* ptz_inout, int64_t n_corr, const double* rays,
                     const double* points, double u, double v, const int64_t* subset_offsets,
                     const int32_t* subset_index, const ptz_refine_opts* opts, double* cost_out, int32_t* iters_out,
                     int32_t* status_out) {
  return refine_poses(device, n_hyp, ptz_inout, n_corr, rays, points, u, v, subset_offsets, subset_index, opts, nullptr,
                      cost_out, iters_out, status_out);
}

int ptz_refine_poses_disp(int device, int32_t n_hyp, double* ptz_inout, int64_t n_corr, const double* rays,
                          const double* points, double u, double v, const int64_t* subset_offsets,
                          const int32_t* subset_index, const ptz_refine_opts* opts, double* cost_out, int32_t* iters_out,
                          int32_t* status_out, const double* displacement6) {
  const double* d6 = nullptr;
  if (displacement_arg(displacement6, d6)) return -1;
  return refine_poses(device, n_hyp, ptz_inout, n_corr, rays, points, u, v, subset_offsets, subset_index, opts, d6,
                      cost_out, iters_out, status_out);
}
