// The pose-only Levenberg-Marquardt loop of pose_refine.hip as device code: one 256-thread workgroup refines one
// hypothesis (residual + 2x3 analytic pose Jacobian per correspondence, block reduction of J^T W J / J^T W r /
// cost, a damped 3x3 solve, gain-ratio acceptance, scipy-style termination).  Shared by k_refine_poses
// (pose_refine.hip) and the refit of the pose RANSAC (pose_ransac.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ptzba.h"
#include "ptzba_common.h"
#include "robust_loss.h"

namespace ptzba {

constexpr int RF_THREADS = 256;

struct RefineArgs {
  int n_hyp;
  double* ptz;             // [n_hyp][3] in/out
  const int64_t* sub_off;  // [n_hyp+1] or nullptr
  const int32_t* sub_idx;
  int64_t n_corr;
  const double* rays;  // [n_corr][2]
  const double* pts;   // [n_corr][2]
  double u, v;
  int max_iter, loss;
  double ftol, xtol, fs2, inv_fs2;
  double* cost_out;
  int* iters_out;
  int* status_out;
  double dc[3], dk[3];  // projection-centre displacement d(f) = dc + dk f; read by the DISP instantiations alone
};

// LDS of one rf_lm call (a __shared__ object of the calling kernel)
struct RefineShared {
  double red[RF_THREADS / WAVE][10];
  double trial[3];
  int ctl[2];  // [0]: 1 = stop, [1]: 1 = accepted
};

// sum over the workgroup of nv values (wave reduce, then LDS)
template <int NV>
__device__ __forceinline__ void block_sum(double (&x)[NV], double (*red)[NV]) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) x[k] = wave_sum(x[k]);
  if (lane_id() == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) red[w][k] = x[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    double s = 0;
    for (int q = 0; q < RF_THREADS / WAVE; ++q) s += red[q][k];
    x[k] = s;
  }
  __syncthreads();
}

// cost (0.5 sum rho) and, with JAC, J^T W J (upper 6) and J^T W r (3) at pose p; with DISP under the displaced model
// K (R p + d(f)) of ptz_project_disp, whose Jacobian carries the extended f column
template <bool JAC, bool DISP>
__device__ void rf_eval(const RefineArgs& a, int h, const double p[3], double (&out)[10], double (*red)[10]) {
  const FrameTab<double> F = make_frame_tab<double>(p[0], p[1], p[2]);
  double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t b0 = a.sub_off ? a.sub_off[h] : 0, b1 = a.sub_off ? a.sub_off[h + 1] : a.n_corr;
  for (int64_t k = b0 + threadIdx.x; k < b1; k += RF_THREADS) {
    const int64_t c = a.sub_off ? (int64_t)a.sub_idx[k] : k;
    const RayTab<double> R = make_ray_tab<double>(a.rays[2 * c], a.rays[2 * c + 1]);
    double x, y, J[2][5];
    if (DISP) {
      if (JAC) ptz_project_jac_disp<double>(F, R, a.u, a.v, a.dc, a.dk, x, y, J);
      else ptz_project_disp<double>(F, R, a.u, a.v, a.dc, a.dk, x, y);
    } else {
      if (JAC) ptz_project_jac<double>(F, R, a.u, a.v, x, y, J);
      else ptz_project<double>(F, R, a.u, a.v, x, y);
    }
    const double rx = x - a.pts[2 * c], ry = y - a.pts[2 * c + 1];
    double wx = 1, wy = 1, c2;
    if (a.loss == PTZBA_LOSS_LINEAR) {
      c2 = rx * rx + ry * ry;
    } else if (a.loss != PTZBA_LOSS_HUBER) {  // soft_l1 / cauchy / arctan (robust_loss.h), IRLS weight rho'(z)
      double px, py, nx, ny;
      robust_eval_id(a.loss, rx * rx * a.inv_fs2, px, wx, nx);
      robust_eval_id(a.loss, ry * ry * a.inv_fs2, py, wy, ny);
      c2 = a.fs2 * (px + py);
    } else {  // scipy 'huber' as in K1: rho(z) = z | 2 sqrt(z) - 1, IRLS weight rho'(z)
      const double zx = rx * rx * a.inv_fs2, zy = ry * ry * a.inv_fs2;
      const double sx = sqrt(zx), sy = sqrt(zy);
      const bool ix = zx <= 1.0, iy = zy <= 1.0;
      wx = ix ? 1.0 : 1.0 / sx;
      wy = iy ? 1.0 : 1.0 / sy;
      c2 = a.fs2 * ((ix ? zx : 2 * sx - 1) + (iy ? zy : 2 * sy - 1));
    }
    acc[9] += c2;
    if (JAC) {
      int t = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) acc[t++] += wx * J[0][i] * J[0][j] + wy * J[1][i] * J[1][j];
#pragma unroll
      for (int i = 0; i < 3; ++i) acc[6 + i] += wx * J[0][i] * rx + wy * J[1][i] * ry;
    }
  }
  block_sum<10>(acc, red);
#pragma unroll
  for (int k = 0; k < 10; ++k) out[k] = acc[k];
  out[9] *= 0.5;
}

// The LM loop of hypothesis h from pose p (in/out), run by all RF_THREADS threads of the workgroup.  Every thread
// returns the same p; thread 0 alone holds cost, it (accepted iterations) and status (2 ftol, 3 xtol, 0 max_iter,
// -1 no decrease).  DISP selects the camera model of rf_eval; the damping, the acceptance and the stop rules are one code.
template <bool DISP>
__device__ __forceinline__ void rf_lm(const RefineArgs& a, int h, double (&p)[3], double& cost, int& it, int& status,
                                      RefineShared& S) {
  double lin[10];
  rf_eval<true, DISP>(a, h, p, lin, S.red);
  cost = lin[9];
  double lam = 1e-4, nu = 2.0, D[3] = {0, 0, 0};
  it = 0;
  status = 0;
  for (; it < a.max_iter;) {
    // damped 3x3 solve (H + lam diag(D)) d = -g with Marquardt scaling D = max over history of diag(H)
    double d[3] = {0, 0, 0}, pred = 0;
    bool ok = true;
    if (threadIdx.x == 0) {
      const double Hd[3] = {lin[0], lin[3], lin[5]};
      for (int i = 0; i < 3; ++i) D[i] = fmax(D[i], fmax(Hd[i], 1e-12));
      double A[3][3] = {{lin[0] + lam * D[0], lin[1], lin[2]},
                        {lin[1], lin[3] + lam * D[1], lin[4]},
                        {lin[2], lin[4], lin[5] + lam * D[2]}};
      double g[3] = {lin[6], lin[7], lin[8]};
      // Cholesky
      double L00 = A[0][0];
      ok = L00 > 0;
      L00 = sqrt(fmax(L00, 1e-300));
      const double L10 = A[1][0] / L00, L20 = A[2][0] / L00;
      double L11 = A[1][1] - L10 * L10;
      ok = ok && L11 > 0;
      L11 = sqrt(fmax(L11, 1e-300));
      const double L21 = (A[2][1] - L20 * L10) / L11;
      double L22 = A[2][2] - L20 * L20 - L21 * L21;
      ok = ok && L22 > 0;
      L22 = sqrt(fmax(L22, 1e-300));
      const double y0 = -g[0] / L00, y1 = (-g[1] - L10 * y0) / L11, y2 = (-g[2] - L20 * y0 - L21 * y1) / L22;
      d[2] = y2 / L22;
      d[1] = (y1 - L21 * d[2]) / L11;
      d[0] = (y0 - L10 * d[1] - L20 * d[2]) / L00;
      for (int i = 0; i < 3; ++i) pred += -0.5 * g[i] * d[i] + 0.5 * lam * D[i] * d[i] * d[i];
      for (int i = 0; i < 3; ++i) S.trial[i] = p[i] + d[i];
    }
    __syncthreads();
    const double t[3] = {S.trial[0], S.trial[1], S.trial[2]};
    double tr[10];
    rf_eval<false, DISP>(a, h, t, tr, S.red);
    if (threadIdx.x == 0) {
      const double new_cost = tr[9];
      const double actual = cost - new_cost;
      const bool num_ok = ok && isfinite(new_cost) && pred > 0;
      const double rho = num_ok ? actual / pred : -1.0;
      int stop = 0, acc = 0;
      if (rho > 0) {
        acc = 1;
        lam = fmax(1e-12, lam * fmax(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) * (2.0 * rho - 1.0) * (2.0 * rho - 1.0)));
        nu = 2.0;
        const double dx2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        const double x2 = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
        if (actual < a.ftol * cost && rho > 0.25) { stop = 1; status = 2; }       // scipy ftol
        else if (sqrt(dx2) < a.xtol * (a.xtol + sqrt(x2))) { stop = 1; status = 3; }  // scipy xtol
        cost = new_cost;
      } else {
        lam = lam > 0 ? lam * nu : 1e-9;
        nu *= 2.0;
        if (lam > 1e16) { stop = 1; status = -1; }
      }
      S.ctl[0] = stop;
      S.ctl[1] = acc;
    }
    __syncthreads();
    const int stop = S.ctl[0], acc = S.ctl[1];
    if (acc) {
      ++it;
      p[0] = t[0]; p[1] = t[1]; p[2] = t[2];
      if (!stop) rf_eval<true, DISP>(a, h, p, lin, S.red);
    }
    __syncthreads();
    if (stop) break;
  }
}

}  // namespace ptzba
