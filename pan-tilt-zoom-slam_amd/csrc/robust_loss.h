// The smooth robust losses of scipy least_squares (soft_l1, cauchy, arctan) per scalar residual, one definition for
// K1 (ba_kernels.hip), the pose LM (pose_lm.h) and the covariance's residual scale (cov_kernels.hip).
//
//   z = (r / f_scale)^2        rho(z)                rho'(z)          Newton curvature rho' + 2 z rho''
//   soft_l1                    2 (sqrt(1+z) - 1)     (1+z)^-1/2       (1+z)^-3/2
//   cauchy                     ln(1+z)               1 / (1+z)        (1 - z) / (1+z)^2
//   arctan                     atan z                1 / (1+z^2)      (1 - 3 z^2) / (1+z^2)^2
//
// cost term = f_scale^2 rho (halved by the caller), gradient weight w1 = rho', curvature weight
// w2 = max(rho' + 2 z rho'', hc rho') (robust_curv): rho'' <= 0 for all three, so hc = 1 is IRLS, and for huber the
// same rule gives K1's 1 | hc rho' (the Newton curvature is 1 inside the unit and 0 beyond it).
//
// Each cost term is accurate relative to itself for z << 1 (the trial cost decides the LM's acceptance):
// 2 z / (sqrt(1+z) + 1) instead of 2 (sqrt(1+z) - 1), a log1p-accurate form instead of log(1 + z).  fp32 takes the
// fast reciprocal / reciprocal square root where the huber fp32 path does; fp64 divides.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ptzba.h"

namespace ptzba {

__host__ __device__ constexpr bool loss_is_smooth(int loss) {
  return loss == PTZBA_LOSS_SOFT_L1 || loss == PTZBA_LOSS_CAUCHY || loss == PTZBA_LOSS_ARCTAN;
}
__host__ __device__ constexpr bool loss_is_known(int loss) {
  return loss >= PTZBA_LOSS_LINEAR && loss <= PTZBA_LOSS_ARCTAN;
}

__device__ __forceinline__ float rl_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ double rl_rcp(double x) { return 1.0 / x; }
// fp32 log1p for x >= 0 by the hardware log2 (1 ulp, relative, also next to 1): with w = fl(1 + x), log(w) x / (w - 1)
// corrects the rounding of 1 + x (Kahan's form; w - 1 is exact), so the value is accurate relative to itself for
// x << 1; w == 1: log1p(x) = x to float precision.  The library log1pf measures 1.97 x Huber's K1 time.
__device__ __forceinline__ float rl_log1p(float x) {
  const float w = 1.0f + x, d = w - 1.0f;
  const float l = __builtin_amdgcn_logf(w) * 0.693147180559945309f;
  return d == 0.0f ? x : l * x * __builtin_amdgcn_rcpf(d);
}
__device__ __forceinline__ double rl_log1p(double x) { return log1p(x); }
__device__ __forceinline__ float rl_atan(float x) { return atanf(x); }
__device__ __forceinline__ double rl_atan(double x) { return atan(x); }

// rho(z), w1 = rho'(z) and wn = rho'(z) + 2 z rho''(z) of a smooth loss (LOSS: PTZBA_LOSS_SOFT_L1 | CAUCHY | ARCTAN)
template <int LOSS, typename T>
__device__ __forceinline__ void robust_eval(T z, T& rho, T& w1, T& wn) {
  static_assert(loss_is_smooth(LOSS), "a smooth loss");
  if constexpr (LOSS == PTZBA_LOSS_SOFT_L1) {
    const T t = (T)1 + z;
    T s;
    if constexpr (sizeof(T) == 4) {
      w1 = __builtin_amdgcn_rsqf(t);
      s = t * w1;
    } else {
      s = sqrt(t);
      w1 = (T)1 / s;
    }
    rho = (T)2 * z * rl_rcp(s + (T)1);
    wn = w1 * w1 * w1;
  } else if constexpr (LOSS == PTZBA_LOSS_CAUCHY) {
    w1 = rl_rcp((T)1 + z);
    rho = rl_log1p(z);
    wn = ((T)1 - z) * w1 * w1;
  } else {
    const T z2 = z * z;
    w1 = rl_rcp((T)1 + z2);
    rho = rl_atan(z);
    wn = ((T)1 - (T)3 * z2) * w1 * w1;
  }
}

// the curvature weight: the loss's Newton curvature, floored at hc rho'
template <typename T>
__device__ __forceinline__ T robust_curv(T w1, T wn, T hc) {
  return fmax(wn, hc * w1);
}

// the same with the loss id at run time (wave-uniform in every caller): fp64 callers off the hot path
__device__ __forceinline__ void robust_eval_id(int loss, double z, double& rho, double& w1, double& wn) {
  if (loss == PTZBA_LOSS_SOFT_L1) robust_eval<PTZBA_LOSS_SOFT_L1, double>(z, rho, w1, wn);
  else if (loss == PTZBA_LOSS_CAUCHY) robust_eval<PTZBA_LOSS_CAUCHY, double>(z, rho, w1, wn);
  else robust_eval<PTZBA_LOSS_ARCTAN, double>(z, rho, w1, wn);
}

}  // namespace ptzba
