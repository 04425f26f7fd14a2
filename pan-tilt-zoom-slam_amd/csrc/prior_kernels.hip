// Gaussian pose priors of the bundle adjuster (include/ptzba.h ptzba_set_pose_priors).
//
//   cost = 1/2 sum rho(r^2) + 1/2 sum_k e_k^T Lambda_k e_k,   e_k = x_{F_k} - mean_k
//
// The prior touches the pose rows only, so the reduced camera system becomes S = U + P - sum W V^-1 W^T with the
// constant P = sum_k Lambda_k, and the pose gradient gains P e.  k_prior_apply runs after k_schur_reduce has written
// S, b, g_pose and dU of a build and adds the prior's terms in place; k_prior_cost gives the prior's share of the
// cost at the current or the trial state.  Both form e in fp64 from the state itself (never from the fp32 tables).
// Every written element has one owning thread and the sums run in a fixed order: results are bitwise repeatable.
// The Gaussian ray priors (ptzba_set_ray_priors) are at the end of the file.
#include <algorithm>

#include "ptzba_common.h"
#include "ptzba_kernels.h"

namespace ptzba {

__device__ __forceinline__ const double* prior_state(const PriorArgs& a) {
  return (a.sel && (((*a.sel) ^ a.sel_xor) & 1)) ? a.x1 : a.x0;
}

// (Lambda_k e_k)[row] for local row `row` of factor k, terms in column order
__device__ __forceinline__ double prior_row_dot(const PriorArgs& a, const double* __restrict__ x, int k, int row) {
  const int f0 = a.f_begin[k], n3 = 3 * (a.f_begin[k + 1] - f0);
  const double* __restrict__ L = a.f_info + a.f_info_off[k] + (int64_t)row * n3;
  const double* __restrict__ mu = a.f_mean + 3 * (int64_t)f0;
  double acc = 0.0;
  for (int j = 0; j < n3; ++j) {
    const int fr = a.f_frames[f0 + j / 3];
    acc += L[j] * (x[3 * (int64_t)fr + j % 3] - mu[j]);
  }
  return acc;
}

// threads [0, n_elem): one element of P each, S[s_off] += s_val (the host merged every factor's contribution to an
// element, so offsets are distinct); threads [n_elem, n_elem + 3 n_pframe): one pose row each -- g_pose, b, dU
__global__ __launch_bounds__(256) void k_prior_apply(PriorArgs a, double* __restrict__ S, double* __restrict__ b,
                                                     double* __restrict__ g_pose, double* __restrict__ dU,
                                                     const int32_t* __restrict__ frame_pos,
                                                     const int* __restrict__ skip_if) {
  if (skip_if && *skip_if) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < a.n_elem) {
    S[a.s_off[t]] += a.s_val[t];
    return;
  }
  const int j = t - a.n_elem;
  if (j >= 3 * a.n_pframe) return;
  const int pf = j / 3, q = j - 3 * pf;
  const double* __restrict__ x = prior_state(a);
  double acc = 0.0;
  for (int e = a.p_begin[pf]; e < a.p_begin[pf + 1]; ++e) {
    const int2 fs = a.p_ent[e];  // (factor, slot of the frame in it)
    acc += prior_row_dot(a, x, fs.x, 3 * fs.y + q);
  }
  const int row = frame_pos[a.p_frame[pf]] + q;
  g_pose[row] += acc;
  b[row] -= acc;
  dU[row] += a.p_diag[j];
}

// Row r's share e_r (Lambda e)_r, one thread per prior row (a row's loads form a dependent chain: a single workgroup
// walking ~4,500 rows at config 3's 997 factors took ~75 us); each workgroup sums its rows in a fixed order and stores a
// partial, and the last workgroup to finish adds the partials in workgroup order -- k_reduce_cols' hand-off
// (ba_kernels.hip): write-through partial stores waited for by the storing wave, one relaxed agent-scope counter add
// per workgroup, an agent-scope acquire before the last workgroup's loads, the counter re-armed for the next launch.
// The grid depends on n_row only, so the sum's order -- and the result, bit for bit -- is the same on every launch.
__global__ __launch_bounds__(256) void k_prior_cost(PriorArgs a, double* __restrict__ out, double mul, int accumulate,
                                                    double* __restrict__ partial, unsigned* __restrict__ counter) {
  __shared__ double red[256 / WAVE];
  __shared__ bool last;
  const double* __restrict__ x = prior_state(a);
  double acc = 0.0;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < a.n_row; r += gridDim.x * blockDim.x) {
    const int k = a.row_factor[r];
    const int f0 = a.f_begin[k], row = r - 3 * f0;
    const int fr = a.f_frames[f0 + row / 3];
    const double e = x[3 * (int64_t)fr + row % 3] - a.f_mean[r];
    acc += e * prior_row_dot(a, x, k, row);
  }
  acc = wave_sum(acc);
  if (lane_id() == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x < WAVE) {
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int w = 0; w < 256 / WAVE; ++w) s += red[w];
      __hip_atomic_store(partial + blockIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (threadIdx.x == 0) {
      const unsigned done = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = (done == gridDim.x - 1);
    }
  }
  __syncthreads();
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int b = 0; b < (int)gridDim.x; ++b)
      s += __hip_atomic_load(partial + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double c = mul * (0.5 * s);
    out[0] = accumulate ? out[0] + c : c;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ------------------------------------------------------------------------------------------------
// Gaussian ray priors (include/ptzba.h ptzba_set_ray_priors).  A prior on a ray is block-diagonal in
// the landmark part: V_l += sum Lambda_k, g_l += sum Lambda_k e_k, the landmark's cost share += 1/2 sum e^T Lambda e,
// and nothing else changes -- every later kernel reads V_l, g_l and the cost from the landmark's lm_out row.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ const double* ray_prior_state(const RayPriorArgs& a) {
  return (a.sel && (((*a.sel) ^ a.sel_xor) & 1)) ? a.x1 : a.x0;
}

// One thread per distinct prior landmark: the sums of its priors in list order, added to the row K1 wrote for the
// landmark (the launch follows K1 on the stream).  A row has one owning thread: plain loads and stores, no atomics.
__global__ __launch_bounds__(256) void k_ray_prior_apply(RayPriorArgs a, double* __restrict__ lm_out,
                                                         double* __restrict__ lm_out1,
                                                         const int* __restrict__ slot_sel, int slot_xor,
                                                         const int* __restrict__ run_if) {
  if (run_if && !*run_if) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.n_lm) return;
  const bool alt = slot_sel && ((*slot_sel ^ slot_xor) & 1);
  const double* __restrict__ x = ray_prior_state(a);
  const int l = a.lm[t];
  const double th = x[2 * (int64_t)l], ph = x[2 * (int64_t)l + 1];
  double v00 = 0.0, v01 = 0.0, v11 = 0.0, g0 = 0.0, g1 = 0.0, c = 0.0;
  for (int k = a.begin[t]; k < a.begin[t + 1]; ++k) {
    const double l00 = a.info[3 * (int64_t)k], l01 = a.info[3 * (int64_t)k + 1], l11 = a.info[3 * (int64_t)k + 2];
    const double e0 = th - a.mean[2 * (int64_t)k], e1 = ph - a.mean[2 * (int64_t)k + 1];
    const double r0 = l00 * e0 + l01 * e1, r1 = l01 * e0 + l11 * e1;
    v00 += l00; v01 += l01; v11 += l11;
    g0 += r0; g1 += r1;
    c += e0 * r0 + e1 * r1;
  }
  double* o = (alt ? lm_out1 : lm_out) + (int64_t)l * 8;
  o[0] += v00; o[1] += v01; o[2] += v11; o[3] += g0; o[4] += g1; o[5] += 0.5 * c;
}

// 1/2 sum e^T Lambda e: thread t sums the landmarks t, t + 256, ... (each landmark's priors in list order), the waves
// and then the workgroup add in a fixed order; the grid is one workgroup, so the result is the same on every launch
__global__ __launch_bounds__(256) void k_ray_prior_cost(RayPriorArgs a, double* __restrict__ out, double mul,
                                                        int accumulate) {
  __shared__ double red[256 / WAVE];
  const double* __restrict__ x = ray_prior_state(a);
  double acc = 0.0;
  for (int t = threadIdx.x; t < a.n_lm; t += blockDim.x) {
    const int l = a.lm[t];
    const double th = x[2 * (int64_t)l], ph = x[2 * (int64_t)l + 1];
    double c = 0.0;
    for (int k = a.begin[t]; k < a.begin[t + 1]; ++k) {
      const double l00 = a.info[3 * (int64_t)k], l01 = a.info[3 * (int64_t)k + 1], l11 = a.info[3 * (int64_t)k + 2];
      const double e0 = th - a.mean[2 * (int64_t)k], e1 = ph - a.mean[2 * (int64_t)k + 1];
      c += e0 * (l00 * e0 + l01 * e1) + e1 * (l01 * e0 + l11 * e1);
    }
    acc += c;
  }
  acc = wave_sum(acc);
  if (lane_id() == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < 256 / WAVE; ++w) s += red[w];
    const double c = mul * (0.5 * s);
    out[0] = accumulate ? out[0] + c : c;
  }
}

void launch_ray_prior_apply(const RayPriorArgs& a, double* lm_out, double* lm_out1, const int* slot_sel, int slot_xor,
                            const int* run_if, hipStream_t st) {
  if (a.n_lm <= 0) return;
  hipLaunchKernelGGL(k_ray_prior_apply, dim3((unsigned)((a.n_lm + 255) / 256)), dim3(256), 0, st, a, lm_out, lm_out1,
                     slot_sel, slot_xor, run_if);
}

void launch_ray_prior_cost(const RayPriorArgs& a, double* out, double mul, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(k_ray_prior_cost, dim3(1), dim3(256), 0, st, a, out, mul, accumulate);
}

void launch_prior_apply(const PriorArgs& a, double* S, double* b, double* g_pose, double* dU, const int32_t* frame_pos,
                        const int* skip_if, hipStream_t st) {
  const int n = a.n_elem + 3 * a.n_pframe;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_prior_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, S, b, g_pose, dU, frame_pos,
                     skip_if);
}

void launch_prior_cost(const PriorArgs& a, double* out, double mul, int accumulate, double* scratch, hipStream_t st) {
  unsigned* counter = reinterpret_cast<unsigned*>(scratch + PRIOR_RED_BLOCKS);
  const int nb = std::min(PRIOR_RED_BLOCKS, std::max(1, (a.n_row + 255) / 256));
  hipLaunchKernelGGL(k_prior_cost, dim3((unsigned)nb), dim3(256), 0, st, a, out, mul, accumulate, scratch, counter);
}

}  // namespace ptzba
