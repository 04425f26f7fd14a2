// Marginalisation of keyframes that leave a sliding window (include/ptzba.h ptzba_marginal_prior /
// ptzba_set_marginal_prior).
//
//   k_marg_weights    the record mask, scattered through the sort permutation into a weight array K1's weighted
//                     instantiation reads: the solver's own K1 / prologue / K2 then linearise and reduce the dropped
//                     records alone (S_D, b_D in the system order)
//   k_marg_eliminate  one workgroup, fp64: gathers the (K | E) rows and columns of S_D and b_D, adds the absorbed
//                     factors, Cholesky-factors A_EE in LDS and writes Lambda = A_KK - A_KE A_EE^-1 A_EK,
//                     eta = a_K - A_KE A_EE^-1 a_E, lin = x_K, the offset and the smallest pivot
//   k_marg_apply / k_marg_cost   the handle's dense information-form factor q(x) = offset + eta^T d + 1/2 d^T Lambda d
//                     in a build and in a cost, as k_prior_apply / k_prior_cost treat the pose priors
//
// Every written element has one owning thread (or one owner per sequential phase) and every sum a fixed order:
// results are bitwise repeatable.
#include "ptzba_common.h"
#include "ptzba_kernels.h"

namespace ptzba {

template <typename real>
__global__ __launch_bounds__(256) void k_marg_weights(const uint8_t* __restrict__ mask, const int64_t* __restrict__ perm,
                                                      const real* __restrict__ rec_w, const int32_t* __restrict__ rec_seg,
                                                      const int32_t* __restrict__ seg_frame,
                                                      const int32_t* __restrict__ seg_lm, int64_t n_rec,
                                                      real* __restrict__ w_out, int32_t* __restrict__ frame_flag,
                                                      int32_t* __restrict__ lm_flag, unsigned long long* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool m = false;
  int new_lm = 0;
  if (i < n_rec) {
    m = mask[perm[i]] != 0;
    w_out[i] = m ? (rec_w ? rec_w[i] : (real)1) : (real)0;
    if (m) {
      const int s = rec_seg[i];
      frame_flag[seg_frame[s]] = 1;  // (every writer stores the same value)
      new_lm = atomicExch(lm_flag + seg_lm[s], 1) == 0;
    }
  }
  // integer counters: the totals do not depend on the order of the adds
  const unsigned long long bm = __ballot(m), bl = __ballot(new_lm != 0);
  if (lane_id() == 0) {
    if (bm) atomicAdd(cnt, (unsigned long long)__popcll(bm));
    if (bl) atomicAdd(cnt + 1, (unsigned long long)__popcll(bl));
  }
}

template <typename real>
void launch_marg_weights(const uint8_t* mask, const int64_t* perm, const void* rec_w, const int32_t* rec_seg,
                         const int32_t* seg_frame, const int32_t* seg_lm, int64_t n_rec, void* w_out,
                         int32_t* frame_flag, int32_t* lm_flag, unsigned long long* cnt, hipStream_t st) {
  if (n_rec <= 0) return;
  hipLaunchKernelGGL(k_marg_weights<real>, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, mask, perm,
                     (const real*)rec_w, rec_seg, seg_frame, seg_lm, n_rec, (real*)w_out, frame_flag, lm_flag, cnt);
}
template void launch_marg_weights<float>(const uint8_t*, const int64_t*, const void*, const int32_t*, const int32_t*,
                                         const int32_t*, int64_t, void*, int32_t*, int32_t*, unsigned long long*,
                                         hipStream_t);
template void launch_marg_weights<double>(const uint8_t*, const int64_t*, const void*, const int32_t*, const int32_t*,
                                          const int32_t*, int64_t, void*, int32_t*, int32_t*, unsigned long long*,
                                          hipStream_t);

// ------------------------------------------------------------------------------------------------
// the elimination
// ------------------------------------------------------------------------------------------------
constexpr int MK3 = 3 * MARG_MAX_K, ME3 = 3 * MARG_MAX_E;
constexpr int PSTR = ME3 + 1;  // LDS row stride of the panel and of A_EE (odd: rows on different banks)

// element (i, j) of the built system in (K | E) numbering, or 0 outside the factor pattern (stale data there)
__device__ __forceinline__ double marg_gather(const EliminateArgs& a, const int* rows, int i, int j) {
  const int ti = a.row_tile[i], tj = a.row_tile[j];
  const int64_t ri = rows[i], rj = rows[j];
  const int64_t hi = ri > rj ? ri : rj, lo = ri > rj ? rj : ri;
  const int th = ri > rj ? ti : tj, tl = ri > rj ? tj : ti;
  if (!a.pat[th * a.n_tile + tl]) return 0.0;
  return a.S[hi * a.ld + lo];
}

__global__ __launch_bounds__(256) void k_marg_eliminate(EliminateArgs a) {
  __shared__ double P[MK3 * PSTR];  // A_KE, then Y = A_KE L^-T
  __shared__ double EE[ME3 * PSTR];  // A_EE, then its Cholesky factor L (lower)
  __shared__ double av[MK3 + ME3];   // a_K | a_E, then z = L^-1 a_E in the E part
  __shared__ double cst[MK3];        // per-row cost shares of the factor being absorbed
  __shared__ int rows[MK3 + ME3];
  __shared__ double s_cost, s_minp, s_maxd;
  __shared__ int s_fail;
  const int t = threadIdx.x, nt = blockDim.x;
  const int nK3 = 3 * a.nK, nE3 = 3 * a.nE, N = nK3 + nE3;
  double* __restrict__ Lam = a.out;
  double* __restrict__ eta = a.out + (int64_t)nK3 * nK3;
  double* __restrict__ lin = eta + nK3;
  double* __restrict__ tail = lin + nK3;

  for (int i = t; i < N; i += nt) rows[i] = a.frame_pos[a.frames[i / 3]] + i % 3;
  if (t == 0) {
    s_cost = a.dcost[0];
    s_minp = 0.0;
    s_maxd = 0.0;
    s_fail = 0;
  }
  __syncthreads();
  // gather: A_KK to the output (both triangles), A_KE and A_EE to LDS, a = -b
  for (int e = t; e < nK3 * nK3; e += nt) {
    const int i = e / nK3, j = e - i * nK3;
    Lam[e] = marg_gather(a, rows, i, j);
  }
  for (int e = t; e < nK3 * nE3; e += nt) {
    const int i = e / nE3, j = e - i * nE3;
    P[i * PSTR + j] = marg_gather(a, rows, i, nK3 + j);
  }
  for (int e = t; e < nE3 * nE3; e += nt) {
    const int i = e / nE3, j = e - i * nE3;
    EE[i * PSTR + j] = marg_gather(a, rows, nK3 + i, nK3 + j);
  }
  for (int i = t; i < N; i += nt) av[i] = -a.b[rows[i]];
  for (int i = t; i < nK3; i += nt) lin[i] = a.x[3 * (int64_t)a.frames[i / 3] + i % 3];
  __syncthreads();
  // absorbed factors, one after the other: within a factor every element has its own target
  for (int k = 0; k < a.n_factor; ++k) {
    const MargFactor f = a.factors[k];
    const int32_t* __restrict__ ffr = a.fac_frames + f.loc_off;
    const int32_t* __restrict__ floc = a.fac_loc + f.loc_off;
    for (int e = t; e < f.n3 * f.n3; e += nt) {
      const int r = e / f.n3, c = e - r * f.n3;
      const int i = 3 * floc[r / 3] + r % 3, j = 3 * floc[c / 3] + c % 3;
      const double v = f.L[e];
      if (i < nK3) {
        if (j < nK3) Lam[i * nK3 + j] += v;
        else P[i * PSTR + j - nK3] += v;
      } else if (j >= nK3) {
        EE[(i - nK3) * PSTR + j - nK3] += v;
      }
    }
    for (int r = t; r < f.n3; r += nt) {
      double acc = 0.0;
      for (int c = 0; c < f.n3; ++c)
        acc += f.L[r * f.n3 + c] * (a.x[3 * (int64_t)ffr[c / 3] + c % 3] - f.mean[c]);
      const double er = a.x[3 * (int64_t)ffr[r / 3] + r % 3] - f.mean[r];
      const double et = f.eta ? f.eta[r] : 0.0;
      av[3 * floc[r / 3] + r % 3] += acc + et;
      cst[r] = er * (et + 0.5 * acc);
    }
    __syncthreads();
    if (t == 0) {
      double s = f.offset;
      for (int r = 0; r < f.n3; ++r) s += cst[r];
      s_cost += s;
    }
    __syncthreads();
  }
  // Cholesky of A_EE (right-looking, in place; <= 24 columns)
  if (t == 0) {
    double md = 0.0;
    for (int i = 0; i < nE3; ++i) md = fmax(md, EE[i * PSTR + i]);
    s_maxd = md;
    s_minp = nE3 ? 1e300 : 0.0;
  }
  __syncthreads();
  for (int c = 0; c < nE3; ++c) {
    if (t == 0) {
      const double piv = EE[c * PSTR + c];
      if (!(piv > a.pivot_tol * s_maxd) && !s_fail) s_fail = 1 + c;
      if (piv < s_minp || !(piv == piv)) s_minp = piv;
      EE[c * PSTR + c] = sqrt(piv);
    }
    __syncthreads();
    if (s_fail) break;
    const double d = EE[c * PSTR + c];
    for (int i = c + 1 + t; i < nE3; i += nt) EE[i * PSTR + c] /= d;
    __syncthreads();
    const int m = nE3 - c - 1;
    for (int e = t; e < m * m; e += nt) {
      const int i = c + 1 + e / m, j = c + 1 + e % m;
      if (j <= i) EE[i * PSTR + j] -= EE[i * PSTR + c] * EE[j * PSTR + c];
    }
    __syncthreads();
  }
  if (t == 0) {
    tail[0] = s_cost;
    tail[1] = s_minp;
    tail[2] = (double)s_fail;
    tail[3] = s_maxd;
  }
  if (s_fail) return;
  // Y = A_KE L^-T: row i solves L y = A_KE[i, :]^T; z = L^-1 a_E (one more row)
  for (int i = t; i <= nK3; i += nt) {
    double* __restrict__ y = i < nK3 ? P + i * PSTR : av + nK3;
    for (int c = 0; c < nE3; ++c) {
      double s = y[c];
      for (int q = 0; q < c; ++q) s -= EE[c * PSTR + q] * y[q];
      y[c] = s / EE[c * PSTR + c];
    }
  }
  __syncthreads();
  for (int e = t; e < nK3 * nK3; e += nt) {
    const int i = e / nK3, j = e - i * nK3;
    double s = 0.0;
    for (int c = 0; c < nE3; ++c) s += P[i * PSTR + c] * P[j * PSTR + c];
    Lam[e] -= s;
  }
  for (int i = t; i < nK3; i += nt) {
    double s = 0.0;
    for (int c = 0; c < nE3; ++c) s += P[i * PSTR + c] * av[nK3 + c];
    eta[i] = av[i] - s;
  }
}

void launch_marg_eliminate(const EliminateArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_marg_eliminate, dim3(1), dim3(256), 0, st, a);
}

// ------------------------------------------------------------------------------------------------
// the handle's dense factor in a build and in a cost
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ const double* marg_state(const MargArgs& a) {
  return (a.sel && (((*a.sel) ^ a.sel_xor) & 1)) ? a.x1 : a.x0;
}

// (Lambda d)[i], terms in column order
__device__ __forceinline__ double marg_row_dot(const MargArgs& a, const double* __restrict__ x, int i) {
  const int n3 = 3 * a.n;
  const double* __restrict__ L = a.info + (int64_t)i * n3;
  double acc = 0.0;
  for (int j = 0; j < n3; ++j) acc += L[j] * (x[3 * (int64_t)a.frames[j / 3] + j % 3] - a.lin[j]);
  return acc;
}

// threads [0, (3n)^2): element (i, j) of Lambda, written where k_schur_reduce puts the pair's block (row of the frame
// later in the system order, see ptzba_set_pose_priors): the pairs with pos[frame i] < pos[frame j] and the full
// diagonal blocks, each target once; threads [(3n)^2, (3n)^2 + 3n): one pose row each
__global__ __launch_bounds__(256) void k_marg_apply(MargArgs a, double* __restrict__ S, int64_t ld, double* __restrict__ b,
                                                    double* __restrict__ g_pose, double* __restrict__ dU,
                                                    const int32_t* __restrict__ frame_pos,
                                                    const int* __restrict__ skip_if) {
  if (skip_if && *skip_if) return;
  const int n3 = 3 * a.n;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n3 * n3) {
    const int i = t / n3, j = t - i * n3;
    const int64_t pa = frame_pos[a.frames[i / 3]], pb = frame_pos[a.frames[j / 3]];
    if (pa < pb || i / 3 == j / 3) S[(pb + j % 3) * ld + pa + i % 3] += a.info[t];
    return;
  }
  const int i = t - n3 * n3;
  if (i >= n3) return;
  const double acc = marg_row_dot(a, marg_state(a), i) + a.eta[i];
  const int row = frame_pos[a.frames[i / 3]] + i % 3;
  g_pose[row] += acc;
  b[row] -= acc;
  dU[row] += a.info[(int64_t)i * n3 + i];
}

__global__ __launch_bounds__(256) void k_marg_cost(MargArgs a, double* __restrict__ out, int accumulate) {
  __shared__ double part[MK3];
  const int n3 = 3 * a.n;
  const double* __restrict__ x = marg_state(a);
  for (int i = threadIdx.x; i < n3; i += blockDim.x) {
    const double d = x[3 * (int64_t)a.frames[i / 3] + i % 3] - a.lin[i];
    part[i] = d * (a.eta[i] + 0.5 * marg_row_dot(a, x, i));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < n3; ++i) s += part[i];
    const double c = a.offset + s;
    out[0] = accumulate ? out[0] + c : c;
  }
}

void launch_marg_apply(const MargArgs& a, double* S, int64_t ld, double* b, double* g_pose, double* dU,
                       const int32_t* frame_pos, const int* skip_if, hipStream_t st) {
  const int n3 = 3 * a.n, n = n3 * n3 + n3;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_marg_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, S, ld, b, g_pose, dU,
                     frame_pos, skip_if);
}

void launch_marg_cost(const MargArgs& a, double* out, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(k_marg_cost, dim3(1), dim3(256), 0, st, a, out, accumulate);
}

}  // namespace ptzba
