// Posterior covariance blocks of a bundle adjustment (gfx950): diagonal blocks of scale * H^-1 by a selected
// inverse through the tile-Cholesky factor of the reduced camera system (chol_kernels.hip).
//
// With H = [U W; W^T V] over [poses | rays] and S = U - sum_l W_l V_l^-1 W_l^T = L L^T:
//   pose block of frame f   = the 3 x 3 diagonal block of S^-1 at frame_pos[f]
//   ray block of landmark l = V_l^-1 + Y_l^T S^-1 Y_l,  Y_l = W_l V_l^-1 scattered to the rows of the frames seeing l
// Both are Gram matrices of a forward substitution: for a 32-column right-hand side B, L Z = B, then
// (B^T S^-1 B) = Z^T Z.  k_cov_gram runs one 32-column block per workgroup (pose blocks: 10 frames x 3 unit
// columns; ray blocks: 16 landmarks x 2 columns of Y, built on the fly from the W slot table) and walks the row
// tiles of L in system order from the block's first non-zero tile:
//   Z_i = M_i (B_i - sum_{k < i, (i, k) in the factor's pattern} L_ik Z_k),   G += Z_i^T Z_i
// with every 32 x 32 product on the fp64 matrix cores (v_mfma_f64_16x16x4_f64, operand maps as chol_kernels.hip).
// The Z tiles of a block live in a global workspace [workgroup][tile][32][32] (a column block of config 3 is 400 KB:
// it does not fit LDS; the workspace stays in L2 / Infinity Cache).  G accumulates tile by tile in system order, so the
// result is deterministic (no atomics).  M_i = L_ii^-1 comes from k_cov_tile_inv (a buffer of the covariance path:
// the solver's own Minv is complete only after a back substitution), with the rows and columns of the augmented
// right-hand-side row, of the rows after it and of padding rows zeroed: Z is exactly zero there, and the rows of the
// off-diagonal tiles at or after the augmented row are never loaded.  Tiles outside the factor's pattern (stale
// memory) are never visited: the walk follows a row CSR of the pattern built by the host.
#include "ptzba_common.h"
#include "ptzba_kernels.h"
#include "robust_loss.h"

namespace ptzba {

namespace {
constexpr int NB = CHOL_NB;
typedef double v4f64 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double cov_rcp(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(r, fma(-d, r, 1.0), r);
  return fma(r, fma(-d, r, 1.0), r);
}

// wave w's 16 x 16 block of C (+)= A B for 32 x 32 operands in LDS.  AT: the left operand is A^T (a(i, k) = A[k][i]).
// MFMA lane maps (gfx950): a(i = l & 15, k = l >> 4), b(k = l >> 4, j = l & 15), D[row = (l >> 4) + 4 r][col = l & 15]
template <bool AT, bool NEG>
__device__ __forceinline__ void cov_mma(v4f64& acc, const double (*A)[NB + 1], const double (*B)[NB + 1]) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int bi = (w >> 1) * 16, bj = (w & 1) * 16;
  const int li = l & 15, lk = l >> 4;
#pragma unroll
  for (int s = 0; s < NB / 4; ++s) {
    double a = AT ? A[4 * s + lk][bi + li] : A[bi + li][4 * s + lk];
    if (NEG) a = -a;
    const double b = B[4 * s + lk][bj + li];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
}
__device__ __forceinline__ void cov_acc_put(double (*C)[NB + 1], const v4f64& acc) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < 4; ++r) C[(w >> 1) * 16 + (l >> 4) + 4 * r][(w & 1) * 16 + (l & 15)] = acc[r];
}
}  // namespace

// M_t = L_tt^-1 (lower, row-major) of the diagonal factor tiles t < n_tiles, masked as described above, and the
// smallest pivot of the tile's system rows (NaN if one is not a number).  One wave per tile: lane j computes column
// j by forward substitution against e_j (as chol_kernels.hip k_tile_inv).
__global__ __launch_bounds__(64) void k_cov_tile_inv(const double* __restrict__ Ldiag, const uint8_t* __restrict__ pad,
                                                     int n_aug, double* __restrict__ Minv,
                                                     double* __restrict__ min_piv) {
  __shared__ double Lt[NB][NB + 1];
  __shared__ double rinv[NB];
  __shared__ int live[NB];
  const int t = blockIdx.x, lane = threadIdx.x, j = lane & (NB - 1);
  const double* src = Ldiag + (int64_t)t * NB * NB;
  for (int e = lane; e < NB * NB; e += WAVE) Lt[e >> 5][e & 31] = src[e];
  if (lane < NB) {
    const int row = t * NB + lane;
    live[lane] = (row < n_aug && !pad[row]) ? 1 : 0;
  }
  __syncthreads();
  if (lane < NB) rinv[lane] = live[lane] ? cov_rcp(Lt[lane][lane]) : 0.0;
  __syncthreads();
  if (lane == 0) {
    double m = 1e300;
    for (int r = 0; r < NB; ++r) {
      if (!live[r]) continue;
      const double d = Lt[r][r];
      if (!(d == d) || !(m == m)) m = __longlong_as_double(0x7ff8000000000000LL);
      else if (d < m) m = d;
    }
    min_piv[t] = m;
  }
  double acc[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) acc[i] = (i == j) ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    const double mk = (k >= j) ? acc[k] * rinv[k] : 0.0;  // (0 above the diagonal and on masked rows)
    acc[k] = mk;
#pragma unroll
    for (int i = k + 1; i < NB; ++i) acc[i] = fma(-Lt[i][k], mk, acc[i]);
  }
  if (lane < NB) {
    double* dst = Minv + (int64_t)t * NB * NB + lane;
    const bool col_live = live[lane] != 0;
#pragma unroll
    for (int i = 0; i < NB; ++i) dst[i * NB] = (col_live && live[i]) ? acc[i] : 0.0;
  }
}

// JOINT (ptzba_covariance_joint's stage 1): one workgroup per block, so the workspace slice belongs to the block; every
// Z_i stays, the block's first tile goes to a.block_t0 and no Gram matrix is formed (k_cov_cross forms them all)
template <typename real, bool JOINT>
__global__ __launch_bounds__(256) void k_cov_gram(CovArgs a) {
  __shared__ __attribute__((aligned(16))) double sA[NB][NB + 1];  // L_ik, then M_i, then G
  __shared__ __attribute__((aligned(16))) double sB[NB][NB + 1];  // Z_k, then the right-hand side, then Z_i
  __shared__ int s_row[NB];        // pose blocks: the system row of each unit column (-1: none)
  __shared__ int s_lm[NB / 2];     // ray blocks: the landmark of each column pair (-1: none)
  __shared__ int4 s_meta[NB / 2];  // ... its {first frame, last frame, slot offset, -}
  __shared__ double s_vinv[NB / 2][3];
  __shared__ int s_t0;
  const int tid = threadIdx.x;
  const real* __restrict__ w_slot = (const real*)a.w_slot;
  double* __restrict__ Zw = a.work + (int64_t)blockIdx.x * a.n_tiles * NB * NB;
  const double scale = a.scale_dev ? a.scale_dev[0] / a.scale_div : a.scale;
  for (int blk = blockIdx.x; blk < a.n_pose_blocks + a.n_ray_blocks; blk += gridDim.x) {
    const bool ray = blk >= a.n_pose_blocks;
    const int rb = blk - a.n_pose_blocks;
    __syncthreads();  // the previous block's epilogue has read sA and the descriptors
    // ---- the block's columns
    if (tid == 0) s_t0 = ray ? a.n_tiles : a.pose_t0[blk];
    if (!ray) {
      if (tid < NB) s_row[tid] = a.pose_rows[(int64_t)blk * NB + tid];
    } else if (tid < NB / 2) {
      const int64_t q = (int64_t)rb * (NB / 2) + tid;
      int l = q < a.n_lm_sel ? (a.lm_index ? a.lm_index[q] : (int)q) : -1;
      int4 m = make_int4(0, -1, 0, 0);
      double v0 = 0, v1 = 0, v2 = 0;
      if (l >= 0) {
        m = a.lm_meta[l];
        const double* vi = a.lm_aux + (int64_t)l * 8;
        v0 = vi[0]; v1 = vi[1]; v2 = vi[2];
        if (a.lm_seg_begin[l + 1] == a.lm_seg_begin[l]) m.y = m.x - 1;  // a landmark without records: no columns
      }
      s_lm[tid] = l;
      s_meta[tid] = m;
      s_vinv[tid][0] = v0; s_vinv[tid][1] = v1; s_vinv[tid][2] = v2;
    }
    __syncthreads();
    if (ray) {  // first non-zero tile: the smallest system row over the frames of the block's landmarks
      int tmin = a.n_tiles;
      for (int q = 0; q < NB / 2; ++q) {
        const int4 m = s_meta[q];
        for (int f = m.x + tid; f <= m.y; f += blockDim.x) {
          const int p = a.frame_pos[f];
          if (p >= 0) tmin = min(tmin, p / NB);
        }
      }
      if (tmin < a.n_tiles) atomicMin(&s_t0, tmin);
      __syncthreads();
    }
    const int t0 = s_t0;
    if (JOINT && tid == 0) a.block_t0[blk] = t0;
    v4f64 G = {0.0, 0.0, 0.0, 0.0};
    for (int i = t0; i < a.n_tiles; ++i) {
      v4f64 acc = {0.0, 0.0, 0.0, 0.0};
      // ---- acc = -sum_k L_ik Z_k over the pattern tiles of row i (k ascending, from the block's first tile)
      const int live_rows = min(NB, a.n_aug - i * NB);  // rows of this tile before the augmented row
      double2 vl[2], vz[2], vm[2];
      // a thread stages two pairs of adjacent elements of a tile (16-B loads, as chol_kernels.hip fetch_tile); the
      // next product's tiles are in flight in registers while the matrix cores work on the current one
      auto fetch = [&](int k) {
        const double* Lik = a.L + (int64_t)i * NB * a.ld + (int64_t)k * NB;
        const double* Zk = Zw + (int64_t)k * NB * NB;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int p = tid + 256 * q, r = p >> 4, c = 2 * (p & 15);
          vl[q] = r < live_rows ? *reinterpret_cast<const double2*>(Lik + (int64_t)r * a.ld + c) : make_double2(0.0, 0.0);
          vz[q] = *reinterpret_cast<const double2*>(Zk + r * NB + c);
        }
      };
      const int e1 = a.row_off[i + 1];
      int e = a.row_off[i];
      while (e < e1 && a.row_col[e] < t0) ++e;  // (Z_k = 0 before the block's first tile)
      if (e < e1) fetch(a.row_col[e]);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int p = tid + 256 * q;
        vm[q] = *reinterpret_cast<const double2*>(a.Minv + (int64_t)i * NB * NB + (p >> 4) * NB + 2 * (p & 15));
      }
      for (; e < e1; ++e) {
        __syncthreads();  // the previous product has read sA / sB
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int p = tid + 256 * q, r = p >> 4, c = 2 * (p & 15);
          sA[r][c] = vl[q].x; sA[r][c + 1] = vl[q].y;
          sB[r][c] = vz[q].x; sB[r][c + 1] = vz[q].y;
        }
        __syncthreads();
        if (e + 1 < e1) fetch(a.row_col[e + 1]);
        cov_mma<false, true>(acc, sA, sB);
      }
      // ---- + B_i, parked in sB; M_i in sA
      {
        const int w = tid >> 6, l = tid & 63;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = (w >> 1) * 16 + (l >> 4) + 4 * r, col = (w & 1) * 16 + (l & 15);
          const int srow = i * NB + row;
          double b = 0.0;
          if (!ray) {
            b = s_row[col] == srow ? 1.0 : 0.0;
          } else if (srow < a.n_aug) {
            const int f = a.row_frame[srow];
            const int4 m = s_meta[col >> 1];
            if (f >= m.x && f <= m.y) {  // (f = -1 on padding rows; slots of frames that do not see l hold 0)
              const int comp = srow - a.frame_pos[f];
              const real* ws = w_slot + ((int64_t)m.z + f - m.x) * W_STRIDE + 2 * comp;
              const double w0 = (double)ws[0], w1 = (double)ws[1];
              const double* vi = s_vinv[col >> 1];
              b = (col & 1) ? w0 * vi[1] + w1 * vi[2] : w0 * vi[0] + w1 * vi[1];
            }
          }
          acc[r] += b;
        }
      }
      __syncthreads();  // the last product has read sA / sB
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int p = tid + 256 * q, r = p >> 4, c = 2 * (p & 15);
        sA[r][c] = vm[q].x; sA[r][c + 1] = vm[q].y;
      }
      cov_acc_put(sB, acc);
      __syncthreads();
      // ---- Z_i = M_i (B_i - ...)
      v4f64 z = {0.0, 0.0, 0.0, 0.0};
      cov_mma<false, false>(z, sA, sB);
      __syncthreads();  // every wave has read the right-hand side
      cov_acc_put(sB, z);
      {
        const int w = tid >> 6, l = tid & 63;
        double* zt = Zw + (int64_t)i * NB * NB;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          zt[((w >> 1) * 16 + (l >> 4) + 4 * r) * NB + (w & 1) * 16 + (l & 15)] = z[r];
      }
      __syncthreads();  // Z_i in LDS; its global copy is visible to this workgroup's later loads
      // ---- G += Z_i^T Z_i
      if (!JOINT) cov_mma<true, false>(G, sB, sB);
    }
    if (JOINT) continue;
    // ---- the diagonal blocks of G (lower triangle mirrored: symmetric bit for bit)
    __syncthreads();
    cov_acc_put(sA, G);
    __syncthreads();
    if (!ray) {
      if (tid < 9 * COV_POSE_F) {
        const int q = tid / 9, x = (tid % 9) / 3, y = tid % 3;
        const int f = a.pose_frame[(int64_t)blk * COV_POSE_F + q];
        if (f >= 0) a.pose_cov[(int64_t)f * 9 + 3 * x + y] = scale * sA[3 * q + max(x, y)][3 * q + min(x, y)];
      }
    } else if (tid < 64) {
      const int q = tid >> 2, x = (tid >> 1) & 1, y = tid & 1;
      const int64_t o = (int64_t)rb * (NB / 2) + q;
      if (o < a.n_lm_sel) {
        const double vi = s_vinv[q][x + y];
        a.ray_cov[o * 4 + 2 * x + y] = scale * (vi +sA[2 * q + max(x, y)][2 * q + min(x, y)]);
      }
    }
  }
}

void launch_cov_tile_inv(const double* Ldiag, const uint8_t* pad, int n_aug, int n_tiles, double* Minv,
                         double* min_piv, hipStream_t st) {
  if (n_tiles > 0) hipLaunchKernelGGL(k_cov_tile_inv, dim3(n_tiles), dim3(64), 0, st, Ldiag, pad, n_aug, Minv, min_piv);
}

template <typename real>
void launch_cov_gram(const CovArgs& a, int n_groups, hipStream_t st) {
  if (n_groups > 0) hipLaunchKernelGGL((k_cov_gram<real, false>), dim3(n_groups), dim3(256), 0, st, a);
}
template void launch_cov_gram<float>(const CovArgs&, int, hipStream_t);
template void launch_cov_gram<double>(const CovArgs&, int, hipStream_t);

// G_ab = sum_{i >= max(t0_a, t0_b)} Z_{a,i}^T Z_{b,i} of the block pair (a, b) = (blockIdx.y, blockIdx.x), a >= b, from
// the Z tiles stage 1 kept (tiles before a block's first tile hold stale memory and are never read), in ascending i:
// deterministic, and for a == b the very sum k_cov_gram forms.  Epilogue: out[oi][oj] = out[oj][oi] = scale * (G_ij
// (+ V_l^-1 on a landmark's own 2 x 2)), negated between a ray and a pose column (stage 1 builds +Y, the joint
// covariance needs B = [E | -Y]); columns with col_out < 0 are skipped (the host zero-filled out).
__global__ __launch_bounds__(256) void k_cov_cross(CovCrossArgs a) {
  __shared__ __attribute__((aligned(16))) double sA[NB][NB + 1];  // Z_{a,i}, then G
  __shared__ __attribute__((aligned(16))) double sB[NB][NB + 1];  // Z_{b,i}
  __shared__ int s_oa[NB], s_ob[NB];
  const int ba = blockIdx.y, bb = blockIdx.x, tid = threadIdx.x;
  if (bb > ba) return;
  if (tid < NB) s_oa[tid] = a.col_out[(int64_t)ba * NB + tid];
  else if (tid < 2 * NB) s_ob[tid - NB] = a.col_out[(int64_t)bb * NB + tid - NB];
  const int t0 = max(a.block_t0[ba], a.block_t0[bb]);
  const double* __restrict__ Za = a.Z + (int64_t)ba * a.n_tiles * NB * NB;
  const double* __restrict__ Zb = a.Z + (int64_t)bb * a.n_tiles * NB * NB;
  double2 va[2], vb[2];
  // as k_cov_gram: two pairs of adjacent elements per thread and tile, the next pair of tiles in flight in registers
  auto fetch = [&](int i) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int64_t o = (int64_t)i * NB * NB + 2 * (tid + 256 * q);
      va[q] = *reinterpret_cast<const double2*>(Za + o);
      vb[q] = *reinterpret_cast<const double2*>(Zb + o);
    }
  };
  v4f64 G = {0.0, 0.0, 0.0, 0.0};
  if (t0 < a.n_tiles) fetch(t0);
  for (int i = t0; i < a.n_tiles; ++i) {
    __syncthreads();  // the previous product has read sA / sB
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int p = tid + 256 * q, r = p >> 4, c = 2 * (p & 15);
      sA[r][c] = va[q].x; sA[r][c + 1] = va[q].y;
      sB[r][c] = vb[q].x; sB[r][c + 1] = vb[q].y;
    }
    __syncthreads();
    if (i + 1 < a.n_tiles) fetch(i + 1);
    cov_mma<true, false>(G, sA, sB);
  }
  __syncthreads();
  cov_acc_put(sA, G);
  __syncthreads();
  const double scale = a.scale_dev ? a.scale_dev[0] / a.scale_div : a.scale;
  const bool ray_a = ba >= a.n_pose_blocks, ray_b = bb >= a.n_pose_blocks;
  for (int e = tid; e < NB * NB; e += 256) {
    const int i = e >> 5, j = e & 31;
    const int oi = s_oa[i], oj = s_ob[j];
    if (oi < 0 || oj < 0 || (ba == bb && j > i)) continue;  // (diagonal pairs: the lower triangle, mirrored)
    double g = sA[i][j];
    if (ba == bb && ray_a && (i >> 1) == (j >> 1)) {
      const int l = a.lm_index[(int64_t)(ba - a.n_pose_blocks) * (NB / 2) + (i >> 1)];
      g = a.lm_aux[(int64_t)l * 8 + (i & 1) + (j & 1)] + g;
    }
    double val = scale * g;
    if (ray_a != ray_b) val = -val;
    a.out[(int64_t)oi * a.n + oj] = val;
    a.out[(int64_t)oj * a.n + oi] = val;
  }
}

template <typename real>
void launch_cov_joint(const CovArgs& z, const CovCrossArgs& x, hipStream_t st) {
  if (x.n_blocks <= 0) return;
  hipLaunchKernelGGL((k_cov_gram<real, true>), dim3(x.n_blocks), dim3(256), 0, st, z);
  hipLaunchKernelGGL(k_cov_cross, dim3(x.n_blocks, x.n_blocks), dim3(256), 0, st, x);
}
template void launch_cov_joint<float>(const CovArgs&, const CovCrossArgs&, hipStream_t);
template void launch_cov_joint<double>(const CovArgs&, const CovCrossArgs&, hipStream_t);

// sum over the scalar residuals of w rho'(z) r^2 (z = (r / f_scale)^2; rho' = 1 for the linear loss and inside the
// huber unit, 1 / sqrt(z) beyond, robust_loss.h's for the smooth losses; `loss` a PTZBA_LOSS_* id): per-workgroup
// partials in a fixed order, summed by the last launch's one workgroup.  DISP: the displaced camera model, d its constants
template <typename real, bool DISP>
__global__ __launch_bounds__(256) void k_cov_resid_part(const int32_t* __restrict__ rec_seg,
                                                        const int32_t* __restrict__ seg_frame,
                                                        const int32_t* __restrict__ seg_lm,
                                                        const double2* __restrict__ seg_base,
                                                        const real* __restrict__ rec_xy, const real* __restrict__ rec_w,
                                                        const FrameTab<double>* __restrict__ ft64,
                                                        const RayTab<double>* __restrict__ rt64, double u, double v,
                                                        Disp6 d, int64_t n_rec, int loss, double inv_fs2,
                                                        double* __restrict__ part) {
  __shared__ double red[256 / WAVE];
  double s = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * blockDim.x) {
    const int sg = rec_seg[r];
    double x, y;
    if constexpr (DISP) ptz_project_disp<double>(ft64[seg_frame[sg]], rt64[seg_lm[sg]], u, v, d.c, d.k, x, y);
    else ptz_project<double>(ft64[seg_frame[sg]], rt64[seg_lm[sg]], u, v, x, y);
    const double2 bs = seg_base[sg];
    const double ex = (double)((real)(x - bs.x) - rec_xy[2 * r]), ey = (double)((real)(y - bs.y) - rec_xy[2 * r + 1]);
    double qx = ex * ex, qy = ey * ey;
    if (loss == PTZBA_LOSS_HUBER) {
      const double zx = qx * inv_fs2, zy = qy * inv_fs2;
      if (zx > 1.0) qx /= sqrt(zx);
      if (zy > 1.0) qy /= sqrt(zy);
    } else if (loss != PTZBA_LOSS_LINEAR) {
      double rho, w1x, w1y, wn;
      robust_eval_id(loss, qx * inv_fs2, rho, w1x, wn);
      robust_eval_id(loss, qy * inv_fs2, rho, w1y, wn);
      qx *= w1x;
      qy *= w1y;
    }
    s += (rec_w ? (double)rec_w[r] : 1.0) * (qx + qy);
  }
  s = wave_sum(s);
  if (lane_id() == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int k = 0; k < 256 / WAVE; ++k) t += red[k];
    part[blockIdx.x] = t;
  }
}
__global__ void k_cov_resid_sum(const double* __restrict__ part, int n, double* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  double t = 0.0;
  for (int k = 0; k < n; ++k) t += part[k];
  out[0] = t;
}

template <typename real>
void launch_cov_resid(const int32_t* rec_seg, const int32_t* seg_frame, const int32_t* seg_lm, const double2* seg_base,
                      const void* rec_xy, const void* rec_w, const void* ft64, const void* rt64, double u, double v,
                      const double* disp6, int64_t n_rec, int loss, double f_scale, double* part, int n_part,
                      double* out, hipStream_t st) {
  auto go = [&](auto kern, const Disp6& d) {
    hipLaunchKernelGGL(kern, dim3(n_part), dim3(256), 0, st, rec_seg, seg_frame, seg_lm, seg_base,
                       (const real*)rec_xy, (const real*)rec_w, (const FrameTab<double>*)ft64,
                       (const RayTab<double>*)rt64, u, v, d, n_rec, loss, 1.0 / (f_scale * f_scale), part);
  };
  if (disp6) go(k_cov_resid_part<real, true>, make_disp6(disp6));
  else go(k_cov_resid_part<real, false>, Disp6{});
  hipLaunchKernelGGL(k_cov_resid_sum, dim3(1), dim3(64), 0, st, part, n_part, out);
}
template void launch_cov_resid<float>(const int32_t*, const int32_t*, const int32_t*, const double2*, const void*,
                                      const void*, const void*, const void*, double, double, const double*, int64_t,
                                      int, double, double*, int, double*, hipStream_t);
template void launch_cov_resid<double>(const int32_t*, const int32_t*, const int32_t*, const double2*, const void*,
                                       const void*, const void*, const void*, double, double, const double*, int64_t,
                                       int, double, double*, int, double*, hipStream_t);

}  // namespace ptzba
