// PTZ pose RANSAC without an initial pose (gfx950, fp64): `ptz_pose_ransac`.
//
// A pan/tilt/zoom camera has no roll and a fixed centre, so two ray-pixel correspondences fix (pan, tilt, f) in
// closed form.  With p = [tan th, -tan ph sqrt(tan^2 th + 1), 1] the ray direction (ptzba_common.h) and
// a = (x - u, y - v) the pixel, a pixel sees the direction [a, f] (q2 > 0), and the rotation keeps the angle
// between two rays:  (s + F)^2 = c^2 (n_i + F)(n_j + F),  s = a_i . a_j, n_k = |a_k|^2, c = cos(p_i, p_j), F = f^2
//   (1 - c^2) F^2 + (2 s - c^2 (n_i + n_j)) F + (s^2 - c^2 n_i n_j) = 0
// solved by the cancellation-free formula (qq = -(B + sgn(B) sqrt(disc)) / 2; roots qq / A and C / qq); a root is
// kept when F > 0 and (s + F) c > 0 (squaring added the other sign).  Pan and tilt then follow from correspondence
// i alone: q = |p_i| [a_i, f] / sqrt(n_i + F),  cos(pan) p0 - sin(pan) = q0 with cos^2 + sin^2 = 1 (two solutions
// from one sqrt), and with w2 = sin(pan) p0 + cos(pan):  (cos tilt, sin tilt) ~ (q1 p1 + q2 w2, q1 w2 - q2 p1).
// Everything stays in (cos, sin) pairs; a candidate is a FrameTab<double>.
//
// Candidate order: sample h owns the slots 4 h + 2 root + branch; root 0 is qq / A, root 1 is C / qq; branch 0 takes
// the '+' square root of the pan equation, branch 1 the '-' one.  The winner has the most inliers (q2 > 0 and squared
// reprojection error < threshold^2); ties go to the lowest slot number, i.e. the lowest sample, then this order.
//
// Launch chain (null stream, no host round trip, work buffers kept per device):
//   k_pr_candidates  one lane per sample: the two draws (ransac_sample.h, the homography sampler's retry rule), up to
//                    four candidates into the slot table; the same grid builds the ray table {p0, p1, ax, ay} (32 B
//                    per correspondence) and clears the best key
//   k_pr_score       512 threads = 64 candidates (one per lane, in registers) x 8 parts; the ray table is staged in
//                    LDS in tiles of 1024 and every lane of a wave reads the same entry (a broadcast); the counts of
//                    the parts are summed and the workgroup's best goes out as one 64-bit atomicMax of
//                    (count << 32 | ~slot)
//   k_pr_select      one workgroup: the winner, its inlier list, the pose LM of pose_lm.h on it (linear loss), the
//                    final mask and count at the refined pose; or status 1 with a zero mask
// and one device-to-host copy of {result record, mask}.
//
// `ptz_pose_ransac_disp` is the same chain under the displaced camera K (R p + d(f)), d(f) = c + k f, the
// DISP = true instantiations of the three kernels.  A pixel at focal length f then sees q = t nh, nh = [a, f], with
// r = q - d(f) = R p, so |r|^2 = |p|^2 =: m fixes t as the positive root of
//   t^2 |nh|^2 - 2 t (nh . d) + |d|^2 - m = 0,      t = (nh . d + sqrt((nh . d)^2 - |nh|^2 (|d|^2 - m))) / |nh|^2
// and the rotation keeps r_i . r_j = p_i . p_j: one scalar equation g(f) = 0, no longer a quadratic in f^2.  It is
// solved by PR_NEWTON Newton steps in f with the analytic dg/df from each accepted root of the closed form (the same
// count for every lane: no data-dependent exit).  A candidate whose f ends non-finite or <= 0, or whose square-root
// argument was negative at any step, is dropped; pan and tilt follow from r_i(f) by the formulas above with q := r_i
// (its norm is |p_i| already).  The slot is that of the closed-form root the iteration started from.  Scoring adds the
// candidate's d(f) (three registers per lane) to the rotated ray; the refit is rf_lm<true>.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/ptzba.h"
#include "host_util.h"
#include "pose_lm.h"
#include "ptzba_common.h"
#include "ransac_sample.h"

namespace ptzba {

constexpr int PR_TILE = 1024;          // ray-table entries per LDS tile (32 KiB)
constexpr int PR_PARTS = 8;            // waves per scoring workgroup, each takes every 8th entry of the tile
constexpr int PR_SCORE_THREADS = WAVE * PR_PARTS;
constexpr double PR_R2D = 57.29577951308232;
constexpr int PR_NEWTON = 6;           // Newton steps of the displaced minimal solver (DESIGN 6.1b has the table)

struct alignas(32) RayPix {
  double p0, p1, ax, ay;  // ray direction [p0, p1, 1], pixel minus principal point
};

// the device-side result record; the mask follows it in the same buffer
struct PrResult {
  double ptz[3], ptz_hyp[3], cost;
  int32_t best_sample, hyp_inliers, n_inliers, status, iters, has_hyp, pad0, pad1;
};
static_assert(sizeof(PrResult) == 88, "PrResult layout");
constexpr size_t PR_RES_BYTES = 96;

// the displacement of the DISP kernels: d(f) = c + k f
struct PrDisp {
  double c[3], k[3];
};

// inlier of candidate (ca, sa, cb, sb, f): in front of the camera and squared reprojection error < thr2, without
// the divide: |f [w0, q1] - a q2|^2 < thr2 q2^2.  With DISP (d0, d1, d2) is the candidate's d(f), added to the rotated
// ray.
template <bool DISP>
__device__ __forceinline__ bool pr_inlier(double ca, double sa, double cb, double sb, double f, double d0, double d1,
                                          double d2, double thr2, const RayPix& r) {
  const double w2 = sa * r.p0 + ca;
  double w0 = ca * r.p0 - sa;
  double q1 = cb * r.p1 + sb * w2, q2 = cb * w2 - sb * r.p1;
  if (DISP) { w0 += d0; q1 += d1; q2 += d2; }
  const double ex = f * w0 - r.ax * q2, ey = f * q1 - r.ay * q2;
  return q2 > 0.0 && ex * ex + ey * ey < thr2 * q2 * q2;
}

// r = t nh - d(f) of pixel a at focal length f under the displacement D (m = |p|^2 of its ray) and dr/df; false when
// the square-root argument is negative.  dt/df by implicit differentiation of the quadratic in t, whose t-derivative
// is 2 sqrt(disc).
__device__ __forceinline__ bool pr_disp_ray(double a0, double a1, double m, double f, const PrDisp& D, double (&r)[3],
                                            double (&dr)[3]) {
  const double d0 = D.c[0] + D.k[0] * f, d1 = D.c[1] + D.k[1] * f, d2 = D.c[2] + D.k[2] * f;
  const double N = a0 * a0 + a1 * a1 + f * f;
  const double b = a0 * d0 + a1 * d1 + f * d2;
  const double dd = d0 * d0 + d1 * d1 + d2 * d2;
  const double disc = b * b - N * (dd - m);
  const double S = sqrt(disc);
  const double t = (b + S) / N;
  const double bp = d2 + a0 * D.k[0] + a1 * D.k[1] + f * D.k[2];
  const double dkd = d0 * D.k[0] + d1 * D.k[1] + d2 * D.k[2];
  const double tp = -(t * t * f - t * bp + dkd) / S;
  r[0] = t * a0 - d0; r[1] = t * a1 - d1; r[2] = t * f - d2;
  dr[0] = tp * a0 - D.k[0]; dr[1] = tp * a1 - D.k[1]; dr[2] = tp * f + t - D.k[2];
  return disc >= 0.0;
}

// the candidates of one sample (pi, pj: ray directions; ai, aj: centred pixels) into out[4]; pad0 = 1 marks a
// filled slot.  With DISP every accepted closed-form root starts the Newton iteration of the file header.
template <bool DISP>
__device__ inline void pr_minimal_solver(double pi0, double pi1, double pj0, double pj1, double ai0, double ai1,
                                         double aj0, double aj1, const PrDisp& D, FrameTab<double> (&out)[4]) {
  const double mi = pi0 * pi0 + pi1 * pi1 + 1.0, mj = pj0 * pj0 + pj1 * pj1 + 1.0;
  const double d = pi0 * pj0 + pi1 * pj1 + 1.0;
  const double cx = pi1 - pj1, cy = pj0 - pi0, cz = pi0 * pj1 - pi1 * pj0;  // p_i x p_j
  const double M = mi * mj;
  const double c2 = d * d / M;
  const double omc2 = (cx * cx + cy * cy + cz * cz) / M;  // 1 - c^2 without the cancellation
  if (!(omc2 > 1e-14)) return;
  const double s = ai0 * aj0 + ai1 * aj1, ni = ai0 * ai0 + ai1 * ai1, nj = aj0 * aj0 + aj1 * aj1;
  const double A = omc2, B = 2.0 * s - c2 * (ni + nj), C = s * s - c2 * ni * nj;
  const double disc = B * B - 4.0 * A * C;
  if (!(disc > 0.0)) return;
  const double sq = sqrt(disc);
  const double qq = -0.5 * (B + (B >= 0.0 ? sq : -sq));
  const double Fr[2] = {qq / A, qq != 0.0 ? C / qq : -1.0};
#pragma unroll
  for (int root = 0; root < 2; ++root) {
    const double F = Fr[root];
    if (!(F > 0.0 && (s + F) * d > 0.0)) continue;
    double f = sqrt(F), q0, q1, q2;
    if (DISP) {
      double ri[3], rj[3], dri[3], drj[3];
      bool ok = true;
#pragma unroll 1
      for (int it = 0; it < PR_NEWTON; ++it) {
        ok = pr_disp_ray(ai0, ai1, mi, f, D, ri, dri) && ok;
        ok = pr_disp_ray(aj0, aj1, mj, f, D, rj, drj) && ok;
        const double g = ri[0] * rj[0] + ri[1] * rj[1] + ri[2] * rj[2] - d;
        const double gp = dri[0] * rj[0] + dri[1] * rj[1] + dri[2] * rj[2] + ri[0] * drj[0] + ri[1] * drj[1] +
                          ri[2] * drj[2];
        f -= g / gp;
      }
      ok = pr_disp_ray(ai0, ai1, mi, f, D, ri, dri) && ok;
      if (!(ok && isfinite(f) && f > 0.0)) continue;
      q0 = ri[0]; q1 = ri[1]; q2 = ri[2];
    } else {
      const double lam = sqrt(mi / (ni + F));
      q0 = lam * ai0; q1 = lam * ai1; q2 = lam * f;
    }
    const double r2 = 1.0 + pi0 * pi0 - q0 * q0;
    if (!(r2 >= 0.0)) continue;
    const double r = sqrt(r2), inv = 1.0 / (1.0 + pi0 * pi0);
#pragma unroll
    for (int branch = 0; branch < 2; ++branch) {
      const double sg = branch ? -1.0 : 1.0;
      const double ca = (pi0 * q0 + sg * r) * inv, sa = (-q0 + sg * pi0 * r) * inv;
      const double w2 = sa * pi0 + ca;
      const double cbn = q1 * pi1 + q2 * w2, sbn = q1 * w2 - q2 * pi1;
      const double nb = sqrt(cbn * cbn + sbn * sbn);
      if (!(nb > 0.0)) continue;
      FrameTab<double>& o = out[2 * root + branch];
      o.ca = ca; o.sa = sa; o.cb = cbn / nb; o.sb = sbn / nb; o.f = f; o.pad0 = 1.0;
    }
  }
}

template <bool DISP>
__global__ __launch_bounds__(256) void k_pr_candidates(int n, const double* __restrict__ rays,
                                                       const double* __restrict__ pts, double u, double v, int n_hyp,
                                                       uint64_t seed, RayPix* __restrict__ tab,
                                                       FrameTab<double>* __restrict__ cand,
                                                       unsigned long long* __restrict__ best, PrDisp D) {
  const int gid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  if (gid == 0) *best = 0ull;
  for (int i = gid; i < n; i += stride) {
    const RayTab<double> R = make_ray_tab<double>(rays[2 * i], rays[2 * i + 1]);
    RayPix e;
    e.p0 = R.p0; e.p1 = R.p1; e.ax = pts[2 * i] - u; e.ay = pts[2 * i + 1] - v;
    tab[i] = e;
  }
  if (gid >= n_hyp) return;
  FrameTab<double> out[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    out[k].ca = out[k].sa = out[k].cb = out[k].sb = out[k].f = out[k].pad0 = out[k].pad1 = out[k].pad2 = 0.0;
  const uint32_t i = ransac_draw(seed, (uint32_t)gid, 0u, 0u, (uint32_t)n);
  uint32_t att = 0, j;
  do {
    j = ransac_draw(seed, (uint32_t)gid, 1u, att++, (uint32_t)n);
  } while (j == i && att < 64);
  if (j != i) {
    const RayTab<double> Ri = make_ray_tab<double>(rays[2 * i], rays[2 * i + 1]);
    const RayTab<double> Rj = make_ray_tab<double>(rays[2 * j], rays[2 * j + 1]);
    pr_minimal_solver<DISP>(Ri.p0, Ri.p1, Rj.p0, Rj.p1, pts[2 * i] - u, pts[2 * i + 1] - v, pts[2 * j] - u,
                            pts[2 * j + 1] - v, D, out);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) cand[4 * (size_t)gid + k] = out[k];
}

template <bool DISP>
__global__ __launch_bounds__(PR_SCORE_THREADS) void k_pr_score(int n, const RayPix* __restrict__ tab,
                                                               const FrameTab<double>* __restrict__ cand,
                                                               unsigned n_cand, double thr2,
                                                               unsigned long long* __restrict__ best, PrDisp D) {
  __shared__ RayPix sTab[PR_TILE];
  __shared__ int sCnt[PR_PARTS][WAVE];
  __shared__ unsigned long long sBest;
  const int t = threadIdx.x, lane = t & (WAVE - 1), part = t >> 6;
  const unsigned g = blockIdx.x * (unsigned)WAVE + (unsigned)lane;
  double ca = 0, sa = 0, cb = 0, sb = 0, f = 0;
  bool ok = false;
  if (g < n_cand) {
    const FrameTab<double> C = cand[g];
    ok = C.pad0 != 0.0;
    ca = C.ca; sa = C.sa; cb = C.cb; sb = C.sb; f = C.f;
  }
  double d0 = 0, d1 = 0, d2 = 0;  // the candidate's d(f)
  if (DISP) { d0 = D.c[0] + D.k[0] * f; d1 = D.c[1] + D.k[1] * f; d2 = D.c[2] + D.k[2] * f; }
  if (t == 0) sBest = 0ull;
  int cnt = 0;
  for (int t0 = 0; t0 < n; t0 += PR_TILE) {
    const int m = min(PR_TILE, n - t0);
    if (t0) __syncthreads();
    for (int k = t; k < m; k += PR_SCORE_THREADS) sTab[k] = tab[t0 + k];
    __syncthreads();
    if (ok)
      for (int k = part; k < m; k += PR_PARTS) cnt += pr_inlier<DISP>(ca, sa, cb, sb, f, d0, d1, d2, thr2, sTab[k]) ? 1 : 0;
  }
  sCnt[part][lane] = cnt;
  __syncthreads();
  if (part == 0 && ok) {
    int c = 0;
#pragma unroll
    for (int q = 0; q < PR_PARTS; ++q) c += sCnt[q][lane];
    atomicMax(&sBest, ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(0xffffffffu - g));
  }
  __syncthreads();
  if (t == 0 && sBest) atomicMax(best, sBest);
}

struct PrSelectArgs {
  int n, min_inliers;
  double thr2;
  const RayPix* tab;
  const FrameTab<double>* cand;
  const unsigned long long* best;
  int64_t* sub_off;  // [2]
  int32_t* sub_idx;  // [n]
  PrResult* res;
  uint8_t* mask;  // [n]
  RefineArgs lm;  // rays, pts, u, v, tolerances; sub_off / sub_idx point at the two above
};

template <bool DISP>
__global__ __launch_bounds__(RF_THREADS) void k_pr_select(PrSelectArgs a) {
  __shared__ RefineShared S;
  __shared__ int sCnt[RF_THREADS];
  __shared__ int sTot;
  const int t = threadIdx.x, n = a.n;
  const unsigned long long key = *a.best;
  const int hyp_in = (int)(key >> 32);
  const unsigned g = 0xffffffffu - (unsigned)(key & 0xffffffffu);
  FrameTab<double> C;
  C.ca = 1.0; C.sa = 0.0; C.cb = 1.0; C.sb = 0.0; C.f = 0.0;
  if (key) C = a.cand[g];
  const double hyp[3] = {atan2(C.sa, C.ca) * PR_R2D, atan2(C.sb, C.cb) * PR_R2D, C.f};
  double d0 = 0, d1 = 0, d2 = 0;  // d(f) of the pose that is scored (a.lm carries the displacement)
  if (DISP) { d0 = a.lm.dc[0] + a.lm.dk[0] * C.f; d1 = a.lm.dc[1] + a.lm.dk[1] * C.f; d2 = a.lm.dc[2] + a.lm.dk[2] * C.f; }
  if (key == 0ull || hyp_in < a.min_inliers) {  // not found (uniform over the workgroup)
    for (int i = t; i < n; i += RF_THREADS) a.mask[i] = 0;
    if (t == 0) {
      PrResult r;
      for (int k = 0; k < 3; ++k) { r.ptz[k] = 0.0; r.ptz_hyp[k] = key ? hyp[k] : 0.0; }
      r.cost = 0.0;
      r.best_sample = key ? (int)(g >> 2) : -1;
      r.hyp_inliers = hyp_in;
      r.n_inliers = 0; r.status = 1; r.iters = 0; r.has_hyp = key ? 1 : 0; r.pad0 = r.pad1 = 0;
      *a.res = r;
    }
    return;
  }
  // the winner's inliers, in index order: thread t owns the chunk [i0, i1)
  const int chunk = (n + RF_THREADS - 1) / RF_THREADS;
  const int i0 = min(n, t * chunk), i1 = min(n, i0 + chunk);
  int cnt = 0;
  for (int i = i0; i < i1; ++i) cnt += pr_inlier<DISP>(C.ca, C.sa, C.cb, C.sb, C.f, d0, d1, d2, a.thr2, a.tab[i]) ? 1 : 0;
  sCnt[t] = cnt;
  __syncthreads();
  if (t == 0) {
    int run = 0;
    for (int k = 0; k < RF_THREADS; ++k) { const int c = sCnt[k]; sCnt[k] = run; run += c; }
    a.sub_off[0] = 0;
    a.sub_off[1] = run;
    sTot = 0;
  }
  __syncthreads();
  int o = sCnt[t];
  for (int i = i0; i < i1; ++i)
    if (pr_inlier<DISP>(C.ca, C.sa, C.cb, C.sb, C.f, d0, d1, d2, a.thr2, a.tab[i])) a.sub_idx[o++] = i;
  __syncthreads();  // the list is read back through a.lm by every thread
  double p[3] = {hyp[0], hyp[1], hyp[2]};
  double cost;
  int it, status;
  rf_lm<DISP>(a.lm, 0, p, cost, it, status, S);
  // mask and count at the refined pose
  const FrameTab<double> F = make_frame_tab<double>(p[0], p[1], p[2]);
  if (DISP) { d0 = a.lm.dc[0] + a.lm.dk[0] * F.f; d1 = a.lm.dc[1] + a.lm.dk[1] * F.f; d2 = a.lm.dc[2] + a.lm.dk[2] * F.f; }
  cnt = 0;
  for (int i = t; i < n; i += RF_THREADS) {
    const bool in = pr_inlier<DISP>(F.ca, F.sa, F.cb, F.sb, F.f, d0, d1, d2, a.thr2, a.tab[i]);
    a.mask[i] = in ? 1 : 0;
    cnt += in ? 1 : 0;
  }
  cnt = wave_sum_i(cnt);
  if (lane_id() == 0) atomicAdd(&sTot, cnt);
  __syncthreads();
  if (t == 0) {
    PrResult r;
    for (int k = 0; k < 3; ++k) { r.ptz[k] = p[k]; r.ptz_hyp[k] = hyp[k]; }
    r.cost = cost;
    r.best_sample = (int)(g >> 2);
    r.hyp_inliers = hyp_in;
    r.n_inliers = sTot; r.status = 0; r.iters = it; r.has_hyp = 1; r.pad0 = r.pad1 = 0;
    *a.res = r;
  }
}

}  // namespace ptzba

using namespace ptzba;

// the launch chain under displacement DISP ? D : none
template <bool DISP>
static void pr_launch(unsigned g1, unsigned n_cand, int n, const double* drays, const double* dpts, double u, double v,
                      int n_hyp, uint64_t seed, double thr2, RayPix* tab, FrameTab<double>* cand,
                      unsigned long long* best, const PrDisp& D, const PrSelectArgs& a) {
  hipLaunchKernelGGL(k_pr_candidates<DISP>, dim3(g1), dim3(256), 0, nullptr, n, drays, dpts, u, v, n_hyp, seed, tab,
                     cand, best, D);
  hipLaunchKernelGGL(k_pr_score<DISP>, dim3((n_cand + WAVE - 1) / WAVE), dim3(PR_SCORE_THREADS), 0, nullptr, n, tab,
                     cand, n_cand, thr2, best, D);
  hipLaunchKernelGGL(k_pr_select<DISP>, dim3(1), dim3(RF_THREADS), 0, nullptr, a);
}

// d6: the six displacement values, or nullptr for the displacement-free kernels
static int pose_ransac(int device, int64_t n_corr, const double* rays, const double* points, double u, double v,
                       const ptz_pose_ransac_opts* opts, const double* d6, double* ptz_out, double* ptz_hyp_out,
                       int32_t* best_sample_out, int32_t* hyp_inliers_out, uint8_t* mask_out, int32_t* n_inliers_out,
                       double* cost_out, int32_t* status_out) {
  if (n_corr < 2) return fail("pose RANSAC needs at least 2 correspondences (got %lld)", (long long)n_corr);
  if (n_corr >= ((int64_t)1 << 31)) return fail("too many correspondences");
  if (!rays || !points) return fail("null argument");
  ptz_pose_ransac_opts o{1024, 3, 100, 0, 3.0, 1e-4, 1e-8, 0};
  if (opts) o = *opts;
  if (o.n_hyp < 1 || o.n_hyp > (1 << 28)) return fail("bad hypothesis count %d", o.n_hyp);
  if (!(o.threshold > 0)) return fail("bad threshold");
  if (o.max_iter < 0 || !(o.ftol >= 0) || !(o.xtol >= 0) || o.reserved != 0) return fail("bad options");
  if (o.min_inliers < 3) o.min_inliers = 3;  // a two-point sample always explains its own two correspondences
  if (select_device(device)) return -1;
  struct PoseRansacWork {
    DBuf in, tab, cand, best, sub, out;
    std::vector<double> hin;
    std::vector<unsigned char> hout;
  };
  auto guard = device_work_lock(device);
  PoseRansacWork& Wk = work_for<PoseRansacWork>(device);
  const size_t n = (size_t)n_corr, n_cand = 4 * (size_t)o.n_hyp;
  if (Wk.in.reserve(n * 32) || Wk.tab.reserve(n * sizeof(RayPix)) || Wk.cand.reserve(n_cand * sizeof(FrameTab<double>)) ||
      Wk.best.reserve(8) || Wk.sub.reserve(16 + n * 4) || Wk.out.reserve(PR_RES_BYTES + n))
    return -1;
  Wk.hin.resize(n * 4);
  std::memcpy(Wk.hin.data(), rays, n * 16);
  std::memcpy(Wk.hin.data() + 2 * n, points, n * 16);
  HIPCHK(hipMemcpy(Wk.in.p, Wk.hin.data(), n * 32, hipMemcpyHostToDevice));
  const double* drays = Wk.in.as<double>();
  const double* dpts = drays + 2 * n;
  const double thr2 = o.threshold * o.threshold;
  const unsigned g1 = (unsigned)((std::max<size_t>((size_t)o.n_hyp, std::min<size_t>(n, 65536)) + 255) / 256);
  PrDisp D{};
  if (d6)
    for (int k = 0; k < 3; ++k) { D.c[k] = d6[k]; D.k[k] = d6[3 + k]; }
  PrSelectArgs a;
  a.n = (int)n_corr;
  a.min_inliers = o.min_inliers;
  a.thr2 = thr2;
  a.tab = Wk.tab.as<RayPix>();
  a.cand = Wk.cand.as<FrameTab<double>>();
  a.best = Wk.best.as<unsigned long long>();
  a.sub_off = Wk.sub.as<int64_t>();
  a.sub_idx = reinterpret_cast<int32_t*>(Wk.sub.as<unsigned char>() + 16);
  a.res = Wk.out.as<PrResult>();
  a.mask = Wk.out.as<uint8_t>() + PR_RES_BYTES;
  a.lm.n_hyp = 1;
  a.lm.ptz = nullptr;
  a.lm.sub_off = a.sub_off;
  a.lm.sub_idx = a.sub_idx;
  a.lm.n_corr = n_corr;
  a.lm.rays = drays;
  a.lm.pts = dpts;
  a.lm.u = u;
  a.lm.v = v;
  a.lm.max_iter = o.max_iter;
  a.lm.loss = PTZBA_LOSS_LINEAR;
  a.lm.ftol = o.ftol;
  a.lm.xtol = o.xtol;
  a.lm.fs2 = a.lm.inv_fs2 = 1.0;
  a.lm.cost_out = nullptr;
  a.lm.iters_out = nullptr;
  a.lm.status_out = nullptr;
  for (int k = 0; k < 3; ++k) { a.lm.dc[k] = D.c[k]; a.lm.dk[k] = D.k[k]; }
  if (d6)
    pr_launch<true>(g1, (unsigned)n_cand, (int)n_corr, drays, dpts, u, v, (int)o.n_hyp, (uint64_t)o.seed, thr2,
                    Wk.tab.as<RayPix>(), Wk.cand.as<FrameTab<double>>(), Wk.best.as<unsigned long long>(), D, a);
  else
    pr_launch<false>(g1, (unsigned)n_cand, (int)n_corr, drays, dpts, u, v, (int)o.n_hyp, (uint64_t)o.seed, thr2,
                     Wk.tab.as<RayPix>(), Wk.cand.as<FrameTab<double>>(), Wk.best.as<unsigned long long>(), D, a);
  HIPCHK(hipGetLastError());
  Wk.hout.resize(PR_RES_BYTES + n);
  HIPCHK(hipMemcpy(Wk.hout.data(), Wk.out.p, PR_RES_BYTES + n, hipMemcpyDeviceToHost));
  PrResult r;
  std::memcpy(&r, Wk.hout.data(), sizeof(r));
  if (status_out) *status_out = r.status;
  if (best_sample_out) *best_sample_out = r.best_sample;
  if (hyp_inliers_out) *hyp_inliers_out = r.hyp_inliers;
  if (n_inliers_out) *n_inliers_out = r.n_inliers;
  if (ptz_hyp_out && r.has_hyp) std::memcpy(ptz_hyp_out, r.ptz_hyp, 24);
  if (mask_out) std::memcpy(mask_out, Wk.hout.data() + PR_RES_BYTES, n);
  if (r.status == 0) {  // not found: the pose and cost outputs stay as the caller left them
    if (ptz_out) std::memcpy(ptz_out, r.ptz, 24);
    if (cost_out) *cost_out = r.cost;
  }
  return 0;
}

int ptz_pose_ransac(int device, int64_t n_corr, const double* rays, const double* points, double u, double v,
                    const ptz_pose_ransac_opts* opts, double* ptz_out, double* ptz_hyp_out, int32_t* best_sample_out,
                    int32_t* hyp_inliers_out, uint8_t* mask_out, int32_t* n_inliers_out, double* cost_out,
                    int32_t* status_out) {
  return pose_ransac(device, n_corr, rays, points, u, v, opts, nullptr, ptz_out, ptz_hyp_out, best_sample_out,
                     hyp_inliers_out, mask_out, n_inliers_out, cost_out, status_out);
}

int ptz_pose_ransac_disp(int device, int64_t n_corr, const double* rays, const double* points, double u, double v,
                         const ptz_pose_ransac_opts* opts, double* ptz_out, double* ptz_hyp_out,
                         int32_t* best_sample_out, int32_t* hyp_inliers_out, uint8_t* mask_out,
                         int32_t* n_inliers_out, double* cost_out, int32_t* status_out, const double* displacement6) {
  const double* d6 = nullptr;
  if (displacement_arg(displacement6, d6)) return -1;
  return pose_ransac(device, n_corr, rays, points, u, v, opts, d6, ptz_out, ptz_hyp_out, best_sample_out,
                     hyp_inliers_out, mask_out, n_inliers_out, cost_out, status_out);
}
