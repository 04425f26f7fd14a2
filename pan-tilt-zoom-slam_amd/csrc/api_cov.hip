// ------------------------------------------------------------------------------------------------
// posterior covariance: diagonal blocks of scale * H^-1 at the current state (cov_kernels.hip)
// ------------------------------------------------------------------------------------------------
#include <algorithm>
#include <cmath>

#include "ba_ctx.h"

using namespace ptzba;

// the covariance plan of the current problem, from the device copies of the solver's own structure (a solve keeps no
// host copy of them): row CSR of the factor's tile pattern, row -> frame map, pose column blocks in system order
constexpr int COV_WG_PER_CU = 2;
constexpr size_t COV_WORK_BYTES = (size_t)192 << 20;  // cap of the Z workspace (MI355X Infinity Cache: 256 MB)
static int cov_prepare(ptzba_ctx* h) {
  auto& c = h->cov;
  if (c.ready) return 0;
  std::vector<int32_t> zt(2 * (size_t)h->n_ztiles), pos(h->n_pose), seg(h->n_lm + 1);
  HIPCHK(hipMemcpyAsync(zt.data(), h->ztiles.p, zt.size() * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(pos.data(), h->frame_pos.p, pos.size() * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(seg.data(), h->lm_seg_begin.p, seg.size() * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  const int T = (h->n_aug + CHOL_NB - 1) / CHOL_NB;
  std::vector<std::vector<int>> rows(T);
  for (int q = 0; q < h->n_ztiles; ++q) {
    const int i = zt[2 * q], j = zt[2 * q + 1];
    if (j < i && i < T) rows[i].push_back(j);
  }
  std::vector<int> off(T + 1, 0), col;
  for (int i = 0; i < T; ++i) {
    std::sort(rows[i].begin(), rows[i].end());
    col.insert(col.end(), rows[i].begin(), rows[i].end());
    off[i + 1] = (int)col.size();
  }
  if (col.empty()) col.push_back(0);
  std::vector<int32_t> row_frame(std::max(h->n_aug, 1), -1);
  std::vector<std::pair<int, int>> free_frames;  // (system row, frame)
  for (int f = 0; f < h->n_pose; ++f) {
    if (pos[f] < 0) continue;
    if (pos[f] + 2 >= h->n_aug) return fail("covariance plan: frame %d lies outside the system", f);
    for (int q = 0; q < 3; ++q) row_frame[pos[f] + q] = f;
    free_frames.emplace_back(pos[f], f);
  }
  std::sort(free_frames.begin(), free_frames.end());
  const int nb = ((int)free_frames.size() + COV_POSE_F - 1) / COV_POSE_F;
  std::vector<int32_t> prow((size_t)std::max(nb, 1) * CHOL_NB, -1), pfr((size_t)std::max(nb, 1) * COV_POSE_F, -1),
      pt0(std::max(nb, 1), 0);
  for (int k = 0; k < (int)free_frames.size(); ++k) {
    const int b = k / COV_POSE_F, q = k % COV_POSE_F;
    for (int x = 0; x < 3; ++x) prow[(size_t)b * CHOL_NB + 3 * q + x] = free_frames[k].first + x;
    pfr[(size_t)b * COV_POSE_F + q] = free_frames[k].second;
    if (q == 0) pt0[b] = free_frames[k].first / CHOL_NB;
  }
  c.n_active = 0;
  for (int l = 0; l < h->n_lm; ++l) c.n_active += seg[l + 1] > seg[l];
  c.seg_host = seg;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, h->device));
  // workgroups in flight: COV_WG_PER_CU per CU (one wave per SIMD each; 18 KB of LDS and ~100 VGPRs would let four be
  // resident), as long as their Z workspaces together stay inside the Infinity Cache (knob: PTZBA_COV_WG_PER_CU)
  const char* gpc = getenv("PTZBA_COV_WG_PER_CU");
  const int per_cu = gpc ? std::min(std::max(atoi(gpc), 1), 8) : COV_WG_PER_CU;
  const size_t per_block = (size_t)std::max(T, 1) * CHOL_NB * CHOL_NB * 8;
  c.max_groups = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(prop.multiProcessorCount, 1) * per_cu,
                                                           COV_WORK_BYTES / per_block));
  if (upload(c.row_off, off, h->st) || upload(c.row_col, col, h->st) || upload(c.row_frame, row_frame, h->st) ||
      upload(c.pose_rows, prow, h->st) || upload(c.pose_frame, pfr, h->st) || upload(c.pose_t0, pt0, h->st) ||
      c.Minv.alloc((size_t)std::max(T, 1) * CHOL_NB * CHOL_NB * 8) || c.min_piv.alloc((size_t)std::max(T, 1) * 8) ||
      c.D_saved.alloc(h->D_pose.bytes + h->D_ray.bytes) || c.resid.alloc((1024 + 8) * 8))
    return -1;
  for (auto& e : c.ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  c.n_tiles = T;
  c.n_pose_blocks = nb;
  c.ready = true;
  return 0;
}

// Between solves (no trial pending): linearises the current state with IRLS curvature, builds and factors the
// undamped reduced system and runs the selected inverse, all on the handle's stream; leaves the handle as
// ptzba_linearize does, with the Marquardt scales, the damping and the huber curvature setting of the caller's run
// restored, so a solve started afterwards takes bitwise the steps it takes without the call.
//
// ptzba_covariance and ptzba_covariance_joint share everything up to the masked tile inverses and the factor's verdict:
// cov_options (the option and handle checks), cov_dof, CovBorrow + cov_front (the queue up to k_cov_tile_inv) and
// cov_verdict (the one synchronisation: factor status, smallest pivot, scale).
static int cov_options(const ptzba_ctx* h, const char* who, const ptzba_cov_opts* o, ptzba_cov_opts& opt) {
  if (!h || !h->have_problem) return fail("no problem set");
  opt = ptzba_cov_opts{(int32_t)sizeof(ptzba_cov_opts), 0, 1.0};
  if (o) {
    if (o->struct_size != (int32_t)sizeof(ptzba_cov_opts))
      return fail("%s: unknown struct_size %d of ptzba_cov_opts (this library knows %d)", who, (int)o->struct_size,
                  (int)sizeof(ptzba_cov_opts));
    opt = *o;
  }
  if (opt.scale_mode < 0 || opt.scale_mode > 2) return fail("%s: bad options (scale_mode %d)", who, opt.scale_mode);
  if (opt.scale_mode == 1 && !(opt.scale > 0.0 && std::isfinite(opt.scale)))
    return fail("%s: bad options (scale must be positive and finite)", who);
  if (h->dist_mode || h->dist_world > 1 || h->has_exchange() || h->ext_exchange)
    return fail("%s is single-rank only (the handle is sharded or has a communicator / hook attached)", who);
  return 0;
}

// free parameters and degrees of freedom of the residual scale (after cov_prepare)
static int cov_dof(const ptzba_ctx* h, const char* who, const ptzba_cov_opts& opt, int& n_free, double& dof) {
  n_free = 3 * (h->n_pose - h->n_fixed) + 2 * h->cov.n_active;
  // pose priors: every prior row counts as a residual (rank-deficient factors over-count, include/ptzba.h)
  // ray priors likewise: two rows each
  const int64_t n_prior_rows = (h->has_priors() ? (int64_t)h->pri.n_row : 0) + (h->has_ray_priors() ? 2 * (int64_t)h->rp.n_prior : 0);
  dof = 2.0 * (double)h->n_rec + (double)n_prior_rows - (double)n_free;
  if (opt.scale_mode == 2 && !(dof > 0)) return fail("%s: residual scale needs more residuals (%lld) than "
                                                     "free parameters (%d)", who, (long long)(2 * h->n_rec + n_prior_rows), n_free);
  return 0;
}

// the caller's run state a covariance call borrows: huber curvature, damping, timing groups, and the fp32 K2 form.
// The one build of a covariance call runs the VALU K2 (k2_valu32: float32 products of the float32 slots,
// flushed to fp64 per batch): the matrix-core K2's split-fp16 products (22 bits, rounded toward zero) leave an error
// in S that an LM step tolerates but an inverse multiplies by the condition number -- 3.5e-3 in the block metric at
// scaled cond 1.6e5 against ~5e-5 from the float32 slots themselves (crafted systems).
struct CovBorrow {
  ptzba_ctx* h;
  double hcurv, lambda;
  int timing;
  bool k2_valu32;
  explicit CovBorrow(ptzba_ctx* h_)
      : h(h_), hcurv(h_->hcurv), lambda(h_->lambda), timing(h_->timing), k2_valu32(h_->k2_valu32) {
    h->hcurv = 1.0;
    h->lambda = 0.0;
    h->timing = 0;
    h->k2_valu32 = true;
  }
  ~CovBorrow() { h->hcurv = hcurv; h->lambda = lambda; h->timing = timing; h->k2_valu32 = k2_valu32; }
};

// queues, under a CovBorrow: the start event, the linearisation with IRLS curvature, the residual sum of scale mode 2
// (cov.resid[0]), the undamped build and its factorisation with the Marquardt scales saved and put back, and the
// masked inverses of the factor's diagonal tiles with their smallest pivots
static int cov_front(ptzba_ctx* h, const ptzba_cov_opts& opt) {
  auto& c = h->cov;
  HIPCHK(hipEventRecord(c.ev[0], h->st));
  // the Marquardt scales are a monotone memory of the run: a build raises them, so they are put back afterwards
  double* dsave = c.D_saved.as<double>();
  HIPCHK(hipMemcpyAsync(dsave, h->D_pose.p, h->D_pose.bytes, hipMemcpyDeviceToDevice, h->st));
  HIPCHK(hipMemcpyAsync(dsave + h->D_pose.bytes / 8, h->D_ray.p, h->D_ray.bytes, hipMemcpyDeviceToDevice, h->st));
  if (ptzba_linearize(h)) return -1;
  double* resid = c.resid.as<double>();  // [0] the weighted residual sum | [8, ...) partials
  if (opt.scale_mode == 2) {
    const int n_part = (int)std::min<int64_t>(1024, (h->n_rec + 255) / 256);
    if (h->precision == PTZBA_FP32)
      launch_cov_resid<float>(h->rec_seg.as<int32_t>(), h->seg_frame.as<int32_t>(), h->seg_lm.as<int32_t>(),
                              h->seg_base.as<double2>(), h->rec_xy.p, h->weighted ? h->rec_w.p : nullptr, h->ft64.p,
                              h->rt64.p, h->u, h->v, h->disp6(), h->n_rec, h->loss, h->fs, resid + 8, n_part,
                              resid, h->st);
    else
      launch_cov_resid<double>(h->rec_seg.as<int32_t>(), h->seg_frame.as<int32_t>(), h->seg_lm.as<int32_t>(),
                               h->seg_base.as<double2>(), h->rec_xy.p, h->weighted ? h->rec_w.p : nullptr, h->ft64.p,
                               h->rt64.p, h->u, h->v, h->disp6(), h->n_rec, h->loss, h->fs, resid + 8, n_part,
                               resid, h->st);
  }
  // ... + sum_k e_k^T Lambda_k e_k, twice the prior cost
  if (opt.scale_mode == 2 && h->has_priors()) launch_prior_cost(prior_args(h, nullptr, 0), resid, 2.0, 1, h->pri.red.as<double>(), h->st);
  if (opt.scale_mode == 2 && h->has_ray_priors()) launch_ray_prior_cost(ray_prior_args(h, nullptr, 0), resid, 2.0, 1, h->st);
  if (build_impl(h, 0.0, nullptr) || factor_impl(h, nullptr, nullptr)) return -1;
  HIPCHK(hipMemcpyAsync(h->D_pose.p, dsave, h->D_pose.bytes, hipMemcpyDeviceToDevice, h->st));
  HIPCHK(hipMemcpyAsync(h->D_ray.p, dsave + h->D_pose.bytes / 8, h->D_ray.bytes, hipMemcpyDeviceToDevice, h->st));
  launch_cov_tile_inv(h->Ldiag.as<double>(), h->row_pad.as<uint8_t>(), h->n_aug, c.n_tiles, c.Minv.as<double>(),
                      c.min_piv.as<double>(), h->st);
  return 0;
}

// the fields of CovArgs that both calls fill alike: the factor, its pattern and the current linearisation
static CovArgs cov_args(const ptzba_ctx* h, const ptzba_cov_opts& opt, double dof) {
  const auto& c = h->cov;
  CovArgs a{};
  a.L = h->S();
  a.ld = h->ld;
  a.n_aug = h->n_aug;
  a.n_tiles = c.n_tiles;
  a.Minv = c.Minv.as<double>();
  a.row_off = c.row_off.as<int>();
  a.row_col = c.row_col.as<int>();
  a.frame_pos = h->frame_pos.as<int32_t>();
  a.row_frame = c.row_frame.as<int32_t>();
  a.scale = opt.scale_mode == 1 ? opt.scale : 1.0;
  a.scale_dev = opt.scale_mode == 2 ? c.resid.as<double>() : nullptr;
  a.scale_div = dof;
  a.w_slot = h->w_slot[h->cur].p;
  a.lm_aux = h->lm_aux.as<double>();
  a.lm_meta = h->lm_meta.as<int4>();
  a.lm_seg_begin = h->lm_seg_begin.as<int32_t>();
  return a;
}

// records the end event, then the factor's verdict first: nothing is copied out of a failed factorisation
static int cov_verdict(ptzba_ctx* h, const char* who, const ptzba_cov_opts& opt, double dof, double given_scale,
                       double& scale, double& min_pivot) {
  auto& c = h->cov;
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c.ev[1], h->st));
  std::vector<double> piv(std::max(c.n_tiles, 1), 1.0);
  int finfo = 0;
  double rsum = 0.0;
  HIPCHK(hipMemcpyAsync(piv.data(), c.min_piv.p, (size_t)c.n_tiles * 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(&finfo, h->info.p, sizeof(int), hipMemcpyDeviceToHost, h->st));
  if (opt.scale_mode == 2) HIPCHK(hipMemcpyAsync(&rsum, c.resid.p, 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  min_pivot = 1e300;
  bool bad = false;
  for (int t = 0; t < c.n_tiles; ++t) {
    if (!(piv[t] > 0.0) || !std::isfinite(piv[t])) bad = true;
    if (piv[t] < min_pivot) min_pivot = piv[t];
  }
  if (finfo != 0 || bad)
    return fail("%s: the undamped reduced system is not positive definite (factorisation info %d, "
                "non-positive pivot: %s) -- a free frame without observations makes it singular", who, finfo,
                bad ? "yes" : "no");
  scale = opt.scale_mode == 2 ? rsum / dof : given_scale;
  if (!(scale > 0.0) || !std::isfinite(scale)) return fail("%s: the residual scale is not positive (%g)", who, scale);
  return 0;
}

int ptzba_covariance(ptzba_handle h, const ptzba_cov_opts* o, double* pose_cov, const int32_t* lm_index, int32_t n_lm,
                     double* ray_cov, double* info) {
  ptzba_cov_opts opt;
  if (cov_options(h, "ptzba_covariance", o, opt)) return -1;
  if (n_lm < -1) return fail("ptzba_covariance: bad landmark count %d", n_lm);
  const int64_t n_sel = n_lm < 0 ? h->n_lm : n_lm;
  if (n_lm > 0 && !lm_index) return fail("ptzba_covariance: null landmark index list");
  if (n_sel > 0 && !ray_cov) return fail("ptzba_covariance: null ray covariance buffer");
  for (int32_t k = 0; k < n_lm; ++k)
    if (lm_index[k] < 0 || lm_index[k] >= h->n_lm)
      return fail("ptzba_covariance: landmark index %d out of range [0, %d)", lm_index[k], h->n_lm);
  HIPCHK(hipSetDevice(h->device));
  if (cov_prepare(h)) return -1;
  auto& c = h->cov;
  int n_free;
  double dof;
  if (cov_dof(h, "ptzba_covariance", opt, n_free, dof)) return -1;
  const int n_ray_blocks = (int)((n_sel + CHOL_NB / 2 - 1) / (CHOL_NB / 2));
  const int n_pose_blocks = pose_cov ? c.n_pose_blocks : 0;
  const int n_groups = std::min(c.max_groups, n_pose_blocks + n_ray_blocks);
  if (c.work.reserve((size_t)std::max(n_groups, 1) * std::max(c.n_tiles, 1) * CHOL_NB * CHOL_NB * 8) ||
      c.pose_out.reserve((size_t)h->n_pose * 9 * 8) || c.ray_out.reserve((size_t)std::max<int64_t>(n_sel, 1) * 4 * 8) ||
      c.lm_index.reserve((size_t)std::max<int32_t>(n_lm, 1) * 4))
    return -1;
  SyncOnExit sync_guard{h->st};  // caller buffers and the stack below outlive every queued copy, also on errors
  CovBorrow borrow(h);
  if (n_lm > 0) HIPCHK(hipMemcpyAsync(c.lm_index.p, lm_index, (size_t)n_lm * 4, hipMemcpyHostToDevice, h->st));
  if (cov_front(h, opt)) return -1;
  if (pose_cov) HIPCHK(hipMemsetAsync(c.pose_out.p, 0, (size_t)h->n_pose * 9 * 8, h->st));
  CovArgs a = cov_args(h, opt, dof);
  a.work = c.work.as<double>();
  a.n_pose_blocks = n_pose_blocks;
  a.pose_rows = c.pose_rows.as<int32_t>();
  a.pose_frame = c.pose_frame.as<int32_t>();
  a.pose_t0 = c.pose_t0.as<int32_t>();
  a.pose_cov = c.pose_out.as<double>();
  a.n_ray_blocks = n_ray_blocks;
  a.n_lm_sel = n_sel;
  a.lm_index = n_lm < 0 ? nullptr : c.lm_index.as<int32_t>();
  a.ray_cov = c.ray_out.as<double>();
  if (h->precision == PTZBA_FP32) launch_cov_gram<float>(a, n_groups, h->st);
  else launch_cov_gram<double>(a, n_groups, h->st);
  double scale, min_pivot;
  if (cov_verdict(h, "ptzba_covariance", opt, dof, a.scale, scale, min_pivot)) return -1;
  if (pose_cov) HIPCHK(hipMemcpyAsync(pose_cov, c.pose_out.p, (size_t)h->n_pose * 9 * 8, hipMemcpyDeviceToHost, h->st));
  if (n_sel > 0) HIPCHK(hipMemcpyAsync(ray_cov, c.ray_out.p, (size_t)n_sel * 4 * 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (info) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    info[0] = scale;
    info[1] = min_pivot;
    info[2] = (double)n_free;
    info[3] = (double)ms;
  }
  return 0;
}

// The dense joint covariance of chosen frames and landmarks: scale * (D + Z^T Z) with L Z = B = [E_F | -Y_L] and
// D = blockdiag(0, V_l^-1) (cov_kernels.hip: k_cov_gram keeping Z per column block, then k_cov_cross over the block
// pairs).  The front half and the verdict are ptzba_covariance's.
int ptzba_covariance_joint(ptzba_handle h, const ptzba_cov_opts* o, const int32_t* frames, int32_t n_frame,
                           const int32_t* landmarks, int32_t n_lm, double* cov_out, double* info) {
  static const char* who = "ptzba_covariance_joint";
  ptzba_cov_opts opt;
  if (cov_options(h, who, o, opt)) return -1;
  if (h->trial_open || h->scal_deferred)
    return fail("%s: an LM trial is pending (accept or reject it first; the call runs between solves)", who);
  if (n_frame < 0 || n_lm < 0 || (n_frame > 0 && !frames) || (n_lm > 0 && !landmarks))
    return fail("%s: bad arguments (n_frame %d, n_lm %d, null index list)", who, n_frame, n_lm);
  const int64_t n = 3 * (int64_t)n_frame + 2 * (int64_t)n_lm;
  if (n < 1 || n > PTZBA_COV_JOINT_MAX_COLS)
    return fail("%s: %lld columns selected (3 per frame, 2 per landmark); 1 to %d are possible", who, (long long)n,
                PTZBA_COV_JOINT_MAX_COLS);
  if (!cov_out) return fail("%s: null output matrix", who);
  {
    std::vector<uint8_t> seen_f(h->n_pose, 0), seen_l(h->n_lm, 0);
    for (int32_t k = 0; k < n_frame; ++k) {
      if (frames[k] < 0 || frames[k] >= h->n_pose) return fail("%s: frame %d out of range [0, %d)", who, frames[k], h->n_pose);
      if (seen_f[frames[k]]++) return fail("%s: frame %d is named twice", who, frames[k]);
    }
    for (int32_t k = 0; k < n_lm; ++k) {
      if (landmarks[k] < 0 || landmarks[k] >= h->n_lm)
        return fail("%s: landmark index %d out of range [0, %d)", who, landmarks[k], h->n_lm);
      if (seen_l[landmarks[k]]++) return fail("%s: landmark %d is named twice", who, landmarks[k]);
    }
  }
  HIPCHK(hipSetDevice(h->device));
  if (cov_prepare(h)) return -1;
  auto& c = h->cov;
  int n_free;
  double dof;
  if (cov_dof(h, who, opt, n_free, dof)) return -1;
  // ---- column blocks: the chosen free frames in system order, COV_POSE_F per block, then the landmarks, 16 per block
  std::vector<std::pair<int, int>> sel;  // (system row, position in `frames`)
  for (int32_t k = 0; k < n_frame; ++k)
    if (h->pos_host[frames[k]] >= 0) sel.emplace_back(h->pos_host[frames[k]], k);
  std::sort(sel.begin(), sel.end());
  const int npb = ((int)sel.size() + COV_POSE_F - 1) / COV_POSE_F;
  const int nrb = (n_lm + CHOL_NB / 2 - 1) / (CHOL_NB / 2);
  const int nblk = npb + nrb;
  std::vector<int32_t> prow((size_t)std::max(npb, 1) * CHOL_NB, -1), pt0(std::max(npb, 1), 0),
      col((size_t)std::max(nblk, 1) * CHOL_NB, -1);
  for (int k = 0; k < (int)sel.size(); ++k) {
    const int b = k / COV_POSE_F, q = k % COV_POSE_F;
    for (int x = 0; x < 3; ++x) {
      prow[(size_t)b * CHOL_NB + 3 * q + x] = sel[k].first + x;
      col[(size_t)b * CHOL_NB + 3 * q + x] = 3 * sel[k].second + x;
    }
    if (q == 0) pt0[b] = sel[k].first / CHOL_NB;
  }
  for (int32_t k = 0; k < n_lm; ++k) {
    const int l = landmarks[k];
    if (c.seg_host[l + 1] == c.seg_host[l]) continue;  // no records: zero rows and columns
    const size_t o2 = (size_t)(npb + k / (CHOL_NB / 2)) * CHOL_NB + 2 * (k % (CHOL_NB / 2));
    col[o2] = 3 * n_frame + 2 * k;
    col[o2 + 1] = 3 * n_frame + 2 * k + 1;
  }
  const size_t tile_bytes = (size_t)CHOL_NB * CHOL_NB * 8;
  if (c.jz.reserve((size_t)std::max(nblk, 1) * std::max(c.n_tiles, 1) * tile_bytes) ||
      c.jt0.reserve((size_t)std::max(nblk, 1) * 4) || c.jcol.reserve(col.size() * 4) ||
      c.jlm.reserve((size_t)std::max(n_lm, 1) * 4) || c.jrows.reserve(prow.size() * 4) ||
      c.jpt0.reserve(pt0.size() * 4) || c.jout.reserve((size_t)(n * n) * 8))
    return -1;
  SyncOnExit sync_guard{h->st};  // caller buffers and the stack outlive every queued copy, also on errors
  CovBorrow borrow(h);
  HIPCHK(hipMemcpyAsync(c.jcol.p, col.data(), col.size() * 4, hipMemcpyHostToDevice, h->st));
  HIPCHK(hipMemcpyAsync(c.jrows.p, prow.data(), prow.size() * 4, hipMemcpyHostToDevice, h->st));
  HIPCHK(hipMemcpyAsync(c.jpt0.p, pt0.data(), pt0.size() * 4, hipMemcpyHostToDevice, h->st));
  if (n_lm > 0) HIPCHK(hipMemcpyAsync(c.jlm.p, landmarks, (size_t)n_lm * 4, hipMemcpyHostToDevice, h->st));
  if (cov_front(h, opt)) return -1;
  HIPCHK(hipMemsetAsync(c.jout.p, 0, (size_t)(n * n) * 8, h->st));
  CovArgs a = cov_args(h, opt, dof);
  a.work = c.jz.as<double>();
  a.n_pose_blocks = npb;
  a.pose_rows = c.jrows.as<int32_t>();
  a.pose_t0 = c.jpt0.as<int32_t>();
  a.n_ray_blocks = nrb;
  a.n_lm_sel = n_lm;
  a.lm_index = c.jlm.as<int32_t>();
  a.block_t0 = c.jt0.as<int32_t>();
  CovCrossArgs x{};
  x.Z = c.jz.as<double>();
  x.n_tiles = c.n_tiles;
  x.n_blocks = nblk;
  x.n_pose_blocks = npb;
  x.block_t0 = c.jt0.as<int32_t>();
  x.col_out = c.jcol.as<int32_t>();
  x.lm_index = c.jlm.as<int32_t>();
  x.lm_aux = h->lm_aux.as<double>();
  x.scale = a.scale;
  x.scale_dev = a.scale_dev;
  x.scale_div = a.scale_div;
  x.out = c.jout.as<double>();
  x.n = n;
  if (h->precision == PTZBA_FP32) launch_cov_joint<float>(a, x, h->st);
  else launch_cov_joint<double>(a, x, h->st);
  double scale, min_pivot;
  if (cov_verdict(h, who, opt, dof, a.scale, scale, min_pivot)) return -1;
  HIPCHK(hipMemcpyAsync(cov_out, c.jout.p, (size_t)(n * n) * 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (info) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c.ev[0], c.ev[1]));
    info[0] = scale;
    info[1] = min_pivot;
    info[2] = (double)n_free;
    info[3] = (double)ms;
  }
  return 0;
}
