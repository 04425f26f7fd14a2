// The solver handle behind ptzba_handle and the helpers its translation units share (private header).
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ptzba.h"
#include "ptzba_kernels.h"
#include "host_util.h"

using ptzba::DBuf, ptzba::LMDev, ptzba::VecRanges;
enum { TM_K1 = 0, TM_SCHUR = 1, TM_CHOL = 2, TM_BACK = 3, TM_N = 4 };
constexpr int LM_RING = 4;
constexpr int TM_POOL = 512;
constexpr int COMM_POOL = 2048;  // timed exchanges per reset_kernel_times

struct ptzba_ctx {
  int device = 0;
  hipStream_t own = nullptr;
  hipStream_t st = nullptr;
  // problem
  bool have_problem = false;
  int n_pose = 0, n_lm = 0, n_fixed = 1, precision = PTZBA_FP64, loss = PTZBA_LOSS_LINEAR;
  double fs = 1.0;
  double hcurv = 1.0;  // huber curvature weight beyond the unit, in units of rho' (LinArgs::hcurv), host-driven LM
  std::vector<std::pair<const char*, double>> setup_phases;  // the last set_problem's host phases (name, ms)
  bool lm_curv_pending = false;  // device-driven LM: the huber curvature switch has not happened yet
  bool lm_relin_mode = false;    // LMParams::relin_mode of the current run
  DBuf curv_pred;                // [8] the curvature-mode reduction's output (the trial's landmark-part prediction)
  int64_t n_rec = 0, n_seg = 0;
  int n_work = 0, max_seg_per_lm = 0;
  int k1_groups = 0, k1_groups_global = 0;  // K1 workgroups; those that read the frame tables from global memory
  int n_sys = 0;
  int64_t ld = 0;
  double u = 0, v = 0;
  bool weighted = false;
  std::vector<int64_t> perm_host;  // sorted -> original record index
  bool perm_uploaded = false;
  // device: structure
  DBuf rec_xy, rec_seg, rec_w, perm, rec_key;
  DBuf seg_frame, seg_lm, seg_rec_begin, lm_seg_begin, lm_order;
  // K1's merged record stream (problem_layout.h): runs of adjacent bit-identical records of a segment as one record of
  // weight multiplicity x user weight; allocated only while k1_merged.  Every other reader of the records (residual,
  // covariance, marginal prior, K1 under w_override) keeps the unmerged arrays above
  DBuf m_rec_xy, m_rec_w, m_rec_key, m_seg_rec_begin, lm_order_m;
  int64_t n_merged = 0;    // runs (n_rec when the pass did not run: the knob, or more segments than half the records)
  bool k1_merged = false;  // K1 reads the merged stream: the runs are at most half the records
  bool k1_one = false;     // ... and it holds exactly one record per segment (k_linearize_one; PTZBA_K1_ONE=0: off)
  DBuf seg_row;  // [n_seg] system row of the segment's frame, -1: fixed (k_trial; launch_seg_row in set_problem)
  DBuf frame_seg_begin, frame_seg_list, frame_win_hi;
  DBuf s2_items, s2_groups, s2_lm, lm_meta;  // K2 work items / tiles / lists, slot ranges
  DBuf s2_part, part_diag;                                    // K2 split partials (blocks, diagonal terms)
  int n_s2_items = 0, n_s2_groups = 0;
  bool k2_valu32 = false;  // fp32 build on the VALU kernel k_schur<float> instead of the matrix-core k_schur_mfp, for
                           // the length of a covariance call (api_cov.hip CovBorrow)
  int k2_info[8] = {};  // ptzba_k2_info
  bool k2_prologue = false;  // PTZBA_K2_PROLOGUE=1: every build launches k_build_prologue (A/B, tests)
  int64_t n_build_prologue = 0, n_build_folded = 0;  // builds enqueued on either path (ptzba_build_info)
  int k2_tile_info[8] = {};  // ptzba_k2_tile_info
  std::vector<int32_t> s2_groups_host;  // ptzba_schur_groups: the tiles' {f1b, chunk, first item, end item}
  int64_t n_slot = 0;  // dense landmark x frame slots (W table rows)
  // device: state
  DBuf ptz, rays, ptz_trial, rays_trial, D_pose, D_ray;
  DBuf ptz_saved, rays_saved;  // ptzba_save_state / ptzba_restore_state (device-resident restart point)
  DBuf ft, rt, ft64, rt64, seg_base;
  DBuf ug_slot[2], w_slot[2], lm_out[2];
  int cur = 0;
  DBuf lm_aux, lm_red, red_scratch;
  DBuf sys;  // [S ld*ld | b ld | g_pose ld | dU ld]
  DBuf scal, info;  // scal: [8 partial scalars | 8 pose partials ("loc")], contiguous for one exchange
  DBuf scal_pack;               // device block [scal 8 | loc 8 | info]
  double* scal_host = nullptr;   // pinned host copy of scal_pack
  uint8_t* out_pin = nullptr;    // pinned landing buffer of ptzba_get_state (grown, kept)
  size_t out_pin_cap = 0;
  DBuf chol_tasks, Ldiag, Minv, dpose;  // Minv: inverses of the diagonal factor tiles (back-substitution)
  std::vector<int> chol_task_off;  // host: per elimination level, offsets into chol_tasks
  std::vector<int32_t> chol_tasks_host;  // host copy of chol_tasks (int4 records)
  DBuf tinv_tail;                        // diagonal tiles inverted after the factorisation
  int n_tinv_tail = 0;
  int chol_levels = 0, n_aug = 0, n_chain = 1;
  bool nested = false;
  int nd_depth = 0;  // dissection levels of the system order (SysOrder::nd_depth)
  DBuf frame_pos, row_pad, bs_chain_off, bs_chain_cols, bs_upd_off, bs_upd_tiles, bs_la_tasks;
  int bs_nupd = 0, bs_npos = 0, bs_ntasks = 0;
  DBuf bs_lo_off, bs_lo_tiles;  // left-looking back substitution lists (large systems)
  DBuf bsb_tasks, bsb_r;  // blocked back substitution (large systems): plan + r scratch [ld]
  std::vector<int> bsb_step_off;
  // persistent blocked back substitution (one launch, per-column update counters): expected counts, per-column
  // totals, the counters (zeroed at set_problem, advanced by one solve's totals per launch: epoch), error flag
  DBuf bsp_expect, bsp_tot, bsp_cnt;
  int* bsp_err = nullptr;  // pinned host flag a persistent kernel sets when a wait gave up (checked by lm_wait)
  // pinned staging of set_problem's small uploads (bump allocated, reset once the stream has drained them)
  uint8_t* stage = nullptr;
  size_t stage_cap = 0, stage_used = 0;
  // set_problem queues its staged uploads and zero fills here and lands them with ONE copy of the staging range into
  // stage_dev plus one scatter launch (flush_stage) instead of ~50 hipMemcpyAsync / hipMemsetAsync calls
  struct StageOp {
    void* dst;
    size_t off;  // offset in the staging buffer; SIZE_MAX: zero fill
    size_t n;
  };
  std::vector<StageOp> stage_ops;
  bool stage_batch = false;
  DBuf stage_dev;
  bool bs_pst = false;
  uint32_t bsp_epoch = 0;
  bool bs_ll = false, bs_blk = false;
  bool chol_delayed = false;  // the plan delays trailing updates (make_plan, DT = 2)
  DBuf xtiles, xbuf;  // packed exchange: tile list, buffer
  int n_xtiles = 0;
  DBuf ztiles;  // tiles zeroed before each build (the rest of the system region stays zero)
  int n_ztiles = 0;
  double lambda = 0;
  // posterior covariance (ptzba_covariance): its plan and buffers, built by the first call after a set_problem
  struct Cov {
    bool ready = false;
    int n_tiles = 0, n_pose_blocks = 0, n_active = 0, max_groups = 256;
    DBuf row_off, row_col, row_frame, pose_rows, pose_frame, pose_t0;  // cov_kernels.hip CovArgs
    DBuf Minv, min_piv, work, D_saved, pose_out, ray_out, lm_index, resid;
    hipEvent_t ev[2] = {nullptr, nullptr};
    // ptzba_covariance_joint: the Z tiles of every column block [blocks][n_tiles][32][32], the blocks' first tiles and
    // column maps, the chosen landmarks, the call's pose blocks, the output; grown on demand, released by set_problem
    DBuf jz, jt0, jcol, jlm, jrows, jpt0, jout;
    std::vector<int32_t> seg_host;  // lm_seg_begin (which landmarks have records)
    void release_joint() {
      for (DBuf* b : {&jz, &jt0, &jcol, &jlm, &jrows, &jpt0, &jout}) b->release();
    }
  } cov;
  // device-driven LM: state, pinned record ring, events
  DBuf lmdev;
  LMDev* lm_host = nullptr;
  // device-driven LM: the value of LMDev::cur at which (ptz, rays) -- not (ptz_trial, rays_trial) -- hold the current
  // state (BacksubArgs::state_xor); lm_wait swaps the pointers when the device's decisions moved it
  int state_base = 0;
  // single-GPU device-driven LM: the trial-cost reduction waits for ptzba_lm_decide, which fuses the decision into it
  bool scal_deferred = false;
  bool scal_exported = false;  // ptzba_exchange handed out the scalar buffer (a caller-run scalar exchange)
  // timing
  int timing = 0;  // bitmask of timed kernel groups (1 K1, 2 Schur, 4 Cholesky solve, 8 back-substitution)
  std::vector<hipEvent_t> ev[TM_N];
  int ev_used[TM_N] = {0, 0, 0, 0};
  int64_t tm_seen[TM_N] = {0, 0, 0, 0};
  bool tm_sampled[TM_N] = {false, false, false, false};
  int tm_stride = 1;
  bool tm_flush = false;  // cold-cache timing: stream a scratch buffer through the caches before each timed K1
  bool tm_flush_read = false;  // ... by reading it (clean lines) instead of writing it
  DBuf flush_buf;
  int64_t gpu_setup_min = -1;  // set_problem's device front from this many records (-1: GPU_SETUP_MIN_REC)
  // collective timing (enable bit PTZBA_TIME_COMM): an event pair around every exchange, its kind and size
  std::vector<hipEvent_t> cev;
  int cev_used = 0;
  std::vector<std::pair<int, int64_t>> clog;

  // multi-GPU (include/ptzba.h): exchanges done by the library, part-owned solve state
  ptzba_comm comm = nullptr;        // attached, not owned
  // communicators of the rank tree's groups, one per tree depth (split off comm at the first exchange; owned)
  ptzba_comm group_comms[4] = {nullptr, nullptr, nullptr, nullptr};
  bool groups_split = false;
  ptzba_exchange_fn hook = nullptr;
  void* hook_ctx = nullptr;
  int dist_world = 1, dist_rank = 0;
  int dist_mode = 0;  // 1: part-owned solve
  // rank-tree phases (make_plan_tree): factorisation levels, the exchange before each phase (kind, rank group,
  // tree depth of its communicator), exchanged tiles / vector ranges and their packing buffer
  struct DistPhase {
    int lv0 = 0, lv1 = 0, kind = 0, r0 = 0, nr = 1, depth = 0, node = -1, n_tiles = 0;
    VecRanges vr{};
    int64_t n_buf = 0;
  };
  static constexpr int MAX_PHASES = 4;
  DistPhase ph[MAX_PHASES];
  DBuf ph_tiles[MAX_PHASES], ph_buf[MAX_PHASES];
  int n_phase = 0, base_node = -1, tree_depth = 0;
  std::vector<int32_t> tree_groups;  // (r0, nr, depth) of every tree group of >= 2 ranks below the root
  DBuf row_phase, fmask;  // [n_aug] phase + 1 of each system row (0: not this rank's), [n_pose] bit 0 owned / bit 1 counted
  std::vector<uint8_t> owned_host;
  void drop_groups() {
    for (auto& c : group_comms)
      if (c) {
        ptzba_comm_delete(c);
        c = nullptr;
      }
    groups_split = false;
  }

  int elem() const { return precision == PTZBA_FP32 ? 4 : 8; }
  double* locp() const { return scal.as<double>() + 8; }
  bool has_exchange() const { return hook != nullptr || comm != nullptr; }
  bool ext_exchange = false;   // the caller ran its own exchange protocol (ptzba_exchange / _packed) once
  bool f1_covered = false;     // every 32-frame block has a chunk-0 Schur tile (all diagonals written by K2)
  // single-GPU builds fold k_chol_prepare into the build (FusedPrep, ptzba_kernels.h)
  bool no_fused_prep = false;  // PTZBA_NO_FUSED_PREP (A/B knob, read at set_problem)
  // Gaussian pose priors (ptzba_set_pose_priors; prior_kernels.hip PriorArgs): the device arrays of the current set.
  // With priors set the build takes the separate prepare launch, which then sees diag P in dU.
  struct Priors {
    int n_factor = 0, n_row = 0, n_elem = 0, n_pframe = 0, n_block = 0;
    DBuf f_begin, f_frames, f_mean, f_info_off, f_info, row_factor, s_off, s_val, p_frame, p_begin, p_ent, p_diag;
    DBuf cost;  // [1] ptzba_pose_prior_info's read-back
    DBuf red;   // [PRIOR_RED_SCRATCH] k_prior_cost's partials and counter (zeroed when allocated)
    std::vector<int32_t> h_begin, h_frames;  // host copies of f_begin / f_frames (ptzba_marginal_prior's absorption)
  } pri;
  // Gaussian ray priors (ptzba_set_ray_priors; prior_kernels.hip RayPriorArgs): a CSR over the distinct landmarks.  They
  // change lm_out's rows (V, g, cost) after K1 and nothing else, so the fused prepare stays on with them alone.
  struct RayPriors {
    int n_prior = 0, n_lm = 0;
    DBuf lm, begin, mean, info;
    DBuf cost;  // [1] ptzba_ray_prior_info's read-back
  } rp;
  // projection-centre displacement (ptzba_set_displacement): d(f) = disp[0..2] + disp[3..5] f, a constant of
  // the problem.  It changes what K1, the residual and the covariance's residual scale project and nothing else, so
  // the slot tables, K2 and the fused prepare stay as they are
  bool displaced = false;
  double disp[6] = {0, 0, 0, 0, 0, 0};
  const double* disp6() const { return displaced ? disp : nullptr; }  // the launchers' argument (nullptr: none)
  std::vector<int32_t> win_host, pos_host;  // the problem's coupling window and system positions (prior validation)
  // marginalisation (ptzba_marginal_prior / ptzba_set_marginal_prior; marg_kernels.hip)
  struct Marg {
    // the handle's dense information-form factor (n == 0: none); host copies for absorption and the info query
    int n = 0;
    double offset = 0.0;
    std::vector<int32_t> h_frames;
    DBuf frames, lin, info, eta, cost;
    // ptzba_marginal_prior's buffers: allocated on first use, released by set_problem (a plain solve keeps none)
    DBuf w, mask, flags, D_saved, dcost, out, fac, fac_frames, fac_loc, kframes, row_tile, pat;
    hipEvent_t ev[2] = {nullptr, nullptr};
    void release_work() {
      for (DBuf* b : {&w, &mask, &flags, &D_saved, &dcost, &out, &fac, &fac_frames, &fac_loc, &kframes, &row_tile, &pat})
        b->release();
    }
  } mg;
  void* w_override = nullptr;       // ptzba_marginal_prior: K1 reads these weights instead of the problem's own
  bool trial_open = false;          // host-step API: a solve_reduced's trial has not been accepted / rejected yet
  std::vector<int32_t> zt_host;     // host copy of ztiles (the factor pattern; ptzba_marginal_prior's gather)
  bool has_priors() const { return pri.n_factor > 0; }
  bool has_marg() const { return mg.n > 0; }
  bool has_ray_priors() const { return rp.n_prior > 0; }
  bool fused_prep() const {
    return !no_fused_prep && !dist_mode && !has_exchange() && !ext_exchange && f1_covered && !has_priors() && !has_marg();
  }
  double* S() const { return sys.as<double>(); }
  double* bvec() const { return sys.as<double>() + ld * ld; }
  double* gpose() const { return sys.as<double>() + ld * ld + ld; }
  double* dU() const { return sys.as<double>() + ld * ld + 2 * ld; }
  int64_t sys_count() const { return ld * ld + 3 * ld; }
};

namespace ptzba {

// event pairs of the timed kernel groups (api.hip)
void tm_begin(ptzba_ctx* h, int k);
void tm_end(ptzba_ctx* h, int k);
hipEvent_t tm_k1_event(ptzba_ctx* h, int which);

// set_problem's uploads: a small array is copied into the handle's pinned staging buffer and its H2D copy queued on
// the handle's stream without waiting (a sliding-window map calls set_problem per keyframe: ~40 uploads, each a
// pageable copy plus a stream synchronisation before); large ones take the blocking path below.  The staging
// buffer is reused only after the stream has drained (set_problem synchronises before its first upload and at the
// end; a full buffer synchronises before wrapping).
constexpr size_t STAGE_MAX = 4u << 20;
int flush_stage(ptzba_ctx* h);
int zero_async(ptzba_ctx* h, void* p, size_t n);
int stage_take(ptzba_ctx* h, size_t n, uint8_t** out);
// blocking upload on stream st (nullptr: the null stream); returns after the copy has landed
template <typename T>
int upload(DBuf& b, const std::vector<T>& v, hipStream_t st) {
  if (b.alloc(v.size() * sizeof(T))) return -1;
  if (!v.empty()) {
    HIPCHK(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return 0;
}
template <typename T>
int upload_st(ptzba_ctx* h, DBuf& b, const std::vector<T>& v) {
  const size_t n = v.size() * sizeof(T);
  if (n > STAGE_MAX) return upload(b, v, h->st);
  if (b.alloc(n)) return -1;
  if (n == 0) return 0;
  uint8_t* p = nullptr;
  if (stage_take(h, n, &p)) return -1;
  std::memcpy(p, v.data(), n);
  if (h->stage_batch) {
    h->stage_ops.push_back({b.p, (size_t)(p - h->stage), n});
    return 0;
  }
  HIPCHK(hipMemcpyAsync(b.p, p, n, hipMemcpyHostToDevice, h->st));
  return 0;
}

// the steps of a solve that the optional features reuse (api.hip)
void tables(ptzba_ctx* h, const double* ptz, const double* rays, const int* run_if = nullptr, double* zero = nullptr,
            int n_zero = 0);
void linearize_into(ptzba_ctx* h, int slot, const int* sel = nullptr, int sel_xor = 0, const int* run_if = nullptr,
                    const double* hc_dev = nullptr, bool trial_state = false);
int build_impl(ptzba_ctx* h, double lambda, const double* lam_dev, const int* skip_if = nullptr,
               const int* sel = nullptr, bool with_priors = true);
int factor_impl(ptzba_ctx* h, const double* lam_dev, const int* sel);
int solve_impl(ptzba_ctx* h, const double* lam_dev, int nx, const int* sel = nullptr);
int exchange(ptzba_ctx* h, int kind, double* buf, int64_t n);
bool single_rank(const ptzba_ctx* h);
PriorArgs prior_args(const ptzba_ctx* h, const int* sel, int flip);         // api_priors.hip
RayPriorArgs ray_prior_args(const ptzba_ctx* h, const int* sel, int flip);  // api_priors.hip
MargArgs marg_args(const ptzba_ctx* h, const int* sel, int flip);           // api_marg.hip

}  // namespace ptzba
