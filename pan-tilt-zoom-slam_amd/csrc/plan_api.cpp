// Handle-free host queries of the C-ABI (include/ptzba.h): coupling window, the plans set_problem would choose,
// landmark partition of a sharded solve, matching-graph landmark ids.  No device work.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/ptzba.h"
#include "chol_plan.h"
#include "host_util.h"
#include "par_util.h"
#include "problem_layout.h"

using namespace ptzba;

int ptzba_coupling_window(int32_t n_pose, int32_t n_landmark, int64_t n_obs, const int32_t* obs_frame,
                          const int32_t* obs_landmark, int32_t* win_out) {
  if (n_pose < 1 || n_landmark < 0 || n_obs < 0 || !win_out || (n_obs > 0 && (!obs_frame || !obs_landmark)))
    return fail("bad arguments");
  std::vector<int32_t> hi(std::max(n_landmark, 1), -1);
  for (int64_t r = 0; r < n_obs; ++r) {
    const int32_t f = obs_frame[r], l = obs_landmark[r];
    if (f < 0 || f >= n_pose || l < 0 || l >= n_landmark) return fail("record %lld out of range", (long long)r);
    hi[l] = std::max(hi[l], f);
  }
  for (int f = 0; f < n_pose; ++f) win_out[f] = f;
  for (int64_t r = 0; r < n_obs; ++r) win_out[obs_frame[r]] = std::max(win_out[obs_frame[r]], hi[obs_landmark[r]]);
  return 0;
}

// host only: the runs set_problem's host front merges for K1 (problem_layout.h), from the same passes
int ptzba_k1_merge_runs(int32_t n_pose, int32_t n_landmark, int64_t n_obs, const int32_t* obs_frame,
                        const int32_t* obs_landmark, const double* obs_xy, const double* obs_weight, int32_t precision,
                        int64_t* counts3, int64_t cap, int64_t* run_first, int64_t* run_mult) {
  if (n_pose < 1 || n_landmark < 0 || n_obs < 0 || !counts3 || (n_obs > 0 && (!obs_frame || !obs_landmark || !obs_xy)) ||
      (precision != PTZBA_FP64 && precision != PTZBA_FP32))
    return fail("bad arguments");
  for (int64_t r = 0; r < n_obs; ++r)
    if (obs_frame[r] < 0 || obs_frame[r] >= n_pose || obs_landmark[r] < 0 || obs_landmark[r] >= n_landmark)
      return fail("record %lld out of range", (long long)r);
  ProblemLayout L;
  const int threads = host_threads(n_obs);
  layout_host_sort(L, n_pose, n_landmark, n_obs, obs_frame, obs_landmark, threads);
  if (const char* e = layout_host_segments(L, n_landmark, n_obs, obs_frame, obs_landmark, threads)) return fail("%s", e);
  std::vector<double> seg_base, xy64, w64;
  std::vector<float> xy32, w32;
  const bool fp32 = precision == PTZBA_FP32;
  if (fp32) {
    xy32.resize(2 * (size_t)n_obs);
    w32.resize(obs_weight ? (size_t)n_obs : 0);
    layout_convert_records<float>(L, n_obs, obs_xy, obs_weight, seg_base, xy32.data(), w32.data());
    layout_host_merge(L, n_obs, xy32.data(), obs_weight ? w32.data() : nullptr, true, threads, true);
  } else {
    xy64.resize(2 * (size_t)n_obs);
    w64.resize(obs_weight ? (size_t)n_obs : 0);
    layout_convert_records<double>(L, n_obs, obs_xy, obs_weight, seg_base, xy64.data(), w64.data());
    layout_host_merge(L, n_obs, xy64.data(), obs_weight ? w64.data() : nullptr, false, threads, true);
  }
  counts3[0] = (int64_t)L.seg_frame.size();
  counts3[1] = L.n_merged;
  counts3[2] = L.k1_merged ? 1 : 0;
  for (int64_t m = 0; m < std::min(cap, L.n_merged); ++m) {
    if (run_first) run_first[m] = L.order[L.m_first[m]];
    if (run_mult) run_mult[m] = L.m_first[m + 1] - L.m_first[m];
  }
  return 0;
}

// Landmark -> rank assignment of a sharded solve (include/ptzba.h): the part-owned split when the frame
// chain has one (landmarks seeing A to rank group 0, B to group 1, C-only landmarks to the group whose part
// their first frame is nearer; equal-record contiguous blocks inside a group), else contiguous landmark
// blocks of equal record counts over all ranks (replicated solve).
// the caller's coupling window as a vector, checked: every frame's last coupled frame lies in [f, n_pose)
static int window_arg(int n_pose, const int32_t* frame_win_hi, std::vector<int32_t>& win) {
  win.assign(frame_win_hi, frame_win_hi + n_pose);
  for (int f = 0; f < n_pose; ++f)
    if (win[f] < f || win[f] >= n_pose) return fail("frame_win_hi[%d] = %d out of range", f, win[f]);
  return 0;
}

// host only (no device): the order and plan set_problem would choose for a coupling window -- for tests and
// tools (include/ptzba.h)
int ptzba_plan_summary(int32_t n_pose, int32_t n_fixed, const int32_t* frame_win_hi, int32_t ordering, int64_t* out8) {
  if (n_pose < 1 || n_fixed < 0 || n_fixed > n_pose || !frame_win_hi || !out8) return fail("bad arguments");
  if (ordering < PTZBA_ORDER_NATURAL || ordering > PTZBA_ORDER_NESTED_FORCE) return fail("bad ordering %d", ordering);
  std::vector<int32_t> win;
  if (window_arg(n_pose, frame_win_hi, win)) return -1;
  SysOrder so;
  CholPlan plan;
  if (choose_order_plan(n_pose, n_fixed, win, ordering, so, plan)) return fail("no factorisation plan");
  int max_tasks = 0;
  for (int L = 0; L < plan.n_levels; ++L) max_tasks = std::max(max_tasks, plan.level_off[L + 1] - plan.level_off[L]);
  int max_chain = 0;
  for (size_t c = 0; c + 1 < plan.chain_off.size(); ++c) max_chain = std::max(max_chain, plan.chain_off[c + 1] - plan.chain_off[c]);
  out8[0] = so.n_aug;
  out8[1] = pad_tile(so.n_aug + 1);
  out8[2] = plan.n_levels;
  out8[3] = so.nd_depth;
  out8[4] = (int64_t)plan.chain_off.size() - 1;
  out8[5] = max_chain;
  out8[6] = (int64_t)plan.bsb_step_off.size() - 1;  // blocked back-solve steps (0: no valid schedule)
  out8[7] = max_tasks | ((int64_t)plan.delayed << 32);
  return 0;
}

// host only: the chosen order's frame positions and the factorisation task list (int4 records, as the level
// launches receive them) with the level offsets -- the plan a CPU executor of the tile tasks can replay
int ptzba_plan_export(int32_t n_pose, int32_t n_fixed, const int32_t* frame_win_hi, int32_t ordering, int32_t* pos_out,
                      int32_t* tasks_out, int64_t tasks_cap, int32_t* level_off_out, int64_t levels_cap, int64_t* counts) {
  if (n_pose < 1 || n_fixed < 0 || n_fixed > n_pose || !frame_win_hi || !counts) return fail("bad arguments");
  std::vector<int32_t> win;
  if (window_arg(n_pose, frame_win_hi, win)) return -1;
  SysOrder so;
  CholPlan plan;
  if (choose_order_plan(n_pose, n_fixed, win, ordering, so, plan)) return fail("no factorisation plan");
  const int64_t nt = (int64_t)plan.tasks.size() / 4, nl = plan.n_levels;
  counts[0] = nt;
  counts[1] = nl;
  counts[2] = so.n_aug;
  counts[3] = plan.delayed ? 1 : 0;
  // a null output buffer only queries the counts; a non-null one that is too small is an error (no partial copy)
  if (tasks_out && tasks_cap < nt) return fail("tasks buffer holds %lld tasks, the plan has %lld", (long long)tasks_cap, (long long)nt);
  if (level_off_out && levels_cap < nl + 1)
    return fail("level offset buffer holds %lld entries, the plan needs %lld", (long long)levels_cap, (long long)(nl + 1));
  if (pos_out) std::copy(so.pos.begin(), so.pos.end(), pos_out);
  if (tasks_out) std::copy(plan.tasks.begin(), plan.tasks.end(), tasks_out);
  if (level_off_out) std::copy(plan.level_off.begin(), plan.level_off.end(), level_off_out);
  return 0;
}

// host only (round 6): which form of an N-rank solve the planner predicts faster -- the rank tree (each rank factors
// its subtree + its ancestors' separators, separator blocks summed per group) or the replicated solve (one all-reduce
// of the packed system, every rank factors all of it).  Both shard the landmarks over all ranks, so K1 / K2 / trial
// cancel out; compared are the slowest rank's factorisation estimate (plan_est_us, the planner's own figure) plus its
// collectives per trial as ring all-reduces, alpha + 2 (p - 1) / p * bytes / B.  At config 3 the tree
// does not shorten the chain (separators ~110 frames), so its extra exchanges lose from 4 ranks on; at config 4 the
// tree's factorisation is 1.5-2x shorter.  out8: [0] tree estimate us (0: no tree), [1] replicated us, [2] the tree's
// slowest-rank factorisation us, [3] the full plan's factorisation us, [4] tree collectives per trial on that rank,
// [5] tree doubles on that rank, [6] replicated doubles (packed system), [7] chosen form (1 tree, 0 replicated).
int ptzba_dist_form_estimate(int32_t n_pose, int32_t n_fixed, const int32_t* frame_win_hi, int32_t world,
                             double alpha_us, double link_gbs, double* out8) {
  if (n_pose < 1 || n_fixed < 0 || n_fixed > n_pose || !frame_win_hi || !out8 || world < 1 || !(alpha_us >= 0) ||
      !(link_gbs > 0))
    return fail("bad arguments");
  std::vector<int32_t> win;
  if (window_arg(n_pose, frame_win_hi, win)) return -1;
  std::fill(out8, out8 + 8, 0.0);
  auto ring_us = [&](double doubles, int p) {
    return p < 2 ? 0.0 : alpha_us + 2.0 * (p - 1) / p * 8.0 * doubles / (link_gbs * 1e3);
  };
  SysOrder so;
  CholPlan plan;
  if (choose_order_plan(n_pose, n_fixed, win, PTZBA_ORDER_NESTED, so, plan)) return fail("no factorisation plan");
  const double sys_doubles = (double)(plan.xtiles.size() / 2) * CHOL_NB * CHOL_NB + 3.0 * (double)pad_tile(so.n_aug + 1);
  const double full_us = plan_est_us(plan);
  const double scal = 2.0 * PTZBA_NSCALARS;
  out8[1] = full_us + ring_us(sys_doubles, world) + ring_us(scal, world);
  out8[3] = full_us;
  out8[6] = sys_doubles;
  SysOrder o;
  DistTree DT;
  if (world >= 2 && dist_order(n_pose, n_fixed, win, world, o) && dist_tree(o, world, DT)) {
    const int64_t ld = pad_tile(o.n_aug + 1);
    double worst = 0;
    for (int r = 0; r < world; ++r) {
      CholPlan P;
      TreePlan Q;
      if (!make_plan_tree(o, DT, r, n_pose, n_fixed, win, ld, P, Q)) return fail("no rank-tree plan for rank %d", r);
      double comm = ring_us(scal, world), nd = 0;
      int nx = 1;
      for (size_t q = 0; q < Q.ph.size(); ++q) {
        const auto& t = Q.ph[q];
        if (q == 0 && t.nr < 2) continue;
        const double n = (double)(t.xt.size() / 2) * CHOL_NB * CHOL_NB + t.vr.count[0] + t.vr.count[1] + t.vr.count[2];
        comm += ring_us(n, t.nr);
        nd += n;
        ++nx;
      }
      const double est = plan_est_us(P);
      if (est + comm > worst) {
        worst = est + comm;
        out8[2] = est;
        out8[4] = nx;
        out8[5] = nd;
      }
    }
    out8[0] = worst;
  }
  out8[7] = (out8[0] > 0 && out8[0] <= out8[1]) ? 1.0 : 0.0;
  return 0;
}

// host only: the rank-tree plan set_problem builds for rank `rank` of `world` (tools/dist_predict.py, tests)
int ptzba_dist_plan_summary(int32_t n_pose, int32_t n_fixed, const int32_t* frame_win_hi, int32_t world, int32_t rank,
                            int64_t* out16) {
  if (n_pose < 1 || n_fixed < 0 || n_fixed > n_pose || !frame_win_hi || !out16 || world < 1 || rank < 0 || rank >= world)
    return fail("bad arguments");
  std::vector<int32_t> win;
  if (window_arg(n_pose, frame_win_hi, win)) return -1;
  std::fill(out16, out16 + 16, 0);
  SysOrder o;
  DistTree DT;
  if (world < 2 || !dist_order(n_pose, n_fixed, win, world, o) || !dist_tree(o, world, DT)) return 0;
  CholPlan P;
  TreePlan Q;
  const int64_t ld = pad_tile(o.n_aug + 1);
  if (!make_plan_tree(o, DT, rank, n_pose, n_fixed, win, ld, P, Q)) return fail("no rank-tree plan");
  out16[0] = 1;
  out16[1] = o.nd_depth;
  out16[2] = Q.base;
  out16[3] = (int64_t)Q.ph.size();
  out16[4] = P.n_levels;
  out16[5] = (int64_t)plan_est_us(P);
  out16[6] = P.level_off[P.n_levels];
  int mx = 0;
  for (int L = 0; L < P.n_levels; ++L) mx = std::max(mx, P.level_off[L + 1] - P.level_off[L]);
  out16[7] = mx;
  for (size_t q = 0; q < Q.ph.size(); ++q) {
    const auto& t = Q.ph[q];
    if (q == 0 && t.nr < 2) continue;
    const int64_t n = (int64_t)(t.xt.size() / 2) * CHOL_NB * CHOL_NB + t.vr.count[0] + t.vr.count[1] + t.vr.count[2];
    out16[t.kind == PTZBA_X_PART ? 8 : (t.kind == PTZBA_X_SUB ? 9 : 10)] += n;
    out16[t.kind == PTZBA_X_PART ? 11 : (t.kind == PTZBA_X_SUB ? 12 : 13)] = t.nr;
  }
  out16[14] = o.n_aug;
  out16[15] = (int64_t)P.bsb_step_off.size() - 1;
  return 0;
}

// host only: rank `rank`'s whole rank-tree plan for a CPU replay (tests/test_plan_replay.py): frame positions, tasks,
// level offsets, per phase {lv0, lv1, exchange kind, group first rank, group size, exchanged tiles}, and the tiles
// (ti, tj) of every phase's exchange concatenated.  counts: [0] tasks, [1] levels, [2] n_aug, [3] phases,
// [4] exchanged tiles.  Null outputs only query the counts.
int ptzba_dist_plan_export(int32_t n_pose, int32_t n_fixed, const int32_t* frame_win_hi, int32_t world, int32_t rank,
                           int32_t* pos_out, int32_t* tasks_out, int64_t tasks_cap, int32_t* level_off_out,
                           int64_t levels_cap, int32_t* phases_out, int32_t phases_cap, int32_t* xt_out, int64_t xt_cap,
                           int64_t* counts) {
  if (n_pose < 1 || n_fixed < 0 || n_fixed > n_pose || !frame_win_hi || !counts || world < 2 || rank < 0 || rank >= world)
    return fail("bad arguments");
  std::vector<int32_t> win;
  if (window_arg(n_pose, frame_win_hi, win)) return -1;
  SysOrder o;
  DistTree DT;
  if (!dist_order(n_pose, n_fixed, win, world, o) || !dist_tree(o, world, DT)) return fail("no rank-tree split");
  CholPlan P;
  TreePlan Q;
  if (!make_plan_tree(o, DT, rank, n_pose, n_fixed, win, pad_tile(o.n_aug + 1), P, Q)) return fail("no rank-tree plan");
  int64_t nxt = 0;
  for (const auto& t : Q.ph) nxt += (int64_t)t.xt.size() / 2;
  counts[0] = (int64_t)P.tasks.size() / 4;
  counts[1] = P.n_levels;
  counts[2] = o.n_aug;
  counts[3] = (int64_t)Q.ph.size();
  counts[4] = nxt;
  if ((tasks_out && tasks_cap < counts[0]) || (level_off_out && levels_cap < counts[1] + 1) ||
      (phases_out && phases_cap < counts[3]) || (xt_out && xt_cap < nxt))
    return fail("an output buffer is too small");
  if (pos_out) std::copy(o.pos.begin(), o.pos.end(), pos_out);
  if (tasks_out) std::copy(P.tasks.begin(), P.tasks.end(), tasks_out);
  if (level_off_out) std::copy(P.level_off.begin(), P.level_off.end(), level_off_out);
  for (size_t q = 0; q < Q.ph.size(); ++q) {
    const auto& t = Q.ph[q];
    if (phases_out) {
      int32_t* r = phases_out + 6 * q;
      r[0] = t.lv0; r[1] = t.lv1; r[2] = t.kind; r[3] = t.r0; r[4] = t.nr; r[5] = (int32_t)(t.xt.size() / 2);
    }
    if (xt_out) {
      std::copy(t.xt.begin(), t.xt.end(), xt_out);
      xt_out += t.xt.size();
    }
  }
  return 0;
}

// host only: the phases of rank `rank` (tests/numpy_handle.py NumpyTreeHandle emulates the protocol from them):
// per phase {exchange kind before it, group first rank, group size, first frame, end frame}
int ptzba_dist_rank_phases(int32_t n_pose, int32_t n_fixed, const int32_t* frame_win_hi, int32_t world, int32_t rank,
                           int32_t* out, int32_t cap, int32_t* n_out) {
  if (n_pose < 1 || n_fixed < 0 || n_fixed > n_pose || !frame_win_hi || !n_out || world < 2 || rank < 0 || rank >= world)
    return fail("bad arguments");
  std::vector<int32_t> win;
  if (window_arg(n_pose, frame_win_hi, win)) return -1;
  SysOrder o;
  DistTree DT;
  *n_out = 0;
  if (!dist_order(n_pose, n_fixed, win, world, o) || !dist_tree(o, world, DT)) return 0;
  std::vector<int> anc;
  const int base = dist_base(DT, rank, &anc);
  const auto& bn = DT.n[base];
  std::vector<int32_t> v;
  if (bn.nr >= 2) v.insert(v.end(), {PTZBA_X_PART, bn.r0, bn.nr, bn.f0, bn.f1});
  else v.insert(v.end(), {PTZBA_X_PART, rank, 1, bn.sf0, bn.sf1});
  for (int u : anc)
    v.insert(v.end(), {DT.n[u].parent < 0 ? PTZBA_X_SEP : PTZBA_X_SUB, DT.n[u].r0, DT.n[u].nr, DT.n[u].f0, DT.n[u].f1});
  *n_out = (int32_t)(v.size() / 5);
  if (out) {
    if (cap < *n_out) return fail("output holds %d phases, %d needed", cap, *n_out);
    std::copy(v.begin(), v.end(), out);
  }
  return 0;
}

int ptzba_partition_landmarks(int32_t n_pose, int32_t n_landmark, int64_t n_obs, const int32_t* obs_frame,
                              const int32_t* obs_landmark, int32_t n_fixed, int32_t world, int32_t* rank_of_landmark,
                              int32_t* mode_out, int32_t* split_out) {
  if (n_pose < 1 || n_landmark < 0 || n_obs < 0 || world < 1 || n_fixed < 0 || n_fixed > n_pose || !rank_of_landmark ||
      (n_obs > 0 && (!obs_frame || !obs_landmark)))
    return fail("bad arguments");
  std::vector<int32_t> win(n_pose);
  if (ptzba_coupling_window(n_pose, n_landmark, n_obs, obs_frame, obs_landmark, win.data())) return -1;
  std::vector<int64_t> cnt(std::max(n_landmark, 1), 0);
  std::vector<int32_t> lo(std::max(n_landmark, 1), INT32_MAX), hi(std::max(n_landmark, 1), -1);
  for (int64_t r = 0; r < n_obs; ++r) {
    const int l = obs_landmark[r], f = obs_frame[r];
    cnt[l]++;
    if (f >= n_fixed) {
      lo[l] = std::min(lo[l], f);
      hi[l] = std::max(hi[l], f);
    }
  }
  // equal-record contiguous blocks of the landmarks in `ids` over ranks [r0, r0 + nr)
  auto blocks = [&](const std::vector<int32_t>& ids, int r0, int nr) {
    int64_t tot = 0;
    for (int l : ids) tot += cnt[l];
    int64_t acc = 0;
    for (int l : ids) {
      const int k = tot > 0 ? (int)std::min<int64_t>(nr - 1, (acc * nr) / std::max<int64_t>(tot, 1)) : 0;
      rank_of_landmark[l] = r0 + k;
      acc += cnt[l];
    }
  };
  for (int l = 0; l < n_landmark; ++l) rank_of_landmark[l] = -1;
  SysOrder o;
  DistTree DT;
  const bool part = world >= 2 && dist_order(n_pose, n_fixed, win, world, o) && dist_tree(o, world, DT);
  if (mode_out) *mode_out = part ? 1 : 0;
  if (split_out) {
    split_out[0] = part ? o.split_m : 0;
    split_out[1] = part ? o.split_cend : 0;
    split_out[2] = n_pose;
  }
  if (!part) {
    std::vector<int32_t> ids;
    for (int l = 0; l < n_landmark; ++l)
      if (cnt[l] > 0) ids.push_back(l);
    blocks(ids, 0, world);
    return 0;
  }
  // rank tree (make_plan_tree): from the root, a landmark goes to the child whose subtree frames it sees (no landmark
  // sees both: the node's separator); one that sees only separator frames goes to the child nearer to it; a node
  // with one rank keeps it; a shared leaf deals its landmarks out in equal-record contiguous blocks
  // the tree nodes each landmark's (non-fixed) frames lie in, as a bit mask; per node the mask of its subtree
  const int nn = (int)DT.n.size();
  if (nn > 32) return fail("rank tree too large");
  std::vector<int32_t> node_of(n_pose, -1);
  for (int v = 0; v < nn; ++v)
    for (int f = DT.n[v].f0; f < DT.n[v].f1; ++f) node_of[f] = v;
  std::vector<uint32_t> lmask(std::max(n_landmark, 1), 0u), smask(nn, 0u);
  for (int64_t r = 0; r < n_obs; ++r)
    if (obs_frame[r] >= n_fixed && node_of[obs_frame[r]] >= 0) lmask[obs_landmark[r]] |= 1u << node_of[obs_frame[r]];
  for (int v = 0; v < nn; ++v)
    for (int u = v; u >= 0; u = DT.n[u].parent) smask[u] |= 1u << v;
  std::vector<std::vector<int32_t>> leaf_ids(DT.n.size());
  for (int l = 0; l < n_landmark; ++l) {
    if (cnt[l] == 0) continue;
    int v = 0;
    for (;;) {
      const auto& x = DT.n[v];
      if (x.nr == 1) {
        rank_of_landmark[l] = x.r0;
        break;
      }
      if (x.nch != 2) {
        leaf_ids[v].push_back(l);
        break;
      }
      int go;
      if (hi[l] < 0) {
        go = 0;  // fixed frames only
      } else {
        const bool in0 = (lmask[l] & smask[x.child[0]]) != 0, in1 = (lmask[l] & smask[x.child[1]]) != 0;
        if (in0 && in1) return fail("landmark %d couples both parts (bad split)", l);
        if (in0) go = 0;
        else if (in1) go = 1;
        else go = (lo[l] - x.f0) < (x.f1 - 1 - hi[l]) ? 0 : 1;  // separator frames only: the nearer part
      }
      v = x.child[go];
    }
  }
  for (size_t v = 0; v < DT.n.size(); ++v)
    if (!leaf_ids[v].empty()) blocks(leaf_ids[v], DT.n[v].r0, DT.n[v].nr);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// matching-graph landmark ids: first-seen rule of image_process.py:611-639 (bit-exact)
// ------------------------------------------------------------------------------------------------
int ptzba_build_landmarks(int32_t n_frames, const int64_t* kp_count, int64_t n_pairs, const int32_t* pair_i,
                          const int32_t* pair_j, const int64_t* pair_count, const int64_t* idx_a, const int64_t* idx_b,
                          int64_t* landmark_out, int64_t* n_landmark, int64_t* n_inconsistent) {
  if (n_frames < 0 || n_pairs < 0) return fail("bad sizes");
  std::vector<std::vector<int64_t>> map(n_frames);
  for (int f = 0; f < n_frames; ++f) {
    if (kp_count[f] < 0) return fail("bad kp_count");
    map[f].assign((size_t)kp_count[f], -1);
  }
  int64_t g = 0, warn = 0, off = 0;
  for (int64_t p = 0; p < n_pairs; ++p) {
    const int i = pair_i[p], j = pair_j[p];
    if (i < 0 || i >= n_frames || j < 0 || j >= n_frames) return fail("pair %lld: frame out of range", (long long)p);
    for (int64_t k = 0; k < pair_count[p]; ++k) {
      const int64_t a = idx_a[off + k], b = idx_b[off + k];
      if (a < 0 || a >= kp_count[i] || b < 0 || b >= kp_count[j]) return fail("pair %lld: keypoint index out of range", (long long)p);
      int64_t& ma = map[i][a];
      int64_t& mb = map[j][b];
      if (ma >= 0 && mb >= 0) {
        if (ma != mb) ++warn;
      } else if (ma >= 0) {
        mb = ma;
      } else if (mb >= 0) {
        ma = mb;
      } else {
        ma = g;
        mb = g;
        ++g;
      }
    }
    off += pair_count[p];
  }
  // landmark of each match = landmark_index_map[i][idx1] after all pairs (image_process.py:652-653)
  off = 0;
  for (int64_t p = 0; p < n_pairs; ++p) {
    for (int64_t k = 0; k < pair_count[p]; ++k) landmark_out[off + k] = map[pair_i[p]][idx_a[off + k]];
    off += pair_count[p];
  }
  *n_landmark = g;
  if (n_inconsistent) *n_inconsistent = warn;
  return 0;
}
