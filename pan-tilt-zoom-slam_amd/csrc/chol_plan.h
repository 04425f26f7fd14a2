// System order of the reduced camera system, the rank tree of a part-owned solve and the tile-level factorisation
// plan with its back-solve schedules: host-only combinatorics (no HIP call, no device code).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/ptzba.h"
#include "ptzba_kernels.h"

namespace ptzba {
inline int pad_tile(int x) { return (x + CHOL_NB - 1) / CHOL_NB * CHOL_NB; }
inline bool getenv_is(const char* name, const char* value) {
  const char* e = getenv(name);
  return e && std::string(e) == value;
}

struct SysOrder {
  std::vector<int32_t> pos;  // [n_pose] system row of the frame's pan (-1: fixed)
  std::vector<uint8_t> pad;  // [n_aug] identity padding rows
  int n_aug = 0;
  bool nested = false;
  int tiles_a = 0, tiles_b = 0;  // nested: tile columns of parts A and B (C follows)
  int split_m = 0, split_cend = 0;  // nested: A = [nf, m), C = [m, c_end), B = [c_end, n_pose)
  // separator tree of a nested order (tile-column ranges [t0, t1); parent -1 = the root separator): the
  // back-substitution chains are its root-to-leaf paths, the blocked back-solve's phases its depths
  struct Node { int t0, t1, parent, f0, f1; };  // (+ the node's frames [f0, f1))
  std::vector<Node> nodes;
  int nd_depth = 0;  // 0 natural, 1 = [A | B reversed | C], 2 = two dissection levels (nested_order2)
};

// Rank tree of a part-owned (multi-GPU) solve (round 4).  The separator tree of a nested order (one or two
// dissection levels) with the world's ranks dealt over it: a node with R >= 2 ranks gives ceil(R / 2) of them to its
// lower-frame child and the rest to the other; a node reached with one rank is that rank's OWN subtree; a leaf
// reached with R >= 2 ranks is SHARED by them.  A rank's phases: its base (own subtree, or shared leaf), then each
// ancestor separator up to the root.  Every subtree's tile columns and frames are contiguous in the orders used.
struct DistTree {
  struct N {
    int t0, t1, parent, f0, f1;  // separator / leaf columns and frames (SysOrder::Node)
    int st0, st1, sf0, sf1;      // the subtree's columns and frames
    int child[2], nch, depth;
    int r0, nr;                  // ranks [r0, r0 + nr) below this node
  };
  std::vector<N> n;
  int depth = 0;  // deepest node
};
bool dist_tree(const SysOrder& o, int world, DistTree& T);
// a rank's base node (own subtree: nr == 1; shared leaf: nr >= 2) and its ancestors, bottom-up
int dist_base(const DistTree& T, int rank, std::vector<int>* anc = nullptr);

struct CholPlan {
  std::vector<int32_t> tasks;  // int4 records
  std::vector<int> level_off;
  std::vector<int> chain_off, chain_cols, upd_off, upd_tiles;
  std::vector<int> la_tasks;  // lookahead back substitution: la [npos] | task_off [n_chain * BS_HELPERS + 1] | tasks
  int n_tasks = 0;
  std::vector<int> lo_off, lo_tiles;  // left-looking back substitution: per position the solved row tiles coupled to it
  std::vector<int32_t> xtiles;  // (ti, tj) pairs the Schur kernel can write (before fill), for the exchange
  std::vector<int32_t> ztiles;  // (ti, tj) lower tiles of the factor's pattern (incl. fill): zeroed per build
  std::vector<int32_t> tinv_tail;  // diagonal tiles inverted after the last level (the others: type-2 tasks)
  int n_levels = 0;
  bool delayed = false;  // tasks carry a second pair of update panels (delayed trailing updates, make_plan)
  // blocked back substitution (large systems): tasks of 3 int4 (block columns | {p, intra-block coupling
  // bits, first-touch bits, 0} | {target column, flags, 0, 0}) and the task offset of each step (one launch
  // per step); empty when no valid schedule exists
  std::vector<int32_t> bsb_tasks;
  std::vector<int> bsb_step_off;
  // persistent form (k_chol_backsolve_pst): per task the updates its block columns / target have received before
  // its step, {E_c0, E_c1, E_c2, E_c3, E_t, 0, 0, 0}, and per column the updates one solve applies to it
  std::vector<int32_t> bsb_expect, bsb_tot;
};

// estimated factorisation time of a plan (us)
double plan_est_us(const CholPlan& P);
// System order and plan of a single-system solve: natural, or the one-level nested order, or two dissection
// levels when that plan has fewer levels (PTZBA_ND_DEPTH=1 / =2: A/B knob, one level only / two levels
// whenever valid).  Returns nonzero if no plan exists.
int choose_order_plan(int n_pose, int nf, const std::vector<int32_t>& win, int ordering, SysOrder& so, CholPlan& plan);

// Rank-tree plan of a part-owned (multi-GPU) solve (api: ptzba_partition_landmarks, round 4).  A rank factors the
// tile columns of its phases in order -- its base (own subtree, or shared leaf), then each ancestor separator, the
// root's with the augmented column -- each phase closed by a flush level that applies its last panels to the later
// phases' tiles.  Between phases the library sums the next phase's columns over that node's rank group (X_SUB for an
// inner separator, X_SEP for the root; a shared leaf's columns before the first phase, X_PART), so a phase always
// starts from the complete sums of its columns.  Exactly-once rule: an update from a phase's panels into a LATER
// phase's tile is applied by one rank of the phase's group only -- tile (i, j) by group member (i + j) mod size --
// and the later exchange sums the members' tiles; inside the phase every member applies everything (they all factor
// the phase).  Each member's own Schur partials enter the sum once, as they are.  So the work on the separators'
// Schur complements is split over the group, not replicated.  Tasks, update rules and the panel packing are
// make_plan's (at most two columns per level, no delayed updates).
struct TreePhase {
  int lv0 = 0, lv1 = 0;      // factorisation levels [lv0, lv1) (incl. the closing flush level)
  int kind = PTZBA_X_PART;   // exchange BEFORE this phase (phase 0: X_PART when shared; later: X_SUB / X_SEP)
  int node = -1, r0 = 0, nr = 1, depth = 0;
  int c0 = 0, c1 = 0;        // tile columns
  std::vector<int32_t> xt;   // exchanged tiles (ti, tj) (phase 0: only when shared)
  VecRanges vr{};            // exchanged vector ranges of [b | g | dU]
};
struct TreePlan {
  std::vector<TreePhase> ph;
  std::vector<int8_t> col_phase;  // [T] phase of each tile column, -1 not this rank's
  int base = -1;
};
bool make_plan_tree(const SysOrder& o, const DistTree& DT, int rank, int n_pose, int nf, const std::vector<int32_t>& win,
                    int64_t ld, CholPlan& P, TreePlan& Q);
// The split of a part-owned (multi-GPU) solve: nested_order's choice when it shortens the critical path,
// else its most balanced split; false when none exists (every frame couples to the last one).  A pure
// function of the coupling window, so ptzba_partition_landmarks and every rank's set_problem agree.
bool dist_order(int n_pose, int nf, const std::vector<int32_t>& win, int world, SysOrder& o);

}  // namespace ptzba
