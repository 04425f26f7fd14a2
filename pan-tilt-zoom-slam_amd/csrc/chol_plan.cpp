// chol_plan.h: the system orders, the rank tree and the factorisation plan.
#include "chol_plan.h"

#include <algorithm>
#include <cmath>
#include <map>
#include <utility>

namespace ptzba {
static SysOrder natural_order(int n_pose, int nf) {
  SysOrder o;
  o.pos.assign(n_pose, -1);
  for (int f = nf; f < n_pose; ++f) o.pos[f] = 3 * (f - nf);
  o.n_aug = 3 * (n_pose - nf);
  o.pad.assign(o.n_aug, 0);
  return o;
}

// One level of nested dissection of the frame chain: A = [nf, m), separator C = [m, c_end) with
// c_end past every frame A couples to, B = [c_end, n_pose) (decoupled from A).  System order
// [A | B reversed | C], each part padded to whole tiles: A and B factor side by side, their couplings
// to C are eliminated last, and the back-substitution splits into two chains after C.  Chosen only when
// it shortens the critical path of tile columns.
static bool nested_order(int n_pose, int nf, const std::vector<int32_t>& win, SysOrder& o, bool force) {
  const int nfree = n_pose - nf;
  if (nfree < (force ? 3 : 16)) return false;
  std::vector<int> pmax(n_pose + 1, -1);
  for (int f = nf; f < n_pose; ++f) pmax[f + 1] = std::max(pmax[f], (int)win[f]);
  const int nat = pad_tile(3 * nfree + 1) / CHOL_NB;
  int best_m = -1, best = nat;
  for (int m = nf + 1; m < n_pose; ++m) {
    const int cend = std::max(m, pmax[m] + 1);
    if (cend >= n_pose) break;
    const int ta = pad_tile(3 * (m - nf)) / CHOL_NB, tb = pad_tile(3 * (n_pose - cend)) / CHOL_NB;
    const int tc = pad_tile(3 * (cend - m)) / CHOL_NB;
    const int chain = std::max(ta, tb) + tc + 1;
    if (chain < best) {
      best = chain;
      best_m = m;
    }
  }
  if (force) {  // testing: the most balanced split with a non-empty B, whatever the gain
    best_m = -1;
    int bal = INT32_MAX;
    for (int m = nf + 1; m < n_pose; ++m) {
      const int cend = std::max(m, pmax[m] + 1);
      if (cend >= n_pose) break;
      const int d = std::abs((m - nf) - (n_pose - cend));
      if (d < bal) { bal = d; best_m = m; }
    }
  }
  if (best_m < 0 || (!force && best + 2 > nat)) return false;
  const int m = best_m, cend = std::max(m, pmax[m] + 1);
  const int ar = 3 * (m - nf), br = 3 * (n_pose - cend), cr = 3 * (cend - m);
  const int ap = pad_tile(ar), bp = pad_tile(br), cp = pad_tile(cr);
  o.pos.assign(n_pose, -1);
  for (int f = nf; f < m; ++f) o.pos[f] = 3 * (f - nf);
  for (int f = n_pose - 1; f >= cend; --f) o.pos[f] = ap + 3 * (n_pose - 1 - f);
  for (int f = m; f < cend; ++f) o.pos[f] = ap + bp + 3 * (f - m);
  o.n_aug = ap + bp + cp;
  o.pad.assign(o.n_aug, 0);
  for (int r = ar; r < ap; ++r) o.pad[r] = 1;
  for (int r = ap + br; r < ap + bp; ++r) o.pad[r] = 1;
  for (int r = ap + bp + cr; r < o.n_aug; ++r) o.pad[r] = 1;
  o.nested = true;
  o.tiles_a = ap / CHOL_NB;
  o.tiles_b = bp / CHOL_NB;
  o.split_m = m;
  o.split_cend = cend;
  o.nd_depth = 1;
  const int c0 = o.tiles_a + o.tiles_b;
  o.nodes = {{c0, o.n_aug / CHOL_NB, -1, m, cend}, {0, o.tiles_a, 0, nf, m}, {o.tiles_a, c0, 0, cend, n_pose}};
  return true;
}

// Two levels of nested dissection (round 3): the top separator C2 = [m, cend) splits the chain into halves,
// each half is split again by its most balanced separator: A1 | C1 | A2 | C2 | A3 | C3 | A4.  System order
// [A1 | A2 | A3 | A4 reversed | C1 | C3 | C2], each part padded to whole tiles: the four leaves factor side by
// side, then C1 and C3, then C2 -- a critical path of max(leaf) + sub-separator + top separator tile columns
// instead of max(A, B) + C (config 3: 26 instead of 30 levels), and four back-substitution chains C2 -> C1 ->
// A1 / A2, C2 -> C3 -> A3 / A4.  A leaf couples only to its ancestors: A1 to C1, A2 to C1 and C2, A3 to C2
// and C3, A4 to C3 (and, where the window reaches that far, C2).  The top split minimises the estimated chain.
static bool nested_order2(int n_pose, int nf, const std::vector<int32_t>& win, SysOrder& o, bool halves = false) {
  if (n_pose - nf < 32) return false;
  std::vector<int> pmax(n_pose + 1, -1);
  for (int f = nf; f < n_pose; ++f) pmax[f + 1] = std::max(pmax[f], (int)win[f]);
  auto tiles = [](int a, int b) { return pad_tile(3 * (b - a)) / CHOL_NB; };
  // most balanced split of [lo, hi) by a separator [m1, c1) (running coupling max from lo); false if none
  auto balanced = [&](int lo, int hi, int& m1_out, int& c1_out) {
    int best = INT32_MAX, run = -1;
    for (int m1 = lo + 1; m1 < hi; ++m1) {
      run = std::max(run, (int)win[m1 - 1]);
      const int c1 = std::max(m1, run + 1);
      if (c1 >= hi) break;
      const int d = std::abs((m1 - lo) - (hi - c1));
      if (d < best) { best = d; m1_out = m1; c1_out = c1; }
    }
    return best != INT32_MAX;
  };
  int best = INT32_MAX, bm = -1, bc = -1, b1 = -1, bc1 = -1, b3 = -1, bc3 = -1;
  for (int m = nf + 2; m < n_pose - 1; ++m) {
    const int cend = std::max(m, pmax[m] + 1);
    if (cend >= n_pose - 1) break;
    int m1, c1, m3, c3;
    if (!balanced(nf, m, m1, c1) || !balanced(cend, n_pose, m3, c3)) continue;
    const int est = std::max(std::max(tiles(nf, m1), tiles(c1, m)) + tiles(m1, c1),
                             std::max(tiles(cend, m3), tiles(c3, n_pose)) + tiles(m3, c3)) + tiles(m, cend) + 1;
    if (est < best) { best = est; bm = m; bc = cend; b1 = m1; bc1 = c1; b3 = m3; bc3 = c3; }
  }
  if (bm < 0) return false;
  // parts in system order: {first frame, end frame, reversed}.  halves (part-owned multi-GPU solve): each half
  // contiguous, [A1 | A2 | C1 | A3 | A4 reversed | C3 | C2], so a rank group owns [A1 | A2 | C1] or [A3 | A4 | C3]
  // and C2 is the separator the groups exchange (the same dependencies, so the same levels)
  const int pa[7][3] = {{nf, b1, 0}, {bc1, bm, 0}, {bc, b3, 0}, {bc3, n_pose, 1}, {b1, bc1, 0}, {b3, bc3, 0}, {bm, bc, 0}};
  const int ph[7][3] = {{nf, b1, 0}, {bc1, bm, 0}, {b1, bc1, 0}, {bc, b3, 0}, {bc3, n_pose, 1}, {b3, bc3, 0}, {bm, bc, 0}};
  const int (*parts)[3] = halves ? ph : pa;
  o = SysOrder{};
  o.pos.assign(n_pose, -1);
  int row = 0, t[8];
  std::vector<std::pair<int, int>> pad_ranges;
  for (int p = 0; p < 7; ++p) {
    const int a = parts[p][0], b = parts[p][1], nr = 3 * (b - a);
    t[p] = row / CHOL_NB;
    for (int f = a; f < b; ++f) o.pos[f] = row + 3 * (parts[p][2] ? (b - 1 - f) : (f - a));
    pad_ranges.push_back({row + nr, row + pad_tile(nr)});
    row += pad_tile(nr);
  }
  t[7] = row / CHOL_NB;
  o.n_aug = row;
  o.pad.assign(o.n_aug, 0);
  for (auto& pr : pad_ranges)
    for (int r = pr.first; r < pr.second; ++r) o.pad[r] = 1;
  o.nested = true;
  o.nd_depth = 2;
  if (halves) {
    // nodes: 0 = C2 (root), 1 = C1, 2 = C3, 3..6 = A1..A4 (part-owned fields: the halves and C2's frames)
    o.nodes = {{t[6], t[7], -1, bm, bc}, {t[2], t[3], 0, b1, bc1}, {t[5], t[6], 0, b3, bc3},
               {t[0], t[1], 1, nf, b1}, {t[1], t[2], 1, bc1, bm}, {t[3], t[4], 2, bc, b3}, {t[4], t[5], 2, bc3, n_pose}};
    o.tiles_a = t[3];
    o.tiles_b = t[6] - t[3];
    o.split_m = bm;
    o.split_cend = bc;
    return true;
  }
  // nodes: 0 = C2 (root), 1 = C1, 2 = C3, 3..6 = A1..A4
  o.nodes = {{t[6], t[7], -1, bm, bc}, {t[4], t[5], 0, b1, bc1}, {t[5], t[6], 0, b3, bc3},
             {t[0], t[1], 1, nf, b1}, {t[1], t[2], 1, bc1, bm}, {t[2], t[3], 2, bc, b3}, {t[3], t[4], 2, bc3, n_pose}};
  return true;
}

bool dist_tree(const SysOrder& o, int world, DistTree& T) {
  const int nn = (int)o.nodes.size();
  if (nn < 3 || world < 2) return false;
  T.n.assign(nn, DistTree::N{});
  for (int v = 0; v < nn; ++v) {
    const auto& a = o.nodes[v];
    T.n[v] = DistTree::N{a.t0, a.t1, a.parent, a.f0, a.f1, a.t0, a.t1, a.f0, a.f1, {-1, -1}, 0, 0, 0, 0};
  }
  for (int v = 0; v < nn; ++v) {
    const int p = T.n[v].parent;
    if (p < 0) continue;
    if (T.n[p].nch >= 2) return false;
    T.n[p].child[T.n[p].nch++] = v;
  }
  T.depth = 0;
  for (int v = 0; v < nn; ++v) {
    for (int u = T.n[v].parent; u >= 0; u = T.n[u].parent) T.n[v].depth++;
    T.depth = std::max(T.depth, T.n[v].depth);
    for (int u = T.n[v].parent; u >= 0; u = T.n[u].parent) {  // extend the ancestors' subtree ranges
      T.n[u].st0 = std::min(T.n[u].st0, T.n[v].t0);
      T.n[u].st1 = std::max(T.n[u].st1, T.n[v].t1);
      T.n[u].sf0 = std::min(T.n[u].sf0, T.n[v].f0);
      T.n[u].sf1 = std::max(T.n[u].sf1, T.n[v].f1);
    }
  }
  for (int v = 0; v < nn; ++v) {
    auto& x = T.n[v];
    if (x.nch == 1) return false;
    if (x.nch == 2 && T.n[x.child[0]].sf0 > T.n[x.child[1]].sf0) std::swap(x.child[0], x.child[1]);
  }
  // contiguity of every subtree (columns and frames): the sum of its nodes' sizes fills its range
  for (int v = 0; v < nn; ++v) {
    int64_t cols = 0, frames = 0;
    for (int u = 0; u < nn; ++u) {
      bool in = false;
      for (int w = u; w >= 0; w = T.n[w].parent) in = in || w == v;
      if (in) { cols += T.n[u].t1 - T.n[u].t0; frames += T.n[u].f1 - T.n[u].f0; }
    }
    if (cols != T.n[v].st1 - T.n[v].st0 || frames != T.n[v].sf1 - T.n[v].sf0) return false;
  }
  std::vector<std::pair<int, std::pair<int, int>>> stack{{0, {0, world}}};
  while (!stack.empty()) {
    const int v = stack.back().first, r0 = stack.back().second.first, nr = stack.back().second.second;
    stack.pop_back();
    T.n[v].r0 = r0;
    T.n[v].nr = nr;
    if (T.n[v].nch == 2) {
      const int k = nr >= 2 ? (nr + 1) / 2 : 1;
      stack.push_back({T.n[v].child[0], {r0, k}});
      stack.push_back({T.n[v].child[1], nr >= 2 ? std::make_pair(r0 + k, nr - k) : std::make_pair(r0, 1)});
    }
  }
  return true;
}
int dist_base(const DistTree& T, int rank, std::vector<int>* anc) {
  int v = 0;
  while (T.n[v].nr >= 2 && T.n[v].nch == 2) {
    const auto& c = T.n[T.n[v].child[0]];
    v = (rank >= c.r0 && rank < c.r0 + c.nr) ? T.n[v].child[0] : T.n[v].child[1];
  }
  if (anc) {
    anc->clear();
    for (int u = T.n[v].parent; u >= 0; u = T.n[u].parent) anc->push_back(u);
  }
  return v;
}

// Steps of the blocked right-looking back substitution (k_chol_backsolve_blk).  The chains' common prefix
// (the separator C of a nested order) is cut into blocks of BSB_P consecutive positions solved one block
// per step; the chains' remainders (A and B) then advance in lockstep, one block of each per step.  A step
// solves its blocks (every workgroup redundantly) and applies their contribution to every later column t
// coupled to them (one workgroup per (block, t): a plain read-modify-write of r_t, as no two tasks of a
// step share a target and steps are stream-ordered).  First-touch flags make a column's first read take
// the forward-substitution result y (the factor's augmented row) instead of r, so r needs no init launch.
// phases: the separator tree's depths (root separator first), each a list of sequences (tile columns in
// back-substitution order) that advance in lockstep.
typedef std::vector<std::vector<std::vector<int>>> BsPhases;
static void make_bs_steps(const std::vector<std::vector<uint8_t>>& nz, int Tx, CholPlan& P, const BsPhases& phases) {
  P.bsb_tasks.clear();
  P.bsb_step_off.assign(1, 0);
  const int T = (int)nz.size(), nch = (int)P.chain_off.size() - 1;
  if (nch < 1) return;
  std::vector<uint8_t> in_any(T, 0), solved(T, 0), touched(T, 0);
  for (int kt : P.chain_cols) in_any[kt] = 1;
  auto fail = [&]() {
    P.bsb_tasks.clear();
    P.bsb_step_off.assign(1, 0);
  };
  for (const auto& seqs : phases) {
    size_t len = 0;
    for (const auto& q : seqs) len = std::max(len, q.size());
    for (size_t q0 = 0; q0 < len; q0 += BSB_P) {
      std::vector<uint8_t> used(T, 0);  // block columns and targets of this step
      std::vector<int> step_targets;
      for (const auto& q : seqs) {
        if (q0 >= q.size()) continue;
        const int p = (int)std::min<size_t>(BSB_P, q.size() - q0);
        int cols[BSB_P] = {-1, -1, -1, -1}, imask = 0, ftouch = 0;
        for (int k = 0; k < p; ++k) {
          cols[k] = q[q0 + k];
          if (used[cols[k]] || solved[cols[k]]) return fail();
          used[cols[k]] = 1;
          if (!touched[cols[k]]) ftouch |= 1 << k;
          for (int j = 0; j < k; ++j) {
            if (cols[j] <= cols[k]) return fail();  // descending within a block
            if (nz[cols[j]][cols[k]]) imask |= 1 << (j * 4 + k);
          }
        }
        auto push_task = [&](int t, int flags) {
          P.bsb_tasks.insert(P.bsb_tasks.end(), {cols[0], cols[1], cols[2], cols[3], p, imask, ftouch, 0, t, flags, 0, 0});
        };
        std::vector<int> tmask(T, 0);
        for (int k = 0; k < p; ++k)
          for (int t = 0; t < cols[k]; ++t)
            if (in_any[t] && nz[cols[k]][t] && !(t == cols[0] || t == cols[1] || t == cols[2] || t == cols[3]))
              tmask[t] |= 1 << k;
        bool first = true;
        for (int t = 0; t < T; ++t) {
          if (!tmask[t]) continue;
          if (used[t] || solved[t]) return fail();
          used[t] = 1;
          step_targets.push_back(t);
          push_task(t, tmask[t] | (first ? 0x100 : 0) | (touched[t] ? 0 : 0x200));
          first = false;
        }
        if (first) push_task(-1, 0x100);
        for (int k = 0; k < p; ++k) solved[cols[k]] = touched[cols[k]] = 1;
      }
      for (int t : step_targets) touched[t] = 1;
      P.bsb_step_off.push_back((int)(P.bsb_tasks.size() / 12));
    }
  }
  for (int kt = 0; kt < Tx; ++kt)
    if (in_any[kt] && !solved[kt]) return fail();
  // expected update counts for the persistent form: replay the steps in order
  const int nt = (int)(P.bsb_tasks.size() / 12);
  P.bsb_expect.assign(8 * (size_t)nt, 0);
  std::vector<int32_t> done(T, 0);
  for (size_t st = 0; st + 1 < P.bsb_step_off.size(); ++st) {
    for (int q = P.bsb_step_off[st]; q < P.bsb_step_off[st + 1]; ++q) {
      const int32_t* tk = &P.bsb_tasks[12 * (size_t)q];
      for (int k = 0; k < 4; ++k) P.bsb_expect[8 * (size_t)q + k] = tk[k] >= 0 ? done[tk[k]] : 0;
      P.bsb_expect[8 * (size_t)q + 4] = tk[8] >= 0 ? done[tk[8]] : 0;
    }
    for (int q = P.bsb_step_off[st]; q < P.bsb_step_off[st + 1]; ++q) {
      const int t = P.bsb_tasks[12 * (size_t)q + 8];
      if (t >= 0) done[t]++;
    }
  }
  P.bsb_tot = done;
}

// the lower tiles that coupled frame pairs touch (what the Schur kernels write, before fill)
typedef std::vector<std::vector<uint8_t>> TileMask;
static TileMask coupled_tiles(const SysOrder& o, int n_pose, int nf, const std::vector<int32_t>& win, int T) {
  TileMask nz(T, std::vector<uint8_t>(T, 0));
  auto mark = [&](int r, int c) {
    int ti = r / CHOL_NB, tj = c / CHOL_NB;
    if (ti < tj) std::swap(ti, tj);
    nz[ti][tj] = 1;
  };
  for (int f1 = nf; f1 < n_pose; ++f1)
    for (int f2 = f1; f2 <= std::min(n_pose - 1, (int)win[f1]); ++f2) {
      const int p1 = o.pos[f1], p2 = o.pos[f2];
      mark(p2, p1); mark(p2 + 2, p1); mark(p2, p1 + 2); mark(p2 + 2, p1 + 2);
    }
  return nz;
}
// adds the dense augmented row (tile row ta), the diagonal and the symbolic fill
static void fill_tiles(TileMask& nz, int ta) {
  const int T = (int)nz.size();
  for (int j = 0; j <= ta; ++j) nz[ta][j] = 1;
  for (int i = 0; i < T; ++i) nz[i][i] = 1;
  for (int k = 0; k < T; ++k) {
    std::vector<int> R;
    for (int i = k + 1; i < T; ++i)
      if (nz[i][k]) R.push_back(i);
    for (size_t x = 0; x < R.size(); ++x)
      for (size_t y = 0; y <= x; ++y) nz[R[x]][R[y]] = 1;
  }
}

// Tile structure (coupled frame pairs + the dense augmented row + symbolic fill), elimination levels
// (at most two tile columns per level), tasks per level and back-substitution chains.
// Rank-tree restriction of make_plan (make_plan_tree, §7): the tile columns this rank factors, phase by phase (each
// phase's columns depend only on the same phase's; a flush level closes every phase but the last and is always a
// trailing level, so it applies the phase's pending panels to the later phases' tiles), and the exactly-once rule:
// an update from phase q's panels into a later phase's tile (i, j) is kept only by group member (i + j) mod size.
struct TreeSpec {
  std::vector<int8_t> col_phase;  // [T] phase of each tile column, -1 not this rank's
  std::vector<int> ph_nr, ph_me;  // per phase: group size, this rank's index in the group
  std::vector<int> chain;         // back-substitution chain (the phases from the root down, columns descending)
  std::vector<int> ph_lv0, ph_lv1;  // out: per phase its levels [lv0, lv1) (the closing flush level included)
};
static int tile_owner(int i, int j, int nr) { return (i + j) % nr; }
// (Round 4's supercolumn plans -- two chain columns per level task, measured slower: 0.31 vs 0.23 ms at config 3 --
// were removed in round 6 with their kernel; DESIGN.md §4.3 keeps the record.)
static bool make_plan(const SysOrder& o, int n_pose, int nf, const std::vector<int32_t>& win, int64_t ld, CholPlan& P,
                      int force_dt = 0, TreeSpec* ts = nullptr) {
  const int T = (int)(ld / CHOL_NB);
  TileMask nz = coupled_tiles(o, n_pose, nf, win, T);
  P.xtiles.clear();
  for (int i = 0; i < T; ++i)
    for (int j = 0; j <= i; ++j)
      if (nz[i][j] || i == j) { P.xtiles.push_back(i); P.xtiles.push_back(j); }
  const int ta = o.n_aug / CHOL_NB;  // tile holding the augmented row
  fill_tiles(nz, ta);
  auto own = [&](int t) { return !ts || ts->col_phase[t] >= 0; };
  auto phase = [&](int t) { return ts ? (int)ts->col_phase[t] : 0; };
  if (ts)
    for (int k = 0; k < T; ++k)  // a column this rank eliminates couples only to rows it holds
      if (own(k))
        for (int i = k + 1; i < T; ++i)
          if (nz[i][k] && !own(i)) return false;
  std::vector<int> level(T, ts ? -1 : 0), count;
  std::vector<uint8_t> flush_lv;
  auto place = [&](int k, int L0) {
    int L = L0;
    for (int p = 0; p < k; ++p)
      if (nz[k][p] && level[p] >= 0 && phase(p) == phase(k)) L = std::max(L, level[p] + 1);
    while (L < (int)count.size() && count[L] >= 4) ++L;  // at most four columns per launch
    if (L >= (int)count.size()) count.resize(L + 1, 0);
    count[L]++;
    level[k] = L;
  };
  if (!ts) {
    for (int k = 0; k < T; ++k) place(k, 0);
  } else {
    const int NP = (int)ts->ph_nr.size();
    ts->ph_lv0.assign(NP, 0);
    ts->ph_lv1.assign(NP, 0);
    for (int q = 0; q < NP; ++q) {
      ts->ph_lv0[q] = (int)count.size();
      for (int k = 0; k < T; ++k)
        if (phase(k) == q) place(k, ts->ph_lv0[q]);
      if (q + 1 < NP) {
        count.push_back(0);
        flush_lv.resize(count.size(), 0);
        flush_lv.back() = 1;
      }
      ts->ph_lv1[q] = (int)count.size();
    }
  }
  flush_lv.resize(count.size(), 0);
  P.ztiles.clear();
  for (int i = 0; i < T; ++i)
    for (int j = 0; j <= i; ++j)
      if (nz[i][j] && own(i) && own(j)) { P.ztiles.push_back(i); P.ztiles.push_back(j); }
  int nL = (int)count.size();
  std::vector<std::vector<int>> K(nL);
  for (int k = 0; k < T; ++k)
    if (level[k] >= 0) K[level[k]].push_back(k);
  P.tasks.clear();
  P.level_off.assign(nL + 1, 0);
  auto push = [&](int type, int i, int j, int w) {
    P.tasks.push_back(type); P.tasks.push_back(i); P.tasks.push_back(j); P.tasks.push_back(w);
  };
  // inverses of the diagonal factor tiles (for the back-substitution): the tiles of level L-1's columns are
  // inverted by type-2 tasks of level L, beside its panels (off the critical path); the last level's after
  // the factorisation (tinv_tail).  Columns >= n_inv (the augmented-row tile) need none.
  const int n_inv = (o.n_aug + CHOL_NB - 1) / CHOL_NB;
  const bool tinv_split = true;  // (round 2 A/B: every inverse after the factorisation instead: +4 us per trial)
  P.tinv_tail.clear();
  // Delayed trailing updates (period DT): trailing tasks run only at levels L = 0 mod DT and apply the
  // panels of levels [L - DT, L - 1] at once (rank <= 2 DT x 32: half the read-modify-writes of the band's
  // tiles at DT = 2); a panel task applies inline every update not yet applied to its tiles, the panels of
  // levels [F, L - 1] with F the last trailing level before L.  Worth it when the levels are dominated by
  // their trailing tasks (config 4: ~1,600 per level), not when they are chain-bound (config 3).
  int64_t trail = 0;
  for (int p = 0; p < T; ++p) {
    if (!own(p)) continue;
    int64_t r = 0;
    for (int i = p + 1; i < T; ++i) r += nz[i][p] && own(i);
    trail += r * (r + 1) / 2;
  }
  int DT = trail > 600 * (int64_t)nL ? 2 : 1;
  if (const char* e = getenv("PTZBA_CHOL_DELAY")) DT = std::max(1, std::min(2, atoi(e)));  // A/B knob
  if (force_dt) DT = force_dt;
  P.delayed = DT > 1;
  size_t max_pd = 0;  // update panels of one task: the P2 kernel takes up to four (any DT), the other two
  bool any_block = false;  // 2 x 2 trailing blocks (type 3) run in the P2 kernel only
  auto pack2 = [](int type, const std::vector<int>& pd, int tm) {  // int4 task: x (type + panels 2, 3), w (0, 1)
    return std::make_pair(chol_pack_type(type, pd.size() > 2 ? pd[2] : -1, pd.size() > 3 ? pd[3] : -1, (tm >> 2) & 3),
                          chol_pack_updates(pd.size() > 0 ? pd[0] : -1, pd.size() > 1 ? pd[1] : -1, tm & 3));
  };
  // trailing levels: every DT-th, and (rank-tree plans) every phase's flush level; a trailing level applies the
  // panels of the levels since the previous trailing level, a panel task inline those since the last one before it
  int last_trailing = 0;
  for (int L = 0; L < nL; ++L) {
    P.level_off[L] = (int)(P.tasks.size() / 4);
    const std::vector<int> none;
    const std::vector<int>& prev = L > 0 ? K[L - 1] : none;
    const bool trailing = L % DT == 0 || flush_lv[L];
    std::vector<int> inl;  // panels applied inline by this level's panel tasks
    if (L > 0)
      for (int l = last_trailing; l < L; ++l) inl.insert(inl.end(), K[l].begin(), K[l].end());
    for (int k : K[L]) {
      std::vector<int> pd;
      for (int pp : inl)
        if (pp < k && nz[k][pp]) pd.push_back(pp);
      for (int i = k; i < T; ++i) {
        if (!nz[i][k] || !own(i)) continue;
        int tm = 0;
        for (size_t u = 0; u < pd.size(); ++u)
          if (i == k || nz[i][pd[u]]) tm |= 1 << u;
        const auto w = pack2(0, pd, tm);
        push(w.first, i, k, w.second);
      }
      max_pd = std::max(max_pd, pd.size());
    }
    // trailing updates from the panels of levels [L - DT, L - 1] into tiles of columns factored after L
    std::vector<std::pair<int64_t, int>> upd;  // (tile key, panel)
    if (trailing && L > 0)
      for (int l = last_trailing; l < L; ++l)
        for (int pp : K[l]) {
          std::vector<int> R;
          for (int i = pp + 1; i < T; ++i)
            if (nz[i][pp] && own(i)) R.push_back(i);
          for (size_t x = 0; x < R.size(); ++x)
            for (size_t y = 0; y <= x; ++y) {
              if (level[R[y]] <= L) continue;
              // rank tree: into a later phase's tile only by its owner in this phase's group (exactly once)
              if (ts && phase(R[y]) != phase(pp) &&
                  tile_owner(R[x], R[y], ts->ph_nr[phase(pp)]) != ts->ph_me[phase(pp)])
                continue;
              upd.push_back({(int64_t)R[x] * T + R[y], pp});
            }
        }
    if (trailing) last_trailing = L;
    std::sort(upd.begin(), upd.end());
    // per tile its panels (ascending); with delayed updates the tiles are grouped into 2 x 2 blocks
    // (rows 2a, 2a + 1 x columns 2b, 2b + 1): one type-3 task per block stages each panel's four row tiles
    // once for up to four output tiles (~6 tile loads per output tile instead of ~10).  A block's panel set
    // is the union of its tiles' sets (at most four); a panel a tile is not coupled to has a zero L tile
    // there, so its product adds exact zeros -- the same arithmetic, in the same panel order, as one task
    // per tile.  PTZBA_CHOL_BLOCKS=0: one task per tile (A/B knob).
    std::map<int64_t, std::pair<int, std::vector<int>>> blocks;  // block key -> (tile mask, panel union)
    std::vector<std::pair<int, int>> single;                      // tiles emitted one by one (key index)
    std::vector<std::pair<int64_t, std::vector<int>>> tiles_pd;
    for (size_t x = 0; x < upd.size();) {
      size_t y = x + 1;
      while (y < upd.size() && upd[y].first == upd[x].first) ++y;
      std::vector<int> pd;
      for (size_t u = x; u < y; ++u) pd.push_back(upd[u].second);
      max_pd = std::max(max_pd, pd.size());
      tiles_pd.push_back({upd[x].first, pd});
      x = y;
    }
    const bool blocked = !getenv_is("PTZBA_CHOL_BLOCKS", "0");
    std::vector<uint8_t> in_block(tiles_pd.size(), 0);
    if (blocked) {
      for (size_t q = 0; q < tiles_pd.size(); ++q) {
        const int i = (int)(tiles_pd[q].first / T), j = (int)(tiles_pd[q].first % T);
        auto& b = blocks[(int64_t)(i / 2) * T + j / 2];
        b.first |= 1 << (2 * (i & 1) + (j & 1));
        for (int pp : tiles_pd[q].second)
          if (std::find(b.second.begin(), b.second.end(), pp) == b.second.end()) b.second.push_back(pp);
      }
      for (size_t q = 0; q < tiles_pd.size(); ++q) {
        const int i = (int)(tiles_pd[q].first / T), j = (int)(tiles_pd[q].first % T);
        const auto& b = blocks[(int64_t)(i / 2) * T + j / 2];
        in_block[q] = b.second.size() <= 4 && __builtin_popcount(b.first) >= 2;
      }
      for (auto& kv : blocks) {
        if (kv.second.second.size() > 4 || __builtin_popcount(kv.second.first) < 2) continue;
        std::vector<int> pd = kv.second.second;
        std::sort(pd.begin(), pd.end());
        const int a = (int)(kv.first / T), bcol = (int)(kv.first % T), mask = kv.second.first;
        push(chol_pack_type(3, pd.size() > 2 ? pd[2] : -1, pd.size() > 3 ? pd[3] : -1, (mask >> 2) & 3), 2 * a, 2 * bcol,
             chol_pack_updates(pd.size() > 0 ? pd[0] : -1, pd.size() > 1 ? pd[1] : -1, mask & 3));
        any_block = true;
      }
    }
    for (size_t q = 0; q < tiles_pd.size(); ++q) {
      if (in_block[q]) continue;
      const int i = (int)(tiles_pd[q].first / T), j = (int)(tiles_pd[q].first % T);
      const auto w = pack2(1, tiles_pd[q].second, 15);
      push(w.first, i, j, w.second);
    }
    // type 2: inverses of the previous level's diagonal tiles
    for (int pp : prev)
      if (tinv_split && pp < n_inv) push(2, pp, pp, 0);
  }
  for (int k = 0; k < n_inv && k < T; ++k)
    if (own(k) && (!tinv_split || level[k] == nL - 1)) P.tinv_tail.push_back(k);
  P.level_off[nL] = (int)(P.tasks.size() / 4);
  P.n_levels = nL;
  if (max_pd > 4) {  // too many panels for one task: DT = 1
    if (DT > 1) return make_plan(o, n_pose, nf, win, ld, P, 1, ts);
    return false;
  }
  if (max_pd > 2 || any_block) P.delayed = true;  // the P2 kernel (second panel pair, trailing blocks)
  // back-substitution: chains of tile columns holding unknowns and, per chain position, the chain's
  // later columns coupled to that row tile (right-looking updates).  Nested orders: one chain per leaf of
  // the separator tree (its root-to-leaf path, each node's columns descending); natural: one chain.
  const int Tx = (o.n_aug + CHOL_NB - 1) / CHOL_NB;
  P.chain_off.assign(1, 0);
  P.chain_cols.clear();
  BsPhases phases;
  if (ts) {  // rank tree: one chain, the phases from the root down
    P.chain_cols = ts->chain;
    P.chain_off.push_back((int)P.chain_cols.size());
    phases.push_back({P.chain_cols});
  } else if (o.nested && !o.nodes.empty()) {
    const int nn = (int)o.nodes.size();
    std::vector<int> depth(nn, 0), nchild(nn, 0);
    for (int v = 0; v < nn; ++v) {
      for (int u = o.nodes[v].parent; u >= 0; u = o.nodes[u].parent) ++depth[v];
      if (o.nodes[v].parent >= 0) ++nchild[o.nodes[v].parent];
    }
    auto desc = [&](int v) {
      std::vector<int> c;
      for (int kt = o.nodes[v].t1 - 1; kt >= o.nodes[v].t0; --kt) c.push_back(kt);
      return c;
    };
    for (int v = 0; v < nn; ++v) {
      if (nchild[v]) continue;  // leaf: the path root -> v
      std::vector<int> path;
      for (int u = v; u >= 0; u = o.nodes[u].parent) path.push_back(u);
      for (auto it = path.rbegin(); it != path.rend(); ++it)
        for (int kt : desc(*it)) P.chain_cols.push_back(kt);
      P.chain_off.push_back((int)P.chain_cols.size());
    }
    for (int v = 0; v < nn; ++v) {
      if ((int)phases.size() <= depth[v]) phases.resize(depth[v] + 1);
      phases[depth[v]].push_back(desc(v));
    }
    // every coupling of a chain column to a later column stays inside the chain (a leaf couples only to its
    // ancestors); otherwise this order is unusable
    for (size_t ch = 0; ch + 1 < P.chain_off.size(); ++ch) {
      std::vector<uint8_t> in_chain(T, 0);
      for (int q = P.chain_off[ch]; q < P.chain_off[ch + 1]; ++q) in_chain[P.chain_cols[q]] = 1;
      for (int q = P.chain_off[ch]; q < P.chain_off[ch + 1]; ++q)
        for (int i = P.chain_cols[q] + 1; i < Tx; ++i)
          if (nz[i][P.chain_cols[q]] && !in_chain[i]) return false;
    }
  } else {
    for (int kt = Tx - 1; kt >= 0; --kt) P.chain_cols.push_back(kt);
    P.chain_off.push_back((int)P.chain_cols.size());
    phases.push_back({P.chain_cols});
  }
  P.upd_off.assign(1, 0);
  P.upd_tiles.clear();
  P.lo_off.assign(1, 0);
  P.lo_tiles.clear();
  for (size_t ch = 0; ch + 1 < P.chain_off.size(); ++ch) {
    std::vector<uint8_t> in_chain(T, 0);
    for (int q = P.chain_off[ch]; q < P.chain_off[ch + 1]; ++q) in_chain[P.chain_cols[q]] = 1;
    for (int q = P.chain_off[ch]; q < P.chain_off[ch + 1]; ++q) {
      const int kt = P.chain_cols[q];
      for (int j = 0; j < kt; ++j)
        if (in_chain[j] && nz[kt][j]) P.upd_tiles.push_back(j);
      P.upd_off.push_back((int)P.upd_tiles.size());
      for (int i = kt + 1; i < Tx; ++i)
        if (in_chain[i] && nz[i][kt]) P.lo_tiles.push_back(i);
      P.lo_off.push_back((int)P.lo_tiles.size());
    }
  }
  // lookahead back substitution: the next position's tile when the current row couples to it, and per
  // (chain, helper wave) the other updates (position, tile j with j % BS_HELPERS == helper) in order
  const int npos = (int)P.chain_cols.size(), nch = (int)P.chain_off.size() - 1;
  std::vector<int> la(npos, -1), toff(1, 0), tasks;
  for (int ch = 0; ch < nch; ++ch)
    for (int q = P.chain_off[ch]; q + 1 < P.chain_off[ch + 1]; ++q)
      for (int e = P.upd_off[q]; e < P.upd_off[q + 1]; ++e)
        if (P.upd_tiles[e] == P.chain_cols[q + 1]) la[q] = P.chain_cols[q + 1];
  for (int ch = 0; ch < nch; ++ch)
    for (int hw = 0; hw < BS_HELPERS; ++hw) {
      for (int q = P.chain_off[ch]; q < P.chain_off[ch + 1]; ++q)
        for (int e = P.upd_off[q]; e < P.upd_off[q + 1]; ++e) {
          const int j = P.upd_tiles[e];
          if (j % BS_HELPERS == hw && j != la[q]) tasks.push_back((q << 16) | j);
        }
      toff.push_back((int)tasks.size());
    }
  P.n_tasks = (int)tasks.size();
  P.la_tasks = la;
  P.la_tasks.insert(P.la_tasks.end(), toff.begin(), toff.end());
  P.la_tasks.insert(P.la_tasks.end(), tasks.begin(), tasks.end());
  make_bs_steps(nz, Tx, P, phases);
  return true;
}

// estimated factorisation time of a plan: per level the longer of the pivot chain (~7 us) and its tasks in
// rounds of the chip (~768 resident workgroups, ~6 us a round) -- fewer levels only pay when the extra fill
// and the wider levels do not turn them into throughput-bound ones (config 4: the two-level order has 189
// levels instead of 265 but up to 18K tasks per level, 7.9 vs 4.7 ms per trial)
double plan_est_us(const CholPlan& P) {
  double t = 0;
  for (int L = 0; L < P.n_levels; ++L) {
    const int n = P.level_off[L + 1] - P.level_off[L];
    t += std::max(7.0, 6.0 * ((n + 767) / 768));
  }
  return t;
}

int choose_order_plan(int n_pose, int nf, const std::vector<int32_t>& win, int ordering, SysOrder& so,
                             CholPlan& plan) {
  if (!(ordering != PTZBA_ORDER_NATURAL && nested_order(n_pose, nf, win, so, ordering == PTZBA_ORDER_NESTED_FORCE)))
    so = natural_order(n_pose, nf);
  if (!make_plan(so, n_pose, nf, win, pad_tile(so.n_aug + 1), plan)) return -1;
  const char* nde = getenv("PTZBA_ND_DEPTH");
  const int nd_env = nde ? atoi(nde) : 0;
  SysOrder s2;
  CholPlan p2;
  if (ordering == PTZBA_ORDER_NESTED && nd_env != 1 && nested_order2(n_pose, nf, win, s2) &&
      pad_tile(s2.n_aug + 1) <= CHOL_MAX_LD && make_plan(s2, n_pose, nf, win, pad_tile(s2.n_aug + 1), p2) &&
      ((p2.n_levels < plan.n_levels && plan_est_us(p2) < plan_est_us(plan)) || nd_env == 2)) {
    so = std::move(s2);
    plan = std::move(p2);
  }
  return 0;
}

bool make_plan_tree(const SysOrder& o, const DistTree& DT, int rank, int n_pose, int nf,
                           const std::vector<int32_t>& win, int64_t ld, CholPlan& P, TreePlan& Q) {
  const int T = (int)(ld / CHOL_NB), taug = o.n_aug / CHOL_NB;
  std::vector<int> anc;
  Q.base = dist_base(DT, rank, &anc);
  const auto& bn = DT.n[Q.base];
  const bool shared = bn.nr >= 2;
  Q.ph.clear();
  {
    TreePhase p0;
    p0.kind = PTZBA_X_PART;
    p0.node = Q.base;
    p0.r0 = shared ? bn.r0 : rank;
    p0.nr = shared ? bn.nr : 1;
    p0.depth = bn.depth;
    p0.c0 = shared ? bn.t0 : bn.st0;
    p0.c1 = shared ? bn.t1 : bn.st1;
    Q.ph.push_back(p0);
  }
  for (int u : anc) {
    TreePhase p;
    p.kind = DT.n[u].parent < 0 ? PTZBA_X_SEP : PTZBA_X_SUB;
    p.node = u;
    p.r0 = DT.n[u].r0;
    p.nr = DT.n[u].nr;
    p.depth = DT.n[u].depth;
    p.c0 = DT.n[u].t0;
    p.c1 = DT.n[u].parent < 0 ? T : DT.n[u].t1;  // the root's phase takes the augmented column too
    Q.ph.push_back(p);
  }
  const int NP = (int)Q.ph.size();
  if (Q.ph.back().c1 != T || taug != T - 1) return false;
  Q.col_phase.assign(T, -1);
  for (int q = 0; q < NP; ++q)
    for (int t = Q.ph[q].c0; t < Q.ph[q].c1; ++t) Q.col_phase[t] = (int8_t)q;
  auto own = [&](int t) { return Q.col_phase[t] >= 0; };
  TileMask nz = coupled_tiles(o, n_pose, nf, win, T);
  if (shared)  // a shared leaf's columns as the Schur kernels write them (before fill), summed before phase 0
    for (int j = Q.ph[0].c0; j < Q.ph[0].c1; ++j)
      for (int i = j; i < T; ++i)
        if ((nz[i][j] || i == j) && own(i)) { Q.ph[0].xt.push_back(i); Q.ph[0].xt.push_back(j); }
  fill_tiles(nz, taug);  // (global: every rank's columns)
  for (int q = 1; q < NP; ++q)  // an ancestor's columns (its rows and the later phases' rows, the augmented row)
    for (int j = Q.ph[q].c0; j < std::min(Q.ph[q].c1, taug); ++j)
      for (int i = j; i < T; ++i)
        if (nz[i][j] && own(i)) { Q.ph[q].xt.push_back(i); Q.ph[q].xt.push_back(j); }
  for (int q = 0; q < NP; ++q) {
    const int64_t r0 = (int64_t)Q.ph[q].c0 * CHOL_NB, r1 = std::min<int64_t>((int64_t)Q.ph[q].c1 * CHOL_NB, o.n_aug);
    const int64_t cnt = std::max<int64_t>(r1 - r0, 0);
    if (q == 0)
      Q.ph[q].vr = VecRanges{{r0, ld + r0, 2 * ld + r0}, {cnt, cnt, cnt}, 3};  // b | g | dU of the shared leaf
    else
      Q.ph[q].vr = VecRanges{{ld + r0, 2 * ld + r0, 0}, {cnt, cnt, 0}, 2};  // g | dU (b rides in the augmented row)
  }
  // the factorisation tasks: make_plan restricted to this rank's phases (delayed trailing updates and 2 x 2
  // trailing blocks included), the exactly-once rule on the later phases' tiles
  TreeSpec ts;
  ts.col_phase = Q.col_phase;
  for (const auto& ph : Q.ph) {
    ts.ph_nr.push_back(ph.nr);
    ts.ph_me.push_back(rank - ph.r0);
  }
  const int n_inv = (o.n_aug + CHOL_NB - 1) / CHOL_NB;
  for (int q = NP - 1; q >= 0; --q)
    for (int kt = std::min(Q.ph[q].c1, n_inv) - 1; kt >= Q.ph[q].c0; --kt) ts.chain.push_back(kt);
  if (!make_plan(o, n_pose, nf, win, ld, P, 0, &ts)) return false;
  for (int q = 0; q < NP; ++q) {
    Q.ph[q].lv0 = ts.ph_lv0[q];
    Q.ph[q].lv1 = ts.ph_lv1[q];
  }
  P.xtiles = Q.ph[0].xt;
  return true;
}

// The order of a part-owned solve: one dissection level (nested_order's choice when it shortens the critical path,
// else its most balanced split) or the two-level order with contiguous halves, whichever gives the slowest rank the
// shorter estimated factorisation (PTZBA_ND_DEPTH=1 keeps one level); false when the chain has no split.  A pure
// function of the coupling window and the world size, so ptzba_partition_landmarks and every rank's set_problem agree.
bool dist_order(int n_pose, int nf, const std::vector<int32_t>& win, int world, SysOrder& o) {
  if (!(nested_order(n_pose, nf, win, o, false) || nested_order(n_pose, nf, win, o, true))) return false;
  if (getenv_is("PTZBA_ND_DEPTH", "1")) return true;
  SysOrder o2;
  if (!nested_order2(n_pose, nf, win, o2, true) || pad_tile(o2.n_aug + 1) > CHOL_MAX_LD) return true;
  double e[2] = {0, 0};
  const SysOrder* os[2] = {&o, &o2};
  for (int v = 0; v < 2; ++v) {
    DistTree DT;
    if (!dist_tree(*os[v], world, DT)) {
      if (v == 0) return false;
      return true;
    }
    for (int r = 0; r < world; ++r) {
      // ranks sharing a base have the same plan shape: one per base
      if (r > 0 && dist_base(DT, r) == dist_base(DT, r - 1)) continue;
      CholPlan P;
      TreePlan Q;
      if (!make_plan_tree(*os[v], DT, r, n_pose, nf, win, pad_tile(os[v]->n_aug + 1), P, Q)) {
        if (v == 0) return false;
        return true;
      }
      e[v] = std::max(e[v], plan_est_us(P));
    }
  }
  if (e[1] < e[0]) o = std::move(o2);
  return true;
}

}  // namespace ptzba
