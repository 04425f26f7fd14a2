// `make host-check`: runs the host-only planner (chol_plan.cpp) and record layout (problem_layout.cpp) under
// AddressSanitizer / UBSan on synthetic inputs (fixed seed, no file input) and checks the structural invariants their
// comments state: indices in range, offsets monotone.  A CPU program; never loaded into Python, never run on a GPU.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>

#include "chol_plan.h"
#include "problem_layout.h"

using namespace ptzba;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("host-check: %s fails (line %d)\n", #c, __LINE__); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

template <typename V>
static void check_offsets(const V& off, size_t end) {  // a CSR offset list: starts at 0, monotone, ends at `end`
  CHECK(!off.empty() && off.front() == 0 && (size_t)off.back() == end);
  for (size_t k = 1; k < off.size(); ++k) CHECK(off[k - 1] <= off[k]);
}
template <typename V>
static void check_range(const V& v, int64_t lo, int64_t hi) {  // every entry in [lo, hi)
  for (auto x : v) CHECK(x >= lo && x < hi);
}

static void check_plan(const SysOrder& o, const CholPlan& P, int n_pose, int nf) {
  const int T = pad_tile(o.n_aug + 1) / CHOL_NB;
  CHECK((int)o.pos.size() == n_pose && (int)o.pad.size() == o.n_aug);
  for (int f = 0; f < n_pose; ++f) CHECK(f < nf ? o.pos[f] == -1 : (o.pos[f] >= 0 && o.pos[f] + 3 <= o.n_aug));
  CHECK(P.n_levels + 1 == (int)P.level_off.size());
  check_offsets(P.level_off, P.tasks.size() / 4);
  for (size_t q = 0; q < P.tasks.size(); q += 4) CHECK(P.tasks[q + 1] >= 0 && P.tasks[q + 1] < T && P.tasks[q + 2] >= 0 && P.tasks[q + 2] < T);
  check_range(P.xtiles, 0, T);
  check_range(P.ztiles, 0, T);
  check_range(P.tinv_tail, 0, T);
  check_range(P.chain_cols, 0, T);
  check_range(P.upd_tiles, 0, T);
  check_range(P.lo_tiles, 0, T);
  check_offsets(P.chain_off, P.chain_cols.size());
  check_offsets(P.upd_off, P.upd_tiles.size());
  check_offsets(P.lo_off, P.lo_tiles.size());
  check_offsets(P.bsb_step_off, P.bsb_tasks.size() / 12);
  for (size_t q = 0; q < P.bsb_tasks.size(); q += 12) {
    for (int k = 0; k < 4; ++k) CHECK(P.bsb_tasks[q + k] >= -1 && P.bsb_tasks[q + k] < T);
    CHECK(P.bsb_tasks[q + 4] >= 1 && P.bsb_tasks[q + 4] <= BSB_P && P.bsb_tasks[q + 8] >= -1 && P.bsb_tasks[q + 8] < T);
  }
  if (!P.bsb_tasks.empty()) CHECK(P.bsb_expect.size() == 8 * (P.bsb_tasks.size() / 12) && (int)P.bsb_tot.size() == T);
}

static void check_layout(const ProblemLayout& L, int n_pose, int n_lm, int64_t n, const int32_t* fr, const int32_t* lm) {
  const int64_t ns = (int64_t)L.seg_frame.size();
  CHECK((int64_t)L.order.size() == n && (int64_t)L.rec_seg.size() == n && (int64_t)L.seg_lm.size() == ns);
  for (int64_t k = 0; k < n; ++k) {  // (landmark, frame, index) order; each record in its segment
    const int64_t r = L.order[k], s = L.rec_seg[k];
    CHECK(r >= 0 && r < n && s >= 0 && s < ns && L.seg_lm[s] == lm[r] && L.seg_frame[s] == fr[r]);
    if (k) CHECK(lm[L.order[k - 1]] < lm[r] || (lm[L.order[k - 1]] == lm[r] && (fr[L.order[k - 1]] < fr[r] || (fr[L.order[k - 1]] == fr[r] && L.order[k - 1] < r))));
  }
  check_offsets(L.seg_rec_begin, n);
  check_offsets(L.lm_seg_begin, ns);
  check_offsets(L.frame_seg_begin, ns);
  CHECK((int)L.lm_seg_begin.size() == n_lm + 1 && (int)L.frame_seg_begin.size() == n_pose + 1);
  check_range(L.frame_seg_list, 0, ns);
  for (int f = 0; f < n_pose; ++f) CHECK(L.frame_win_hi[f] >= f && L.frame_win_hi[f] < n_pose);
  check_range(L.lm_work, 0, std::max<int64_t>({n + 1, ns + 1, n_lm, n_pose, L.n_slot}));
  CHECK(L.lm_work.size() == 8 * (size_t)L.n_work && L.n_work <= n_lm && L.s2_lm.size() % 4 == 0);
  for (size_t q = 0; q < L.s2_items.size(); q += 4) CHECK(L.s2_items[q + 2] >= 0 && L.s2_items[q + 2] < L.s2_items[q + 3] && L.s2_items[q + 3] <= (int)(L.s2_lm.size() / 4));
  for (size_t g = 0; g < L.s2_groups.size(); g += 4) CHECK(L.s2_groups[g + 2] >= 0 && L.s2_groups[g + 2] < L.s2_groups[g + 3] && L.s2_groups[g + 3] <= (int)(L.s2_items.size() / 4));
  for (size_t q = 0; q < L.s2_lm.size(); q += 4) CHECK(L.s2_lm[q] >= 0 && L.s2_lm[q] < n_lm && L.s2_lm[q + 3] >= 0 && L.s2_lm[q + 3] + L.s2_lm[q + 2] - L.s2_lm[q + 1] < L.n_slot);
}

// K1's merged stream against a sequential statement of the run rule: a run starts at a segment's first record and
// wherever the stored record (delta pair in the record precision, weight) differs in a bit from the one before
template <typename real>
static void check_merge(const ProblemLayout& L, int64_t n, const double* xy, const double* w) {
  const int64_t ns = (int64_t)L.seg_frame.size();
  std::vector<int64_t> first;
  auto bits_differ = [](real a, real b) { return std::memcmp(&a, &b, sizeof(real)) != 0; };
  for (int64_t k = 0; k < n; ++k) {
    const int64_t s = L.rec_seg[k], b = L.order[L.seg_rec_begin[s]], r = L.order[k];
    bool start = k == L.seg_rec_begin[s];
    if (!start) {
      const int64_t q = L.order[k - 1];
      start = bits_differ((real)(xy[2 * r] - xy[2 * b]), (real)(xy[2 * q] - xy[2 * b])) ||
              bits_differ((real)(xy[2 * r + 1] - xy[2 * b + 1]), (real)(xy[2 * q + 1] - xy[2 * b + 1])) ||
              (w && bits_differ((real)w[r], (real)w[q]));
    }
    if (start) first.push_back(k);
  }
  CHECK(L.n_merged == (int64_t)first.size() && L.k1_merged == (n > 0 && 2 * L.n_merged <= n));
  CHECK((int64_t)L.m_first.size() == L.n_merged + 1 && L.m_first.back() == n && (int64_t)L.m_seg_rec_begin.size() == ns + 1);
  for (int64_t m = 0; m < L.n_merged; ++m) CHECK(L.m_first[m] == first[m]);
  check_offsets(L.m_seg_rec_begin, (size_t)L.n_merged);
  for (int64_t s = 0; s < ns; ++s) CHECK(L.m_first[L.m_seg_rec_begin[s]] == L.seg_rec_begin[s]);
}

static void run_layout(int n_pose, int n_lm, const std::vector<int32_t>& fr, const std::vector<int32_t>& lm,
                       const std::vector<double>& xy = {}, const std::vector<double>& w = {}) {
  ProblemLayout A[2];
  const int64_t n = (int64_t)fr.size();
  for (int v = 0; v < 2; ++v) {  // the single-thread passes, then the threaded ones over four chunks
    ProblemLayout& L = A[v];
    layout_host_sort(L, n_pose, n_lm, n, fr.data(), lm.data(), v ? 4 : 1);
    CHECK(!layout_host_segments(L, n_lm, n, fr.data(), lm.data(), v ? 4 : 1));
    layout_frame_csr(L, n_pose, v != 0, v ? 4 : 1);
    CHECK(!layout_k2(L, n_pose, n_lm, 1));
    layout_k1_order(L, n_pose, n_lm);
    check_layout(L, n_pose, n_lm, n, fr.data(), lm.data());
    CHECK(L.lm_work_m.empty());
    if (xy.empty()) continue;
    for (int fp32 = 0; fp32 < 2; ++fp32)
      for (int wt = 0; wt < 2; ++wt) {  // both record precisions, without and with user weights
        const double* pw = wt ? w.data() : nullptr;
        std::vector<double> sb, x64(2 * n), w64(n);
        std::vector<float> x32(2 * n), w32(n);
        if (fp32) {
          layout_convert_records<float>(L, n, xy.data(), pw, sb, x32.data(), w32.data());
          layout_host_merge(L, n, x32.data(), pw ? w32.data() : nullptr, true, v ? 4 : 1, true);
        } else {
          layout_convert_records<double>(L, n, xy.data(), pw, sb, x64.data(), w64.data());
          layout_host_merge(L, n, x64.data(), pw ? w64.data() : nullptr, false, v ? 4 : 1, true);
        }
        if (fp32) check_merge<float>(L, n, xy.data(), pw);
        else check_merge<double>(L, n, xy.data(), pw);
        layout_k1_order(L, n_pose, n_lm);
        if (L.k1_merged) {  // the merged descriptors: the same landmarks, record bounds inside the merged stream
          CHECK(L.lm_work_m.size() == L.lm_work.size());
          for (int k = 0; k < L.n_work; ++k) {
            for (int q : {0, 1, 2, 4, 5, 6}) CHECK(L.lm_work_m[8 * k + q] == L.lm_work[8 * k + q]);
            CHECK(L.lm_work_m[8 * k + 3] >= 0 && L.lm_work_m[8 * k + 3] < L.lm_work_m[8 * k + 7] && L.lm_work_m[8 * k + 7] <= L.n_merged);
          }
        } else {
          CHECK(L.lm_work_m.empty());
        }
      }
  }
  CHECK(A[0].order == A[1].order && A[0].rec_seg == A[1].rec_seg && A[0].seg_rec_begin == A[1].seg_rec_begin &&
        A[0].lm_seg_begin == A[1].lm_seg_begin && A[0].frame_seg_list == A[1].frame_seg_list && A[0].lm_work == A[1].lm_work);
  CHECK(A[0].m_first == A[1].m_first && A[0].m_seg_rec_begin == A[1].m_seg_rec_begin && A[0].lm_work_m == A[1].lm_work_m);
}

int main() {
  int plans = 0, trees = 0;
  for (int n : {2, 12, 33, 100, 500})
    for (int w : {1, 7, 40, 120}) {
      std::vector<int32_t> win(n);
      for (int f = 0; f < n; ++f) win[f] = std::min(n - 1, f + w);
      for (int nf = 0; nf < 2; ++nf) {
        for (int ord = PTZBA_ORDER_NATURAL; ord <= PTZBA_ORDER_NESTED_FORCE; ++ord) {
          SysOrder so;
          CholPlan P;
          if (choose_order_plan(n, nf, win, ord, so, P) == 0) check_plan(so, P, n, nf), ++plans;
        }
        for (int world = 2; n == 500 && world <= 8; world *= 2) {
          SysOrder o;
          DistTree DT;
          if (!dist_order(n, nf, win, world, o) || !dist_tree(o, world, DT)) continue;
          for (int r = 0; r < world; ++r) {
            CholPlan P;
            TreePlan Q;
            if (!make_plan_tree(o, DT, r, n, nf, win, pad_tile(o.n_aug + 1), P, Q)) continue;
            check_plan(o, P, n, nf), ++trees;
            for (const auto& ph : Q.ph) {
              CHECK(ph.lv0 <= ph.lv1 && ph.lv1 <= P.n_levels && ph.c0 <= ph.c1);
              check_range(ph.xt, 0, pad_tile(o.n_aug + 1) / CHOL_NB);
            }
          }
        }
      }
    }
  run_layout(3, 0, {}, {});
  run_layout(1, 1, {0}, {0});
  std::mt19937 rng(12345);  // ~20K records: 700 landmarks (every seventh without records) over 90 frames, with gaps
  std::vector<int32_t> fr, lm;
  for (int l = 0; l < 700; ++l)
    for (int k = 0, f0 = (int)(rng() % 80); l % 7 != 3 && k < 34; ++k)
      if (rng() % 8) fr.push_back(std::min(89, f0 + (int)(rng() % 10) * (k % 3 ? 1 : 4))), lm.push_back(l);
  for (size_t k = fr.size(); k > 1; --k) {  // records arrive in no particular order
    const size_t j = rng() % k;
    std::swap(fr[k - 1], fr[j]), std::swap(lm[k - 1], lm[j]);
  }
  run_layout(90, 700, fr, lm);
  // the same records with observations for the merge pass: one keypoint per segment repeated (pair form), some
  // records off it by a sign of zero, by less than an fp32 ulp or by a pixel, weights that split runs; then a set whose
  // repeats are rare (the merged stream is not built)
  for (int rare = 0; rare < 2; ++rare) {
    std::vector<double> xy(2 * fr.size()), w(fr.size());
    for (size_t k = 0; k < fr.size(); ++k) {
      const double bx = 100.0 + 3.0 * fr[k] + 0.25 * lm[k], by = 50.0 + 0.5 * lm[k];
      const unsigned c = rng() % (rare ? 3 : 16);
      xy[2 * k] = c == 0 ? bx + 1.0 : (c == 1 ? bx + 1e-9 : bx);
      xy[2 * k + 1] = (rare || c == 2) ? by + (double)(rng() % 5) : by;
      w[k] = rng() % 8 ? 1.0 : 2.0;
    }
    run_layout(90, 700, fr, lm, xy, w);
  }
  {  // +0.0 and -0.0 deltas are different records: the stored bits decide, not the inputs'
    const std::vector<int32_t> f4{0, 0, 0, 0}, l4{0, 0, 0, 0};
    ProblemLayout L;
    layout_host_sort(L, 1, 1, 4, f4.data(), l4.data(), 1);
    CHECK(!layout_host_segments(L, 1, 4, f4.data(), l4.data(), 1));
    std::vector<double> sb;
    std::vector<float> st(8);
    const std::vector<double> xy{5.0, 0.0, 5.0, -0.0, 5.0, -0.0, 5.0, 0.0};
    layout_convert_records<float>(L, 4, xy.data(), nullptr, sb, st.data(), (float*)nullptr);
    layout_host_merge(L, 4, st.data(), nullptr, true, 1, true);
    CHECK(L.n_merged == 3);  // (the y deltas: 0.0 - 0.0 = +0.0, -0.0 - 0.0 = -0.0: three runs)
    const std::vector<double> xz{-0.0, 1.0, 0.0, 1.0, 0.0, 1.0, -0.0, 1.0};
    layout_convert_records<float>(L, 4, xz.data(), nullptr, sb, st.data(), (float*)nullptr);
    layout_host_merge(L, 4, st.data(), nullptr, true, 1, true);
    CHECK(L.n_merged == 1);  // (-0.0 - -0.0 = +0.0 and 0.0 - -0.0 = +0.0)
  }
  std::printf("host-check: %d plans, %d rank-tree plans, 5 record sets (%zu records) ok\n", plans, trees, fr.size());
  return 0;
}
