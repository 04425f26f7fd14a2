// Host-side layout of a problem's records, built by ptzba_set_problem between validation and the factorisation plan:
// the (landmark, frame, index) order, the segments (unique landmark x frame), the frame CSR and coupling window, the K2
// tiles / work items and the K1 work order.  Host only (no HIP call); one function per set_problem phase, each filling
// the struct in place.  A function that can fail returns the message for fail(), nullptr otherwise.
#pragma once
#include <cstdint>
#include <vector>

namespace ptzba {

struct ProblemLayout {
  std::vector<int64_t> order;          // [n_obs] sorted -> original record (host fronts only)
  std::vector<int32_t> rec_seg;        // [n_obs] segment of each sorted record (host fronts only)
  std::vector<int32_t> seg_frame, seg_lm;
  std::vector<int64_t> seg_rec_begin;  // [n_seg + 1]
  std::vector<int32_t> lm_seg_begin;   // [n_lm + 1]
  std::vector<int32_t> frame_seg_begin, frame_seg_list, frame_win_hi;
  std::vector<int32_t> lm_meta, s2_items, s2_groups, s2_lm, lm_work;
  int64_t n_slot = 0;  // dense landmark x frame slots (W table rows)
  int n_work = 0, max_seg = 0, k1_groups = 0, k1_groups_global = 0;
  int k2_info[8] = {}, k2_tile_info[8] = {};  // ptzba_k2_info / ptzba_k2_tile_info
  bool f1_covered = false;
  // K1's merged record stream: a run is a maximal sequence of adjacent records of one segment whose stored records
  // (the delta pair in the record precision, the user weight) are bit-identical; a run becomes one K1 record of weight
  // multiplicity x user weight.  n_merged: the run count (n_obs when the pass did not run); k1_merged: K1 reads the
  // merged stream (the runs are at most half the records)
  int64_t n_merged = 0;
  bool k1_merged = false;
  std::vector<int64_t> m_first;          // [n_merged + 1] first sorted record of each run, then n_obs (host fronts only)
  std::vector<int64_t> m_seg_rec_begin;  // [n_seg + 1] the segments' CSR into the runs
  std::vector<int32_t> lm_work_m;        // lm_work with the merged stream's record bounds
  // the single-thread sort's by-products, read by its segment pass: record ranges of the landmarks, frames in order
  std::vector<int64_t> lm_start;
  std::vector<int32_t> sorted_frame;
};

// threads: host_threads(n_obs); > 1 takes the threaded passes (the same results, par_util.h)
void layout_host_sort(ProblemLayout& L, int n_pose, int n_lm, int64_t n_obs, const int32_t* obs_frame,
                      const int32_t* obs_lm, int threads);
const char* layout_host_segments(ProblemLayout& L, int n_lm, int64_t n_obs, const int32_t* obs_frame,
                                 const int32_t* obs_lm, int threads);
// lm_seg_begin from seg_lm (segments are landmark-ordered): each landmark's first segment, landmarks without one take
// the next's (the device front and the threaded host pass)
void lm_first_segments(ProblemLayout& L, int n_lm);
// par: the threaded or the device front ran (the frame passes then use host threads as well)
void layout_frame_csr(ProblemLayout& L, int n_pose, bool par, int threads);
const char* layout_k2(ProblemLayout& L, int n_pose, int n_lm, int n_fixed);
// the host fronts' stored records (after layout_host_segments): seg_base [2 n_seg] = each segment's first observation,
// xy [2 n_obs] = the sorted records' deltas from it in the record precision, ww [n_obs] the weights (w == nullptr: none)
template <typename real>
void layout_convert_records(const ProblemLayout& L, int64_t n_obs, const double* obs_xy, const double* w,
                            std::vector<double>& seg_base, real* xy, real* ww);
// the runs of the host fronts, on those stored arrays (rec_w == nullptr: unweighted): counts them, and where they are at
// most half the records (k1_merged; fill_always: in any case) fills m_first / m_seg_rec_begin.  fp32: the arrays' type
void layout_host_merge(ProblemLayout& L, int64_t n_obs, const void* rec_xy, const void* rec_w, bool fp32, int threads,
                       bool fill_always = false);
// whether K1 takes the merged stream: it must at least halve the record count (the weighted instantiation costs ~8 %
// more per record, and a nearly duplicate-free problem keeps its memory)
inline bool k1_merge_pays(int64_t n_merged, int64_t n_obs) { return n_obs > 0 && 2 * n_merged <= n_obs; }
// (with k1_merged the order weighs a landmark by its merged records and lm_work_m holds their bounds)
void layout_k1_order(ProblemLayout& L, int n_pose, int n_lm);

}  // namespace ptzba
