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
void layout_k1_order(ProblemLayout& L, int n_pose, int n_lm);

}  // namespace ptzba
