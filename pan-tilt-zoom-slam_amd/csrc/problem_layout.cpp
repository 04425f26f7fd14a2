// problem_layout.h: the host passes of ptzba_set_problem over the records.
#include "problem_layout.h"

#include <algorithm>
#include <cstring>
#include <utility>

#include "ptzba_kernels.h"
#include "par_util.h"

namespace ptzba {

constexpr int WAVE = 64;  // partner frames of a K2 chunk: one per lane (ptzba_common.h, which is device code)

// ---- stable counting sorts: by frame, then by landmark -> (landmark, frame, original index)
void layout_host_sort(ProblemLayout& L, int n_pose, int n_lm, int64_t n_obs, const int32_t* obs_frame,
                      const int32_t* obs_lm, int threads) {
  std::vector<int64_t> tmp(n_obs);
  L.order.resize(n_obs);
  if (threads > 1) {  // large problems (config 4: 410M records) sort on host threads: the same stable order (par_util.h)
    parallel_counting_sort(n_obs, n_pose, (const int64_t*)nullptr, tmp.data(), [&](int64_t r) { return obs_frame[r]; });
    parallel_counting_sort(n_obs, n_lm, tmp.data(), L.order.data(), [&](int64_t r) { return obs_lm[r]; });
    return;
  }
  // two stable counting passes (by frame, then by landmark) -> (landmark, frame, record) order; the second pass
  // walks the records frame by frame, so each record's frame is known without a lookup and lands in sorted_frame
  // beside `order` -- the segment pass then streams over it (per-landmark comparison sorts measured 2.4x
  // slower at a window's ~250 records per landmark)
  std::vector<int64_t> fo(n_pose + 1, 0);
  for (int64_t r = 0; r < n_obs; ++r) fo[obs_frame[r] + 1]++;
  for (int f = 0; f < n_pose; ++f) fo[f + 1] += fo[f];
  {
    std::vector<int64_t> c(fo.begin(), fo.end() - 1);
    for (int64_t r = 0; r < n_obs; ++r) tmp[c[obs_frame[r]]++] = r;
  }
  L.lm_start.assign(n_lm + 1, 0);
  for (int64_t r = 0; r < n_obs; ++r) L.lm_start[obs_lm[r] + 1]++;
  for (int l = 0; l < n_lm; ++l) L.lm_start[l + 1] += L.lm_start[l];
  L.sorted_frame.resize(n_obs);
  {
    std::vector<int64_t> c(L.lm_start.begin(), L.lm_start.end() - 1);
    for (int f = 0; f < n_pose; ++f)
      for (int64_t k = fo[f]; k < fo[f + 1]; ++k) {
        const int64_t r = tmp[k];
        const int64_t q = c[obs_lm[r]]++;
        L.order[q] = r;
        L.sorted_frame[q] = f;
      }
  }
}

// ---- segments (unique landmark, frame)
const char* layout_host_segments(ProblemLayout& L, int n_lm, int64_t n_obs, const int32_t* obs_frame,
                                 const int32_t* obs_lm, int threads) {
  L.rec_seg.resize(n_obs);
  if (threads > 1) {
    // two passes over the same record chunks: count the segment starts per chunk, then fill at the prefix offsets
    const int T = threads;
    const auto& order = L.order;
    auto is_start = [&](int64_t k) {
      return k == 0 || obs_lm[order[k]] != obs_lm[order[k - 1]] || obs_frame[order[k]] != obs_frame[order[k - 1]];
    };
    std::vector<int64_t> base(T + 1, 0);
    parallel_chunks(n_obs, T, [&](int64_t lo, int64_t hi, int t) {
      int64_t c = 0;
      for (int64_t k = lo; k < hi; ++k) c += is_start(k);
      base[t + 1] = c;
    });
    for (int t = 0; t < T; ++t) base[t + 1] += base[t];
    if (base[T] >= INT32_MAX - 1) return "too many segments";
    L.seg_frame.resize(base[T]);
    L.seg_lm.resize(base[T]);
    L.seg_rec_begin.resize(base[T]);
    parallel_chunks(n_obs, T, [&](int64_t lo, int64_t hi, int t) {
      int64_t sg = base[t] - 1;
      for (int64_t k = lo; k < hi; ++k) {
        if (is_start(k)) {
          const int64_t r = order[k];
          ++sg;
          L.seg_frame[sg] = obs_frame[r];
          L.seg_lm[sg] = obs_lm[r];
          L.seg_rec_begin[sg] = k;
        }
        L.rec_seg[k] = (int32_t)sg;
      }
    });
    lm_first_segments(L, n_lm);
  } else {
    L.lm_seg_begin.assign(n_lm + 1, 0);
    L.seg_frame.reserve(n_obs / 4 + 16);
    L.seg_lm.reserve(n_obs / 4 + 16);
    L.seg_rec_begin.reserve(n_obs / 4 + 16);
    for (int l = 0; l < n_lm; ++l) {
      L.lm_seg_begin[l] = (int32_t)L.seg_frame.size();
      for (int64_t k = L.lm_start[l]; k < L.lm_start[l + 1]; ++k) {
        if (k == L.lm_start[l] || L.sorted_frame[k] != L.sorted_frame[k - 1]) {
          if ((int64_t)L.seg_frame.size() >= INT32_MAX - 1) return "too many segments";
          L.seg_frame.push_back(L.sorted_frame[k]);
          L.seg_lm.push_back(l);
          L.seg_rec_begin.push_back(k);
        }
        L.rec_seg[k] = (int32_t)L.seg_frame.size() - 1;
      }
    }
    L.lm_seg_begin[n_lm] = (int32_t)L.seg_frame.size();
  }
  L.seg_rec_begin.push_back(n_obs);  // (the device front returns the end entry with the segments)
  return nullptr;
}

// ---- the stored records of the host fronts: deltas from each segment's base observation in the record precision
template <typename real>
void layout_convert_records(const ProblemLayout& L, int64_t n_obs, const double* obs_xy, const double* w,
                            std::vector<double>& seg_base, real* xy, real* ww) {
  const int64_t n_seg = (int64_t)L.seg_frame.size();
  seg_base.resize(2 * n_seg);
  for (int64_t s = 0; s < n_seg; ++s) {
    const int64_t r = L.order[L.seg_rec_begin[s]];
    seg_base[2 * s] = obs_xy[2 * r];
    seg_base[2 * s + 1] = obs_xy[2 * r + 1];
  }
  const auto &order = L.order;
  const auto& rec_seg = L.rec_seg;
  parallel_chunks(n_obs, host_threads(n_obs), [&](int64_t lo, int64_t hi, int) {
    for (int64_t r = lo; r < hi; ++r) {
      const int32_t s = rec_seg[r];
      xy[2 * r] = (real)(obs_xy[2 * order[r]] - seg_base[2 * s]);
      xy[2 * r + 1] = (real)(obs_xy[2 * order[r] + 1] - seg_base[2 * s + 1]);
      if (w) ww[r] = (real)w[order[r]];
    }
  });
}
template void layout_convert_records<float>(const ProblemLayout&, int64_t, const double*, const double*,
                                            std::vector<double>&, float*, float*);
template void layout_convert_records<double>(const ProblemLayout&, int64_t, const double*, const double*,
                                             std::vector<double>&, double*, double*);

// ---- K1's merged stream: runs of adjacent bit-identical stored records inside a segment
template <typename real>
static void host_merge(ProblemLayout& L, int64_t n_obs, const real* xy, const real* w, int threads, bool fill_always) {
  const auto& rec_seg = L.rec_seg;
  const int64_t n_seg = (int64_t)L.seg_frame.size();
  // on the stored arrays, as the device front does (bits compared: -0.0 and +0.0 differ); cheap enough to evaluate in
  // the counting pass and again in the fill
  auto is_start = [&](int64_t k) {
    return k == 0 || rec_seg[k] != rec_seg[k - 1] || std::memcmp(xy + 2 * k, xy + 2 * k - 2, 2 * sizeof(real)) != 0 ||
           (w && std::memcmp(w + k, w + k - 1, sizeof(real)) != 0);
  };
  const int T = std::max(threads, 1);
  std::vector<int64_t> base(T + 1, 0);
  parallel_chunks(n_obs, T, [&](int64_t lo, int64_t hi, int t) {
    int64_t c = 0;
    for (int64_t k = lo; k < hi; ++k) c += is_start(k);
    base[t + 1] = c;
  });
  for (int t = 0; t < T; ++t) base[t + 1] += base[t];
  L.n_merged = base[T];
  L.k1_merged = k1_merge_pays(L.n_merged, n_obs);
  if (!L.k1_merged && !fill_always) return;
  L.m_first.resize(L.n_merged + 1);
  L.m_seg_rec_begin.resize(n_seg + 1);
  parallel_chunks(n_obs, T, [&](int64_t lo, int64_t hi, int t) {
    int64_t m = base[t];
    for (int64_t k = lo; k < hi; ++k)
      if (is_start(k)) {
        if (k == 0 || rec_seg[k] != rec_seg[k - 1]) L.m_seg_rec_begin[rec_seg[k]] = m;
        L.m_first[m++] = k;
      }
  });
  L.m_first[L.n_merged] = n_obs;
  L.m_seg_rec_begin[n_seg] = L.n_merged;
}

void layout_host_merge(ProblemLayout& L, int64_t n_obs, const void* rec_xy, const void* rec_w, bool fp32, int threads,
                       bool fill_always) {
  if (fp32) host_merge<float>(L, n_obs, (const float*)rec_xy, (const float*)rec_w, threads, fill_always);
  else host_merge<double>(L, n_obs, (const double*)rec_xy, (const double*)rec_w, threads, fill_always);
}

void lm_first_segments(ProblemLayout& L, int n_lm) {
  const int64_t ns = (int64_t)L.seg_lm.size();
  auto& first = L.lm_seg_begin;
  first.assign(n_lm + 1, -1);
  first[n_lm] = (int32_t)ns;
  for (int64_t sg = 0; sg < ns; ++sg)
    if (sg == 0 || L.seg_lm[sg] != L.seg_lm[sg - 1]) first[L.seg_lm[sg]] = (int32_t)sg;
  for (int l = n_lm - 1; l >= 0; --l)
    if (first[l] < 0) first[l] = first[l + 1];
}

// ---- frame CSR over segments (stable: landmark ascending within a frame) and each frame's coupling window
void layout_frame_csr(ProblemLayout& L, int n_pose, bool par, int threads) {
  const int64_t n_seg = (int64_t)L.seg_frame.size();
  const auto& seg_frame = L.seg_frame;
  L.frame_seg_begin.assign(n_pose + 1, 0);
  L.frame_seg_list.assign(n_seg, 0);
  L.frame_win_hi.assign(n_pose, 0);
  for (int64_t s = 0; s < n_seg; ++s) L.frame_seg_begin[seg_frame[s] + 1]++;
  for (int f = 0; f < n_pose; ++f) L.frame_seg_begin[f + 1] += L.frame_seg_begin[f];
  if (par && host_threads(n_seg) > 1) {
    parallel_counting_sort(n_seg, n_pose, (const int32_t*)nullptr, L.frame_seg_list.data(),
                           [&](int32_t sg) { return seg_frame[sg]; });
  } else {
    std::vector<int32_t> c(L.frame_seg_begin.begin(), L.frame_seg_begin.end() - 1);
    for (int64_t s = 0; s < n_seg; ++s) L.frame_seg_list[c[seg_frame[s]]++] = (int32_t)s;
  }
  parallel_chunks(n_pose, par ? std::min(threads, n_pose) : 1, [&](int64_t f0, int64_t f1, int) {
    for (int64_t f = f0; f < f1; ++f) {
      int hi = (int)f;
      for (int e = L.frame_seg_begin[f]; e < L.frame_seg_begin[f + 1]; ++e) {
        int l = L.seg_lm[L.frame_seg_list[e]];
        hi = std::max(hi, seg_frame[L.lm_seg_begin[l + 1] - 1]);
      }
      L.frame_win_hi[f] = hi;
    }
  });
}

// ---- register-blocked K2 structure: per landmark its frame range [first, last] and a dense W slot
// per frame in it; K2 tiles (SCHUR_F1 frames x 64 partner frames) with the landmarks that reach them,
const char* layout_k2(ProblemLayout& L, int n_pose, int n_lm, int n_fixed) {
  const auto &seg_frame = L.seg_frame, &lm_seg_begin = L.lm_seg_begin;
  auto &lm_meta = L.lm_meta, &s2_items = L.s2_items, &s2_groups = L.s2_groups, &s2_lm = L.s2_lm;
  lm_meta.assign(4 * (size_t)std::max(n_lm, 1), 0);
  int64_t toff = 0;
  for (int l = 0; l < n_lm; ++l) {
    const int s0 = lm_seg_begin[l], s1 = lm_seg_begin[l + 1];
    if (s1 == s0) continue;
    const int lo = seg_frame[s0], hi = seg_frame[s1 - 1];  // segments are frame-ordered per landmark
    lm_meta[4 * l] = lo;
    lm_meta[4 * l + 1] = hi;
    lm_meta[4 * l + 2] = (int32_t)toff;
    toff += hi - lo + 1;
    if (toff >= INT32_MAX) return "landmark x frame slot table exceeds 2^31 rows";
  }
  L.n_slot = toff;
  // split size: about two work items per CU over the whole list volume, at least 64 landmarks
  std::vector<std::vector<int32_t>> tiles;
  std::vector<int32_t> tile_key;
  std::vector<int32_t> un;
  // the landmarks of an F1 block, ascending and unique: marked in a bitmap, then read out word by word between the
  // lowest and highest marked word (no sort: a config-5 window's single block holds ~100K segments)
  std::vector<uint64_t> lm_bits((size_t)n_lm / 64 + 1, 0);
  for (int f1b = n_fixed; f1b < n_pose; f1b += SCHUR_F1) {
    un.clear();
    size_t w_lo = lm_bits.size(), w_hi = 0;
    for (int f = f1b; f < std::min(n_pose, f1b + SCHUR_F1); ++f)
      for (int e = L.frame_seg_begin[f]; e < L.frame_seg_begin[f + 1]; ++e) {
        const uint32_t l = (uint32_t)L.seg_lm[L.frame_seg_list[e]];
        lm_bits[l >> 6] |= 1ull << (l & 63);
        w_lo = std::min<size_t>(w_lo, l >> 6);
        w_hi = std::max<size_t>(w_hi, l >> 6);
      }
    for (size_t wd = w_lo; wd <= w_hi && w_lo < lm_bits.size(); ++wd) {
      uint64_t m = lm_bits[wd];
      lm_bits[wd] = 0;
      while (m) {
        un.push_back((int32_t)(wd * 64 + __builtin_ctzll(m)));
        m &= m - 1;
      }
    }
    int hi = f1b;
    for (int l : un) hi = std::max(hi, lm_meta[4 * l + 1]);
    const int nc = (hi - f1b) / WAVE + 1;
    for (int c = 0; c < nc; ++c) {
      // a landmark enters chunk c only when it sees a frame of the chunk (its frame set can have gaps:
      // on a multi-row keyframe grid a landmark seen by two tilt rows spans a whole row of frames)
      std::vector<int32_t> lst;
      const int c_lo = f1b + WAVE * c, c_hi = c_lo + WAVE - 1;
      for (int l : un) {
        if (c > 0) {
          if (lm_meta[4 * l + 1] < c_lo) continue;
          const int32_t* fb = seg_frame.data() + lm_seg_begin[l];
          const int32_t* fe = seg_frame.data() + lm_seg_begin[l + 1];
          const int32_t* it = std::lower_bound(fb, fe, c_lo);
          if (it == fe || *it > c_hi) continue;
        }
        lst.push_back(l);
      }
      if (lst.empty()) continue;
      tiles.push_back(std::move(lst));
      tile_key.push_back(f1b);
      tile_key.push_back(c);
    }
  }
  // split size: at most 256 work items (one round of one workgroup per CU) counting the per-tile rounding, at
  // least 64 landmarks, at most SCHUR_LMAX (the LDS list).  Chunk-0 items also sum the diagonal terms: their
  // lists are weighted (6 / 4; per-item clock stamps, tools/schur_items.py, put a chunk-0 landmark at 1.5-1.9x
  // the time of another's; 5 / 4 before round 5) so that the items of the round end together.
  int64_t W0 = 6;
  constexpr int64_t WD = 4;  // chunk-0 weight W0 / WD
  int64_t total_w = 0;
  for (size_t k = 0; k < tiles.size(); ++k)
    total_w += (int64_t)tiles[k].size() * (tile_key[2 * k + 1] == 0 ? W0 : WD);
  // item target: at most 256 (ONE round of one 512-thread workgroup per CU: k_schur_mfp's 116 KB of LDS allows one
  // per CU) -- same-box A/B at config 3 (r04j, r04p): 256 items 64.7-64.8 us per build against 73.3-74.6 with 512
  // (two rounds), 68.0 with 192, 84.8 with 320; proportionally fewer for less work -- a rank's shard of a sharded
  // solve: each item's 74 KB split partial and the reduce over its tile's splits are fixed costs (measured at
  // config 3, tools/dist_model.py: N = 8 shard 44-66 -> 37-47 us with 64-128 items)
  int64_t target_items = std::min<int64_t>(256, std::max<int64_t>(64, (512 * total_w) / 480000));
  // the smallest split weight whose per-tile rounding still fits the target (binary search: the item count falls as
  // the split grows), so the items are as short -- and the one round as even -- as the target allows
  auto items_for = [&](int64_t sw) {
    int64_t c = 0;
    for (size_t k = 0; k < tiles.size(); ++k) {
      const int64_t n = (int64_t)tiles[k].size(), nw = n * (tile_key[2 * k + 1] == 0 ? W0 : WD);
      c += std::max<int64_t>((nw + sw - 1) / sw, (n + SCHUR_LMAX - 1) / SCHUR_LMAX);
    }
    return c;
  };
  int64_t sw_lo = 64 * WD, sw_hi = std::max<int64_t>(sw_lo, total_w);
  if (items_for(sw_lo) <= target_items) {
    sw_hi = sw_lo;
  } else {
    while (sw_hi - sw_lo > 1) {  // items_for(sw_lo) > target >= items_for(sw_hi)
      const int64_t mid = (sw_lo + sw_hi) / 2;
      if (items_for(mid) <= target_items) sw_hi = mid;
      else sw_lo = mid;
    }
  }
  const int64_t split_w = sw_hi;
  for (size_t k = 0; k < tiles.size(); ++k) {
    const auto& lst = tiles[k];
    const int n = (int)lst.size();
    const int64_t nw = (int64_t)n * (tile_key[2 * k + 1] == 0 ? W0 : WD);
    const int nparts = (int)std::max<int64_t>((nw + split_w - 1) / split_w, (n + SCHUR_LMAX - 1) / SCHUR_LMAX);
    const int i0 = (int)(s2_items.size() / 4);
    for (int pp = 0; pp < nparts; ++pp) {
      const int a0 = (int)((int64_t)n * pp / nparts), a1 = (int)((int64_t)n * (pp + 1) / nparts);
      const int b0 = (int)(s2_lm.size() / 4);
      for (int q = a0; q < a1; ++q) {
        const int l = lst[q];
        s2_lm.insert(s2_lm.end(), {l, lm_meta[4 * l], lm_meta[4 * l + 1], lm_meta[4 * l + 2]});
      }
      s2_items.insert(s2_items.end(), {tile_key[2 * k], tile_key[2 * k + 1], b0, (int32_t)(s2_lm.size() / 4)});
    }
    s2_groups.insert(s2_groups.end(), {tile_key[2 * k], tile_key[2 * k + 1], i0, (int32_t)(s2_items.size() / 4)});
  }
  // which pipeline shapes the items run (ptzba_k2_info): batches of 16 landmarks, two per ring round trip
  {
    int* ki = L.k2_info;
    ki[0] = (int)(s2_items.size() / 4);
    for (size_t k = 0; k < s2_items.size(); k += 4) {
      const int nl = s2_items[k + 3] - s2_items[k + 2], m = nl % 32;
      if (s2_items[k + 1] == 0) ++ki[1];
      ki[2] = k == 0 ? nl : std::min(ki[2], nl);
      ki[3] = std::max(ki[3], nl);
      if (nl <= 16) ++ki[4];
      ++ki[m == 0 ? 7 : (m <= 16 ? 5 : 6)];
    }
  }
  // which reduce shapes the tiles run (ptzba_k2_tile_info): splits per tile against the reduce's 8 partials in
  // flight, the farthest partner chunk, partner ranges that pass the last frame (the clamped reads)
  {
    int* ti = L.k2_tile_info;
    ti[0] = (int)(s2_groups.size() / 4);
    for (size_t g = 0; g < s2_groups.size(); g += 4) {
      const int ns = s2_groups[g + 3] - s2_groups[g + 2];
      ti[1] = g == 0 ? ns : std::min(ti[1], ns);
      ti[2] = std::max(ti[2], ns);
      if (ns >= 9) ++ti[3];
      ti[4] = std::max(ti[4], s2_groups[g + 1]);
      if (s2_groups[g] + WAVE * (s2_groups[g + 1] + 1) > n_pose) ++ti[5];
    }
  }
  {
    std::vector<uint8_t> cov((n_pose + SCHUR_F1) / SCHUR_F1 + 1, 0);
    for (size_t g = 0; g < s2_groups.size(); g += 4)
      if (s2_groups[g + 1] == 0) cov[(s2_groups[g] - n_fixed) / SCHUR_F1] = 1;
    L.f1_covered = true;
    for (int f1b = n_fixed; f1b < n_pose; f1b += SCHUR_F1)
      if (!cov[(f1b - n_fixed) / SCHUR_F1]) L.f1_covered = false;
  }
  return nullptr;
}

// ---- landmark work order: heaviest (most records) first
void layout_k1_order(ProblemLayout& L, int n_pose, int n_lm) {
  const auto &lm_seg_begin = L.lm_seg_begin, &lm_meta = L.lm_meta;
  const auto& seg_rec_begin = L.seg_rec_begin;
  // the record stream K1 reads: the order weighs a landmark by its work there
  const auto& k1_rec_begin = L.k1_merged ? L.m_seg_rec_begin : L.seg_rec_begin;
  auto& lm_work = L.lm_work;
  std::vector<int32_t> lm_order;
  L.max_seg = 0;
  for (int l = 0; l < n_lm; ++l) {
    int ns = lm_seg_begin[l + 1] - lm_seg_begin[l];
    if (ns > 0) lm_order.push_back(l);
    L.max_seg = std::max(L.max_seg, ns);
  }
  {
    // heaviest first (LPT over the workgroup slots) at 1/8-octave resolution of the record count, and inside such a
    // size class by first frame: a K1 workgroup's landmarks then see neighbouring frames, so it stages ~a coupling
    // window of frame tables instead of the whole table (k1_device.h k1_stage_frames)
    auto nrec = [&](int l) { return k1_rec_begin[lm_seg_begin[l + 1]] - k1_rec_begin[lm_seg_begin[l]]; };
    auto size_class = [&](int l) {
      const uint64_t c = (uint64_t)nrec(l);
      if (c < 16) return (int)c;
      const int msb = 63 - __builtin_clzll(c);
      return 16 + 8 * (msb - 4) + (int)((c >> (msb - 3)) & 7);
    };
    std::vector<int64_t> key(n_lm, 0);
    for (int l : lm_order) key[l] = ((int64_t)(1 << 20) - size_class(l)) * ((int64_t)1 << 40) + ((int64_t)lm_meta[4 * l] << 20);
    std::sort(lm_order.begin(), lm_order.end(), [&](int a, int b) { return key[a] != key[b] ? key[a] < key[b] : a < b; });
  }
  L.n_work = (int)lm_order.size();
  // K1 work descriptors, 32 B: {landmark, first segment, end segment, first record | first frame, last
  // frame, slot offset (lm_meta), end record of the first K1_SEGW-segment window}
  lm_work.assign(8 * (size_t)L.n_work, 0);
  for (int k = 0; k < L.n_work; ++k) {
    const int l = lm_order[k];
    lm_work[8 * k + 0] = l;
    lm_work[8 * k + 1] = lm_seg_begin[l];
    lm_work[8 * k + 2] = lm_seg_begin[l + 1];
    lm_work[8 * k + 3] = (int32_t)seg_rec_begin[lm_seg_begin[l]];
    for (int q = 0; q < 3; ++q) lm_work[8 * k + 4 + q] = lm_meta[4 * l + q];
    lm_work[8 * k + 7] = (int32_t)seg_rec_begin[std::min(lm_seg_begin[l + 1], lm_seg_begin[l] + K1_SEGW)];
  }
  L.lm_work_m.clear();
  if (L.k1_merged) {  // the same descriptors with the merged stream's record bounds
    L.lm_work_m = lm_work;
    for (int k = 0; k < L.n_work; ++k) {
      const int l = lm_order[k];
      L.lm_work_m[8 * k + 3] = (int32_t)L.m_seg_rec_begin[lm_seg_begin[l]];
      L.lm_work_m[8 * k + 7] = (int32_t)L.m_seg_rec_begin[std::min(lm_seg_begin[l + 1], lm_seg_begin[l] + K1_SEGW)];
    }
  }
  // which table path each K1 workgroup takes (ptzba_k1_info): the kernel's own frame range and predicate
  L.k1_groups = (L.n_work + K1_WPB - 1) / K1_WPB;
  L.k1_groups_global = 0;
  for (int g = 0; g < L.k1_groups; ++g) {
    int fmin = n_pose, fmax = -1;
    for (int q = 0; q < K1_WPB; ++q) {
      const int k = std::min(g * K1_WPB + q, L.n_work - 1);
      fmin = std::min(fmin, lm_work[8 * k + 4]);
      fmax = std::max(fmax, lm_work[8 * k + 5]);
    }
    if (!k1_ftl_fits(fmin, fmax)) ++L.k1_groups_global;
  }
}

}  // namespace ptzba
