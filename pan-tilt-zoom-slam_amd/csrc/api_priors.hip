// Gaussian pose and ray priors of the C-ABI (include/ptzba.h; prior_kernels.hip)
#include <algorithm>
#include <array>
#include <cmath>
#include <map>

#include "ba_ctx.h"

using namespace ptzba;

// the handle's priors over the state pair (ptz, ptz_trial): sel == nullptr the host-driven pair (current = ptz), else
// the device-driven LM's selection as in k_trial's sflip; flip = 1 picks the trial state instead of the current one
PriorArgs ptzba::prior_args(const ptzba_ctx* h, const int* sel, int flip) {
  const auto& p = h->pri;
  PriorArgs a;
  a.n_factor = p.n_factor;
  a.n_row = p.n_row;
  a.f_begin = p.f_begin.as<int32_t>();
  a.f_frames = p.f_frames.as<int32_t>();
  a.f_mean = p.f_mean.as<double>();
  a.f_info_off = p.f_info_off.as<int64_t>();
  a.f_info = p.f_info.as<double>();
  a.row_factor = p.row_factor.as<int32_t>();
  a.n_elem = p.n_elem;
  a.s_off = p.s_off.as<int64_t>();
  a.s_val = p.s_val.as<double>();
  a.n_pframe = p.n_pframe;
  a.p_frame = p.p_frame.as<int32_t>();
  a.p_begin = p.p_begin.as<int32_t>();
  a.p_ent = p.p_ent.as<int2>();
  a.p_diag = p.p_diag.as<double>();
  const double* cur = h->ptz.as<double>();
  const double* oth = h->ptz_trial.as<double>();
  if (sel) {
    a.x0 = cur;
    a.x1 = oth;
    a.sel = sel;
    a.sel_xor = h->state_base ^ flip;
  } else {
    a.x0 = flip ? oth : cur;
    a.x1 = nullptr;
    a.sel = nullptr;
    a.sel_xor = 0;
  }
  return a;
}

// the handle's ray priors over the state pair (rays, rays_trial), selected as prior_args selects (ptz, ptz_trial)
RayPriorArgs ptzba::ray_prior_args(const ptzba_ctx* h, const int* sel, int flip) {
  const auto& p = h->rp;
  RayPriorArgs a;
  a.n_lm = p.n_lm;
  a.lm = p.lm.as<int32_t>();
  a.begin = p.begin.as<int32_t>();
  a.mean = p.mean.as<double>();
  a.info = p.info.as<double>();
  const double* cur = h->rays.as<double>();
  const double* oth = h->rays_trial.as<double>();
  if (sel) {
    a.x0 = cur;
    a.x1 = oth;
    a.sel = sel;
    a.sel_xor = h->state_base ^ flip;
  } else {
    a.x0 = flip ? oth : cur;
    a.x1 = nullptr;
    a.sel = nullptr;
    a.sel_xor = 0;
  }
  return a;
}

// ------------------------------------------------------------------------------------------------
// Gaussian pose priors (include/ptzba.h ptzba_set_pose_priors; prior_kernels.hip)
// ------------------------------------------------------------------------------------------------
// Everything is validated on the host before the handle is touched.  P = sum_k Lambda_k is summed per unordered
// frame pair in factor order (fp64) and resolved to elements of S's lower triangle through the system positions:
// block (fa, fb) entry (q, r) lands where k_schur_reduce puts U / W V^-1 W^T of that pair, i.e. at row pos[fb] + r,
// column pos[fa] + q when pos[fb] >= pos[fa] and transposed otherwise (the reversed part of a nested order).
// Elements are addressed one by one, so a frame whose three rows straddle a 32-row tile needs no special case.
int ptzba_set_pose_priors(ptzba_handle h, const ptzba_pose_priors* pr) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (pr && pr->struct_size != (int32_t)sizeof(ptzba_pose_priors))
    return fail("ptzba_set_pose_priors: unknown struct_size %d of ptzba_pose_priors (this library knows %d)",
                (int)pr->struct_size, (int)sizeof(ptzba_pose_priors));
  HIPCHK(hipSetDevice(h->device));
  if (!pr || pr->n_factor == 0) {
    HIPCHK(hipStreamSynchronize(h->st));
    h->pri.n_factor = 0;
    HIPCHK(hipMemsetAsync(h->locp() + 5, 0, 8, h->st));  // the trial-cost slot of the decisions
    return 0;
  }
  if (h->dist_mode || h->dist_world > 1 || h->has_exchange() || h->ext_exchange || h->scal_exported)
    return fail("ptzba_set_pose_priors: single rank only (the handle is sharded, has a communicator / hook attached "
                "or runs a caller-side exchange)");
  const int nF = pr->n_factor;
  if (nF < 0 || !pr->factor_begin || !pr->frames || !pr->mean || !pr->info)
    return fail("ptzba_set_pose_priors: bad arguments (n_factor %d, null array)", nF);
  if (pr->factor_begin[0] != 0) return fail("ptzba_set_pose_priors: factor_begin[0] must be 0");
  std::vector<int32_t> f_begin(pr->factor_begin, pr->factor_begin + nF + 1), row_factor;
  std::vector<int64_t> info_off(nF);
  int64_t n_info = 0;
  for (int k = 0; k < nF; ++k) {
    const int G = f_begin[k + 1] - f_begin[k];
    if (G < 1 || G > 8) return fail("ptzba_set_pose_priors: factor %d names %d frames (1..8 allowed)", k, G);
    info_off[k] = n_info;
    n_info += (int64_t)9 * G * G;
  }
  const int n_fr = f_begin[nF];
  std::vector<int32_t> frames(pr->frames, pr->frames + n_fr);
  std::vector<double> mean(pr->mean, pr->mean + 3 * (size_t)n_fr), info(pr->info, pr->info + n_info);
  std::map<std::pair<int, int>, std::array<double, 9>> blocks;  // (fa <= fb) -> P block, rows fa, columns fb
  std::map<int, std::vector<int2>> by_frame;                    // frame -> (factor, slot), factor order
  for (int k = 0; k < nF; ++k) {
    const int f0 = f_begin[k], G = f_begin[k + 1] - f0, n3 = 3 * G;
    for (int a = 0; a < G; ++a) {
      const int f = frames[f0 + a];
      if (f < h->n_fixed || f >= h->n_pose)
        return fail("ptzba_set_pose_priors: factor %d names frame %d, not a free frame [%d, %d)", k, f, h->n_fixed, h->n_pose);
      for (int c = 0; c < a; ++c)
        if (frames[f0 + c] == f) return fail("ptzba_set_pose_priors: factor %d names frame %d twice", k, f);
    }
    double* L = info.data() + info_off[k];
    double amax = 0.0;
    for (int e = 0; e < n3 * n3; ++e) {
      if (!std::isfinite(L[e])) return fail("ptzba_set_pose_priors: factor %d: non-finite information entry", k);
      amax = std::max(amax, std::fabs(L[e]));
    }
    for (int e = 0; e < n3; ++e) {
      if (!std::isfinite(mean[3 * (size_t)f0 + e])) return fail("ptzba_set_pose_priors: factor %d: non-finite mean", k);
      if (L[e * n3 + e] < 0.0)
        return fail("ptzba_set_pose_priors: factor %d: negative diagonal entry %g of the information matrix", k, L[e * n3 + e]);
    }
    for (int i = 0; i < n3; ++i)
      for (int j = 0; j < i; ++j) {
        if (std::fabs(L[i * n3 + j] - L[j * n3 + i]) > 1e-12 * amax)
          return fail("ptzba_set_pose_priors: factor %d: information matrix not symmetric (entries %d,%d differ by %g)", k,
                      i, j, std::fabs(L[i * n3 + j] - L[j * n3 + i]));
        L[i * n3 + j] = L[j * n3 + i] = 0.5 * (L[i * n3 + j] + L[j * n3 + i]);
      }
    for (int a = 0; a < G; ++a)
      for (int c = 0; c < G; ++c) {
        const int fa = frames[f0 + a], fb = frames[f0 + c];
        if (fa < fb && fb > h->win_host[fa])
          return fail("ptzba_set_pose_priors: factor %d couples frames %d and %d, but the handle's coupling window of "
                      "frame %d ends at %d: pass frame_win_hi[%d] >= %d to ptzba_set_problem", k, fa, fb, fa,
                      h->win_host[fa], fa, fb);
        if (fa > fb) continue;  // the pair's block is summed from its (lower frame, higher frame) side
        auto it = blocks.find({fa, fb});
        if (it == blocks.end()) it = blocks.emplace(std::make_pair(fa, fb), std::array<double, 9>{}).first;
        for (int q = 0; q < 3; ++q)
          for (int r = 0; r < 3; ++r) it->second[3 * q + r] += L[(3 * a + q) * n3 + 3 * c + r];
      }
    for (int a = 0; a < G; ++a) by_frame[frames[f0 + a]].push_back(make_int2(k, a));
    for (int e = 0; e < n3; ++e) row_factor.push_back(k);
  }
  std::vector<int64_t> s_off;
  std::vector<double> s_val;
  const int64_t ld = h->ld;
  for (const auto& kv : blocks) {
    const int fa = kv.first.first, fb = kv.first.second;
    const int64_t pa = h->pos_host[fa], pb = h->pos_host[fb];
    if (pa < 0 || pb < 0 || pa + 2 >= h->n_aug || pb + 2 >= h->n_aug)
      return fail("ptzba_set_pose_priors: frames %d / %d lie outside the reduced system", fa, fb);
    for (int q = 0; q < 3; ++q)
      for (int r = 0; r < 3; ++r) {
        s_off.push_back(pb >= pa ? (pb + r) * ld + pa + q : (pa + q) * ld + pb + r);
        s_val.push_back(kv.second[3 * q + r]);
      }
  }
  std::vector<int32_t> p_frame, p_begin{0};
  std::vector<int2> p_ent;
  std::vector<double> p_diag;
  for (const auto& kv : by_frame) {
    p_frame.push_back(kv.first);
    p_ent.insert(p_ent.end(), kv.second.begin(), kv.second.end());
    p_begin.push_back((int32_t)p_ent.size());
    const auto& d = blocks.at({kv.first, kv.first});
    p_diag.insert(p_diag.end(), {d[0], d[4], d[8]});
  }
  // queued work may still read the previous set's arrays
  HIPCHK(hipStreamSynchronize(h->st));
  auto& p = h->pri;
  p.n_factor = 0;
  if (!p.red.p) {
    if (p.red.alloc(PRIOR_RED_SCRATCH * 8)) return -1;
    HIPCHK(hipMemsetAsync(p.red.p, 0, PRIOR_RED_SCRATCH * 8, h->st));
  }
  if (upload(p.f_begin, f_begin, h->st) || upload(p.f_frames, frames, h->st) || upload(p.f_mean, mean, h->st) ||
      upload(p.f_info_off, info_off, h->st) || upload(p.f_info, info, h->st) || upload(p.row_factor, row_factor, h->st) ||
      upload(p.s_off, s_off, h->st) || upload(p.s_val, s_val, h->st) || upload(p.p_frame, p_frame, h->st) ||
      upload(p.p_begin, p_begin, h->st) || upload(p.p_ent, p_ent, h->st) || upload(p.p_diag, p_diag, h->st))
    return -1;
  p.h_begin = f_begin;
  p.h_frames = frames;
  p.n_row = 3 * n_fr;
  p.n_elem = (int)s_off.size();
  p.n_pframe = (int)p_frame.size();
  p.n_block = (int)blocks.size();
  p.n_factor = nF;
  return 0;
}

int ptzba_pose_prior_info(ptzba_handle h, double* out4) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!out4) return fail("ptzba_pose_prior_info: null output");
  const auto& p = h->pri;
  out4[0] = p.n_factor;
  out4[1] = p.n_factor ? p.n_row : 0;
  out4[2] = p.n_factor ? p.n_block : 0;
  out4[3] = 0.0;
  if (!h->has_priors()) return 0;
  HIPCHK(hipSetDevice(h->device));
  if (!h->pri.cost.p && h->pri.cost.alloc(8)) return -1;
  launch_prior_cost(prior_args(h, nullptr, 0), h->pri.cost.as<double>(), 1.0, 0, h->pri.red.as<double>(), h->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out4 + 3, h->pri.cost.p, 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Gaussian ray priors (include/ptzba.h ptzba_set_ray_priors; prior_kernels.hip)
// ------------------------------------------------------------------------------------------------
// Everything is validated on the host before the handle is touched.  The priors are sorted by landmark (stable, so a
// landmark's priors keep their list order) into the CSR k_ray_prior_apply walks: one thread per distinct landmark.
int ptzba_set_ray_priors(ptzba_handle h, const ptzba_ray_priors* pr) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (pr && pr->struct_size != (int32_t)sizeof(ptzba_ray_priors))
    return fail("ptzba_set_ray_priors: unknown struct_size %d of ptzba_ray_priors (this library knows %d)",
                (int)pr->struct_size, (int)sizeof(ptzba_ray_priors));
  if (h->trial_open)
    return fail("ptzba_set_ray_priors: an LM trial is pending (accept or reject it first; the call runs between solves)");
  HIPCHK(hipSetDevice(h->device));
  if (!pr || pr->n_prior == 0) {
    HIPCHK(hipStreamSynchronize(h->st));  // queued work may still read the set's arrays
    h->rp.n_prior = 0;
    h->rp.n_lm = 0;
    return 0;
  }
  if (h->dist_mode || h->dist_world > 1 || h->has_exchange() || h->ext_exchange || h->scal_exported)
    return fail("ptzba_set_ray_priors: single rank only (the handle is sharded, has a communicator / hook attached "
                "or runs a caller-side exchange)");
  const int n = pr->n_prior;
  if (n < 0 || !pr->landmark || !pr->mean || !pr->info)
    return fail("ptzba_set_ray_priors: bad arguments (n_prior %d, null array)", n);
  std::vector<int32_t> seg((size_t)h->n_lm + 1);
  HIPCHK(hipMemcpyAsync(seg.data(), h->lm_seg_begin.p, seg.size() * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  for (int k = 0; k < n; ++k) {
    const int l = pr->landmark[k];
    if (l < 0 || l >= h->n_lm) return fail("ptzba_set_ray_priors: prior %d names landmark %d, out of range [0, %d)", k, l, h->n_lm);
    if (seg[l + 1] == seg[l])
      return fail("ptzba_set_ray_priors: prior %d names landmark %d, which has no records (prior-only landmarks are "
                  "not supported)", k, l);
    const double* m = pr->mean + 2 * (size_t)k;
    const double* L = pr->info + 3 * (size_t)k;
    if (!std::isfinite(m[0]) || !std::isfinite(m[1])) return fail("ptzba_set_ray_priors: prior %d: non-finite mean", k);
    if (!std::isfinite(L[0]) || !std::isfinite(L[1]) || !std::isfinite(L[2]))
      return fail("ptzba_set_ray_priors: prior %d: non-finite information entry", k);
    if (L[0] < 0.0 || L[2] < 0.0)
      return fail("ptzba_set_ray_priors: prior %d: negative diagonal entry %g of the information matrix", k,
                  L[0] < 0.0 ? L[0] : L[2]);
    if (L[1] * L[1] > L[0] * L[2] * (1.0 + 1e-12))
      return fail("ptzba_set_ray_priors: prior %d: information matrix not positive semi-definite (L01^2 = %g > L00 L11 = %g)",
                  k, L[1] * L[1], L[0] * L[2]);
  }
  std::vector<int32_t> order(n);
  for (int k = 0; k < n; ++k) order[k] = k;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return pr->landmark[a] < pr->landmark[b]; });
  std::vector<int32_t> lm, begin;
  std::vector<double> mean(2 * (size_t)n), info(3 * (size_t)n);
  for (int q = 0; q < n; ++q) {
    const int k = order[q], l = pr->landmark[k];
    if (lm.empty() || lm.back() != l) {
      lm.push_back(l);
      begin.push_back(q);
    }
    for (int e = 0; e < 2; ++e) mean[2 * (size_t)q + e] = pr->mean[2 * (size_t)k + e];
    for (int e = 0; e < 3; ++e) info[3 * (size_t)q + e] = pr->info[3 * (size_t)k + e];
  }
  begin.push_back(n);
  // queued work may still read the previous set's arrays
  HIPCHK(hipStreamSynchronize(h->st));
  auto& p = h->rp;
  p.n_prior = 0;
  p.n_lm = 0;
  if (upload(p.lm, lm, h->st) || upload(p.begin, begin, h->st) || upload(p.mean, mean, h->st) || upload(p.info, info, h->st))
    return -1;
  p.n_lm = (int)lm.size();
  p.n_prior = n;
  return 0;
}

int ptzba_ray_prior_info(ptzba_handle h, double* out4) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!out4) return fail("ptzba_ray_prior_info: null output");
  const auto& p = h->rp;
  out4[0] = p.n_prior;
  out4[1] = p.n_prior ? p.n_lm : 0;
  out4[2] = 2.0 * p.n_prior;
  out4[3] = 0.0;
  if (!h->has_ray_priors()) return 0;
  HIPCHK(hipSetDevice(h->device));
  if (!h->rp.cost.p && h->rp.cost.alloc(8)) return -1;
  launch_ray_prior_cost(ray_prior_args(h, nullptr, 0), h->rp.cost.as<double>(), 1.0, 0, h->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out4 + 3, h->rp.cost.p, 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}
