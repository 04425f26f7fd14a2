// ------------------------------------------------------------------------------------------------
// marginalisation of leaving keyframes (include/ptzba.h ptzba_marginal_prior; marg_kernels.hip)
// ------------------------------------------------------------------------------------------------
#include <algorithm>
#include <cmath>
#include <map>

#include "ba_ctx.h"

using namespace ptzba;

// the handle's marginal factor over the same state pair
MargArgs ptzba::marg_args(const ptzba_ctx* h, const int* sel, int flip) {
  const auto& m = h->mg;
  MargArgs a;
  a.n = m.n;
  a.frames = m.frames.as<int32_t>();
  a.lin = m.lin.as<double>();
  a.info = m.info.as<double>();
  a.eta = m.eta.as<double>();
  a.offset = m.offset;
  const PriorArgs s = prior_args(h, sel, flip);
  a.x0 = s.x0;
  a.x1 = s.x1;
  a.sel = s.sel;
  a.sel_xor = s.sel_xor;
  return a;
}

int ptzba_set_marginal_prior(ptzba_handle h, const ptzba_marginal* m) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (m && m->struct_size != (int32_t)sizeof(ptzba_marginal))
    return fail("ptzba_set_marginal_prior: unknown struct_size %d of ptzba_marginal (this library knows %d)",
                (int)m->struct_size, (int)sizeof(ptzba_marginal));
  HIPCHK(hipSetDevice(h->device));
  if (!m || m->n_frame == 0) {
    HIPCHK(hipStreamSynchronize(h->st));
    h->mg.n = 0;
    h->mg.h_frames.clear();
    if (!h->has_priors()) HIPCHK(hipMemsetAsync(h->locp() + 5, 0, 8, h->st));  // the trial-cost slot of the decisions
    return 0;
  }
  if (!single_rank(h))
    return fail("ptzba_set_marginal_prior: single rank only (the handle is sharded, has a communicator / hook attached "
                "or runs a caller-side exchange)");
  const int n = m->n_frame;
  if (n < 0 || !m->frames || !m->lin || !m->info || !m->grad)
    return fail("ptzba_set_marginal_prior: bad arguments (n_frame %d, null array)", n);
  if (n > PTZBA_MARG_MAX_FRAMES)
    return fail("ptzba_set_marginal_prior: %d frames (1..%d allowed)", n, PTZBA_MARG_MAX_FRAMES);
  const int n3 = 3 * n;
  std::vector<int32_t> frames(m->frames, m->frames + n);
  std::vector<double> lin(m->lin, m->lin + n3), eta(m->grad, m->grad + n3), L(m->info, m->info + (size_t)n3 * n3);
  for (int a = 0; a < n; ++a) {
    const int f = frames[a];
    if (f < h->n_fixed || f >= h->n_pose)
      return fail("ptzba_set_marginal_prior: frame %d is not a free frame [%d, %d)", f, h->n_fixed, h->n_pose);
    for (int c = 0; c < a; ++c)
      if (frames[c] == f) return fail("ptzba_set_marginal_prior: frame %d is named twice", f);
  }
  double amax = 0.0;
  for (double v : L) {
    if (!std::isfinite(v)) return fail("ptzba_set_marginal_prior: non-finite information entry");
    amax = std::max(amax, std::fabs(v));
  }
  if (!std::isfinite(m->offset)) return fail("ptzba_set_marginal_prior: non-finite offset");
  for (int e = 0; e < n3; ++e) {
    if (!std::isfinite(lin[e]) || !std::isfinite(eta[e]))
      return fail("ptzba_set_marginal_prior: non-finite linearisation point or gradient");
    if (L[(size_t)e * n3 + e] < 0.0)
      return fail("ptzba_set_marginal_prior: negative diagonal entry %g of the information matrix", L[(size_t)e * n3 + e]);
  }
  for (int i = 0; i < n3; ++i)
    for (int j = 0; j < i; ++j) {
      double &x = L[(size_t)i * n3 + j], &y = L[(size_t)j * n3 + i];
      if (std::fabs(x - y) > 1e-12 * amax)
        return fail("ptzba_set_marginal_prior: information matrix not symmetric (entries %d,%d differ by %g)", i, j,
                    std::fabs(x - y));
      x = y = 0.5 * (x + y);
    }
  for (int a = 0; a < n; ++a) {
    const int fa = frames[a];
    const int64_t pa = h->pos_host[fa];
    if (pa < 0 || pa + 2 >= h->n_aug) return fail("ptzba_set_marginal_prior: frame %d lies outside the reduced system", fa);
    for (int c = 0; c < n; ++c) {
      const int fb = frames[c];
      if (fa < fb && fb > h->win_host[fa])
        return fail("ptzba_set_marginal_prior: the factor couples frames %d and %d, but the handle's coupling window of "
                    "frame %d ends at %d: pass frame_win_hi[%d] >= %d to ptzba_set_problem", fa, fb, fa,
                    h->win_host[fa], fa, fb);
    }
  }
  HIPCHK(hipStreamSynchronize(h->st));  // queued work may still read the previous factor's arrays
  auto& g = h->mg;
  g.n = 0;
  if (upload(g.frames, frames, h->st) || upload(g.lin, lin, h->st) || upload(g.info, L, h->st) || upload(g.eta, eta, h->st))
    return -1;
  g.h_frames = frames;
  g.offset = m->offset;
  g.n = n;
  return 0;
}

int ptzba_marginal_prior_info(ptzba_handle h, double* out4) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!out4) return fail("ptzba_marginal_prior_info: null output");
  out4[0] = h->mg.n;
  out4[1] = 3 * h->mg.n;
  out4[2] = h->mg.n ? h->mg.offset : 0.0;
  out4[3] = 0.0;
  if (!h->has_marg()) return 0;
  HIPCHK(hipSetDevice(h->device));
  if (!h->mg.cost.p && h->mg.cost.alloc(8)) return -1;
  launch_marg_cost(marg_args(h, nullptr, 0), h->mg.cost.as<double>(), 0, h->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out4 + 3, h->mg.cost.p, 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

int ptzba_marginal_prior(ptzba_handle h, const ptzba_marg_opts* o, const int32_t* drop_frames, int32_t n_drop,
                         const uint8_t* drop_mask, int64_t n_mask, int32_t cap, int32_t* frames_out, int32_t* n_out,
                         double* lin_out, double* info_out, double* grad_out, double* offset_out,
                         ptzba_marg_stats* stats) {
  if (!h || !h->have_problem) return fail("no problem set");
  ptzba_marg_opts opt{(int32_t)sizeof(ptzba_marg_opts), 0, 0.0};
  if (o) {
    if (o->struct_size != (int32_t)sizeof(ptzba_marg_opts))
      return fail("ptzba_marginal_prior: unknown struct_size %d of ptzba_marg_opts (this library knows %d)",
                  (int)o->struct_size, (int)sizeof(ptzba_marg_opts));
    opt = *o;
  }
  if (stats && stats->struct_size != (int32_t)sizeof(ptzba_marg_stats))
    return fail("ptzba_marginal_prior: unknown struct_size %d of ptzba_marg_stats (this library knows %d)",
                (int)stats->struct_size, (int)sizeof(ptzba_marg_stats));
  const double pivot_tol = opt.pivot_tol == 0.0 ? 1e-13 : opt.pivot_tol;
  if (!(pivot_tol > 0.0) || !std::isfinite(pivot_tol)) return fail("ptzba_marginal_prior: bad options (pivot_tol)");
  if (!single_rank(h))
    return fail("ptzba_marginal_prior: single rank only (the handle is sharded, has a communicator / hook attached or "
                "runs a caller-side exchange)");
  if (h->trial_open || h->scal_deferred)
    return fail("ptzba_marginal_prior: an LM trial is pending (accept or reject it first; the call runs between solves)");
  if (n_drop < 0 || (n_drop > 0 && !drop_frames) || !n_out)
    return fail("ptzba_marginal_prior: bad arguments (n_drop %d, null array)", n_drop);
  if (n_mask != h->n_rec || (n_mask > 0 && !drop_mask))
    return fail("ptzba_marginal_prior: the record mask has %lld entries, the problem %lld records", (long long)n_mask,
                (long long)h->n_rec);
  if (frames_out && (!lin_out || !info_out || !grad_out || !offset_out))
    return fail("ptzba_marginal_prior: null output array");
  std::vector<uint8_t> in_E(h->n_pose, 0);
  std::vector<int32_t> E_free;
  for (int k = 0; k < n_drop; ++k) {
    const int f = drop_frames[k];
    if (f < 0 || f >= h->n_pose) return fail("ptzba_marginal_prior: leaving frame %d out of range [0, %d)", f, h->n_pose);
    if (in_E[f]) return fail("ptzba_marginal_prior: leaving frame %d is named twice", f);
    in_E[f] = 1;
    if (f >= h->n_fixed) E_free.push_back(f);
  }
  if ((int)E_free.size() > MARG_MAX_E)
    return fail("ptzba_marginal_prior: %d free leaving frames (at most %d)", (int)E_free.size(), MARG_MAX_E);
  HIPCHK(hipSetDevice(h->device));
  auto& g = h->mg;
  // the absorbed factors: every factor naming a free leaving frame, whole
  std::vector<int32_t> absorbed;
  for (int k = 0; k < h->pri.n_factor; ++k)
    for (int s = h->pri.h_begin[k]; s < h->pri.h_begin[k + 1]; ++s)
      if (in_E[h->pri.h_frames[s]]) {
        absorbed.push_back(k);
        break;
      }
  bool marg_absorbed = false;
  for (int s = 0; s < g.n; ++s) marg_absorbed |= in_E[g.h_frames[s]] != 0;
  // the weights of the dropped records, the frames and landmarks they touch
  const size_t e = h->elem();
  const size_t n_flag = 4 + (size_t)h->n_pose + (size_t)h->n_lm;  // [2 x uint64 counters | frame flags | landmark flags]
  if (g.w.reserve(((size_t)h->n_rec + 16) * e) || g.mask.reserve((size_t)h->n_rec + 16) || g.flags.reserve(n_flag * 4) ||
      g.dcost.reserve(64) || g.D_saved.reserve(h->D_pose.bytes + h->D_ray.bytes))
    return -1;
  for (auto& ev : g.ev)
    if (!ev) HIPCHK(hipEventCreate(&ev));
  if (!h->perm_uploaded) {
    if (upload(h->perm, h->perm_host, h->st)) return -1;
    h->perm_uploaded = true;
  }
  SyncOnExit sync_guard{h->st};  // caller buffers and the stack below outlive every queued copy, also on errors
  HIPCHK(hipEventRecord(g.ev[0], h->st));
  HIPCHK(hipMemsetAsync(g.flags.p, 0, n_flag * 4, h->st));
  if (h->n_rec) HIPCHK(hipMemcpyAsync(g.mask.p, drop_mask, (size_t)h->n_rec, hipMemcpyHostToDevice, h->st));
  auto* cnt = g.flags.as<unsigned long long>();
  int32_t* frame_flag = g.flags.as<int32_t>() + 4;
  int32_t* lm_flag = frame_flag + h->n_pose;
  if (h->precision == PTZBA_FP32)
    launch_marg_weights<float>(g.mask.as<uint8_t>(), h->perm.as<int64_t>(), h->weighted ? h->rec_w.p : nullptr,
                               h->rec_seg.as<int32_t>(), h->seg_frame.as<int32_t>(), h->seg_lm.as<int32_t>(), h->n_rec,
                               g.w.p, frame_flag, lm_flag, cnt, h->st);
  else
    launch_marg_weights<double>(g.mask.as<uint8_t>(), h->perm.as<int64_t>(), h->weighted ? h->rec_w.p : nullptr,
                                h->rec_seg.as<int32_t>(), h->seg_frame.as<int32_t>(), h->seg_lm.as<int32_t>(), h->n_rec,
                                g.w.p, frame_flag, lm_flag, cnt, h->st);
  HIPCHK(hipGetLastError());
  std::vector<int32_t> touched(h->n_pose, 0);
  unsigned long long counts[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(counts, cnt, 16, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(touched.data(), frame_flag, (size_t)h->n_pose * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (counts[0] == 0 && absorbed.empty() && !marg_absorbed)
    return fail("ptzba_marginal_prior: no record is dropped and no factor names a leaving frame: nothing to marginalise");
  // K: the free frames outside E with a dropped record or named by an absorbed factor, ascending
  for (int k : absorbed)
    for (int s = h->pri.h_begin[k]; s < h->pri.h_begin[k + 1]; ++s) touched[h->pri.h_frames[s]] = 1;
  if (marg_absorbed)
    for (int f : g.h_frames) touched[f] = 1;
  std::vector<int32_t> KE;
  for (int f = h->n_fixed; f < h->n_pose; ++f)
    if (touched[f] && !in_E[f]) KE.push_back(f);
  const int nK = (int)KE.size(), nE = (int)E_free.size();
  if (nK > MARG_MAX_K)
    return fail("ptzba_marginal_prior: the marginal would name %d frames (at most %d)", nK, MARG_MAX_K);
  *n_out = nK;
  if (stats) {
    stats->marginal_absorbed = marg_absorbed ? 1 : 0;
    stats->dropped_records = (int64_t)counts[0];
    stats->dropped_landmarks = (int64_t)counts[1];
    stats->n_absorbed = (int32_t)absorbed.size();
    if (stats->absorbed)
      for (int k = 0; k < std::min<int>(stats->absorbed_cap, (int)absorbed.size()); ++k) stats->absorbed[k] = absorbed[k];
    stats->min_pivot = 0.0;
    stats->device_ms = 0.0;
  }
  if (!frames_out) return 0;  // the size query
  if (cap < nK) return fail("ptzba_marginal_prior: the marginal names %d frames, the output arrays hold %d", nK, cap);
  KE.insert(KE.end(), E_free.begin(), E_free.end());
  const int N = 3 * (nK + nE), nK3 = 3 * nK;
  // rows of (K | E) in the system, their tiles and the pattern among those tiles
  std::map<int, int> tile_id;
  for (int f : KE) {
    const int64_t p = h->pos_host[f];
    if (p < 0 || p + 2 >= h->n_aug) return fail("ptzba_marginal_prior: frame %d lies outside the reduced system", f);
    for (int q = 0; q < 3; ++q) tile_id.emplace((int)((p + q) / CHOL_NB), 0);
  }
  int nt = 0;
  for (auto& kv : tile_id) kv.second = nt++;
  std::vector<int32_t> row_tile(N);
  for (int i = 0; i < N; ++i) row_tile[i] = tile_id[(int)((h->pos_host[KE[i / 3]] + i % 3) / CHOL_NB)];
  std::vector<uint8_t> pat((size_t)nt * nt, 0);
  for (size_t q = 0; q + 1 < h->zt_host.size(); q += 2) {
    const auto a = tile_id.find(h->zt_host[q]), b = tile_id.find(h->zt_host[q + 1]);
    if (a != tile_id.end() && b != tile_id.end()) pat[(size_t)a->second * nt + b->second] = 1;
  }
  // the absorbed factors' descriptors: the pose priors in list order, then the handle's marginal
  std::vector<int32_t> loc_of(h->n_pose, -1), fac_frames, fac_loc;
  for (int i = 0; i < nK + nE; ++i) loc_of[KE[i]] = i;
  std::vector<MargFactor> fac;
  {
    int64_t info_off = 0;
    size_t a = 0;
    for (int k = 0; k < h->pri.n_factor; ++k) {
      const int f0 = h->pri.h_begin[k], G = h->pri.h_begin[k + 1] - f0;
      if (a < absorbed.size() && absorbed[a] == k) {
        ++a;
        fac.push_back(MargFactor{3 * G, (int)fac_frames.size(), h->pri.f_info.as<double>() + info_off,
                                 h->pri.f_mean.as<double>() + 3 * (int64_t)f0, nullptr, 0.0});
        for (int s = 0; s < G; ++s) {
          fac_frames.push_back(h->pri.h_frames[f0 + s]);
          fac_loc.push_back(loc_of[h->pri.h_frames[f0 + s]]);
        }
      }
      info_off += (int64_t)9 * G * G;
    }
  }
  if (marg_absorbed) {
    fac.push_back(MargFactor{3 * g.n, (int)fac_frames.size(), g.info.as<double>(), g.lin.as<double>(), g.eta.as<double>(),
                             g.offset});
    for (int f : g.h_frames) {
      fac_frames.push_back(f);
      fac_loc.push_back(loc_of[f]);
    }
  }
  for (int l : fac_loc)
    if (l < 0) return fail("ptzba_marginal_prior: an absorbed factor names a fixed frame");
  const size_t n_outd = (size_t)nK3 * nK3 + 2 * (size_t)nK3 + 4;
  if (g.out.reserve(n_outd * 8) || upload(g.kframes, KE, h->st) || upload(g.row_tile, row_tile, h->st) ||
      upload(g.pat, pat, h->st) || upload(g.fac, fac, h->st) || upload(g.fac_frames, fac_frames, h->st) ||
      upload(g.fac_loc, fac_loc, h->st))
    return -1;
  // the caller's run state this call borrows: the robust losses' ("huber") curvature, damping, timing groups, K1's weight array
  struct Restore {
    ptzba_ctx* h;
    double hcurv, lambda;
    int timing;
    ~Restore() { h->hcurv = hcurv; h->lambda = lambda; h->timing = timing; h->w_override = nullptr; }
  } restore{h, h->hcurv, h->lambda, h->timing};
  h->hcurv = 1.0;
  h->lambda = 0.0;
  h->timing = 0;
  // the Marquardt scales are a monotone memory of the run: a build raises them, so they are put back afterwards
  double* dsave = g.D_saved.as<double>();
  HIPCHK(hipMemcpyAsync(dsave, h->D_pose.p, h->D_pose.bytes, hipMemcpyDeviceToDevice, h->st));
  HIPCHK(hipMemcpyAsync(dsave + h->D_pose.bytes / 8, h->D_ray.p, h->D_ray.bytes, hipMemcpyDeviceToDevice, h->st));
  // D alone: K1's weighted instantiation over the mask, the solver's own build at lambda = 0 without the priors
  h->w_override = g.w.p;
  tables(h, h->ptz.as<double>(), h->rays.as<double>());
  linearize_into(h, h->cur);
  launch_reduce_cols(h->lm_out[h->cur].as<double>() + 5, h->n_lm, 8, 1, 0, g.dcost.as<double>(), h->red_scratch.as<double>(),
                     h->st);
  if (build_impl(h, 0.0, nullptr, nullptr, nullptr, false)) return -1;
  EliminateArgs a;
  a.nK = nK;
  a.nE = nE;
  a.frames = g.kframes.as<int32_t>();
  a.frame_pos = h->frame_pos.as<int32_t>();
  a.S = h->S();
  a.b = h->bvec();
  a.ld = h->ld;
  a.row_tile = g.row_tile.as<int32_t>();
  a.pat = g.pat.as<uint8_t>();
  a.n_tile = nt;
  a.n_factor = (int)fac.size();
  a.factors = g.fac.as<MargFactor>();
  a.fac_frames = g.fac_frames.as<int32_t>();
  a.fac_loc = g.fac_loc.as<int32_t>();
  a.x = h->ptz.as<double>();
  a.dcost = g.dcost.as<double>();
  a.pivot_tol = pivot_tol;
  a.out = g.out.as<double>();
  launch_marg_eliminate(a, h->st);
  HIPCHK(hipGetLastError());
  // the handle back as ptzba_linearize leaves it: the problem's own weights, the full linearisation, the scales
  h->w_override = nullptr;
  HIPCHK(hipMemcpyAsync(h->D_pose.p, dsave, h->D_pose.bytes, hipMemcpyDeviceToDevice, h->st));
  HIPCHK(hipMemcpyAsync(h->D_ray.p, dsave + h->D_pose.bytes / 8, h->D_ray.bytes, hipMemcpyDeviceToDevice, h->st));
  if (ptzba_linearize(h)) return -1;
  HIPCHK(hipEventRecord(g.ev[1], h->st));
  // the elimination's verdict first: nothing is copied out of a failed one
  double tail[4] = {0, 0, 0, 0};
  const double* outd = g.out.as<double>();
  HIPCHK(hipMemcpyAsync(tail, outd + (size_t)nK3 * nK3 + 2 * (size_t)nK3, 32, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (tail[2] != 0.0) {
    const int row = (int)tail[2] - 1;
    return fail("ptzba_marginal_prior: leaving frame %d is not determined by the dropped records and absorbed factors "
                "(pivot %g of A_EE at its parameter %d, largest diagonal entry %g): it cannot be marginalised",
                E_free[std::min(row / 3, nE - 1)], tail[1], row % 3, tail[3]);
  }
  if (!std::isfinite(tail[0])) return fail("ptzba_marginal_prior: non-finite offset");
  if (nK3) {
    HIPCHK(hipMemcpyAsync(info_out, outd, (size_t)nK3 * nK3 * 8, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipMemcpyAsync(grad_out, outd + (size_t)nK3 * nK3, (size_t)nK3 * 8, hipMemcpyDeviceToHost, h->st));
    HIPCHK(hipMemcpyAsync(lin_out, outd + (size_t)nK3 * nK3 + nK3, (size_t)nK3 * 8, hipMemcpyDeviceToHost, h->st));
  }
  HIPCHK(hipStreamSynchronize(h->st));
  std::copy(KE.begin(), KE.begin() + nK, frames_out);
  *offset_out = tail[0];
  if (stats) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
    stats->min_pivot = tail[1];
    stats->device_ms = (double)ms;
  }
  return 0;
}
