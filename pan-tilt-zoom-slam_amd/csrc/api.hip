// libptzba C-ABI (see include/ptzba.h): host-side problem preparation (native C++: stable counting
// sorts into landmark-major records, segment / landmark / frame CSR, work ordering), device buffer
// ownership, and the Levenberg-Marquardt step sequence over the gfx950 kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "ptzba_common.h"
#include "par_util.h"
#include "ba_ctx.h"
#include "chol_plan.h"
#include "problem_layout.h"
#include "robust_loss.h"

using namespace ptzba;

static size_t g_total_bytes(std::initializer_list<const DBuf*> l) {
  size_t s = 0;
  for (auto* b : l) s += b->bytes;
  return s;
}


// Cold-cache K1 timing: 16-B vector stores over a scratch buffer larger than L2 + Infinity Cache (256 MB
// MALL, MI355X_MICROARCH.md) evict the record stream before the timed launch, so K1 reads from HBM.
// ptzba_restore_state: state <- snapshot, Marquardt scales <- 0
__global__ void __launch_bounds__(256) k_restore_state(double* __restrict__ ptz, const double* __restrict__ ptz_saved,
                                                       int64_t n_ptz, double* __restrict__ rays,
                                                       const double* __restrict__ rays_saved, int64_t n_rays,
                                                       double* __restrict__ D_pose, int64_t n_dp,
                                                       double* __restrict__ D_ray, int64_t n_dr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_ptz) ptz[i] = ptz_saved[i];
  if (i < n_rays) rays[i] = rays_saved[i];
  if (i < n_dp) D_pose[i] = 0.0;
  if (i < n_dr) D_ray[i] = 0.0;
}

__global__ void __launch_bounds__(256) k_flush_caches(float4* buf, int64_t n16, float v) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x)
    buf[i] = make_float4(v, v, v, v);
}
// the read flush: streams the scratch buffer (filled once by k_flush_caches) through the caches, leaving clean lines;
// the sum is stored only if it equals an impossible value (the buffer holds small positive numbers), which keeps the
// loads alive
__global__ void __launch_bounds__(256) k_flush_caches_read(float4* buf, int64_t n16, float v) {
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 x = buf[i];
    s += x.x + x.y + x.z + x.w;
  }
  if (s == -v) buf[0] = make_float4(s, s, s, s);
}
constexpr size_t FLUSH_BYTES = (size_t)1 << 30;

// a timed group records an event pair around every tm_stride-th launch (each record adds a gap to the
// stream; sampling keeps that overhead out of most launches)
void ptzba::tm_begin(ptzba_ctx* h, int k) {
  h->tm_sampled[k] = false;
  if (!((h->timing >> k) & 1) || h->ev_used[k] + 2 > (int)h->ev[k].size()) return;
  if (h->tm_seen[k]++ % h->tm_stride != 0) return;
  h->tm_sampled[k] = true;
  if (k == TM_K1 && h->tm_flush && h->flush_buf.p) {
    if (h->tm_flush_read)
      k_flush_caches_read<<<4096, 256, 0, h->st>>>(h->flush_buf.as<float4>(), (int64_t)(h->flush_buf.bytes / 16), 1.0f);
    else
      k_flush_caches<<<4096, 256, 0, h->st>>>(h->flush_buf.as<float4>(), (int64_t)(h->flush_buf.bytes / 16),
                                               (float)h->tm_seen[k]);
  }
  if (k == TM_K1) return;  // K1 carries its event pair in its own launch (tm_k1_events)
  (void)hipEventRecord(h->ev[k][h->ev_used[k]], h->st);
}
void ptzba::tm_end(ptzba_ctx* h, int k) {
  if (!h->tm_sampled[k]) return;
  if (k != TM_K1) (void)hipEventRecord(h->ev[k][h->ev_used[k] + 1], h->st);
  h->ev_used[k] += 2;
  h->tm_sampled[k] = false;
}
// the event pair of a sampled K1 launch, for hipExtLaunchKernelGGL (the kernel packet's own start / end timestamps:
// the figure rocprofv3 reports, without the marker packets' dispatch gaps); nullptrs when this launch is not sampled
hipEvent_t ptzba::tm_k1_event(ptzba_ctx* h, int which) {
  return h->tm_sampled[TM_K1] ? h->ev[TM_K1][h->ev_used[TM_K1] + which] : nullptr;
}

const char* ptzba_last_error(void) { return g_err.c_str(); }
// 0.2 (round 6): ptzba_lm_opts carries huber_curvature / curvature_switch (11 fields; 0.1 had 9).  They are read
// for the robust losses only (0.9: every one, Huber alone before), and huber_curvature 0 means the default 0.1, so a zero-filled tail keeps 0.1's behaviour.
// 0.3: ptzba_covariance / ptzba_cov_opts (sized by its struct_size field); ptzba_lm_opts as in 0.2.
// 0.4: ptzba_set_pose_priors / ptzba_pose_priors (sized by struct_size) / ptzba_pose_prior_info.
// 0.5: ptzba_marginal_prior / ptzba_set_marginal_prior / ptzba_marginal_prior_info (structs sized by struct_size).
// 0.6: ptzba_set_ray_priors / ptzba_ray_priors (sized by struct_size) / ptzba_ray_prior_info.
// 0.7: ptzba_build_info (read-only counters of the builds' launch path).
// 0.8: ptzba_covariance_joint (ptzba_cov_opts as 0.3).
// 0.9: PTZBA_LOSS_SOFT_L1 / _CAUCHY / _ARCTAN (no struct changes; huber_curvature / curvature_switch are read for
// every robust loss); ptzba_set_displacement / ptzba_displacement_info (no struct changes).
// 0.10: ptz_refine_poses_disp / ptz_pose_ransac_disp / ptz_back_project_rays_exact (new entry points, no struct changes).
const char* ptzba_version(void) {
  return "ptzba 0.10 gfx950 (ptzba_lm_opts: 11 fields as 0.2; ptzba_covariance as 0.3; ptzba_set_pose_priors as 0.4; "
         "ptzba_marginal_prior as 0.5; ptzba_set_ray_priors as 0.6; ptzba_build_info as 0.7; ptzba_covariance_joint "
         "as ptzba 0.8; losses soft_l1 / cauchy / arctan; ptzba_set_displacement as 0.9; ptz_refine_poses_disp, "
         "ptz_pose_ransac_disp, ptz_back_project_rays_exact)";
}

ptzba_handle ptzba_new(int device) {
  if (select_device(device)) return nullptr;
  auto* h = new ptzba_ctx();
  h->device = device;
  if (hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    fail("hipStreamCreate failed");
    return nullptr;
  }
  h->st = h->own;
  return h;
}

void ptzba_delete(ptzba_handle h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->st) (void)hipStreamSynchronize(h->st);
  for (int k = 0; k < TM_N; ++k)
    for (auto e : h->ev[k]) (void)hipEventDestroy(e);
  for (auto e : h->cev) (void)hipEventDestroy(e);
  for (auto e : h->cov.ev)
    if (e) (void)hipEventDestroy(e);
  if (h->own) (void)hipStreamDestroy(h->own);
  if (h->scal_host) (void)hipHostFree(h->scal_host);
  if (h->out_pin) (void)hipHostFree(h->out_pin);
  if (h->bsp_err) (void)hipHostFree(h->bsp_err);
  if (h->stage) (void)hipHostFree(h->stage);
  h->drop_groups();
  if (h->lm_host) (void)hipHostFree(h->lm_host);
  delete h;
}

int ptzba_set_stream(ptzba_handle h, void* stream) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->st));  // work already queued on the previous stream completes first
  h->st = (hipStream_t)stream;          // NULL = the default stream (torch's current_stream() is often it)
  return 0;
}

int ptzba_use_own_stream(ptzba_handle h) { return h ? ptzba_set_stream(h, h->own) : fail("null handle"); }

constexpr size_t STAGE_MIN_CAP = 8u << 20;
constexpr int STAGE_OPS_PER_LAUNCH = 48;
struct StageScatterArgs {
  const uint8_t* src;
  int n_ops;
  uint8_t* dst[STAGE_OPS_PER_LAUNCH];
  uint64_t off[STAGE_OPS_PER_LAUNCH];  // ~0: zero fill
  uint64_t n[STAGE_OPS_PER_LAUNCH];
};
// every op's bytes over the grid: 16-B vectors when both ends are 16-B aligned (staging offsets and device
// allocations are 256-B aligned), the tail (or an unaligned op) byte by byte
__global__ __launch_bounds__(256) void k_stage_scatter(StageScatterArgs a) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
  for (int q = 0; q < a.n_ops; ++q) {
    uint8_t* d = a.dst[q];
    const bool zero = a.off[q] == ~(uint64_t)0;
    const uint8_t* sp = zero ? nullptr : a.src + a.off[q];
    const bool vec = (((uintptr_t)d | (uintptr_t)sp) & 15) == 0;  // (a sub-buffer fill may start unaligned)
    const size_t n = a.n[q], n16 = vec ? n / 16 : 0;
    for (size_t i = tid; i < n16; i += nt)
      reinterpret_cast<uint4*>(d)[i] = zero ? make_uint4(0, 0, 0, 0) : reinterpret_cast<const uint4*>(sp)[i];
    for (size_t i = 16 * n16 + tid; i < n; i += nt) d[i] = zero ? 0 : sp[i];
  }
}
// lands the queued staged uploads and zero fills (stream-ordered after everything queued before)
int ptzba::flush_stage(ptzba_ctx* h) {
  if (h->stage_ops.empty()) return 0;
  bool any_copy = false;
  for (const auto& o : h->stage_ops) any_copy |= o.off != SIZE_MAX;
  if (any_copy) {
    if (h->stage_dev.reserve(h->stage_cap)) return -1;
    HIPCHK(hipMemcpyAsync(h->stage_dev.p, h->stage, h->stage_used, hipMemcpyHostToDevice, h->st));
  }
  size_t tot = 0;
  for (const auto& o : h->stage_ops) tot += o.n;
  const unsigned blocks = (unsigned)std::min<size_t>(1024, std::max<size_t>(1, tot / 32768));
  for (size_t q0 = 0; q0 < h->stage_ops.size(); q0 += STAGE_OPS_PER_LAUNCH) {
    StageScatterArgs a{};
    a.src = h->stage_dev.as<uint8_t>();
    a.n_ops = (int)std::min<size_t>(STAGE_OPS_PER_LAUNCH, h->stage_ops.size() - q0);
    for (int q = 0; q < a.n_ops; ++q) {
      const auto& o = h->stage_ops[q0 + q];
      a.dst[q] = (uint8_t*)o.dst;
      a.off[q] = o.off == SIZE_MAX ? ~(uint64_t)0 : (uint64_t)o.off;
      a.n[q] = o.n;
    }
    hipLaunchKernelGGL(k_stage_scatter, dim3(blocks), dim3(256), 0, h->st, a);
    HIPCHK(hipGetLastError());
  }
  h->stage_ops.clear();
  return 0;
}
// n zero bytes at p on the handle's stream (queued with the staged uploads while set_problem batches them)
int ptzba::zero_async(ptzba_ctx* h, void* p, size_t n) {
  if (!p || !n) return 0;
  if (h->stage_batch) {
    h->stage_ops.push_back({p, SIZE_MAX, n});
    return 0;
  }
  HIPCHK(hipMemsetAsync(p, 0, n, h->st));
  return 0;
}
// a pinned staging slot of n bytes for one queued copy (*out = nullptr when n is too large for the staging path)
int ptzba::stage_take(ptzba_ctx* h, size_t n, uint8_t** out) {
  *out = nullptr;
  if (n > STAGE_MAX) return 0;
  size_t off = (h->stage_used + 255) & ~(size_t)255;
  if (!h->stage || off + n > h->stage_cap) {
    if (flush_stage(h)) return -1;         // the queued copies read the staging buffer: land them first
    HIPCHK(hipStreamSynchronize(h->st));  // every staged copy so far has landed
    off = 0;
    if (!h->stage) {
      HIPCHK(hipHostMalloc((void**)&h->stage, STAGE_MIN_CAP, hipHostMallocDefault));
      h->stage_cap = STAGE_MIN_CAP;
    }
  }
  *out = h->stage + off;
  h->stage_used = off + n;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// records hold obs - base(segment) in `real`; the per-segment base observation stays fp64, so the
// per-record arithmetic of K1 works on O(residual) magnitudes even in fp32
// the host fronts' stored records, converted once (layout_convert_records): the merge pass compares them, the upload
// copies them
struct HostRecords {
  std::vector<double> seg_base;
  std::vector<uint8_t> xy, w;  // [2 n_rec] / [n_rec] (empty: unweighted) in the record precision
};
template <typename real>
static void convert_records(const ProblemLayout& L, int64_t n_obs, const double* obs_xy, const double* w, HostRecords& hr) {
  hr.xy.resize(2 * (size_t)n_obs * sizeof(real));
  hr.w.resize(w ? (size_t)n_obs * sizeof(real) : 0);
  layout_convert_records<real>(L, n_obs, obs_xy, w, hr.seg_base, reinterpret_cast<real*>(hr.xy.data()),
                               reinterpret_cast<real*>(hr.w.data()));
}
static int upload_records(ptzba_ctx* h, const HostRecords& hr) {
  // the copies below read host vectors of set_problem: every exit path (errors included) waits for the handle's
  // stream first (the stream does not order itself behind the legacy null stream, so every upload / memset of
  // set_problem goes on h->st)
  const size_t e = h->elem(), bxy = hr.xy.size(), bw = hr.w.size();
  // allocate everything before queuing any copy; padded by 8 records: K1's coarsened loads read whole groups
  if (h->rec_xy.alloc(bxy + 16 * e)) return -1;
  if (bw) {
    if (h->rec_w.alloc(bw)) return -1;
  } else {
    h->rec_w.release();
  }
  // small problems (a sliding window's ~170K records) go through the pinned staging buffer with set_problem's other
  // staged uploads; large ones copy from the vectors with a synchronisation
  uint8_t *pxy = nullptr, *pw = nullptr;
  if (stage_take(h, bxy, &pxy)) return -1;
  if (pxy && bw && stage_take(h, bw, &pw)) return -1;
  const bool staged = pxy && (!bw || pw);
  struct SyncIf {  // the vector path: every exit waits for the copies reading the vectors (errors included)
    hipStream_t s;
    bool on;
    ~SyncIf() {
      if (on) (void)hipStreamSynchronize(s);
    }
  } sync_guard{h->st, !staged};
  uint8_t* pad = h->rec_xy.as<uint8_t>() + bxy;
  if (staged) {
    std::memcpy(pxy, hr.xy.data(), bxy);
    if (bw) std::memcpy(pw, hr.w.data(), bw);
    if (h->stage_batch) {  // queued with set_problem's other staged uploads
      h->stage_ops.push_back({h->rec_xy.p, (size_t)(pxy - h->stage), bxy});
      if (bw) h->stage_ops.push_back({h->rec_w.p, (size_t)(pw - h->stage), bw});
      return zero_async(h, pad, 16 * e);
    }
  }
  HIPCHK(hipMemcpyAsync(h->rec_xy.p, staged ? pxy : hr.xy.data(), bxy, hipMemcpyHostToDevice, h->st));
  HIPCHK(hipMemsetAsync(pad, 0, 16 * e, h->st));
  if (bw) HIPCHK(hipMemcpyAsync(h->rec_w.p, staged ? pw : hr.w.data(), bw, hipMemcpyHostToDevice, h->st));
  return 0;
}

// set_problem's device front for large problems (setup_kernels.hip): the records' (landmark, frame, index) order,
// segments and device record arrays (rec_seg, seg_frame / seg_lm / seg_rec_begin, seg_base, rec_xy / rec_w, rec_key,
// perm), bit for bit what the host path uploads; returns the per-segment arrays the host passes read (seg_rec_begin
// with the end entry)
// From 64K records on (round 6; 4M before): a 30-keyframe window's ~170K records take 1.3 ms on the device front against
// 2.2 ms on the host (set_problem per keyframe, config 5: keyframe BA 8.7-9.2 -> 7.9-8.1 ms mean, profiles/r06f_*)
constexpr int64_t GPU_SETUP_MIN_REC = (int64_t)1 << 16;
static int gpu_front(ptzba_ctx* h, int64_t n, int n_pose, int n_lm, const int32_t* frame, const int32_t* lm,
                     const double* xy, const double* w, bool merge, ProblemLayout& L) {
  auto &seg_frame = L.seg_frame, &seg_lm = L.seg_lm;
  auto& seg_rec_begin = L.seg_rec_begin;
  DBuf order, key;
  int64_t ns = 0;
  {
    DBuf d_frame, d_lm;
    if (d_frame.alloc(4 * (size_t)n) || d_lm.alloc(4 * (size_t)n) || order.alloc(4 * (size_t)n) ||
        key.alloc(4 * (size_t)n) || h->rec_seg.alloc(4 * (size_t)n))
      return -1;
    HIPCHK(hipMemcpyAsync(d_frame.p, frame, 4 * (size_t)n, hipMemcpyHostToDevice, h->st));
    HIPCHK(hipMemcpyAsync(d_lm.p, lm, 4 * (size_t)n, hipMemcpyHostToDevice, h->st));
    // (synchronises: the inputs die here)
    if (setup_sort_runs(h->st, n, n_pose, n_lm, d_frame.as<int32_t>(), d_lm.as<int32_t>(), order.as<uint32_t>(),
                        key.as<uint32_t>(), h->rec_seg.as<int32_t>(), &ns))
      return -1;
  }
  if (ns >= INT32_MAX - 1) return fail("too many segments");
  DBuf lm_first;
  if (h->seg_frame.alloc(4 * (size_t)ns) || h->seg_lm.alloc(4 * (size_t)ns) || h->seg_rec_begin.alloc(8 * (size_t)(ns + 1)) ||
      lm_first.alloc(4 * (size_t)std::max(n_lm, 1)))
    return -1;
  if (setup_fill_segments(h->st, n, n_pose, ns, key.as<uint32_t>(), h->rec_seg.as<int32_t>(), h->seg_frame.as<int32_t>(),
                          h->seg_lm.as<int32_t>(), h->seg_rec_begin.as<int64_t>(), lm_first.as<int32_t>()))
    return -1;
  seg_frame.resize(ns);
  seg_lm.resize(ns);
  seg_rec_begin.resize(ns + 1);
  HIPCHK(hipMemcpyAsync(seg_frame.data(), h->seg_frame.p, 4 * (size_t)ns, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(seg_lm.data(), h->seg_lm.p, 4 * (size_t)ns, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipMemcpyAsync(seg_rec_begin.data(), h->seg_rec_begin.p, 8 * (size_t)(ns + 1), hipMemcpyDeviceToHost, h->st));
  // the records: the raw observations up, the deltas from each segment's base in the record precision
  const size_t e = h->elem();
  DBuf d_xy, d_w;
  if (d_xy.alloc(16 * (size_t)n) || (w && d_w.alloc(8 * (size_t)n)) || h->seg_base.alloc(16 * (size_t)ns) ||
      h->rec_xy.alloc((2 * (size_t)n + 16) * e) || h->rec_key.alloc((size_t)n + 8) || h->perm.alloc(8 * (size_t)n))
    return -1;
  if (w) {
    if (h->rec_w.alloc((size_t)n * e)) return -1;
  } else {
    h->rec_w.release();
  }
  HIPCHK(hipMemcpyAsync(d_xy.p, xy, 16 * (size_t)n, hipMemcpyHostToDevice, h->st));
  if (w) HIPCHK(hipMemcpyAsync(d_w.p, w, 8 * (size_t)n, hipMemcpyHostToDevice, h->st));
  const int rc = h->precision == PTZBA_FP32
                     ? setup_records<float>(h->st, n, ns, order.as<uint32_t>(), h->rec_seg.as<int32_t>(),
                                            h->seg_lm.as<int32_t>(), h->seg_rec_begin.as<int64_t>(), lm_first.as<int32_t>(),
                                            d_xy.as<double>(), w ? d_w.as<double>() : nullptr, h->seg_base.as<double>(),
                                            h->rec_xy.as<float>(), w ? h->rec_w.as<float>() : nullptr,
                                            h->rec_key.as<uint8_t>(), h->perm.as<int64_t>())
                     : setup_records<double>(h->st, n, ns, order.as<uint32_t>(), h->rec_seg.as<int32_t>(),
                                             h->seg_lm.as<int32_t>(), h->seg_rec_begin.as<int64_t>(), lm_first.as<int32_t>(),
                                             d_xy.as<double>(), w ? d_w.as<double>() : nullptr, h->seg_base.as<double>(),
                                             h->rec_xy.as<double>(), w ? h->rec_w.as<double>() : nullptr,
                                             h->rec_key.as<uint8_t>(), h->perm.as<int64_t>());
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(h->rec_xy.as<uint8_t>() + 2 * (size_t)n * e, 0, 16 * e, h->st));  // K1's padded record groups
  HIPCHK(hipMemsetAsync(h->rec_key.as<uint8_t>() + n, 0, 8, h->st));
  // K1's merged stream: the runs flagged and scanned over the stored records (the sort's order and keys are dead: the
  // scan's scratch); built when the runs are at most half the records, with the padding K1 relies on above
  DBuf m_first;
  L.n_merged = n;
  L.k1_merged = false;
  if (merge && 2 * ns <= n) {  // (a run never spans segments: more segments than half the records cannot halve them)
    int64_t nm = 0;
    const int32_t* rs = h->rec_seg.as<int32_t>();
    if (h->precision == PTZBA_FP32
            ? setup_merge_runs<float>(h->st, n, rs, h->rec_xy.as<float>(), w ? h->rec_w.as<float>() : nullptr,
                                      key.as<int32_t>(), order.as<int32_t>(), &nm)
            : setup_merge_runs<double>(h->st, n, rs, h->rec_xy.as<double>(), w ? h->rec_w.as<double>() : nullptr,
                                       key.as<int32_t>(), order.as<int32_t>(), &nm))
      return -1;
    L.n_merged = nm;
    L.k1_merged = k1_merge_pays(nm, n);
  }
  if (L.k1_merged) {
    const int64_t nm = L.n_merged;
    if (m_first.alloc(4 * (size_t)(nm + 1)) || h->m_rec_xy.alloc((2 * (size_t)nm + 16) * e) || h->m_rec_w.alloc((size_t)nm * e) ||
        h->m_rec_key.alloc((size_t)nm + 8) || h->m_seg_rec_begin.alloc(8 * (size_t)(ns + 1)))
      return -1;
    const int32_t* rs = h->rec_seg.as<int32_t>();
    if (h->precision == PTZBA_FP32
            ? setup_merge_fill<float>(h->st, n, ns, nm, rs, order.as<int32_t>(), h->rec_xy.as<float>(),
                                      w ? h->rec_w.as<float>() : nullptr, h->rec_key.as<uint8_t>(), m_first.as<uint32_t>(),
                                      h->m_rec_xy.as<float>(), h->m_rec_w.as<float>(), h->m_rec_key.as<uint8_t>(),
                                      h->m_seg_rec_begin.as<int64_t>())
            : setup_merge_fill<double>(h->st, n, ns, nm, rs, order.as<int32_t>(), h->rec_xy.as<double>(),
                                       w ? h->rec_w.as<double>() : nullptr, h->rec_key.as<uint8_t>(), m_first.as<uint32_t>(),
                                       h->m_rec_xy.as<double>(), h->m_rec_w.as<double>(), h->m_rec_key.as<uint8_t>(),
                                       h->m_seg_rec_begin.as<int64_t>()))
      return -1;
    HIPCHK(hipMemsetAsync(h->m_rec_xy.as<uint8_t>() + 2 * (size_t)nm * e, 0, 16 * e, h->st));
    HIPCHK(hipMemsetAsync(h->m_rec_key.as<uint8_t>() + nm, 0, 8, h->st));
    L.m_seg_rec_begin.resize(ns + 1);
    HIPCHK(hipMemcpyAsync(L.m_seg_rec_begin.data(), h->m_seg_rec_begin.p, 8 * (size_t)(ns + 1), hipMemcpyDeviceToHost, h->st));
  }
  HIPCHK(hipStreamSynchronize(h->st));  // the temporaries and the host vectors' copies above complete here
  return 0;
}

// the host fronts' merged stream (ProblemLayout::m_first): each run's stored record, its key, multiplicity x user weight
template <typename real>
static int upload_merged(ptzba_ctx* h, const ProblemLayout& L, const HostRecords& hr) {
  const int64_t nm = L.n_merged;
  const real* sxy = reinterpret_cast<const real*>(hr.xy.data());
  const real* sw = hr.w.empty() ? nullptr : reinterpret_cast<const real*>(hr.w.data());
  std::vector<real> xy(2 * (size_t)nm + 16, (real)0), ww((size_t)nm);  // + 8 records, + 8 keys: K1 reads whole groups
  std::vector<uint8_t> key((size_t)nm + 8, 0);
  parallel_chunks(nm, host_threads(nm), [&](int64_t lo, int64_t hi, int) {
    for (int64_t m = lo; m < hi; ++m) {
      const int64_t k = L.m_first[m];
      const int32_t sg = L.rec_seg[k];
      xy[2 * m] = sxy[2 * k];
      xy[2 * m + 1] = sxy[2 * k + 1];
      ww[m] = (real)(L.m_first[m + 1] - k) * (sw ? sw[k] : (real)1);
      key[m] = (uint8_t)((sg - L.lm_seg_begin[L.seg_lm[sg]]) % K1_SEGW);
    }
  });
  return upload_st(h, h->m_rec_xy, xy) || upload_st(h, h->m_rec_w, ww) || upload_st(h, h->m_rec_key, key) ||
                 upload_st(h, h->m_seg_rec_begin, L.m_seg_rec_begin)
             ? -1
             : 0;
}

// host phase times of a set_problem call (ptzba_setup_timing: where a config-4 set_problem spends its seconds)
struct PhaseClock {
  ptzba_ctx* h;
  std::chrono::steady_clock::time_point t0;
  void operator()(const char* what) {
    const auto t = std::chrono::steady_clock::now();
    h->setup_phases.emplace_back(what, std::chrono::duration<double, std::milli>(t - t0).count());
    t0 = t;
  }
};

// set_problem's second half: the records (host fronts), the layout, the plan and the back-solve form onto the device,
// every solver buffer allocated and initialised.  The staged batch is one copy plus one scatter: its layout follows the
// call order below.
static int upload_problem(ptzba_ctx* h, const ProblemLayout& L, const SysOrder& sorder, const CholPlan& plan,
                          const TreePlan& tplan, bool gpu_setup, bool part_mode, const std::vector<uint8_t>& row_phase,
                          const std::vector<uint8_t>& fmask, const HostRecords& hr, PhaseClock& st_mark) {
  const int n_pose = h->n_pose, n_landmark = h->n_lm;
  const int64_t n_obs = h->n_rec;
  // ---- upload (staged: the stream has drained, so the staging buffer is free)
  HIPCHK(hipStreamSynchronize(h->st));
  h->stage_used = 0;
  h->stage_ops.clear();
  // the staged uploads / zero fills land with one copy + one scatter launch (0.73 -> 0.66 ms per config-5 call, r04z4)
  h->stage_batch = true;
  struct BatchOff {  // every exit (errors included) leaves the batching off
    ptzba_ctx* h;
    ~BatchOff() { h->stage_batch = false; }
  } batch_off{h};
  st_mark("pre-upload sync");
  if (!gpu_setup) {  // (the device front has built these on the device)
    if (upload_records(h, hr)) return -1;
    if (upload_st(h, h->seg_base, hr.seg_base)) return -1;
    {  // K1's 1-byte segment key: the record's segment within its landmark's window of K1_SEGW segments
      std::vector<uint8_t> key(n_obs + 8);  // + 8: K1 reads whole 8-record key groups
      for (int64_t k = 0; k < n_obs; ++k) {
        const int32_t sg = L.rec_seg[k];
        key[k] = (uint8_t)((sg - L.lm_seg_begin[L.seg_lm[sg]]) % K1_SEGW);
      }
      if (upload_st(h, h->rec_key, key)) return -1;
    }
    if (upload_st(h, h->rec_seg, L.rec_seg) || upload_st(h, h->seg_frame, L.seg_frame) || upload_st(h, h->seg_lm, L.seg_lm) ||
        upload_st(h, h->seg_rec_begin, L.seg_rec_begin))
      return -1;
    if (L.k1_merged && (h->precision == PTZBA_FP32 ? upload_merged<float>(h, L, hr)
                                                   : upload_merged<double>(h, L, hr)))
      return -1;
  }
  if (L.k1_merged) {
    if (upload_st(h, h->lm_order_m, L.lm_work_m)) return -1;
  } else {  // a problem whose runs do not halve its records keeps today's memory
    for (DBuf* b : {&h->m_rec_xy, &h->m_rec_w, &h->m_rec_key, &h->m_seg_rec_begin, &h->lm_order_m}) b->release();
  }
  h->s2_groups_host = L.s2_groups;
  if (upload_st(h, h->lm_seg_begin, L.lm_seg_begin) ||
      upload_st(h, h->lm_order, L.lm_work) || upload_st(h, h->frame_seg_begin, L.frame_seg_begin) ||
      upload_st(h, h->frame_seg_list, L.frame_seg_list) || upload_st(h, h->frame_win_hi, L.frame_win_hi) ||
      upload_st(h, h->s2_items, L.s2_items) || upload_st(h, h->s2_groups, L.s2_groups) || upload_st(h, h->s2_lm, L.s2_lm) ||
      upload_st(h, h->lm_meta, L.lm_meta))
    return -1;
  const size_t e = h->elem();
  if (h->ptz.alloc(3 * n_pose * 8) || h->ptz_trial.alloc(3 * n_pose * 8) || h->rays.alloc(2 * (size_t)n_landmark * 8) ||
      h->rays_trial.alloc(2 * (size_t)n_landmark * 8) || h->D_pose.alloc(3 * n_pose * 8) ||
      h->D_ray.alloc(2 * (size_t)n_landmark * 8) || h->ft.alloc((size_t)n_pose * 8 * e) ||
      h->rt.alloc((size_t)n_landmark * 8 * e) || h->ft64.alloc((size_t)n_pose * 64) ||
      h->rt64.alloc((size_t)n_landmark * 64) || h->ug_slot[0].alloc((size_t)std::max<int64_t>(h->n_slot, 1) * UG_STRIDE * e) ||
      h->ug_slot[1].alloc((size_t)std::max<int64_t>(h->n_slot, 1) * UG_STRIDE * e) || h->w_slot[0].alloc((size_t)std::max<int64_t>(h->n_slot, 1) * W_STRIDE * e) ||
      h->w_slot[1].alloc((size_t)std::max<int64_t>(h->n_slot, 1) * W_STRIDE * e) || h->lm_out[0].alloc((size_t)n_landmark * 8 * 8) ||
      h->lm_out[1].alloc((size_t)n_landmark * 8 * 8) || h->lm_aux.alloc((size_t)n_landmark * 8 * 8) ||
      h->lm_red.alloc((size_t)n_landmark * 4 * 8) || h->sys.alloc((size_t)h->sys_count() * 8) ||
      h->scal.alloc(2 * PTZBA_NSCALARS * 8) || h->red_scratch.alloc(RED_SCRATCH * 8) || h->info.alloc(16) ||
      h->Ldiag.alloc((size_t)h->ld * CHOL_NB * 8) || h->Minv.alloc((size_t)h->ld * CHOL_NB * 8) ||
      h->dpose.alloc((size_t)h->ld * 8) ||
      h->s2_part.alloc((size_t)std::max(h->n_s2_items, 1) * SCHUR_F1 * 9 * WAVE * 8) ||
      h->part_diag.alloc((size_t)std::max(h->n_s2_items, 1) * SCHUR_F1 * 12 * 8))
    return -1;
  if (upload_st(h, h->chol_tasks, plan.tasks) || upload_st(h, h->tinv_tail, plan.tinv_tail) || upload_st(h, h->frame_pos, sorder.pos) || upload_st(h, h->row_pad, sorder.pad) ||
      upload_st(h, h->bs_chain_off, plan.chain_off) || upload_st(h, h->bs_chain_cols, plan.chain_cols) ||
      upload_st(h, h->bs_upd_off, plan.upd_off) || upload_st(h, h->bs_upd_tiles, plan.upd_tiles) || upload_st(h, h->xtiles, plan.xtiles) || upload_st(h, h->ztiles, plan.ztiles) ||
      upload_st(h, h->bs_la_tasks, plan.la_tasks) || upload_st(h, h->bs_lo_off, plan.lo_off) || upload_st(h, h->bs_lo_tiles, plan.lo_tiles))
    return -1;
  if (part_mode) {
    if (upload_st(h, h->row_phase, row_phase) || upload_st(h, h->fmask, fmask)) return -1;
    for (int q = 0; q < h->n_phase; ++q)
      if (upload_st(h, h->ph_tiles[q], tplan.ph[q].xt) || h->ph_buf[q].alloc((size_t)std::max<int64_t>(h->ph[q].n_buf, 1) * 8))
        return -1;
  } else {
    h->row_phase.release();
    h->fmask.release();
  }
  for (int q = h->n_phase; q < ptzba_ctx::MAX_PHASES; ++q) {
    h->ph_tiles[q].release();
    h->ph_buf[q].release();
  }
  if (zero_async(h, h->dpose.p, h->dpose.bytes)) return -1;  // rows a part-owned rank never solves
  h->n_xtiles = (int)(plan.xtiles.size() / 2);
  h->n_ztiles = (int)(plan.ztiles.size() / 2);
  if (zero_async(h, h->sys.p, h->sys.bytes)) return -1;  // outside the factor's tiles it is never written
  h->bs_nupd = (int)plan.upd_tiles.size();
  h->bs_npos = (int)plan.chain_cols.size();
  h->bs_ntasks = plan.n_tasks;
  // the back-substitution keeps r and its update lists in LDS (plus ~9 KiB of static staging)
  // (lookahead form: + 48 KiB ring of M / L blocks); larger systems take the left-looking form, whose lists
  // stay in global memory
  h->bs_ll = h->ld * 8 + (std::max(h->bs_npos + 1 + h->bs_nupd, 2 * h->bs_npos + h->bs_ntasks)) * 4 > 100 * 1024;
  // systems of >= 512 rows take the blocked right-looking form (many CUs per step) when the plan has a valid
  // schedule: the lookahead form reads the whole band of L through one CU per chain (config 3, same-box A/B
  // r03ab: cholesky_solve 0.261 -> 0.248 ms per trial); smaller ones (sliding windows) keep the lookahead form.
  // Knobs: PTZBA_BACKSOLVE=la (lookahead while its lists fit LDS) / =ll (left-looking) / =blk (blocked, any size)
  const char* bse = getenv("PTZBA_BACKSOLVE");
  const std::string bsk = bse ? bse : "";
  const bool want_blk = bsk == "blk" || (bsk.empty() && (h->bs_ll || h->n_aug >= 512));
  h->bs_blk = (want_blk || (h->bs_ll && bsk != "ll")) && bsk != "ll" && !plan.bsb_tasks.empty();
  h->bs_ll = (h->bs_ll || bsk == "ll") && !h->bs_blk;
  h->bsb_step_off = plan.bsb_step_off;
  // persistent form: every step's tasks in one launch (all resident at <= 512 workgroups); PTZBA_BS_PERSIST=0 keeps
  // one launch per step (the bitwise schedule test compares both; same-box A/B r04a: cholesky_solve 245 -> 241 us
  // per trial at config 3)
  h->bs_pst = h->bs_blk && !getenv_is("PTZBA_BS_PERSIST", "0") &&
              plan.bsb_tasks.size() / 12 <= 512;  // (2 workgroups per CU resident: 190 VGPRs)
  h->bsp_epoch = 0;
  h->no_fused_prep = getenv("PTZBA_NO_FUSED_PREP") != nullptr;
  if (h->bs_pst && !h->bsp_err) HIPCHK(hipHostMalloc((void**)&h->bsp_err, sizeof(int), hipHostMallocDefault));
  if (h->bsp_err) *h->bsp_err = 0;  // (a wait that gave up under an earlier problem does not outlive it)
  if (h->bs_pst) {
    if (upload_st(h, h->bsp_expect, plan.bsb_expect) || upload_st(h, h->bsp_tot, plan.bsb_tot) ||
        h->bsp_cnt.alloc(4 * plan.bsb_tot.size()))
      return -1;
    if (zero_async(h, h->bsp_cnt.p, h->bsp_cnt.bytes)) return -1;
  }
  if (h->bs_blk) {
    if (upload_st(h, h->bsb_tasks, plan.bsb_tasks) ||
        h->bsb_r.alloc((size_t)h->ld * 8))
      return -1;
  } else {
    h->bsb_tasks.release();
    h->bsb_r.release();
  }
  h->xbuf.release();  // allocated on first ptzba_exchange_packed
  if (zero_async(h, h->D_pose.p, h->D_pose.bytes) || zero_async(h, h->D_ray.p, h->D_ray.bytes) ||
      zero_async(h, h->w_slot[0].p, h->w_slot[0].bytes) ||  // slots of unobserved frames stay zero
      zero_async(h, h->w_slot[1].p, h->w_slot[1].bytes) ||
      zero_async(h, h->lm_out[0].p, h->lm_out[0].bytes) ||  // landmarks without records keep zero rows
      zero_async(h, h->lm_out[1].p, h->lm_out[1].bytes) || zero_async(h, h->ug_slot[0].p, h->ug_slot[0].bytes) ||
      zero_async(h, h->ug_slot[1].p, h->ug_slot[1].bytes) || zero_async(h, h->ptz.p, h->ptz.bytes) ||
      zero_async(h, h->rays.p, h->rays.bytes) || zero_async(h, h->scal.p, h->scal.bytes) ||
      zero_async(h, h->red_scratch.p, h->red_scratch.bytes))
    return -1;
  if (flush_stage(h)) return -1;
  h->stage_batch = false;
  // k_trial's per-segment system rows: seg_frame (uploaded, or made by the device front) and frame_pos have landed
  if (h->seg_row.alloc(4 * (size_t)std::max<int64_t>(h->n_seg, 1))) return -1;
  launch_seg_row(h->seg_frame.as<int32_t>(), h->frame_pos.as<int32_t>(), h->n_seg, h->n_fixed, h->seg_row.as<int32_t>(),
                 h->st);
  HIPCHK(hipGetLastError());
  st_mark("upload+alloc");
  if (!h->scal_host) HIPCHK(hipHostMalloc((void**)&h->scal_host, 24 * sizeof(double), hipHostMallocDefault));
  if (!h->scal_pack.p && h->scal_pack.alloc(24 * sizeof(double))) return -1;
  h->cur = 0;
  h->lambda = 0;
  h->cov.ready = false;  // (the covariance plan of the previous problem)
  HIPCHK(hipStreamSynchronize(h->st));  // every initialisation above has landed before the handle is used
  return 0;
}

int ptzba_set_problem(ptzba_handle h, int32_t n_pose, int32_t n_landmark, int64_t n_obs, const int32_t* obs_frame,
                      const int32_t* obs_landmark, const double* obs_xy, const double* obs_weight, double u, double v,
                      const ptzba_problem_opts* opts) {
  if (!h) return fail("null handle");
  h->setup_phases.clear();
  PhaseClock st_mark{h, std::chrono::steady_clock::now()};
  if (n_pose < 1 || n_landmark < 0 || n_obs < 0) return fail("bad sizes n_pose=%d n_landmark=%d n_obs=%lld", n_pose, n_landmark, (long long)n_obs);
  if (n_obs > 0 && (!obs_frame || !obs_landmark || !obs_xy)) return fail("null observation pointer");
  ptzba_problem_opts o{PTZBA_FP64, PTZBA_LOSS_LINEAR, 1.0, 1, PTZBA_ORDER_NESTED, nullptr};
  if (opts) o = *opts;
  if (o.precision != PTZBA_FP64 && o.precision != PTZBA_FP32) return fail("bad precision %d", o.precision);
  if (!loss_is_known(o.loss)) return fail("bad loss %d", o.loss);
  if (o.n_fixed < 0 || o.n_fixed > n_pose) return fail("bad n_fixed %d", o.n_fixed);
  if (o.loss != PTZBA_LOSS_LINEAR && !(o.f_scale > 0)) return fail("a robust loss needs f_scale > 0");
  if (o.ordering < PTZBA_ORDER_NATURAL || o.ordering > PTZBA_ORDER_NESTED_FORCE) return fail("bad ordering %d", o.ordering);
  if (o.frame_win_hi)
    for (int f = 0; f < n_pose; ++f)
      if (o.frame_win_hi[f] < f || o.frame_win_hi[f] >= n_pose) return fail("frame_win_hi[%d] = %d out of range", f, o.frame_win_hi[f]);
  {
    // record validation over host threads; the error reported is the first bad record's, as a sequential scan's
    const int T = host_threads(n_obs);
    std::vector<int64_t> first_bad(T, n_obs);
    parallel_chunks(n_obs, T, [&](int64_t lo, int64_t hi, int t) {
      for (int64_t r = lo; r < hi; ++r)
        if (obs_frame[r] < 0 || obs_frame[r] >= n_pose || obs_landmark[r] < 0 || obs_landmark[r] >= n_landmark ||
            !std::isfinite(obs_xy[2 * r]) || !std::isfinite(obs_xy[2 * r + 1]) || (obs_weight && !(obs_weight[r] >= 0))) {
          first_bad[t] = r;
          return;
        }
    });
    const int64_t r = *std::min_element(first_bad.begin(), first_bad.end());
    if (r < n_obs) {
      if (obs_frame[r] < 0 || obs_frame[r] >= n_pose) return fail("record %lld: frame %d out of range", (long long)r, obs_frame[r]);
      if (obs_landmark[r] < 0 || obs_landmark[r] >= n_landmark)
        return fail("record %lld: landmark %d out of range", (long long)r, obs_landmark[r]);
      if (!std::isfinite(obs_xy[2 * r]) || !std::isfinite(obs_xy[2 * r + 1])) return fail("record %lld: non-finite observation", (long long)r);
      return fail("record %lld: negative weight", (long long)r);
    }
  }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->st));
  h->have_problem = false;
  h->pri.n_factor = 0;  // a new problem starts without pose priors
  h->mg.n = 0;          // ... without a marginal factor, and without ptzba_marginal_prior's work buffers
  h->mg.release_work();
  h->cov.release_joint();  // ... and without ptzba_covariance_joint's workspace
  h->rp.n_prior = 0;    // ... and without ray priors
  h->displaced = false;  // ... and without a projection-centre displacement
  for (double& d : h->disp) d = 0.0;
  h->w_override = nullptr;
  h->trial_open = false;
  // ... and without the pending decision of a device-driven run that stopped between ptzba_lm_solve and ptzba_lm_decide
  // (the between-solves calls would refuse the new problem for it)
  h->scal_deferred = false;
  h->ptz_saved.release();
  h->rays_saved.release();
  h->n_pose = n_pose;
  h->n_lm = n_landmark;
  h->n_rec = n_obs;
  h->precision = o.precision;
  h->loss = o.loss;
  h->fs = o.f_scale;
  h->hcurv = 1.0;
  h->n_fixed = o.n_fixed;
  h->u = u;
  h->v = v;
  h->weighted = obs_weight != nullptr;

  st_mark("validate");
  // large problems (configs 3 and 4: 14.6M / 410M records): the order, the segment runs and the record arrays are
  // built on the device (setup_kernels.hip: one stable radix sort of the composite key landmark * n_pose + frame --
  // the same order as the host's two stable counting sorts); the host keeps only the per-segment arrays its
  // structure passes read.  Smaller ones (a sliding window's ~170K records) stay on the host.
  const bool gpu_setup = n_obs >= (h->gpu_setup_min >= 0 ? h->gpu_setup_min : GPU_SETUP_MIN_REC) && n_obs > 0 &&
                         n_obs < ((int64_t)1 << 31) &&
                         (uint64_t)n_landmark * (uint64_t)n_pose <= ((uint64_t)1 << 32);
  // the host fronts sort by two stable counting passes (the device front sorts in its segment phase)
  ProblemLayout L;
  HostRecords hr;
  // PTZBA_K1_MERGE=0: K1 keeps the unmerged record stream (A/B and the parity tests)
  const bool k1_merge = !getenv_is("PTZBA_K1_MERGE", "0");
  const int threads = host_threads(n_obs);
  const bool par_host = !gpu_setup && threads > 1;
  if (!gpu_setup) layout_host_sort(L, n_pose, n_landmark, n_obs, obs_frame, obs_landmark, threads);
  st_mark("sort");
  if (gpu_setup) {
    if (gpu_front(h, n_obs, n_pose, n_landmark, obs_frame, obs_landmark, obs_xy, obs_weight, k1_merge, L)) return -1;
    lm_first_segments(L, n_landmark);
  } else if (const char* e = layout_host_segments(L, n_landmark, n_obs, obs_frame, obs_landmark, threads)) {
    return fail("%s", e);
  } else {
    // the stored records, converted once: the merge pass compares them, upload_problem copies them
    if (o.precision == PTZBA_FP32) convert_records<float>(L, n_obs, obs_xy, obs_weight, hr);
    else convert_records<double>(L, n_obs, obs_xy, obs_weight, hr);
    L.n_merged = n_obs;
    // (a run never spans segments: with more segments than half the records the pass cannot halve them and is skipped)
    if (k1_merge && 2 * (int64_t)L.seg_frame.size() <= n_obs)
      layout_host_merge(L, n_obs, hr.xy.data(), hr.w.empty() ? nullptr : hr.w.data(), o.precision == PTZBA_FP32, threads);
  }
  h->n_merged = L.n_merged;
  h->k1_merged = L.k1_merged;
  // pair-form input whose repeats are all adjacent: one merged record per segment (PTZBA_K1_ONE=0: the general kernel)
  h->k1_one = L.k1_merged && L.n_merged == (int64_t)L.seg_frame.size() && !getenv_is("PTZBA_K1_ONE", "0");
  h->n_seg = (int64_t)L.seg_frame.size();
  layout_frame_csr(L, n_pose, par_host || gpu_setup, threads);
  st_mark("segments+frame csr");
  if (const char* e = layout_k2(L, n_pose, n_landmark, o.n_fixed)) return fail("%s", e);
  h->n_slot = L.n_slot;
  h->n_s2_groups = (int)(L.s2_groups.size() / 4);
  h->n_s2_items = (int)(L.s2_items.size() / 4);
  std::copy(L.k2_info, L.k2_info + 8, h->k2_info);
  std::copy(L.k2_tile_info, L.k2_tile_info + 8, h->k2_tile_info);
  h->f1_covered = L.f1_covered;
  // PTZBA_K2_PROLOGUE=1: keep the k_build_prologue launch in front of every build (build_impl)
  h->k2_prologue = getenv_is("PTZBA_K2_PROLOGUE", "1");
  h->n_build_prologue = h->n_build_folded = 0;
  st_mark("k2 structure");
  if (n_obs >= ((int64_t)1 << 31)) return fail("n_obs %lld exceeds the 2^31 record limit of a handle (shard it)", (long long)n_obs);
  layout_k1_order(L, n_pose, n_landmark);
  h->n_work = L.n_work;
  h->max_seg_per_lm = L.max_seg;
  h->k1_groups = L.k1_groups;
  h->k1_groups_global = L.k1_groups_global;
  h->n_sys = 3 * (n_pose - o.n_fixed);
  // system order and factorisation plan (from the coupling window; a sharded problem passes the global one)
  std::vector<int32_t> win(L.frame_win_hi);
  if (o.frame_win_hi)
    for (int f = 0; f < n_pose; ++f) win[f] = std::max(win[f], o.frame_win_hi[f]);
  // multi-GPU: part-owned solve when the frame chain splits (the landmarks partitioned accordingly by
  // ptzba_partition_landmarks), else every rank factors the whole summed system (replicated)
  const bool dist = o.dist_world >= 2;
  if (dist && (o.dist_rank < 0 || o.dist_rank >= o.dist_world))
    return fail("bad rank %d of %d", o.dist_rank, o.dist_world);
  if (dist && !o.frame_win_hi) return fail("a sharded solve needs the global coupling window (frame_win_hi)");
  SysOrder sorder;
  const bool part_mode = dist && dist_order(n_pose, o.n_fixed, win, o.dist_world, sorder);
  CholPlan plan;
  if (!part_mode && choose_order_plan(n_pose, o.n_fixed, win, o.ordering, sorder, plan))
    return fail("factorisation plan: an update task needs more than four panels");
  h->n_aug = sorder.n_aug;
  h->nested = sorder.nested;
  h->nd_depth = sorder.nd_depth;
  h->ld = pad_tile(h->n_aug + 1);  // + augmented rhs row
  // the back-substitution keeps x ([ld] doubles) in LDS
  if (h->ld > CHOL_MAX_LD) return fail("reduced system %d too large for the dense solver", h->n_sys);
  TreePlan tplan;
  h->dist_world = dist ? o.dist_world : 1;
  h->dist_rank = dist ? o.dist_rank : 0;
  h->dist_mode = part_mode ? 1 : 0;
  h->n_phase = 0;
  h->base_node = -1;
  h->tree_depth = 0;
  h->tree_groups.clear();
  std::vector<uint8_t> row_phase, fmask;
  h->owned_host.assign(n_pose, 1);
  if (part_mode) {
    DistTree DT;
    if (!dist_tree(sorder, o.dist_world, DT) ||
        !make_plan_tree(sorder, DT, o.dist_rank, n_pose, o.n_fixed, win, h->ld, plan, tplan))
      return fail("part-owned plan: the parts are coupled (bad coupling window)");
    if ((int)tplan.ph.size() > ptzba_ctx::MAX_PHASES) return fail("rank tree deeper than %d phases", ptzba_ctx::MAX_PHASES);
    h->base_node = tplan.base;
    h->tree_depth = DT.depth;
    for (int v = 1; v < (int)DT.n.size(); ++v)
      if (DT.n[v].nr >= 2) {
        bool dup = false;
        for (size_t q = 0; q < h->tree_groups.size(); q += 3)
          dup = dup || (h->tree_groups[q] == DT.n[v].r0 && h->tree_groups[q + 1] == DT.n[v].nr);
        if (!dup) h->tree_groups.insert(h->tree_groups.end(), {DT.n[v].r0, DT.n[v].nr, DT.n[v].depth});
      }
    auto fphase = [&](int f) { return sorder.pos[f] < 0 ? -1 : (int)tplan.col_phase[sorder.pos[f] / CHOL_NB]; };
    for (int64_t r = 0; r < n_obs; ++r)
      if (obs_frame[r] >= o.n_fixed && fphase(obs_frame[r]) < 0)
        return fail("record %lld sees frame %d outside rank %d's part (partition the landmarks with "
                    "ptzba_partition_landmarks)", (long long)r, obs_frame[r], o.dist_rank);
    fmask.assign(n_pose, 0);
    for (int f = 0; f < n_pose; ++f) {
      const int q = f < o.n_fixed ? -1 : fphase(f);
      const bool owned = q >= 0;
      h->owned_host[f] = owned ? 1 : 0;
      // each frame's pose partials counted by one rank: its phase group's first rank (fixed frames: rank 0)
      const bool counted = f < o.n_fixed ? o.dist_rank == 0 : (owned && o.dist_rank == tplan.ph[q].r0);
      fmask[f] = (uint8_t)((owned ? 1 : 0) | (counted ? 2 : 0));
    }
    row_phase.assign(h->n_aug, 0);
    for (int r = 0; r < h->n_aug; ++r) row_phase[r] = (uint8_t)(tplan.col_phase[r / CHOL_NB] + 1);
    h->n_phase = (int)tplan.ph.size();
    for (int q = 0; q < h->n_phase; ++q) {
      const auto& tp = tplan.ph[q];
      auto& d = h->ph[q];
      d.lv0 = tp.lv0;
      d.lv1 = tp.lv1;
      d.kind = tp.kind;
      d.r0 = tp.r0;
      d.nr = tp.nr;
      d.depth = tp.depth;
      d.node = tp.node;
      d.n_tiles = (int)(tp.xt.size() / 2);
      d.vr = tp.vr;
      d.n_buf = (q == 0 && tp.nr < 2) ? 0 : (int64_t)d.n_tiles * CHOL_NB * CHOL_NB + tp.vr.count[0] + tp.vr.count[1] + tp.vr.count[2];
    }
  }
  h->chol_task_off = plan.level_off;
  h->chol_tasks_host = plan.tasks;
  h->n_tinv_tail = (int)plan.tinv_tail.size();
  h->chol_levels = plan.n_levels;
  h->chol_delayed = plan.delayed;
  h->n_chain = (int)plan.chain_off.size() - 1;
  L.frame_win_hi = win;  // K2 windows follow the same (possibly global) coupling
  h->win_host = win;
  h->pos_host = sorder.pos;
  h->zt_host = plan.ztiles;
  h->perm_uploaded = gpu_setup;  // (the device front wrote the permutation itself)
  if (gpu_setup) h->perm_host.clear();

  st_mark("work order+plan");
  if (upload_problem(h, L, sorder, plan, tplan, gpu_setup, part_mode, row_phase, fmask, hr, st_mark)) return -1;
  if (!gpu_setup) h->perm_host = std::move(L.order);
  st_mark("final sync");
  h->have_problem = true;
  h->drop_groups();  // the groups of the previous problem; split anew at the first exchange of this one
  // no collective here: a rank whose set_problem failed validation above must not leave the others blocked in a
  // split.  The group communicator is split by the first exchange (ensure_group_comm), which every rank reaches.
  return 0;
}

int ptzba_problem_info(ptzba_handle h, int64_t* info) {
  if (!h || !h->have_problem) return fail("no problem set");
  info[0] = h->n_pose;
  info[1] = h->n_lm;
  info[2] = h->n_rec;
  info[3] = h->n_seg;
  info[4] = h->n_sys;
  info[5] = h->n_work;
  info[6] = h->max_seg_per_lm;
  info[7] = (int64_t)g_total_bytes({&h->rec_xy, &h->rec_seg, &h->rec_w, &h->perm, &h->seg_frame, &h->seg_lm,
                                    &h->seg_base, &h->ft64, &h->rt64,
                                    &h->seg_rec_begin, &h->lm_seg_begin, &h->lm_order, &h->frame_seg_begin,
                                    &h->frame_seg_list, &h->frame_win_hi, &h->ptz, &h->rays, &h->ptz_trial,
                                    &h->rays_trial, &h->D_pose, &h->D_ray, &h->ft, &h->rt, &h->ug_slot[0],
                                    &h->ug_slot[1], &h->w_slot[0], &h->w_slot[1], &h->lm_out[0], &h->lm_out[1], &h->lm_aux, &h->lm_red, &h->sys,
                                    &h->scal});
  // the host fronts upload the permutation on first use: until then the buffer is the previous problem's
  if (!h->perm_uploaded) info[7] -= (int64_t)h->perm.bytes;
  return 0;
}

int ptzba_k2_info(ptzba_handle h, int* out) {
  if (!h || !h->have_problem) return fail("no problem set");
  for (int k = 0; k < 8; ++k) out[k] = h->k2_info[k];
  return 0;
}

int ptzba_build_info(ptzba_handle h, int64_t* out4) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!out4) return fail("bad arguments");
  out4[0] = h->n_build_prologue;
  out4[1] = h->n_build_folded;
  out4[2] = h->k2_prologue ? 1 : 0;
  out4[3] = 0;
  return 0;
}

int ptzba_schur_groups(ptzba_handle h, int32_t cap, int32_t* out4, int32_t* n_out) {
  if (!h || !h->have_problem) return fail("no problem set");
  const int32_t n = (int32_t)(h->s2_groups_host.size() / 4);
  if (n_out) *n_out = n;
  for (int32_t k = 0; out4 && k < 4 * std::min(cap, n); ++k) out4[k] = h->s2_groups_host[k];
  return 0;
}

int ptzba_k2_tile_info(ptzba_handle h, int32_t* out) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!out) return fail("bad arguments");
  for (int k = 0; k < 8; ++k) out[k] = h->k2_tile_info[k];
  return 0;
}

int ptzba_k1_info(ptzba_handle h, int64_t* info) {
  if (!h || !h->have_problem) return fail("no problem set");
  info[0] = h->n_work;
  info[1] = h->k1_groups;
  info[2] = h->k1_groups_global;
  info[3] = (h->max_seg_per_lm + K1_SEGW - 1) / K1_SEGW;
  return 0;
}

int ptzba_k1_merge_info(ptzba_handle h, int64_t* out4) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!out4) return fail("bad arguments");
  out4[0] = h->n_merged;
  out4[1] = h->k1_merged ? 1 : 0;
  out4[2] = h->k1_one ? 1 : 0;
  out4[3] = 0;
  return 0;
}

// ------------------------------------------------------------------------------------------------
static void* ft_real(ptzba_ctx* h) { return h->precision == PTZBA_FP32 ? h->ft.p : h->ft64.p; }
static void* rt_real(ptzba_ctx* h) { return h->precision == PTZBA_FP32 ? h->rt.p : h->rt64.p; }

void ptzba::tables(ptzba_ctx* h, const double* ptz, const double* rays, const int* run_if, double* zero, int n_zero) {
  if (h->precision == PTZBA_FP32)
    launch_tables<float>(ptz, rays, h->n_pose, h->n_lm, h->ft64.p, h->rt64.p, h->ft.p, h->rt.p, run_if, h->st, zero,
                         n_zero);
  else
    launch_tables<double>(ptz, rays, h->n_pose, h->n_lm, h->ft64.p, h->rt64.p, h->ft64.p, h->rt64.p, run_if, h->st, zero,
                          n_zero);
}

// sel != nullptr (device-driven LM): the kernel writes slot (*sel ^ sel_xor), chosen on the device
// run_if != nullptr: a conditional re-linearisation of the current point (device-driven LM, after the curvature
// switch): the launch exits at once unless *run_if; not timed as a K1 launch (the roofline averages real ones)
// hc_dev: device-driven LM, the huber curvature weight from device memory (LMDev::hc / hc_trial); nullptr: h->hcurv
// trial_state: the tables of this linearisation were made from the trial state (k_trial's output), not the current
// one (the ray priors form e from the same rays)
void ptzba::linearize_into(ptzba_ctx* h, int slot, const int* sel, int sel_xor, const int* run_if, const double* hc_dev,
                           bool trial_state) {
  LinArgs a;
  // the merged record stream when the problem has one; ptzba_marginal_prior's per-record weights split runs, so a
  // launch under w_override reads the unmerged records
  const bool merged = h->k1_merged && !h->w_override;
  a.lm_work = (merged ? h->lm_order_m : h->lm_order).as<int4>();
  a.n_work = h->n_work;
  a.lm_seg_begin = h->lm_seg_begin.as<int32_t>();
  a.seg_frame = h->seg_frame.as<int32_t>();
  a.seg_rec_begin = (merged ? h->m_seg_rec_begin : h->seg_rec_begin).as<int64_t>();
  a.rec_seg = h->rec_seg.as<int32_t>();
  a.rec_key = (merged ? h->m_rec_key : h->rec_key).as<uint8_t>();
  a.rec_xy = merged ? h->m_rec_xy.p : h->rec_xy.p;
  a.rec_w = merged ? h->m_rec_w.p : (h->w_override ? h->w_override : (h->weighted ? h->rec_w.p : nullptr));
  a.ft = ft_real(h);
  a.rt = rt_real(h);
  a.ft64 = h->ft64.p;
  a.rt64 = h->rt64.p;
  a.seg_base = h->seg_base.as<double2>();
  a.u = h->u;
  a.v = h->v;
  a.fs2 = h->fs * h->fs;
  a.inv_fs2 = 1.0 / (h->fs * h->fs);
  a.hcurv = h->hcurv;
  a.hcurv_dev = hc_dev;
  a.run_if = run_if;
  a.ug_slot = h->ug_slot[slot].p;
  a.w_slot = h->w_slot[slot].p;
  a.lm_meta = h->lm_meta.as<int4>();
  a.lm_out = h->lm_out[slot].as<double>();
  a.sel = sel;
  a.sel_xor = sel_xor;
  if (sel) {
    a.ug_slot = h->ug_slot[0].p;
    a.w_slot = h->w_slot[0].p;
    a.lm_out = h->lm_out[0].as<double>();
  }
  a.ug_slot1 = h->ug_slot[1].p;
  a.w_slot1 = h->w_slot[1].p;
  a.lm_out1 = h->lm_out[1].as<double>();
  a.n_pose = h->n_pose;
  a.displaced = h->displaced;
  for (int k = 0; k < 6; ++k) {
    a.disp[k] = h->disp[k];
    a.disp32[k] = (float)h->disp[k];
  }
  if (!run_if) tm_begin(h, TM_K1);
  hipEvent_t e0 = run_if ? nullptr : tm_k1_event(h, 0), e1 = run_if ? nullptr : tm_k1_event(h, 1);
  if (merged && h->k1_one) {  // one merged record per segment: the kernel without a record phase (k1_one_kernel.hip)
    if (h->precision == PTZBA_FP32) launch_linearize_one<float>(a, h->loss, h->st, e0, e1);
    else launch_linearize_one<double>(a, h->loss, h->st, e0, e1);
  } else if (h->precision == PTZBA_FP32)
    launch_linearize<float>(a, h->loss, h->st, e0, e1);
  else
    launch_linearize<double>(a, h->loss, h->st, e0, e1);
  if (!run_if) tm_end(h, TM_K1);
  // ray priors: V_l, g_l and the landmark's cost share of the rows K1 has just written -- the same slot selector and
  // gate as K1, e from the rays its tables were made from (outside the timed K1 group).  Not under w_override:
  // ptzba_marginal_prior linearises the dropped records alone, the priors stay with the landmarks that remain
  if (h->has_ray_priors() && !h->w_override)
    launch_ray_prior_apply(ray_prior_args(h, sel, trial_state ? 1 : 0), a.lm_out, a.lm_out1, sel, sel_xor, run_if, h->st);
}

int ptzba_solver_info(ptzba_handle h, int64_t* info8) {
  if (!h || !h->have_problem) return fail("no problem set");
  info8[0] = h->n_aug;
  info8[1] = h->ld;
  info8[2] = h->chol_levels;
  info8[3] = (h->nested ? PTZBA_ORDER_NESTED : PTZBA_ORDER_NATURAL) | ((int64_t)h->nd_depth << 8);
  info8[4] = h->bs_blk ? 2 : (h->bs_ll ? 1 : 0);
  info8[5] = h->n_slot;
  info8[6] = h->n_s2_items;
  info8[7] = h->n_ztiles;
  return 0;
}

int ptzba_solver_buffers(ptzba_handle h, void** ptrs, int64_t* counts) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!ptrs || !counts) return fail("bad arguments");
  ptrs[0] = h->Ldiag.p;
  ptrs[1] = h->Minv.p;
  ptrs[2] = h->dpose.p;
  ptrs[3] = h->info.p;
  counts[0] = counts[1] = h->ld * CHOL_NB;
  counts[2] = h->ld;
  counts[3] = 1;
  return 0;
}

int ptzba_residual(ptzba_handle h, const double* x_full, double* r_out) {
  if (!h || !h->have_problem) return fail("no problem set");
  HIPCHK(hipSetDevice(h->device));
  if (!h->perm_uploaded) {
    if (upload(h->perm, h->perm_host, h->st)) return -1;
    h->perm_uploaded = true;
  }
  DBuf x, r;
  if (x.alloc((3 * (size_t)h->n_pose + 2 * (size_t)h->n_lm) * 8) || r.alloc(2 * (size_t)h->n_rec * 8)) return -1;
  SyncOnExit sync_guard{h->st};  // destroyed before x and r: queued work on them ends first, also on errors
  HIPCHK(hipMemcpyAsync(x.p, x_full, x.bytes, hipMemcpyHostToDevice, h->st));
  const double* px = x.as<double>();
  tables(h, px, px + 3 * h->n_pose);
  if (h->precision == PTZBA_FP32)
    launch_residual<float>(h->rec_seg.as<int32_t>(), h->seg_frame.as<int32_t>(), h->seg_lm.as<int32_t>(),
                           h->seg_base.as<double2>(), h->rec_xy.p, h->perm.as<int64_t>(), h->ft64.p, h->rt64.p, h->u,
                           h->v, h->disp6(), h->n_rec, r.as<double>(), h->st);
  else
    launch_residual<double>(h->rec_seg.as<int32_t>(), h->seg_frame.as<int32_t>(), h->seg_lm.as<int32_t>(),
                            h->seg_base.as<double2>(), h->rec_xy.p, h->perm.as<int64_t>(), h->ft64.p, h->rt64.p, h->u,
                            h->v, h->disp6(), h->n_rec, r.as<double>(), h->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(r_out, r.p, 2 * (size_t)h->n_rec * 8, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

int ptzba_set_state(ptzba_handle h, const double* ptz, const double* rays) {
  if (!h || !h->have_problem) return fail("no problem set");
  HIPCHK(hipSetDevice(h->device));
  h->trial_open = false;
  SyncOnExit sync_guard{h->st};  // caller buffers: no copy outlives the call, also on errors
  HIPCHK(hipMemcpyAsync(h->ptz.p, ptz, 3 * (size_t)h->n_pose * 8, hipMemcpyHostToDevice, h->st));
  if (h->n_lm) HIPCHK(hipMemcpyAsync(h->rays.p, rays, 2 * (size_t)h->n_lm * 8, hipMemcpyHostToDevice, h->st));
  HIPCHK(hipMemsetAsync(h->D_pose.p, 0, h->D_pose.bytes, h->st));
  HIPCHK(hipMemsetAsync(h->D_ray.p, 0, h->D_ray.bytes, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

// device-resident restart point: snapshot the current state / restore it (stream-ordered, no host sync)
int ptzba_save_state(ptzba_handle h) {
  if (!h || !h->have_problem) return fail("no problem set");
  HIPCHK(hipSetDevice(h->device));
  if (h->ptz_saved.alloc(h->ptz.bytes) || h->rays_saved.alloc(std::max<size_t>(h->rays.bytes, 8))) return -1;
  HIPCHK(hipMemcpyAsync(h->ptz_saved.p, h->ptz.p, 3 * (size_t)h->n_pose * 8, hipMemcpyDeviceToDevice, h->st));
  if (h->n_lm)
    HIPCHK(hipMemcpyAsync(h->rays_saved.p, h->rays.p, 2 * (size_t)h->n_lm * 8, hipMemcpyDeviceToDevice, h->st));
  return 0;
}

int ptzba_restore_state(ptzba_handle h) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!h->ptz_saved.p) return fail("no saved state (ptzba_save_state)");
  HIPCHK(hipSetDevice(h->device));
  // one launch instead of two copies and two fills (four stream operations at ~4-5 us each)
  const int64_t n_ptz = 3 * (int64_t)h->n_pose, n_rays = 2 * (int64_t)h->n_lm;
  const int64_t n_dp = (int64_t)(h->D_pose.bytes / 8), n_dr = (int64_t)(h->D_ray.bytes / 8);
  const int64_t n = std::max(std::max(n_ptz, n_rays), std::max(n_dp, n_dr));
  if (n > 0)
    hipLaunchKernelGGL(k_restore_state, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->st, h->ptz.as<double>(),
                       h->ptz_saved.as<double>(), n_ptz, h->rays.as<double>(), h->rays_saved.as<double>(), n_rays,
                       h->D_pose.as<double>(), n_dp, h->D_ray.as<double>(), n_dr);
  HIPCHK(hipGetLastError());
  return 0;
}

int ptzba_get_state(ptzba_handle h, double* ptz, double* rays) {
  if (!h || !h->have_problem) return fail("no problem set");
  HIPCHK(hipSetDevice(h->device));
  SyncOnExit sync_guard{h->st};  // no copy outlives the call, also on errors
  // through a pinned landing buffer kept by the handle: a pageable destination sent the copy down the runtime's
  // pageable path, whose cost jumped at some sizes (a 30-KF stream's keyframe call: 0.4 -> 6 ms once)
  const size_t nb_ptz = ptz ? 3 * (size_t)h->n_pose * 8 : 0, nb_rays = (rays && h->n_lm) ? 2 * (size_t)h->n_lm * 8 : 0;
  if (nb_ptz + nb_rays == 0) return 0;
  if (h->out_pin_cap < nb_ptz + nb_rays) {
    if (h->out_pin) {
      HIPCHK(hipStreamSynchronize(h->st));
      HIPCHK(hipHostFree(h->out_pin));
      h->out_pin = nullptr;
      h->out_pin_cap = 0;
    }
    const size_t cap = (nb_ptz + nb_rays) + (nb_ptz + nb_rays) / 2 + 4096;
    HIPCHK(hipHostMalloc((void**)&h->out_pin, cap, hipHostMallocDefault));
    h->out_pin_cap = cap;
  }
  if (nb_ptz) HIPCHK(hipMemcpyAsync(h->out_pin, h->ptz.p, nb_ptz, hipMemcpyDeviceToHost, h->st));
  if (nb_rays) HIPCHK(hipMemcpyAsync(h->out_pin + nb_ptz, h->rays.p, nb_rays, hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (nb_ptz) std::memcpy(ptz, h->out_pin, nb_ptz);
  if (nb_rays) std::memcpy(rays, h->out_pin + nb_ptz, nb_rays);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// exchanges of a multi-GPU solve (include/ptzba.h PTZBA_X_*): in-place sums on the handle's stream through
// the attached RCCL communicator or the caller's hook
// ------------------------------------------------------------------------------------------------
static int ensure_group_comms(ptzba_ctx* h);
// the tree depth of the group an exchange kind runs over on this rank (0: the whole world)
static int exchange_depth(const ptzba_ctx* h, int kind) {
  if (!h->dist_mode || kind == PTZBA_X_SEP || kind == PTZBA_X_SCAL || kind == PTZBA_X_SYS) return 0;
  for (int q = 0; q < h->n_phase; ++q)
    if (h->ph[q].kind == kind) return h->ph[q].depth;
  return -1;
}
static int exchange_run(ptzba_ctx* h, int kind, double* buf, int64_t n);
// every exchange goes through here: with collective timing on (PTZBA_TIME_COMM) an event pair brackets it on the
// handle's stream (RCCL's kernel, or a hook's stream work), so a multi-rank run reports its collectives' time and
// bytes per kind (ptzba_comm_times) -- alpha and bandwidth measured instead of assumed
int ptzba::exchange(ptzba_ctx* h, int kind, double* buf, int64_t n) {
  const bool tm = (h->timing & PTZBA_TIME_COMM) && h->cev_used + 2 <= (int)h->cev.size();
  if (tm) (void)hipEventRecord(h->cev[h->cev_used], h->st);
  const int rc = exchange_run(h, kind, buf, n);
  if (tm) {
    (void)hipEventRecord(h->cev[h->cev_used + 1], h->st);
    h->cev_used += 2;
    h->clog.emplace_back(kind, n);
  }
  return rc;
}
static int exchange_run(ptzba_ctx* h, int kind, double* buf, int64_t n) {
  if (h->hook) {
    if (h->hook(h->hook_ctx, kind, buf, n, (void*)h->st)) return fail("exchange hook failed (kind %d)", kind);
    return 0;
  }
  if (h->comm) {
    // ncclCommSplit is collective over comm: done before this rank's first exchange of the problem, where every
    // rank of a sharded solve arrives in the same order
    if (ensure_group_comms(h)) return fail("group communicator split failed");
    const int d = exchange_depth(h, kind);
    if (d < 0 || d >= 4) return fail("no rank group for exchange kind %d", kind);
    ptzba_comm c = d == 0 ? h->comm : h->group_comms[d];
    if (!c) return fail("part-owned exchange kind %d has no group communicator (ptzba_attach_comm)", kind);
    return ptzba_comm_allreduce(c, buf, n, (void*)h->st);
  }
  return 0;
}
// the trial's reduction (k_reduce_cols): column 0 the trial cost, columns 1-4 lm_red's pred, |d|^2, |x|^2 (sums) and the
// rays' max |gradient| (a maximum: bit 4) -> scal[1..5]
constexpr int LM_RED_MAXMASK = 1 << 4;
static int64_t scal_count(const ptzba_ctx* h) { return h->dist_mode ? 2 * PTZBA_NSCALARS : PTZBA_NSCALARS; }

// the rank tree's group communicators, one split per tree depth 1..depth (collective over ALL ranks of comm, in the
// same order everywhere: a rank whose path does not reach that depth, or whose node there holds it alone, joins a
// one-rank communicator it never uses)
static int ensure_group_comms(ptzba_ctx* h) {
  if (!h->comm || !h->have_problem || !h->dist_mode || h->groups_split) return 0;
  for (int d = 1; d <= h->tree_depth && d < 4; ++d) {
    int color = 1 << 20 | h->dist_rank;
    for (int q = 0; q < h->n_phase; ++q)
      if (h->ph[q].depth == d && h->ph[q].nr >= 2) color = h->ph[q].node;
    h->group_comms[d] = ptzba_comm_split(h->comm, color, h->dist_rank);
    if (!h->group_comms[d]) return -1;
  }
  h->groups_split = true;
  return 0;
}


int ptzba_linearize(ptzba_handle h) {
  if (!h || !h->have_problem) return fail("no problem set");
  HIPCHK(hipSetDevice(h->device));
  // the scalar block is zeroed by the tables launch (one launch less than a memset)
  tables(h, h->ptz.as<double>(), h->rays.as<double>(), nullptr, h->scal.as<double>(), (int)(h->scal.bytes / 8));
  linearize_into(h, h->cur);
  launch_reduce_cols(h->lm_out[h->cur].as<double>() + 5, h->n_lm, 8, 1, 0, h->scal.as<double>(),
                     h->red_scratch.as<double>(), h->st);
  // scal[0], the cost at the current state, includes the prior (the reduction above stored the records' share)
  if (h->has_priors()) launch_prior_cost(prior_args(h, nullptr, 0), h->scal.as<double>(), 1.0, 1, h->pri.red.as<double>(), h->st);
  if (h->has_marg()) launch_marg_cost(marg_args(h, nullptr, 0), h->scal.as<double>(), 1, h->st);
  h->trial_open = false;
  HIPCHK(hipGetLastError());
  if (h->has_exchange()) return exchange(h, PTZBA_X_SCAL, h->scal.as<double>(), scal_count(h));
  return 0;
}

// reduced camera system at the current linearisation (slot h->cur, or in the device-driven LM slot *sel);
// lambda from the argument or, in the device-driven LM (lam_dev != nullptr), from device memory
int ptzba::build_impl(ptzba_ctx* h, double lambda, const double* lam_dev, const int* skip_if, const int* sel,
                      bool with_priors) {
  const int c = sel ? 0 : h->cur;
  FusedPrep fp{};
  // fused only in the device-driven LM (sel != nullptr): the host-step API (ptzba_build_reduced) leaves the
  // system raw for callers that sum it between build and solve (include/ptzba.h, the round-2 protocol)
  if (sel && h->fused_prep())
    fp = FusedPrep{h->row_pad.as<uint8_t>(), h->n_aug, h->info.as<int>(), h->D_pose.as<double>(), lambda, lam_dev};
  // Device-driven single-GPU fp32 builds on the matrix-core K2 need no prologue launch: K2 zeroes the
  // pattern tiles, the vectors and info itself and forms the landmark damping in its list build, k_trial forms its
  // own and keeps D_ray (SchurArgs::ztiles, lm_damp).  Every other build launches the prologue as before.
  const bool fold = sel && fp.pad && h->precision == PTZBA_FP32 && !h->k2_valu32 && !h->k2_prologue &&
                    h->n_s2_items > 0 && h->n_pose - h->n_fixed > 0;
  if (!fold)
    launch_build_prologue(h->S(), h->ld, h->ztiles.as<int2>(), h->n_ztiles, h->bvec(), 3 * h->ld,
                          h->lm_out[c].as<double>(), h->lm_seg_begin.as<int32_t>(), h->D_ray.as<double>(),
                          h->lm_aux.as<double>(), h->n_lm, lambda, lam_dev, skip_if, h->st, h->lm_out[1].as<double>(),
                          sel, fp);
  ++(fold ? h->n_build_folded : h->n_build_prologue);
  SchurArgs a;
  a.items = h->s2_items.as<int4>();
  a.groups = h->s2_groups.as<int4>();
  a.part = h->s2_part.as<double>();
  a.part_diag = h->part_diag.as<double>();
  a.item_lm = h->s2_lm.as<int4>();
  a.frame_win_hi = h->frame_win_hi.as<int32_t>();
  a.ug_slot = h->ug_slot[c].p;
  a.w_slot = h->w_slot[c].p;
  a.lm_aux = h->lm_aux.as<double>();
  a.frame_pos = h->frame_pos.as<int32_t>();
  a.S = h->S();
  a.b = h->bvec();
  a.g_pose = h->gpose();
  a.dU = h->dU();
  a.ld = h->ld;
  a.n_pose = h->n_pose;
  a.skip_if = skip_if;
  a.ug_slot1 = h->ug_slot[1].p;
  a.w_slot1 = h->w_slot[1].p;
  a.sel = sel;
  a.prep = fp;
  a.ztiles = fold ? h->ztiles.as<int2>() : nullptr;
  a.n_ztiles = h->n_ztiles;
  a.vec = h->bvec();
  a.n_vec = 3 * h->ld;
  a.lm_out = h->lm_out[c].as<double>();
  a.lm_out1 = h->lm_out[1].as<double>();
  a.D_ray = h->D_ray.as<double>();
  tm_begin(h, TM_SCHUR);
  if (h->precision == PTZBA_FP32)
    launch_schur<float>(a, h->n_s2_items, h->n_s2_groups, h->n_fixed, h->st, h->k2_valu32);
  else
    launch_schur<double>(a, h->n_s2_items, h->n_s2_groups, h->n_fixed, h->st, false);
  tm_end(h, TM_SCHUR);
  // pose priors: S += P, g_pose += P e, b -= P e, dU += diag P at the build's state (not part of the timed Schur group)
  // (with_priors == false: ptzba_marginal_prior's build of the dropped records alone)
  if (h->has_priors() && with_priors)
    launch_prior_apply(prior_args(h, sel, 0), h->S(), h->bvec(), h->gpose(), h->dU(), h->frame_pos.as<int32_t>(), skip_if,
                       h->st);
  if (h->has_marg() && with_priors)
    launch_marg_apply(marg_args(h, sel, 0), h->S(), h->ld, h->bvec(), h->gpose(), h->dU(), h->frame_pos.as<int32_t>(),
                      skip_if, h->st);
  HIPCHK(hipGetLastError());
  if (h->dist_mode) {
    if (!h->has_exchange()) return fail("a part-owned handle needs an exchange (ptzba_attach_comm / ptzba_set_exchange_hook)");
    const auto& p0 = h->ph[0];
    if (p0.nr > 1) {  // a shared leaf: its columns (and b | g | dU over its rows) summed inside the leaf's group
      launch_pack_region(h->S(), h->ld, h->ph_tiles[0].as<int2>(), p0.n_tiles, h->bvec(), p0.vr, h->ph_buf[0].as<double>(), 0, h->st);
      if (exchange(h, PTZBA_X_PART, h->ph_buf[0].as<double>(), p0.n_buf)) return -1;
      launch_pack_region(h->S(), h->ld, h->ph_tiles[0].as<int2>(), p0.n_tiles, h->bvec(), p0.vr, h->ph_buf[0].as<double>(), 1, h->st);
      HIPCHK(hipGetLastError());
    }
  } else if (h->has_exchange()) {  // replicated: the packed reduced system summed over all ranks
    if (ptzba_exchange_packed(h, nullptr, nullptr)) return -1;
    const int64_t n = (int64_t)h->n_xtiles * CHOL_NB * CHOL_NB + 3 * h->ld;
    launch_pack_exchange(h->S(), h->ld, h->xtiles.as<int2>(), h->n_xtiles, h->bvec(), h->xbuf.as<double>(), 0, h->st);
    if (exchange(h, PTZBA_X_SYS, h->xbuf.as<double>(), n)) return -1;
    launch_pack_exchange(h->S(), h->ld, h->xtiles.as<int2>(), h->n_xtiles, h->bvec(), h->xbuf.as<double>(), 1, h->st);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

int ptzba_build_reduced(ptzba_handle h, double lambda) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!(lambda >= 0) || !std::isfinite(lambda)) return fail("bad lambda");
  HIPCHK(hipSetDevice(h->device));
  h->lambda = lambda;
  return build_impl(h, lambda, nullptr);
}

// prepare (augmented row, padding, pose damping with h->lambda or *lam_dev) and factor the built reduced system: the
// front of a solve, and of ptzba_covariance at lambda = 0
int ptzba::factor_impl(ptzba_ctx* h, const double* lam_dev, const int* sel) {
  const int4* th = reinterpret_cast<const int4*>(h->chol_tasks_host.data());
  if (h->dist_mode) {
    // the rank's phases (make_plan_tree): before each later phase its columns are summed over its node's group
    for (int q = 0; q < h->n_phase; ++q) {
      const auto& d = h->ph[q];
      if (q > 0) {
        launch_pack_region(h->S(), h->ld, h->ph_tiles[q].as<int2>(), d.n_tiles, h->bvec(), d.vr, h->ph_buf[q].as<double>(), 0, h->st);
        HIPCHK(hipGetLastError());
        if (exchange(h, d.kind, h->ph_buf[q].as<double>(), d.n_buf)) return -1;
        launch_pack_region(h->S(), h->ld, h->ph_tiles[q].as<int2>(), d.n_tiles, h->bvec(), d.vr, h->ph_buf[q].as<double>(), 1, h->st);
      }
      launch_chol_prepare_damped(h->S(), h->ld, h->n_aug, h->bvec(), h->row_pad.as<uint8_t>(), h->info.as<int>(),
                                 h->dU(), h->D_pose.as<double>(), h->frame_pos.as<int32_t>(), h->n_pose, h->n_fixed,
                                 h->lambda, lam_dev, h->st, h->row_phase.as<uint8_t>(), q + 1);
      launch_cholesky(h->S(), h->ld, h->chol_tasks.as<int4>(), h->chol_task_off.data(), d.lv1, h->Ldiag.as<double>(),
                      h->info.as<int>(), h->st, nullptr, th, h->Minv.as<double>(), d.lv0, h->chol_delayed);
      HIPCHK(hipGetLastError());
    }
  } else {
    if (!(sel && h->fused_prep()))  // device-driven single-GPU builds wrote the augmented row, padding, damping
      launch_chol_prepare_damped(h->S(), h->ld, h->n_aug, h->bvec(), h->row_pad.as<uint8_t>(), h->info.as<int>(),
                                 h->dU(), h->D_pose.as<double>(), h->frame_pos.as<int32_t>(), h->n_pose, h->n_fixed,
                                 h->lambda, lam_dev, h->st);
    launch_cholesky(h->S(), h->ld, h->chol_tasks.as<int4>(), h->chol_task_off.data(), h->chol_levels,
                      h->Ldiag.as<double>(), h->info.as<int>(), h->st, nullptr, th, h->Minv.as<double>(), 0,
                      h->chol_delayed);
  }
  return 0;
}

// damped solve, trial state, trial linearisation into slot `nx` and the trial scalars (device-driven LM:
// current slot *sel, trial slot *sel ^ 1, chosen on the device)
int ptzba::solve_impl(ptzba_ctx* h, const double* lam_dev, int nx, const int* sel) {
  const int c = sel ? 0 : h->cur;
  if (sel) nx = 1;  // the trial's slot, with the other slot as the selector's alternative
  tm_begin(h, TM_CHOL);
  if (factor_impl(h, lam_dev, sel)) return -1;
  if (h->bs_pst)
    launch_chol_backsolve_pst(h->S(), h->ld, h->n_aug, h->bsb_tasks.as<int4>(), h->bsp_expect.as<int4>(),
                              h->bsb_step_off.back(), h->Ldiag.as<double>(), h->Minv.as<double>(), h->bsb_r.as<double>(),
                              h->dpose.as<double>(), h->bsp_cnt.as<unsigned>(), h->bsp_tot.as<int>(), h->bsp_epoch++,
                              h->bsp_err, h->st, h->tinv_tail.as<int>(), h->n_tinv_tail);
  else if (h->bs_blk)
    launch_chol_backsolve_blk(h->S(), h->ld, h->n_aug, h->bsb_tasks.as<int4>(), h->bsb_step_off.data(), (int)h->bsb_step_off.size() - 1, h->Ldiag.as<double>(),
                              h->Minv.as<double>(), h->bsb_r.as<double>(), h->dpose.as<double>(), h->st,
                              h->tinv_tail.as<int>(), h->n_tinv_tail);
  else
    launch_chol_backsolve(h->S(), h->ld, h->n_aug, h->n_chain, h->bs_npos, h->bs_chain_off.as<int>(),
                          h->bs_chain_cols.as<int>(), h->bs_upd_off.as<int>(), h->bs_upd_tiles.as<int>(), h->bs_nupd,
                          h->bs_la_tasks.as<int>(), h->bs_ntasks,
                          h->Ldiag.as<double>(), h->Minv.as<double>(), h->dpose.as<double>(),
                          h->bs_ll ? h->bs_lo_off.as<int>() : nullptr, h->bs_lo_tiles.as<int>(), h->st,
                          h->tinv_tail.as<int>(), h->n_tinv_tail);
  tm_end(h, TM_CHOL);
  HIPCHK(hipGetLastError());
  tm_begin(h, TM_BACK);
  BacksubArgs b;
  b.lm_seg_begin = h->lm_seg_begin.as<int32_t>();
  b.seg_frame = h->seg_frame.as<int32_t>();
  b.seg_row = h->seg_row.as<int32_t>();
  b.w_slot = h->w_slot[c].p;
  b.lm_meta = h->lm_meta.as<int4>();
  b.lm_out = h->lm_out[c].as<double>();
  b.lm_aux = h->lm_aux.as<double>();
  b.D_ray = h->D_ray.as<double>();
  b.dpose = h->dpose.as<double>();
  b.frame_pos = h->frame_pos.as<int32_t>();
  b.rays = h->rays.as<double>();
  b.rays_trial = h->rays_trial.as<double>();
  b.lm_red = h->lm_red.as<double>();
  b.n_lm = h->n_lm;
  b.n_fixed = h->n_fixed;
  b.lambda = h->lambda;
  b.lam_dev = lam_dev;
  b.w_slot1 = h->w_slot[1].p;
  b.lm_out1 = h->lm_out[1].as<double>();
  b.sel = sel;
  b.state_xor = h->state_base;
  // ray back-substitution, trial poses and the trial's frame / ray tables: one launch
  const uint8_t* fm = h->dist_mode ? h->fmask.as<uint8_t>() : nullptr;
  const int* finfo = h->dist_mode ? h->info.as<int>() : nullptr;
  if (h->precision == PTZBA_FP32)
    launch_trial<float>(b, h->ptz.as<double>(), h->gpose(), h->D_pose.as<double>(), h->ptz_trial.as<double>(),
                        h->locp(), h->n_pose, h->ft64.p, h->rt64.p, h->ft.p, h->rt.p, h->st, fm, finfo);
  else
    launch_trial<double>(b, h->ptz.as<double>(), h->gpose(), h->D_pose.as<double>(), h->ptz_trial.as<double>(),
                         h->locp(), h->n_pose, h->ft64.p, h->rt64.p, h->ft64.p, h->rt64.p, h->st, fm, finfo);
  tm_end(h, TM_BACK);
  // the prior's cost at the trial state into loc[5], which the decision (host or device, fused or not) adds to the
  // trial cost; without priors the slot stays zero
  if (h->has_priors()) launch_prior_cost(prior_args(h, sel, 1), h->locp() + 5, 1.0, 0, h->pri.red.as<double>(), h->st);
  if (h->has_marg()) launch_marg_cost(marg_args(h, sel, 1), h->locp() + 5, h->has_priors() ? 1 : 0, h->st);
  // trial linearisation (its cost decides acceptance; kept as the next linearisation if accepted).  Device-driven LM
  // with the huber curvature switch pending: single GPU (relin_mode 0), the trial's predicted reduction is reduced
  // first and picks the curvature of this linearisation (LMDev::hc_trial); ranks (relin_mode 1) use LMDev::hc
  const double* hc_dev = nullptr;
  if (sel) {
    LMDev* st = h->lmdev.as<LMDev>();
    hc_dev = h->lm_relin_mode ? &st->hc : &st->hc_trial;
    if (!h->lm_relin_mode && h->lm_curv_pending) {
      const DecideArgs cd{st, h->locp(), nullptr, nullptr, 0, 1};
      launch_reduce_cols(h->lm_red.as<double>(), h->n_lm, 4, 1, 0, h->curv_pred.as<double>(), h->red_scratch.as<double>(),
                         h->st, nullptr, 0, 0, nullptr, nullptr, nullptr, 0, &cd);
    }
  }
  linearize_into(h, nx, sel, 1, nullptr, hc_dev, true);
  // scal[1] (trial cost) and scal[2..5] are overwritten below, loc[0..3] by the trial kernel: no memsets
  if (sel && !h->has_exchange() && !h->ext_exchange && !h->scal_exported && !h->dist_mode) {
    // launched by ptzba_lm_decide with the decision fused into it (nothing runs between the two calls)
    h->scal_deferred = true;
    return 0;
  }
  launch_reduce_cols(h->lm_out[sel ? 0 : nx].as<double>() + 5, h->n_lm, 8, 1, LM_RED_MAXMASK, h->scal.as<double>() + 1,
                     h->red_scratch.as<double>(), h->st, h->lm_red.as<double>(), 4, 4, h->scal.as<double>() + 2,
                     h->lm_out[1].as<double>() + 5, sel, 1);
  HIPCHK(hipGetLastError());
  // partial scalars (replicated: the landmark sums; part-owned: also the pose partials, each frame counted
  // by one rank -- the gradient max then sums the ranks' maxima, an upper bound: gtol can only stop later)
  if (h->has_exchange()) return exchange(h, PTZBA_X_SCAL, h->scal.as<double>(), scal_count(h));
  return 0;
}

int ptzba_solve_reduced(ptzba_handle h) {
  if (!h || !h->have_problem) return fail("no problem set");
  HIPCHK(hipSetDevice(h->device));
  h->trial_open = true;
  return solve_impl(h, nullptr, 1 - h->cur);
}

// ------------------------------------------------------------------------------------------------
// device-driven Levenberg-Marquardt (the decisions of ptzba.LMSolver on the device): the host only
// enqueues trials and polls a pinned record ring, so no trial waits for a host round trip.  The two
// linearisation slots are selected on the device (LMDev::cur): a trial linearises into the other slot, an
// accepted trial flips cur, a rejected one leaves the current linearisation in place (no re-linearisation).
// ------------------------------------------------------------------------------------------------
static int lm_check(ptzba_ctx* h) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!h->lmdev.p) return fail("call ptzba_lm_start first");
  return 0;
}

int ptzba_lm_start(ptzba_handle h) {
  if (!h || !h->have_problem) return fail("no problem set");
  HIPCHK(hipSetDevice(h->device));
  if (!h->lmdev.p && h->lmdev.alloc(sizeof(LMDev))) return -1;
  if (!h->curv_pred.p && h->curv_pred.alloc(64)) return -1;
  h->hcurv = 1.0;  // the initial linearisation: IRLS (the host-driven LM's setting does not carry over)
  if (!h->lm_host) {
    HIPCHK(hipHostMalloc((void**)&h->lm_host, LM_RING * sizeof(LMDev), hipHostMallocCoherent));
  }
  h->cur = 0;
  return ptzba_linearize(h);
}

int ptzba_lm_init(ptzba_handle h, const ptzba_lm_opts* o) {
  if (lm_check(h)) return -1;
  if (!o) return fail("null options");
  if (!(o->lambda0 >= 0) || !(o->min_lambda > 0) || !(o->max_lambda > 0) || o->max_iter < 0 || o->max_retries < 1)
    return fail("bad LM options");
  HIPCHK(hipSetDevice(h->device));
  // the two curvature fields (added in version 5 of the options struct) matter for the robust losses only; a caller that
  // zero-fills them gets the default curvature (0.1) and no switch (curvature_switch 0)
  const double hcv = o->huber_curvature == 0.0 ? 0.1 : o->huber_curvature;
  const bool robust = h->loss != PTZBA_LOSS_LINEAR;
  if (robust && (!(hcv > 0.0 && hcv <= 1.0) || !(o->curvature_switch >= 0.0)))
    return fail("bad LM options (huber_curvature in (0, 1], curvature_switch >= 0)");
  const bool sw = robust && o->curvature_switch > 0.0 && hcv < 1.0;
  LMParams p{o->ftol, o->xtol, o->gtol, o->lambda0, o->min_lambda, o->max_lambda,
             sw ? hcv : 1.0, sw ? o->curvature_switch : 0.0, o->max_iter, o->max_retries,
             o->gauss_newton ? 1 : 0, 0};
  // the switch's launches (relin_mode 1: the conditional re-linearisation in lm_build; 0: the predicted-reduction
  // reduce in front of the trial K1) are queued until the host sees the switch in a decision record
  h->lm_curv_pending = sw;
  h->lm_relin_mode = h->has_exchange() || h->ext_exchange || h->scal_exported || h->dist_mode;
  p.relin_mode = h->lm_relin_mode ? 1 : 0;
  // no decision of an earlier run is in flight (its lm_wait returned): clear the ring's sequence tags
  for (int k = 0; k < LM_RING; ++k) __atomic_store_n(&h->lm_host[k].seq, 0, __ATOMIC_RELAXED);
  launch_lm_init(h->lmdev.as<LMDev>(), h->scal.as<double>(), p, h->cur, h->st);
  h->state_base = h->cur;  // (ptz, rays) hold the current state now
  if (h->bsp_err) *h->bsp_err = 0;  // a run starts without an earlier run's gave-up flag (nothing of it is in flight)
  h->scal_deferred = false;
  HIPCHK(hipGetLastError());
  return 0;
}

int ptzba_lm_build(ptzba_handle h) {
  if (lm_check(h)) return -1;
  HIPCHK(hipSetDevice(h->device));
  // the curvature switch of the last decision (LMDev::relin): re-linearise the current point into its slot first.
  // Queued only until the host has seen the switch in a decision record; the launch reads the flag on the device
  if (h->lm_curv_pending && h->lm_relin_mode)
    linearize_into(h, 0, &h->lmdev.as<LMDev>()->cur, 0, &h->lmdev.as<LMDev>()->relin, &h->lmdev.as<LMDev>()->hc);
  // a build queued after the final decision (the host pipelines one trial ahead) exits at once
  return build_impl(h, 0.0, &h->lmdev.as<LMDev>()->lam, &h->lmdev.as<LMDev>()->done, &h->lmdev.as<LMDev>()->cur);
}

int ptzba_lm_solve(ptzba_handle h) {
  if (lm_check(h)) return -1;
  HIPCHK(hipSetDevice(h->device));
  return solve_impl(h, &h->lmdev.as<LMDev>()->lam, 1 - h->cur, &h->lmdev.as<LMDev>()->cur);
}

int ptzba_lm_decide(ptzba_handle h, int trial) {
  if (lm_check(h)) return -1;
  if (trial < 0) return fail("bad trial index");
  HIPCHK(hipSetDevice(h->device));
  LMDev* st = h->lmdev.as<LMDev>();
  const int k = trial % LM_RING;
  // the record is written by the decision straight into pinned host memory.  No commit copy: an accepted trial
  // flips LMDev::cur, which selects the state pair as it selects the linearisation slot (BacksubArgs::state_xor)
  if (h->scal_deferred) {
    // single GPU: the trial-cost reduction (deferred by lm_solve) with the decision in its last workgroup
    h->scal_deferred = false;
    const int* sel = &h->lmdev.as<LMDev>()->cur;
    const DecideArgs dec{st, h->locp(), h->info.as<int>(), h->lm_host + k, trial + 1};
    launch_reduce_cols(h->lm_out[0].as<double>() + 5, h->n_lm, 8, 1, LM_RED_MAXMASK, h->scal.as<double>() + 1,
                       h->red_scratch.as<double>(), h->st, h->lm_red.as<double>(), 4, 4, h->scal.as<double>() + 2,
                       h->lm_out[1].as<double>() + 5, sel, 1, &dec);
  } else {
    launch_lm_decide(st, h->scal.as<double>(), h->locp(), h->info.as<int>(), h->lm_host + k, trial + 1,
                     h->st, h->dist_mode);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int ptzba_lm_wait(ptzba_handle h, int trial, ptzba_lm_record* out) {
  if (lm_check(h)) return -1;
  if (trial < 0 || !out) return fail("bad arguments");
  HIPCHK(hipSetDevice(h->device));
  const int k = trial % LM_RING;
  // the decision kernel tags its record last; poll the tag (an event record per trial would add a
  // ~6 us gap to the stream).  Every 4096 polls check that the stream is still alive.
  for (int64_t n = 0; __atomic_load_n(&h->lm_host[k].seq, __ATOMIC_ACQUIRE) != trial + 1; ++n) {
    if ((n & 4095) == 4095) {
      const hipError_t q = hipStreamQuery(h->st);
      if (q != hipSuccess && q != hipErrorNotReady) return fail("lm_wait: stream error %s", hipGetErrorString(q));
      if (q == hipSuccess && __atomic_load_n(&h->lm_host[k].seq, __ATOMIC_ACQUIRE) != trial + 1)
        return fail("lm_wait: no decision record for trial %d (was ptzba_lm_decide called?)", trial);
    }
    __builtin_ia32_pause();
  }
  if (h->bs_pst && __atomic_load_n(h->bsp_err, __ATOMIC_ACQUIRE))
    return fail("lm_wait: a persistent factorisation / back-substitution kernel gave up waiting (workgroups not "
                "co-resident?); PTZBA_BS_PERSIST=0 selects the per-step form");
  const LMDev& r = h->lm_host[k];
  out->cost = r.cost;
  out->initial_cost = r.initial_cost;
  out->lambda = r.lam;
  out->iterations = r.it;
  out->nfev = r.nfev;
  out->trials = r.trials;
  out->retries = r.retries;
  out->status = r.status;
  out->done = r.done;
  out->accepted = r.accepted;
  if (r.hc != 1.0) h->lm_curv_pending = false;  // switched: the launches already queued behind it suffice
  h->cur = r.cur;  // the host's view of the current slot follows the device (ptzba_accept / linearize)
  if ((r.cur ^ h->state_base) & 1) {
    // the device's decisions moved the current state to the other pair: swap the pointers and the base together,
    // so that kernels already queued (old pair, old base) and later ones (new pair, new base) select the same buffer
    std::swap(h->ptz.p, h->ptz_trial.p);
    std::swap(h->ptz.bytes, h->ptz_trial.bytes);
    std::swap(h->ptz.cap, h->ptz_trial.cap);
    std::swap(h->rays.p, h->rays_trial.p);
    std::swap(h->rays.bytes, h->rays_trial.bytes);
    std::swap(h->rays.cap, h->rays_trial.cap);
    h->state_base ^= 1;
  }
  return 0;
}

// One-shot solve: the device-driven LM run to termination in C (the sequence ptzba.LMSolver drives from
// Python, single process).  Replaces the optimizer call least_squares(_compute_residual, x0, x_scale='jac',
// ftol=1e-4, method='trf') of bundle_adjustment.py:200-202 and the empty C stub bundle_adjustment_opt
// (rf_map/python_package/backup/bundle_adjustment_python.hpp:21-24): the state goes in and the optimum
// comes out through the caller's buffers (rf_map.cpp:77, 113-116 in/out convention).
// the device-driven LM from the handle's current device state to termination (shared by the one-shot entries)
static int lm_run(ptzba_ctx* h, const ptzba_lm_opts& o, ptzba_lm_record& rec) {
  if (ptzba_lm_start(h) || ptzba_lm_init(h, &o)) return -1;
  rec = ptzba_lm_record{};
  if (o.max_iter > 0) {
    const int64_t limit = (int64_t)o.max_iter * (o.max_retries + 1);
    if (ptzba_lm_build(h)) return -1;
    for (int k = 0;; ) {
      if (ptzba_lm_solve(h) || ptzba_lm_decide(h, k)) return -1;
      if (k + 1 < limit && ptzba_lm_build(h)) return -1;  // next trial queued behind this decision
      if (ptzba_lm_wait(h, k, &rec)) return -1;
      ++k;
      if (rec.done || k >= limit) break;
    }
  } else {
    double s[PTZBA_NSCALARS];
    if (ptzba_read_scalars(h, s)) return -1;
    rec.cost = rec.initial_cost = s[0];
    rec.nfev = 1;
  }
  return 0;
}
static const ptzba_lm_opts k_default_opts{1e-4, 1e-8, 0.0, 1e-12, 1e-12, 1e16, 100, 30, 0, 0.1, 0.25};

int ptzba_solve_resident(ptzba_handle h, int restore, const ptzba_lm_opts* opts, ptzba_report* report) {
  if (!h || !h->have_problem) return fail("no problem set");
  const ptzba_lm_opts o = opts ? *opts : k_default_opts;
  const auto t0 = std::chrono::steady_clock::now();
  if (restore && ptzba_restore_state(h)) return -1;
  ptzba_lm_record rec{};
  if (lm_run(h, o, rec)) return -1;
  if (report) {
    report->cost = rec.cost;
    report->initial_cost = rec.initial_cost;
    report->time_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    report->iterations = rec.iterations;
    report->nfev = rec.nfev;
    report->trials = rec.trials;
    report->status = rec.status;
  }
  return 0;
}

int ptzba_solve(ptzba_handle h, double* ptz_inout, double* rays_inout, const ptzba_lm_opts* opts,
                ptzba_report* report) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!ptz_inout || (h->n_lm > 0 && !rays_inout)) return fail("null state buffer");
  const ptzba_lm_opts o = opts ? *opts : k_default_opts;
  const auto t0 = std::chrono::steady_clock::now();
  if (ptzba_set_state(h, ptz_inout, rays_inout)) return -1;
  ptzba_lm_record rec{};
  if (lm_run(h, o, rec)) return -1;
  std::vector<double> ptz(3 * (size_t)h->n_pose), rays(2 * (size_t)h->n_lm);
  if (ptzba_get_state(h, ptz.data(), rays.data())) return -1;
  std::copy(ptz.begin(), ptz.end(), ptz_inout);
  if (h->n_lm) std::copy(rays.begin(), rays.end(), rays_inout);
  if (report) {
    report->cost = rec.cost;
    report->initial_cost = rec.initial_cost;
    report->time_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    report->iterations = rec.iterations;
    report->nfev = rec.nfev;
    report->trials = rec.trials;
    report->status = rec.status;
  }
  return 0;
}

int ptzba_step(ptzba_handle h, double lambda) {
  int rc = ptzba_build_reduced(h, lambda);
  if (rc) return rc;
  return ptzba_solve_reduced(h);
}

int ptzba_read_scalars(ptzba_handle h, double* out) {
  if (!h || !h->have_problem) return fail("no problem set");
  HIPCHK(hipSetDevice(h->device));
  // one kernel packs scal | loc | info, one copy brings the block to pinned host memory
  launch_pack_scalars(h->scal.as<double>(), h->locp(), h->info.as<int>(), h->scal_pack.as<double>(), h->st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h->scal_host, h->scal_pack.p, 17 * sizeof(double), hipMemcpyDeviceToHost, h->st));
  HIPCHK(hipStreamSynchronize(h->st));
  if (h->bs_pst && __atomic_load_n(h->bsp_err, __ATOMIC_ACQUIRE))
    return fail("the persistent back-substitution kernel gave up waiting (PTZBA_BS_PERSIST=0 selects the per-step form)");
  const double* s = h->scal_host;
  const double* l = h->scal_host + 8;
  out[0] = s[0];
  out[1] = s[1] + l[5];  // l[5]: the pose priors' cost at the trial state (zero without priors)
  out[2] = s[2] + l[0];
  out[3] = s[3] + l[1];
  out[4] = s[4] + l[2];
  out[5] = h->dist_mode ? l[4] : h->scal_host[16];  // part-owned: the status summed over ranks
  out[6] = std::max(l[3], s[5]);  // the gradient's largest entry over the free poses (loc) and the rays (scal)
  out[7] = 0;
  return 0;
}

int ptzba_accept(ptzba_handle h, int accept) {
  if (!h || !h->have_problem) return fail("no problem set");
  h->trial_open = false;
  if (accept) {
    h->cur = 1 - h->cur;
    std::swap(h->ptz.p, h->ptz_trial.p);
    std::swap(h->ptz.bytes, h->ptz_trial.bytes);
    std::swap(h->ptz.cap, h->ptz_trial.cap);
    std::swap(h->rays.p, h->rays_trial.p);
    std::swap(h->rays.bytes, h->rays_trial.bytes);
    std::swap(h->rays.cap, h->rays_trial.cap);
  }
  return 0;
}

int ptzba_exchange(ptzba_handle h, void** sys_ptr, int64_t* sys_count, void** scal_ptr) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (sys_ptr) h->ext_exchange = true;  // the caller may sum the system between build and solve: prepare after it
  if (sys_ptr) *sys_ptr = h->sys.p;
  if (sys_count) *sys_count = h->sys_count();
  if (scal_ptr) {
    *scal_ptr = h->scal.p;
    h->scal_exported = true;  // the caller may sum the scalars between lm_solve and lm_decide: no fused decision
  }
  return 0;
}

int ptzba_exchange_packed(ptzba_handle h, void** buf, int64_t* count) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (buf && !h->has_exchange()) h->ext_exchange = true;  // the caller's own protocol (see ptzba_exchange)
  const int64_t n = (int64_t)h->n_xtiles * CHOL_NB * CHOL_NB + 3 * h->ld;
  if (!h->xbuf.p && h->xbuf.alloc((size_t)n * 8)) return -1;
  if (buf) *buf = h->xbuf.p;
  if (count) *count = n;
  return 0;
}

static int pack_impl(ptzba_handle h, int unpack) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!h->xbuf.p) return fail("call ptzba_exchange_packed first");
  HIPCHK(hipSetDevice(h->device));
  launch_pack_exchange(h->S(), h->ld, h->xtiles.as<int2>(), h->n_xtiles, h->bvec(), h->xbuf.as<double>(), unpack, h->st);
  HIPCHK(hipGetLastError());
  return 0;
}
int ptzba_pack(ptzba_handle h) { return pack_impl(h, 0); }
int ptzba_unpack(ptzba_handle h) { return pack_impl(h, 1); }

int ptzba_set_exchange_hook(ptzba_handle h, ptzba_exchange_fn fn, void* ctx) {
  if (!h) return fail("null handle");
  if (fn && h->has_marg()) return fail("ptzba_set_exchange_hook: the handle has a marginal prior set (single rank only)");
  if (fn && h->has_priors()) return fail("ptzba_set_exchange_hook: the handle has pose priors set (single rank only)");
  if (fn && h->has_ray_priors()) return fail("ptzba_set_exchange_hook: the handle has ray priors set (single rank only)");
  if (fn && h->displaced) return fail("ptzba_set_exchange_hook: the handle has a displacement set (single rank only)");
  h->hook = fn;
  h->hook_ctx = ctx;
  return 0;
}

int ptzba_attach_comm(ptzba_handle h, ptzba_comm comm) {
  if (!h) return fail("null handle");
  if (comm && h->has_marg()) return fail("ptzba_attach_comm: the handle has a marginal prior set (single rank only)");
  if (comm && h->has_priors()) return fail("ptzba_attach_comm: the handle has pose priors set (single rank only)");
  if (comm && h->has_ray_priors()) return fail("ptzba_attach_comm: the handle has ray priors set (single rank only)");
  if (comm && h->displaced) return fail("ptzba_attach_comm: the handle has a displacement set (single rank only)");
  h->drop_groups();
  h->comm = comm;
  return 0;  // the group communicator is split lazily by the first exchange (collective, every rank reaches it)
}

int ptzba_dist_info(ptzba_handle h, int64_t* info8) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!info8) return fail("null output");
  info8[0] = h->dist_mode;
  info8[1] = h->dist_mode ? h->base_node : -1;
  info8[2] = h->dist_mode ? h->ph[0].nr : 1;
  info8[3] = h->dist_mode ? (h->dist_rank == h->ph[0].r0) : 1;
  int64_t sep = 0, sub = 0;
  for (int q = 1; q < h->n_phase; ++q) (h->ph[q].kind == PTZBA_X_SEP ? sep : sub) += h->ph[q].n_buf;
  info8[4] = sep;
  info8[5] = h->dist_mode && h->ph[0].nr > 1 ? h->ph[0].n_buf : 0;
  info8[6] = h->dist_mode || h->dist_world < 2 ? 0 : (int64_t)h->n_xtiles * CHOL_NB * CHOL_NB + 3 * h->ld;
  info8[7] = scal_count(h);
  return 0;
}

int ptzba_dist_exchanges(ptzba_handle h, int64_t* out, int32_t cap, int32_t* n_out) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!n_out) return fail("null output");
  std::vector<int64_t> v;
  if (h->dist_mode) {
    if (h->ph[0].nr > 1) v.insert(v.end(), {PTZBA_X_PART, h->ph[0].r0, h->ph[0].nr, h->ph[0].n_buf});
    for (int q = 1; q < h->n_phase; ++q) v.insert(v.end(), {h->ph[q].kind, h->ph[q].r0, h->ph[q].nr, h->ph[q].n_buf});
    v.insert(v.end(), {PTZBA_X_SCAL, 0, h->dist_world, scal_count(h)});
  } else if (h->dist_world >= 2) {
    v.insert(v.end(), {PTZBA_X_SYS, 0, h->dist_world, (int64_t)h->n_xtiles * CHOL_NB * CHOL_NB + 3 * h->ld});
    v.insert(v.end(), {PTZBA_X_SCAL, 0, h->dist_world, scal_count(h)});
  }
  *n_out = (int32_t)(v.size() / 4);
  if (out) {
    if (cap < *n_out) return fail("output holds %d exchanges, %d needed", cap, *n_out);
    std::copy(v.begin(), v.end(), out);
  }
  return 0;
}
int ptzba_dist_groups(ptzba_handle h, int32_t* out, int32_t cap, int32_t* n_out) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!n_out) return fail("null output");
  *n_out = (int32_t)(h->tree_groups.size() / 3);
  if (out) {
    if (cap < *n_out) return fail("output holds %d groups, %d needed", cap, *n_out);
    std::copy(h->tree_groups.begin(), h->tree_groups.end(), out);
  }
  return 0;
}
int ptzba_exchange_group(ptzba_handle h, int32_t kind, int32_t* r0_nr) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!r0_nr) return fail("null output");
  r0_nr[0] = 0;
  r0_nr[1] = h->dist_world;
  if (h->dist_mode && kind != PTZBA_X_SEP && kind != PTZBA_X_SCAL) {
    for (int q = 0; q < h->n_phase; ++q)
      if (h->ph[q].kind == kind && (q > 0 || h->ph[0].nr > 1)) {
        r0_nr[0] = h->ph[q].r0;
        r0_nr[1] = h->ph[q].nr;
        return 0;
      }
    return fail("this rank runs no exchange of kind %d", kind);
  }
  return 0;
}
int ptzba_owned_frames(ptzba_handle h, uint8_t* mask_out) {
  if (!h || !h->have_problem) return fail("no problem set");
  if (!mask_out) return fail("null output");
  std::copy(h->owned_host.begin(), h->owned_host.end(), mask_out);
  return 0;
}

int ptzba_sync(ptzba_handle h) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->st));
  return 0;
}

int ptzba_reset_kernel_times(ptzba_handle h, int enable) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->st));
  for (int k = 0; k < TM_N; ++k) {
    if (((enable >> k) & 1) && h->ev[k].empty()) {
      h->ev[k].resize(TM_POOL);
      for (auto& e : h->ev[k]) HIPCHK(hipEventCreate(&e));
    }
    h->ev_used[k] = 0;
    h->tm_seen[k] = 0;
    h->tm_sampled[k] = false;
  }
  h->timing = enable & (((1 << TM_N) - 1) | PTZBA_TIME_COMM);
  if ((enable & PTZBA_TIME_COMM) && h->cev.empty()) {
    h->cev.resize(2 * COMM_POOL);
    for (auto& e : h->cev) HIPCHK(hipEventCreate(&e));
  }
  h->cev_used = 0;
  h->clog.clear();
  h->tm_stride = std::max(1, (enable >> 8) & 0xff);
  h->tm_flush = (enable & PTZBA_TIME_FLUSH) != 0;
  h->tm_flush_read = h->tm_flush && (enable & PTZBA_TIME_FLUSH_READ) != 0;
  if (h->tm_flush && !h->flush_buf.p) {
    if (h->flush_buf.alloc(FLUSH_BYTES)) return -1;
    k_flush_caches<<<4096, 256, 0, h->st>>>(h->flush_buf.as<float4>(), (int64_t)(FLUSH_BYTES / 16), 1.0f);
    HIPCHK(hipGetLastError());
  }
  if (!h->tm_flush) h->flush_buf.release();
  return 0;
}

int ptzba_kernel_times(ptzba_handle h, double* ms_out, int64_t* count_out) {
  if (!h) return fail("null handle");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->st));
  for (int k = 0; k < TM_N; ++k) {
    double tot = 0;
    int n = h->ev_used[k] / 2;
    for (int i = 0; i < n; ++i) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, h->ev[k][2 * i], h->ev[k][2 * i + 1]));
      tot += ms;
    }
    ms_out[k] = n ? tot / n : 0.0;
    count_out[k] = n;
  }
  return 0;
}

int ptzba_comm_times(ptzba_handle h, int32_t cap, int32_t* kinds, int64_t* doubles, double* ms, int32_t* n_out) {
  if (!h || !n_out || cap < 0 || (cap > 0 && (!kinds || !doubles || !ms))) return fail("ptzba_comm_times: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipStreamSynchronize(h->st));
  const int32_t n = (int32_t)h->clog.size();
  for (int32_t i = 0; i < std::min(n, cap); ++i) {
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, h->cev[2 * i], h->cev[2 * i + 1]));
    kinds[i] = h->clog[i].first;
    doubles[i] = h->clog[i].second;
    ms[i] = t;
  }
  *n_out = n;
  return 0;
}


// host-driven LM (ptzba.LMSolver._run_host, ptzba_linearize / ptzba_step): the huber curvature weight of the
// following linearisations (the device-driven LM keeps its own in LMDev::hc)
int ptzba_set_huber_curvature(ptzba_handle h, double hc) {
  if (!h) return fail("null handle");
  if (!(hc > 0.0 && hc <= 1.0)) return fail("huber curvature must lie in (0, 1]");
  h->hcurv = hc;
  return 0;
}

bool ptzba::single_rank(const ptzba_ctx* h) {
  return !(h->dist_mode || h->dist_world > 1 || h->has_exchange() || h->ext_exchange || h->scal_exported);
}


// which front the following set_problem calls use (round 6): the device front from min_records records on
// (0: always, INT64_MAX: never, -1: the default GPU_SETUP_MIN_REC = 64K).  Both fronts build the same arrays bit for bit
// (tests/test_gpu_ba.py compares them); the knob is the test hook and a per-handle tuning point.
int ptzba_set_setup_front(ptzba_handle h, int64_t min_records) {
  if (!h) return fail("null handle");
  h->gpu_setup_min = min_records < 0 ? -1 : min_records;
  return 0;
}

// host phase times of the last ptzba_set_problem: names[k] (static strings) and ms[k], k < *n_out (<= cap)
int ptzba_setup_timing(ptzba_handle h, int32_t cap, const char** names, double* ms, int32_t* n_out) {
  if (!h || !n_out || cap < 0 || (cap > 0 && (!names || !ms))) return fail("ptzba_setup_timing: bad arguments");
  const int32_t n = (int32_t)std::min<size_t>(h->setup_phases.size(), (size_t)cap);
  for (int32_t k = 0; k < n; ++k) {
    names[k] = h->setup_phases[k].first;
    ms[k] = h->setup_phases[k].second;
  }
  *n_out = (int32_t)h->setup_phases.size();
  return 0;
}
