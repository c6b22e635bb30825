// mlf_debug.hip -- timing, statistics and diagnostics entry points: nothing a sampling run calls.  Host code only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <vector>

#include "../../include/mlfriends_hip.h"
#include "mlf_host.hpp"
#include "mlf_sample.hpp"

using namespace mlf;

extern "C" {

int mlf_debug_forget_grants(unsigned long long *grants_so_far) {
  if (grants_so_far) *grants_so_far = g_grant_calls.load(std::memory_order_relaxed);
  g_grant_epoch.fetch_add(1u, std::memory_order_acq_rel);
  return 0;
}

int mlf_debug_around_points_wide(int on) {
  force_around_points_wide(on != 0);
  return 0;
}

int mlf_debug_philox(uint64_t seed, unsigned stream, size_t nblocks, uint32_t *out) {
  if (!out) return fail_arg(MLF_E_BADARG, "null pointer");
  if (nblocks == 0) return 0;
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  CK(c.out.reserve(nblocks * 4 * sizeof(unsigned)));
  launch_philox_words(seed, stream, (long long)nblocks, c.out.as<unsigned>(), c.stream);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(out, c.out.p, nblocks * 4 * sizeof(unsigned), hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  return 0;
}

int mlf_region_inside_dev_timed(mlf_region *r, const double *d_pts, size_t np, uint8_t *d_mask,
                                void *stream) {
  if (!r) return fail_arg(MLF_E_BADARG, "null region");
  if (!r->ready) return fail_arg(MLF_E_STATE, "region used before mlf_region_set");
  if (!np || !d_pts || !d_mask) return fail_arg(MLF_E_BADARG, "bad argument");
  while (r->events.size() < r->events_used + 4) {
    hipEvent_t e;
    CK(hipEventCreate(&e));
    r->events.push_back(e);
  }
  hipEvent_t *ev = r->events.data() + r->events_used;
  r->events_used += 4;
  return region_inside_enqueue(r, d_pts, np, d_mask, (hipStream_t)stream, ev);
}

int mlf_region_timing_collect(mlf_region *r, int *ncalls, double *ms_prep, double *ms_scan,
                              double *ms_rest) {
  if (!r || !ncalls || !ms_prep || !ms_scan || !ms_rest) return fail_arg(MLF_E_BADARG, "null pointer");
  double prep = 0.0, scan = 0.0, rest = 0.0;
  const size_t calls = r->events_used / 4;
  for (size_t i = 0; i < calls; ++i) {
    hipEvent_t *ev = r->events.data() + 4 * i;
    CK(hipEventSynchronize(ev[3]));
    float a = 0.f, b = 0.f, c2 = 0.f;
    CK(hipEventElapsedTime(&a, ev[0], ev[1]));
    CK(hipEventElapsedTime(&b, ev[1], ev[2]));
    CK(hipEventElapsedTime(&c2, ev[2], ev[3]));
    prep += a;
    scan += b;
    rest += c2;
  }
  r->events_used = 0;
  *ncalls = (int)calls;
  *ms_prep = prep;
  *ms_scan = scan;
  *ms_rest = rest;
  return 0;
}

int mlf_region_timing_filter_launches(mlf_region *r, int *nlaunches, double *ms_total) {
  if (!r || !nlaunches || !ms_total) return fail_arg(MLF_E_BADARG, "null pointer");
  FilterCtx &f = r->filter;
  double total = 0.0;
  for (size_t i = 0; i + 1 < f.kev_used; i += 2) {
    CK(hipEventSynchronize(f.kev[i + 1]));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, f.kev[i], f.kev[i + 1]));
    total += ms;
  }
  *nlaunches = (int)(f.kev_used / 2);
  *ms_total = total;
  f.kev_used = 0;
  return 0;
}

int mlf_region_timing_filter_launch_ms(mlf_region *r, double *ms, int cap, int *nlaunches) {
  if (!r || !nlaunches || (cap > 0 && !ms)) return fail_arg(MLF_E_BADARG, "null pointer");
  FilterCtx &f = r->filter;
  int n = 0;
  for (size_t i = 0; i + 1 < f.kev_used; i += 2, ++n) {
    if (n >= cap) continue;
    CK(hipEventSynchronize(f.kev[i + 1]));
    float t = 0.f;
    CK(hipEventElapsedTime(&t, f.kev[i], f.kev[i + 1]));
    ms[n] = t;
  }
  *nlaunches = n;
  return 0;
}

int mlf_region_filter_info(mlf_region *r, size_t np, int *active, int *kdim, int *ntiles32) {
  if (!r || !active || !kdim || !ntiles32) return fail_arg(MLF_E_BADARG, "null pointer");
  *active = (r->ready && r->use_scan && plan_batch(r->filter, r, BATCH_INSIDE, (long long)np, r->r2).filter) ? 1 : 0;
  *kdim = r->filter.ks * 16;
  *ntiles32 = r->filter.ntiles32;
  return 0;
}

int mlf_region_debug_fused_stamps(mlf_region *r, int block, unsigned long long *out, int cap) {
  if (!r) return fail_arg(MLF_E_BADARG, "null region");
  FilterCtx &f = r->filter;
  if (out && cap > 0) {
    for (int i = 0; i < cap; ++i) out[i] = 0ull;
    if (f.fstamps.p && f.stamp_block >= 0) {
      CK(hipStreamSynchronize(g_ctx.stream));
      CK(hipMemcpy(out, f.fstamps.p, (size_t)(cap < 16 ? cap : 16) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
  }
  f.stamp_block = block;
  return 0;
}

int mlf_region_debug_stats(mlf_region *r, unsigned long long *out, int cap) {
  // counters of the LAST filtered batch of this region (after a synchronisation): [0] proposals in the binary32
  // ellipsoid band, [1] queries whitened in the reference arithmetic, [2] uncertain pairs listed, [3] largest list
  // segment, [4] list segments, [5] 32-query groups left for the second live-point range
  if (!r || !out || cap < 6) return fail_arg(MLF_E_BADARG, "bad argument");
  FilterCtx &f = r->filter;
  for (int i = 0; i < cap; ++i) out[i] = 0;
  CK(hipDeviceSynchronize());
  if (f.misc.p) {
    unsigned m[8];
    CK(hipMemcpy(m, f.misc.p, sizeof m, hipMemcpyDeviceToHost));
    out[0] = m[4];
  }
  if (f.segcnt.p && f.segcnt.cap >= sizeof(unsigned)) {
    const size_t n = (size_t)f.last.nsegs;
    std::vector<unsigned> c(n);
    if (n) CK(hipMemcpy(c.data(), f.segcnt.p, n * sizeof(unsigned), hipMemcpyDeviceToHost));
    unsigned long long sum = 0, mx = 0;
    for (unsigned v : c) {
      sum += v;
      mx = v > mx ? v : mx;
    }
    out[2] = sum;
    out[3] = mx;
    out[4] = n;
  }
  if (f.png.p) {
    unsigned g[6];
    CK(hipMemcpy(g, f.png.p, sizeof g, hipMemcpyDeviceToHost));
    out[5] = g[0];
    if (cap > 6) out[6] = g[1];   // queries of the last min-only batch whose minimum ended in the band (uncertain set; above 128 dimensions: left to the exact scan)
    if (f.last.wide) {   // above 128 dimensions: every query the pre-filter left to the exact scan (guard cases + band)
      unsigned w[8];
      CK(hipMemcpy(w, f.png.p, sizeof w, hipMemcpyDeviceToHost));
      out[1] = w[6];
    }
    if (cap > 7) out[7] = g[5];   // three ranges: groups that entered the third
  }
  if (cap > 17) {
    out[16] = (unsigned long long)f.last_min.cut[0];
    out[17] = (unsigned long long)f.last_min.cut[1];
  }
  // the fused first launch took the ellipsoid form from the whitening chain
  if (cap > 18) out[18] = (f.last_min.defer && (f.last_min.fused_variant & 2u)) ? 1ull : 0ull;
  {
    if (cap >= 16 && f.last.mid && f.last.time_launches && f.segcnt.p) {   // k_inside_mid, workgroup (0, 0): stage boundaries
      unsigned st[8];
      CK(hipMemcpy(st, f.segcnt.p, sizeof st, hipMemcpyDeviceToHost));
      for (int i = 0; i < 8; ++i) out[8 + i] = st[i];
    } else if (cap >= 16 && f.last.nsegs == uncertain_blocks() && f.segcnt.cap >= (size_t)(f.last.nsegs + 8) * sizeof(unsigned)) {
      unsigned st[8];   // shader-clock stamps of k_uncertain's workgroup 0 (stage boundaries of its first set)
      CK(hipMemcpy(st, f.segcnt.as<unsigned>() + uncertain_stamp_base(), sizeof st, hipMemcpyDeviceToHost));
      for (int i = 0; i < 8; ++i) out[8 + i] = st[i];
    }
  }
  return 0;
}

int mlf_bench_fp64_valu(double *tflops) {
  if (!tflops) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  CK(c.out.reserve(1 << 20));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int blocks = 256 * 8, iters = 2000;
  double ops = launch_fp64_probe(c.out.as<double>(), blocks, iters, c.stream);  // warm-up
  CK(hipEventRecord(e0, c.stream));
  ops = launch_fp64_probe(c.out.as<double>(), blocks, iters, c.stream);
  CK(hipEventRecord(e1, c.stream));
  CK(hipEventSynchronize(e1));
  float ms = 0.f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  *tflops = ops / (ms * 1e-3) / 1e12;
  return 0;
}

int mlf_region_time_inside_dev(mlf_region *r, const double *d_pts, size_t np, uint8_t *d_mask,
                               void *stream, int reps, float *ms_total, float *ms_scan) {
  if (!r) return fail_arg(MLF_E_BADARG, "null region");
  if (!r->ready) return fail_arg(MLF_E_STATE, "region used before mlf_region_set");
  if (!d_pts || !d_mask || !ms_total || !ms_scan || reps <= 0 || np == 0)
    return fail_arg(MLF_E_BADARG, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  hipEvent_t ev[4];
  for (auto &e : ev) CK(hipEventCreate(&e));
  double tot = 0.0, scan = 0.0;
  for (int i = 0; i < reps; ++i) {
    if (int rc = region_inside_enqueue(r, d_pts, np, d_mask, s, ev)) return rc;
    CK(hipEventSynchronize(ev[3]));
    float a = 0.f, b = 0.f;
    CK(hipEventElapsedTime(&a, ev[0], ev[3]));
    CK(hipEventElapsedTime(&b, ev[1], ev[3]));
    tot += a;
    scan += b;
  }
  for (auto &e : ev) CK(hipEventDestroy(e));
  *ms_total = (float)(tot / reps);
  *ms_scan = (float)(scan / reps);
  return 0;
}

}  // extern "C"
