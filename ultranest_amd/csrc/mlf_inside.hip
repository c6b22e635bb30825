// mlf_inside.hip -- the region's membership test: per-proposal stage and neighbour test of a batch on the device
// (region_inside_enqueue), the one-launch routes for small and medium batches, and their entry points.  Host code only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>

#include "../../include/mlfriends_hip.h"
#include "mlf_host.hpp"
#include "mlf_prep3.hpp"
#include "mlf_prep64.hpp"
#include "mlf_sample.hpp"

namespace {

using namespace mlf;

ExactSrc region_exact_src(const mlf_region *r, const double *pts) {
  ExactSrc x{};
  x.pts = pts;
  x.lay_ctr = r->lay_ctr.as<double>();
  x.T8 = r->lay_T8.as<double>();
  x.ldt = (r->dp + 7) / 8 * 8;
  x.T64 = r->lay_T64.as<double>();
  return x;
}

// Arguments of the bounded per-proposal stage (k_prep4) of np rows: the ellipsoid test into `gate`, its band proposals listed
// for the exact test (region_ell_args); whiten: also the approximate whitening into this batch's filter operand (filter_reserve
// first, and the batch's parity turned)
int region_prep4_args(mlf_region *r, const double *pts, long long np, uint8_t *gate, bool whiten, Prep4Args *out) {
  FilterCtx &f = r->filter;
  if (int rc = misc_reserve(f)) return rc;
  CK(f.ell_list.reserve((size_t)np * sizeof(int)));
  Prep4Args &pa = *out;
  pa = Prep4Args{};
  pa.pts = pts;
  pa.np = np;
  pa.d = r->d;
  pa.dp = r->dp;
  pa.LtF = r->p4_LtF.p;
  pa.y0 = r->p4_y0.as<float>();
  pa.TtF = r->p4_TtF.p;
  pa.lay_ctr = r->use_scan ? r->lay_ctr.as<double>() : r->ell_ctr.as<double>();   // the centre the chain's start values belong to
  pa.c = r->p4c;
  pa.c.enl_lo = f32_dn(r->enlarge);
  pa.c.enl_hi = f32_up(r->enlarge);
  pa.gate = gate;
  pa.do_tr = whiten ? 1 : 0;
  pa.ell_count = f.misc.as<unsigned>();
  pa.ell_list = f.ell_list.as<int>();
  pa.ell_cap = (unsigned)np;
  if (whiten) {
    pa.stats = f.stats.as<double>();
    pa.r2 = r->r2;
    pa.qF = f.qF.p;
    pa.tlo = f.tlo.as<float>();
    pa.thi = f.thi.as<float>();
    pa.route = f.route.as<uint8_t>();
    pa.best = f.best.as<int>();
    pa.counters = f.counters.as<unsigned>();
    pa.scan_flag = f.misc.as<unsigned>() + 2 + f.batch_parity;
    pa.ks = f.ks;
    pa.nqpad = (np + 31) / 32 * 32;
  }
  return 0;
}

// the exact test of the ellipsoid band that k_prep4 listed (k_ell_exact, or trailing waves of a later launch of the batch)
EllExactArgs region_ell_args(mlf_region *r, const double *pts, long long np, uint8_t *gate, uint8_t *route) {
  FilterCtx &f = r->filter;
  EllExactArgs ea{};
  ea.count = f.misc.as<unsigned>();
  ea.done = f.misc.as<unsigned>() + 1;
  ea.last = f.misc.as<unsigned>() + 4;
  ea.list = f.ell_list.as<int>();
  ea.cap = (unsigned)np;
  ea.pts = pts;
  ea.d = r->d;
  ea.dp = r->dp;
  ea.ell_ctr = r->ell_ctr.as<double>();
  ea.ell_Lt = r->ell_Lt.as<double>();
  ea.ell_L = r->ell_L.as<double>();
  ea.ell_A = r->ell_A.as<double>();
  ea.eps_scale = r->ell_eps_scale;
  ea.enlarge = r->enlarge;
  ea.chol_ok = r->chol_ok ? 1 : 0;
  ea.gate = gate;
  ea.route = route;
  return ea;
}

// plan.mid: the whole batch in one launch (k_inside_mid) and the exact scan behind it, idle unless a proposal was routed to it
int region_inside_mid(mlf_region *r, const BatchPlan &p, const double *d_pts, long long np, uint8_t *d_mask, hipStream_t s,
                      hipEvent_t *ev) {
  FilterCtx &f = r->filter;
  f.last = p;
  if (int rc = misc_reserve(f)) return rc;
  CK(f.route.reserve((size_t)np));
  CK(f.counters.reserve(4 * sizeof(unsigned)));
  const long long ngroups = (np + 31) / 32, nsets = (ngroups + 3) / 4;
  const int ny = mid_range_quads(ngroups, f.ntiles32), R = 4 * ny;
  CK(f.mid_rec.reserve((size_t)nsets * R * 3 * sizeof(unsigned long long)));
  CK(f.mid_meta.reserve((size_t)nsets * 4 * sizeof(unsigned long long)));
  {
    const size_t before = f.mid_arrive.cap;
    CK(f.mid_arrive.reserve((size_t)nsets * sizeof(unsigned)));
    // they return to zero by themselves afterwards -- unless a launch failed part-way: then the next batch starts clean
    if (f.mid_arrive.cap != before || f.mid_dirty) CK(hipMemsetAsync(f.mid_arrive.p, 0, f.mid_arrive.cap, s));
    if (f.mid_dirty && f.misc.p) CK(hipMemsetAsync(f.misc.p, 0, 8 * sizeof(unsigned), s));
    f.mid_dirty = false;
  }
  MidArgs ma{};
  ma.pts = d_pts;
  ma.np = np;
  ma.d = r->d;
  ma.dp = r->dp;
  ma.ks = f.ks;
  ma.LtF = r->p4_LtF.p;
  ma.y0 = r->p4_y0.as<float>();
  ma.TtF = r->p4_TtF.p;
  ma.lay_ctr = r->lay_ctr.as<double>();
  ma.c = r->p4c;
  ma.c.enl_lo = f32_dn(r->enlarge);
  ma.c.enl_hi = f32_up(r->enlarge);
  ma.stats = f.stats.as<double>();
  ma.r2 = r->r2;
  ma.ell = region_ell_args(r, d_pts, np, nullptr, nullptr);
  ma.ell.count = ma.ell.done = ma.ell.last = nullptr;   // the band proposals are decided on the spot: no list
  ma.ell.list = nullptr;
  ma.refF = p.ordered ? f.refFm.p : f.refF.p;
  ma.ntiles32 = f.ntiles32;
  ma.refR = p.ordered ? f.refRm.as<double>() : r->refR.as<double>();
  ma.n = r->n;
  ma.T64 = r->lay_T64.as<double>();
  ma.rec = f.mid_rec.as<unsigned long long>();
  ma.meta = f.mid_meta.as<unsigned long long>();
  ma.arrive = f.mid_arrive.as<unsigned>();
  ma.mask = d_mask;
  ma.route = f.route.as<uint8_t>();
  f.batch_parity ^= 1u;
  ma.scan_flag = f.misc.as<unsigned>() + 2 + f.batch_parity;
  ma.counters = f.counters.as<unsigned>();
  if (p.time_launches) {   // diagnostics: stage stamps of workgroup (0, 0) (mlf_region_debug_stats)
    CK(f.segcnt.reserve(16 * sizeof(unsigned)));
    ma.stamps = f.segcnt.as<unsigned>();
  }
  if (hipError_t le = launch_inside_mid(ma, ny, s); le != hipSuccess) {
    f.mid_dirty = true;
    CK(le);
  }
  if (ev) {
    CK(hipEventRecord(ev[1], s));
    CK(hipEventRecord(ev[2], s));
  }
  ScanArgs a = scan_args(region_live(r), d_pts, r->d, 1, np, SCAN_MASK);   // proposals the pre-filter cannot take (route 2)
  a.out_mask = d_mask;
  scan_finalise(a, f, region_exact_src(r, d_pts));
  if (hipError_t le = launch_scan(r->dp, a, s); le != hipSuccess) {
    f.mid_dirty = true;
    CK(le);
  }
  if (ev) CK(hipEventRecord(ev[3], s));
  return 0;
}

}  // namespace

namespace mlf {

int region_inside_enqueue(mlf_region *r, const double *d_pts, size_t np, uint8_t *d_mask,
                          hipStream_t s, hipEvent_t *ev /* 4 events or null */,
                          long long *d_idx, const uint8_t *pregate) {
  if (np == 0) return 0;
  if (d_idx && !r->use_scan) return fail_arg(MLF_E_STATE, "region has no live points set");
  if (r->use_scan)
    if (int rc = filter_refresh_refs(r->filter, r->refR.as<double>(), r->n, r->d, r->dp, s)) return rc;
  CK(r->gate.reserve(np));
  uint8_t *gate = r->use_scan ? r->gate.as<uint8_t>() : d_mask;
  FilterCtx &f = r->filter;
  const BatchPlan p = plan_batch(f, r, BATCH_INSIDE, (long long)np, r->r2, d_idx != nullptr, pregate != nullptr, d_pts);
  long long ldq = r->d, ldk = 1;
  if (r->use_scan && p.stage != STAGE_PREP4) CK(r->tq.reserve(np * (size_t)r->d * sizeof(double)));
  if (ev) CK(hipEventRecord(ev[0], s));
  if (p.mid) return region_inside_mid(r, p, d_pts, (long long)np, d_mask, s, ev);
  if (p.filter)
    if (int rc = filter_reserve(f, p, (long long)np)) return rc;
  ExactSrc xs = region_exact_src(r, d_pts);
  if (p.stage == STAGE_PREP4) {   // matrix cores (split binary16): bounded ellipsoid test + approximate whitening straight into the filter operand
    if (r->use_scan) f.batch_parity ^= 1u;
    Prep4Args pa;
    if (int rc = region_prep4_args(r, d_pts, (long long)np, gate, r->use_scan != 0, &pa)) return rc;
    if (p.defer) {   // the stage runs inside the first sweep launch
      xs.prep = pa;
      xs.same = r->p4c_same;
      xs.same.enl_lo = pa.c.enl_lo;
      xs.same.enl_hi = pa.c.enl_hi;
      if (pregate) {   // the fused first launch reads the pre-gate out of the gate array and writes its own verdict over it
        CK(hipMemcpyAsync(gate, pregate, np, hipMemcpyDeviceToDevice, s));
        pregate = nullptr;   // honoured there: no k_apply_pregate, and the ellipsoid band rides in the re-check launch as usual
      }
    } else {
      CK(launch_prep4(pa, s));
    }
    const EllExactArgs ea = region_ell_args(r, d_pts, (long long)np, gate, r->use_scan ? f.route.as<uint8_t>() : nullptr);
    if (r->use_scan && !pregate) {   // decided by the tail of the re-check launch (k_recheck_whiten, k_sweep, k_uncertain)
      xs.ell = ea;
    } else {
      launch_ell_exact(ea, s);
      CK(hipGetLastError());
    }
  } else if (p.stage == STAGE_PREP3) {   // FP64 matrix-core version of the fused stage (v_mfma_f64_16x16x4_f64: the reference's FMA chain bit for bit)
    Prep3Args pa{};
    pa.pts = d_pts;
    pa.np = (long long)np;
    pa.d = r->d;
    pa.dp = r->dp;
    pa.nk = (r->d + 3) / 4;
    pa.ell_ctr = r->ell_ctr.as<double>();
    pa.ell_A = r->ell_A.as<double>();
    pa.lda = r->dp;
    pa.LtF = r->ell_LtF.as<double>();
    pa.ell_eps_scale = r->ell_eps_scale;
    pa.chol_ok = r->chol_ok ? 1 : 0;
    pa.enlarge = r->enlarge;
    pa.gate = gate;
    if (r->use_scan) {
      pa.do_tr = 1;
      pa.lay_ctr = r->lay_ctr.as<double>();
      pa.TtF = r->lay_TtF.as<double>();
      pa.wrap_shift = r->has_wrap ? r->wrap.as<double>() : nullptr;
      pa.t_out = r->tq.as<double>();
      pa.t_ldq = 1;
      pa.t_ldk = (long long)np;
      ldq = 1;
      ldk = (long long)np;
      if (p.filter) {   // the exact re-check gathers single proposals: rows of d contiguous doubles
        pa.t_ldq = ldq = (long long)r->d;
        pa.t_ldk = ldk = 1;
        pa.qF = f.qF.p;
        pa.tlo = f.tlo.as<float>();
        pa.thi = f.thi.as<float>();
        pa.route = f.route.as<uint8_t>();
        pa.best = f.best.as<int>();
        pa.counters = f.counters.as<unsigned>();
        pa.stats = f.stats.as<double>();
        pa.r2 = r->r2;
        pa.ks = f.ks;
        pa.nqpad = ((long long)np + 31) / 32 * 32;
      }
    }
    CK(launch_prep3(pa, s));
  } else if (p.stage == STAGE_PREP64) {
    // 65 ... 128 dimensions: the bounded quadratic form and the whitening chain on the FP64 matrix cores, the matrices streamed
    // from L2 (mlf_prep64.hip; rounds 1-4: the vector kernel below, 4-6 ms per 10^6 x 100)
    Prep64Args pa{};
    pa.pts = d_pts;
    pa.np = (long long)np;
    pa.d = r->d;
    pa.dp = r->dp;
    pa.ell_ctr = r->ell_ctr.as<double>();
    pa.ell_L = r->ell_L.as<double>();
    pa.ell_A = r->ell_A.as<double>();
    pa.lda = r->dp;
    pa.ell_eps_scale = r->ell_eps_scale;
    pa.chol_ok = 1;
    pa.enlarge = r->enlarge;
    pa.gate = gate;
    if (r->use_scan) {
      pa.do_tr = 1;
      pa.lay_ctr = r->lay_ctr.as<double>();
      pa.T8 = r->lay_T8.as<double>();
      pa.ldt8 = (r->dp + 7) / 8 * 8;
      pa.wrap_shift = r->has_wrap ? r->wrap.as<double>() : nullptr;
      pa.t_out = r->tq.as<double>();
      pa.ldt = r->d;
    }
    if (prep64_wide_usable(r->d)) {   // above 128 dimensions: the run-time-dimension form with its own band (2^-28 |A|_F, mlf_prep64.hip)
      pa.ell_eps_scale = 64.0 * r->ell_eps_scale;
      CK(launch_prep64_wide(pa, s));
    } else {
      CK(launch_prep64(pa, s));
    }
  } else {
    PrepArgs pa{};
    pa.pts = d_pts;
    pa.np = (long long)np;
    pa.d = r->d;
    pa.do_ell = 1;
    pa.ell_ctr = r->ell_ctr.as<double>();
    pa.ell_A = r->ell_A.as<double>();
    pa.enlarge = r->enlarge;
    pa.mask = gate;
    pa.q_out = nullptr;
    if (r->use_scan) {
      pa.t_out = r->tq.as<double>();
      pa.ldt = r->d;
      if (r->layer_kind == 0) {
        pa.do_tr = 1;
        pa.lay_ctr = r->lay_ctr.as<double>();
        pa.lay_Tt = r->lay_mat.as<double>();
        pa.wrap_shift = r->has_wrap ? r->wrap.as<double>() : nullptr;
      }
    }
    CK(launch_prep(r->dp, pa, s));
    if (r->use_scan && r->layer_kind == 1) {
      launch_scaling_transform(d_pts, (long long)np, r->d, r->lay_ctr.as<double>(), r->lay_mat.as<double>(),
                               r->has_wrap ? r->wrap.as<double>() : nullptr, gate, r->tq.as<double>(),
                               r->d, s);
      CK(hipGetLastError());
    }
  }
  if (pregate) {   // proposals rejected before the region test (outside the unit cube): never scanned
    const bool ff = p.filter && (p.stage == STAGE_PREP4 || p.stage == STAGE_PREP3);   // the stage has routed the batch
    launch_apply_pregate(pregate, (long long)np, gate, ff ? f.route.as<uint8_t>() : nullptr, ff ? f.tlo.as<float>() : nullptr,
                         ff ? f.thi.as<float>() : nullptr, s);
    CK(hipGetLastError());
  }
  if (ev) CK(hipEventRecord(ev[1], s));
  if (p.filter) {
    if (int rc = filter_run({f, p, region_live(r), r->tq.as<double>(), ldq, ldk, (long long)np, gate, d_idx ? nullptr : d_mask,
                             d_idx, s, ev ? ev[2] : nullptr, p.stage == STAGE_PREP4 ? &xs : nullptr}))
      return rc;
  } else if (r->use_scan) {
    ScanArgs a = scan_args(region_live(r), r->tq.as<double>(), ldq, ldk, (long long)np, d_idx ? SCAN_FIRST : SCAN_MASK);
    a.gate = gate;
    a.out_mask = d_mask;
    a.out_idx = d_idx;
    CK(launch_scan(r->dp, a, s));
    if (ev) CK(hipEventRecord(ev[2], s));
    if (d_idx) {
      launch_mark_gated(gate, (long long)np, d_idx, s);
      CK(hipGetLastError());
    }
  }
  if (ev) {
    if (!r->use_scan) CK(hipEventRecord(ev[2], s));
    CK(hipEventRecord(ev[3], s));
  }
  return 0;
}

// wrapping-ellipsoid test alone (H3, mlfriends.pyx:882-912) of `np` cube-space rows: the bounded matrix-core form with the exact
// test behind its band where the region has it (what a region without a neighbour scan runs), else the binary64 kernel
int region_ellipsoid_gate(mlf_region *r, const double *d_pts, size_t np, uint8_t *gate, hipStream_t s) {
  if (np == 0) return 0;
  if (plan_batch(r->filter, r, BATCH_GATE, (long long)np, r->r2, false, false, d_pts).stage != STAGE_PREP4) {
    PrepArgs pa{};
    pa.pts = d_pts;
    pa.np = (long long)np;
    pa.d = r->d;
    pa.do_ell = 1;
    pa.ell_ctr = r->ell_ctr.as<double>();
    pa.ell_A = r->ell_A.as<double>();
    pa.enlarge = r->enlarge;
    pa.mask = gate;
    CK(launch_prep(r->dp, pa, s));
    return 0;
  }
  Prep4Args pa;
  if (int rc = region_prep4_args(r, d_pts, (long long)np, gate, false, &pa)) return rc;
  CK(launch_prep4(pa, s));
  launch_ell_exact(region_ell_args(r, d_pts, (long long)np, gate, nullptr), s);
  CK(hipGetLastError());
  return 0;
}

// Pinned, device-mapped staging of the single-launch membership call (proposals in, mask and completion word out) and
// of the row replacements: created on first use.
int small_staging(Ctx &c) {
  if (c.pin_pts) return 0;
  CK(hipHostMalloc(reinterpret_cast<void **>(&c.pin_pts), kSmallStagingBytes, hipHostMallocMapped));
  CK(hipHostMalloc(reinterpret_cast<void **>(&c.pin_mask), (size_t)kSmallMaxPoints + 64, hipHostMallocMapped));
  memset(c.pin_mask, 0, (size_t)kSmallMaxPoints + 64);
  CK(hipHostGetDevicePointer(reinterpret_cast<void **>(&c.pin_pts_dev), c.pin_pts, 0));
  CK(hipHostGetDevicePointer(reinterpret_cast<void **>(&c.pin_mask_dev), c.pin_mask, 0));
  CK(c.small_words.reserve(2 * kSmallMaxPoints * sizeof(unsigned)));
  CK(hipMemsetAsync(c.small_words.p, 0, 2 * kSmallMaxPoints * sizeof(unsigned), c.stream));
  return 0;
}

}  // namespace mlf

namespace {

using namespace mlf;

// One launch, no copies on the stream: the proposals go through a pinned staging buffer the kernel reads directly,
// the mask comes back the same way.
int region_inside_small(mlf_region *r, const double *pts, size_t np, uint8_t *mask) {
  Ctx &c = g_ctx;
  if (int rc = small_staging(c)) return rc;
  memcpy(c.pin_pts, pts, np * (size_t)r->d * sizeof(double));
  SmallArgs a{};
  a.pts = c.pin_pts_dev;
  a.np = (int)np;
  a.d = r->d;
  a.dp = r->dp;
  a.ell_ctr = r->ell_ctr.as<double>();
  a.ell_A = r->ell_A.as<double>();
  a.ell_Lt = r->ell_Lt.as<double>();
  a.eps_scale = r->ell_eps_scale;
  a.enlarge = r->enlarge;
  a.chol_ok = (r->chol_ready && r->chol_ok) ? 1 : 0;
  a.use_scan = r->use_scan;
  a.layer_kind = r->layer_kind;
  a.wpp = 1;
  if (r->use_scan) {
    a.lay_ctr = r->lay_ctr.as<double>();
    if (r->layer_kind == 0) {
      a.lay_T8 = r->lay_T8.as<double>();
      a.ldt8 = (r->dp + 7) / 8 * 8;
    } else {
      a.lay_std = r->lay_mat.as<double>();
    }
    a.wrap = r->has_wrap ? r->wrap.as<double>() : nullptr;
    a.refT = r->refT.as<double>();
    a.n = r->n;
    a.npad = r->npad;
    a.r2 = r->r2;
    // enough workgroups per proposal to spread its live points over the chip, but no more than ~512 in all
    const int shares = (r->n + 255) / 256;
    int wpp = 512 / (int)np;
    if (wpp > shares) wpp = shares;
    a.wpp = wpp < 1 ? 1 : wpp;
  }
  a.state = c.small_words.as<unsigned>();
  a.finished = c.small_words.as<unsigned>() + kSmallMaxPoints;
  a.mask = c.pin_mask_dev;
  a.flag = reinterpret_cast<unsigned *>(c.pin_mask_dev + kSmallMaxPoints);
  a.seq = ++c.small_seq;
  if (a.seq == 0u) a.seq = ++c.small_seq;   // 0 is the initial content of the word
  launch_inside_small(a, c.stream);
  CK(hipGetLastError());
  {   // spin on the completion word; a kernel that does not report within ~40 ms is left to the stream and its error path
    volatile unsigned *flag = reinterpret_cast<volatile unsigned *>(c.pin_mask + kSmallMaxPoints);
    bool seen = false;
    for (long spin = 0; spin < 4000000; ++spin) {
      if (*flag == a.seq) {
        seen = true;
        break;
      }
      __builtin_ia32_pause();
    }
    if (!seen) {
      CK(hipStreamSynchronize(c.stream));
      if (*flag != a.seq) return fail_arg(MLF_E_STATE, "single-launch membership kernel did not complete");
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  memcpy(mask, c.pin_mask, np);
  return 0;
}

}  // namespace

extern "C" {

int mlf_region_inside(mlf_region *r, const double *pts, size_t np, uint8_t *mask) {
  if (!r) return fail_arg(MLF_E_BADARG, "null region");
  if (!r->ready) return fail_arg(MLF_E_STATE, "region used before mlf_region_set");
  if (np == 0) return 0;
  if (!pts || !mask) return fail_arg(MLF_E_BADARG, "null pointer");
  if (opt(r->filter, OPT_SMALL_PATH) && np <= (size_t)kSmallMaxPoints && r->d <= kSmallMaxDim) return region_inside_small(r, pts, np, mask);
  Ctx &c = g_ctx;
  const size_t row_bytes = (size_t)r->d * sizeof(double);
  CK(r->mask.reserve(np));
  // Large host batches (what integrator.py:1776-1804 hands over: 400 MB at 10^6 x 50) are sent in chunks on a copy
  // stream; the kernels of chunk k run while chunk k + 1 crosses PCIe, so that only the last chunk's kernels and the
  // mask's way back are not hidden behind the transfer (round 2: upload, then 0.55 ms of kernels, then the mask).
  constexpr size_t kChunkRows = 131072;
  if (np >= 3 * kChunkRows && !is_device_pointer(pts)) {
    if (!c.copy_stream) {
      CK(hipStreamCreateWithFlags(&c.copy_stream, hipStreamNonBlocking));
      CK(hipEventCreateWithFlags(&c.copy_event, hipEventDisableTiming));
    }
    CK(r->pts.reserve(np * row_bytes));
    CK(hipStreamSynchronize(c.stream));   // the staging buffer may still be read by an earlier call's kernels
    for (size_t row0 = 0; row0 < np; row0 += kChunkRows) {
      const size_t rows = np - row0 < kChunkRows ? np - row0 : kChunkRows;
      double *dst = r->pts.as<double>() + row0 * (size_t)r->d;
      CK(hipMemcpyAsync(dst, pts + row0 * (size_t)r->d, rows * row_bytes, hipMemcpyHostToDevice, c.copy_stream));
      CK(hipEventRecord(c.copy_event, c.copy_stream));
      CK(hipStreamWaitEvent(c.stream, c.copy_event, 0));
      if (int rc = region_inside_enqueue(r, dst, rows, r->mask.as<uint8_t>() + row0, c.stream, nullptr)) return rc;
    }
  } else {
    if (int rc = upload(r->pts, pts, np * row_bytes, c.stream)) return rc;
    if (int rc = region_inside_enqueue(r, r->pts.as<double>(), np, r->mask.as<uint8_t>(), c.stream, nullptr))
      return rc;
  }
  CK(hipMemcpyAsync(mask, r->mask.p, np, hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  return 0;
}

int mlf_region_inside_dev(mlf_region *r, const double *d_pts, size_t np, uint8_t *d_mask,
                          void *stream) {
  if (!r) return fail_arg(MLF_E_BADARG, "null region");
  if (!r->ready) return fail_arg(MLF_E_STATE, "region used before mlf_region_set");
  if (np && (!d_pts || !d_mask)) return fail_arg(MLF_E_BADARG, "null pointer");
  return region_inside_enqueue(r, d_pts, np, d_mask, (hipStream_t)stream, nullptr);
}

int mlf_region_find_nearby_dev(mlf_region *r, const double *d_tpts, size_t np, int64_t *d_idx,
                               void *stream) {
  if (!r) return fail_arg(MLF_E_BADARG, "null region");
  if (!r->ready || !r->use_scan) return fail_arg(MLF_E_STATE, "region has no live points set");
  if (np == 0) return 0;
  if (!d_tpts || !d_idx) return fail_arg(MLF_E_BADARG, "null pointer");
  ScanArgs a = scan_args(region_live(r), d_tpts, r->d, 0, (long long)np, SCAN_FIRST);
  a.out_idx = reinterpret_cast<long long *>(d_idx);
  CK(launch_scan(r->dp, a, (hipStream_t)stream));
  return 0;
}

int mlf_region_first_index_dev(mlf_region *r, const double *d_pts, size_t np, int64_t *d_idx,
                               void *stream) {
  if (!r) return fail_arg(MLF_E_BADARG, "null region");
  if (!r->ready) return fail_arg(MLF_E_STATE, "region used before mlf_region_set");
  if (np && (!d_pts || !d_idx)) return fail_arg(MLF_E_BADARG, "null pointer");
  return region_inside_enqueue(r, d_pts, np, nullptr, (hipStream_t)stream, nullptr,
                               reinterpret_cast<long long *>(d_idx));
}

}  // extern "C"
