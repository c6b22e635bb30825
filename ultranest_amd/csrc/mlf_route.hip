// mlf_route.hip -- one batch of rows through the membership / neighbour test: plan_batch decides the route once, the
// filter_* stages launch along it (matrix-core pre-filter, re-check, exact-scan tail).  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mlfriends_hip.h"
#include "mlf_host.hpp"
#include "mlf_prep3.hpp"
#include "mlf_prep64.hpp"

namespace mlf {

// Quantise the live points for the filter.  host_sync = true also fetches the statistics that the
// host-side eligibility test uses (done when the live set is installed, not per batch).
int filter_prepare_refs(FilterCtx &f, const double *refR, int n, int d, int dp, hipStream_t s,
                        bool host_sync, bool mask_mode) {
  f.refs_ready = false;
  f.wide = false;
  const int ks = prep4_ks(dp);   // filter dimensionality = padded DP (zero columns are harmless)
  // above 9 k-steps (128 dimensions): the run-time-dimension operands of mlf_wide_filter.hip, which serve mask mode only
  const bool wide = ks > 9;
  if ((wide && (!mask_mode || ks > kWideFilterMaxKs)) || n < 1 ||
      (long long)round_up(n, 32) / 32 * ks * 1024 >= (1ll << 31)) {   // k_sweep addresses the tiles with 32-bit buffer offsets
    f.usable = false;
    return 0;
  }
  f.ks = ks;
  const int npad32 = round_up(n, 32);
  f.ntiles32 = npad32 / 32;
  if (wide) {   // storage order only: no centre-first copy up here
    CK(f.stats.reserve((8 + kWideStatCols) * sizeof(double)));
    CK(f.refF.reserve((size_t)npad32 * ks * 16 * 2));
    {
      const void *before = f.wstatscratch.p;
      CK(f.wstatscratch.reserve(wide_stat_scratch_bytes()));
      if (f.wstatscratch.p != before) CK(hipMemsetAsync(f.wstatscratch.p, 0, wide_stat_scratch_bytes(), s));   // running maxima start at zero
    }
    launch_wide_ref_stats(refR, n, dp, f.stats.as<double>(), f.wstatscratch.as<double>(), s);
    launch_wide_quant_refs(refR, n, npad32, dp, ks, f.stats.as<double>(), f.refF.p, s);
    CK(hipGetLastError());
    f.ordered = false;
    if (host_sync) {
      f.order_n = -1;
      double h[4];
      CK(hipMemcpyAsync(h, f.stats.p, sizeof h, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      f.sigma = h[0];
      f.amax = h[2];
      f.usable = h[3] == 1.0 && h[2] > 0.0 && h[2] < 1e150;
    }
    f.wide = true;
    f.refs_ready = true;
    f.refs_dirty = false;
    return 0;
  }
  CK(f.stats.reserve((8 + MLF_FILTER_MAXD) * sizeof(double)));
  CK(f.refF.reserve((size_t)npad32 * ks * 16 * 2));
  (void)d;
  {
    const void *before = f.statscratch.p;
    const size_t bytes = ((size_t)64 * 128 + 2) * sizeof(double);
    CK(f.statscratch.reserve(bytes));
    if (f.statscratch.p != before) CK(hipMemsetAsync(f.statscratch.p, 0, bytes, s));   // running maxima start at zero
  }
  // the mask-mode operand: the live points nearest to the centre first.  A NEW live set (host_sync) is ranked -- the keys
  // come out of the statistics pass --; a refresh behind row replacements keeps the permutation (the replaced rows stay in
  // their slots: the order is a heuristic of the sweep, not part of any answer) and only requantises
  const bool want_order = opt(f, OPT_ORDER) && n <= 65536;
  const bool rerank = want_order && (host_sync || f.order_n != n);
  if (want_order) {
    CK(f.okeys.reserve((size_t)n * sizeof(unsigned long long)));
    CK(f.operm.reserve((size_t)n * sizeof(int)));
  }
  launch_ref_stats(refR, n, dp, dp, f.stats.as<double>(), f.statscratch.as<double>(), s, rerank ? f.okeys.as<unsigned long long>() : nullptr);
  f.ordered = false;
  if (want_order) {
    const int nrows = round_up(n, 64) + 1;   // the re-check requests whole 16-coordinate blocks: a spare row behind the last
    CK(f.refFm.reserve((size_t)npad32 * ks * 16 * 2));
    CK(f.refRm.reserve((size_t)nrows * dp * sizeof(double)));
    if (rerank) launch_ref_rank(f.okeys.as<unsigned long long>(), n, f.operm.as<int>(), s);
    launch_quant_refs(refR, n, npad32, dp, dp, ks, f.stats.as<double>(), f.refF.p, s, f.refFm.p, f.operm.as<int>(), f.refRm.as<double>(), nrows);
    CK(hipGetLastError());
    f.ordered = true;
    f.order_n = n;
  } else {
    launch_quant_refs(refR, n, npad32, dp, dp, ks, f.stats.as<double>(), f.refF.p, s);
    CK(hipGetLastError());
    if (host_sync) f.order_n = -1;
  }
  if (host_sync) {
    double h[4];
    CK(hipMemcpyAsync(h, f.stats.p, sizeof h, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    f.sigma = h[0];
    f.amax = h[2];
    f.usable = h[3] == 1.0 && h[2] > 0.0 && h[2] < 1e150;
  }
  f.refs_ready = true;
  f.refs_dirty = false;
  return 0;
}

// requantise the live points if one was replaced since the operands were built (mlf_region_update_point)
int filter_refresh_refs(FilterCtx &f, const double *refR, int n, int d, int dp, hipStream_t s) {
  if (!f.refs_ready || !f.refs_dirty) return 0;
  if (int rc = filter_prepare_refs(f, refR, n, d, dp, s, false)) return rc;
  f.refs_dirty = false;
  return 0;
}

// self-resetting counters of the bounded stage: zeroed once, when allocated
int misc_reserve(FilterCtx &f) {
  if (f.misc.p) return 0;
  CK(f.misc.reserve(8 * sizeof(unsigned)));
  CK(hipMemset(f.misc.p, 0, 8 * sizeof(unsigned)));
  return 0;
}

// The routing of one batch of nq rows.  `r` is null for BATCH_HOST (the stateless call: live set of host_nlive rows);
// first_index: the first neighbour's index per row instead of the membership mask; pregate: the gate array arrives with
// a pre-gate (device-side sampling: the cube test); pts: the rows on the device (the bounded stage reads 16-byte pieces).
BatchPlan plan_batch(const FilterCtx &f, const mlf_region *r, BatchKind kind, long long nq, double r2, bool first_index, bool pregate,
                     const void *pts, size_t host_nlive) {
  BatchPlan p{};
  p.time_launches = opt(f, OPT_TIME_LAUNCHES) != 0;
  const bool scan = kind == BATCH_HOST || kind == BATCH_TSPACE || (kind == BATCH_INSIDE && r->use_scan);
  // host-side eligibility of the filter (the kernels re-check per query and fall back on their own)
  bool eligible = opt(f, OPT_FILTER) && f.refs_ready && f.usable && nq >= opt(f, OPT_MIN_QUERIES);
  // below ~2000 proposals the five launches of the filter path (~45 us) only pay when the exact scan has real work:
  // 400 proposals against 400 x 5 live coordinates take 43 us through the exact scan, 51 us through the filter
  if (opt(f, OPT_MIN_QUERIES) == kFilterMinQueriesDefault && nq < 2048 && (long long)f.ntiles32 * 32 * f.ks * 16 < 40000) eligible = false;
  const double sr2 = f.sigma * f.sigma * r2;
  eligible = eligible && r2 > 0.0 && r2 < 1e150 && sr2 < 4096.0 && sr2 > 1e-30;
  // 129 ... 1024 dimensions: the operands serve the mask-mode sweep of mlf_wide_filter.hip; first-index batches keep the exact scan
  if (f.wide) eligible = eligible && !first_index && kind != BATCH_HOST;
  if (kind == BATCH_HOST) {
    // The stateless call pays the filter's live-point preparation every time and first-index mode keeps sweeping after
    // a hit, so the pre-filter only pays for larger batches than in the resident mask path (measured at N = 4000,
    // d = 50: exact scan 0.23-0.35 ms against 0.45-1.05 ms at 4000 queries; break-even between 16000 and 50000)
    const long long host_min = opt(f, OPT_MIN_QUERIES) != kFilterMinQueriesDefault ? opt(f, OPT_MIN_QUERIES) : 32768;
    p.host_refs = first_index && opt(f, OPT_FILTER) && nq >= host_min && host_nlive >= 256;
    p.filter = p.host_refs && eligible;
  } else {
    p.filter = scan && eligible;
  }
  if (kind == BATCH_INSIDE || kind == BATCH_GATE) {
    // fused stage (coalesced staging, coordinate-major output, optional quantisation) for affine layers
    const bool fused = r->layer_kind == 0 && opt(f, OPT_FUSED_PREP) && prep3_usable(r->d) && r->chol_ready;
    const bool bounded = fused && opt(f, OPT_PREP_BOUNDED) && r->p4_ready && !r->has_wrap && (p.filter || !scan) &&
                         nq < 0x7fffffffll && (reinterpret_cast<uintptr_t>(pts) & 15) == 0;   // 16-byte pieces
    if (bounded)
      p.stage = STAGE_PREP4;
    else if (kind == BATCH_GATE)
      p.stage = STAGE_PREP;   // the binary64 ellipsoid test alone
    else if (fused)
      p.stage = STAGE_PREP3;
    else if (r->layer_kind == 0 && prep64_usable(r->d) && r->chol_ready && r->chol_ok && opt(f, OPT_FUSED_PREP))
      p.stage = STAGE_PREP64;
    // 129 ... 1024 dimensions: the run-time-dimension form of that stage comes with the pre-filter ("filter" = 0 stays the
    // exact route throughout: k_prep_wide + k_scan_wide)
    else if (r->layer_kind == 0 && prep64_wide_usable(r->d) && p.filter && f.wide && kind == BATCH_INSIDE && r->chol_ready && r->chol_ok &&
             opt(f, OPT_FUSED_PREP))
      p.stage = STAGE_PREP64;
    else
      p.stage = STAGE_PREP;
  }
  if (!p.filter) return p;
  if (f.wide) {   // quantise, one min-only sweep, exact tail over the list of the proposals left: nothing else to choose
    p.wide = true;
    return p;
  }
  // mask mode sweeps the centre-first copy of the live points (any hit decides); the first-index mode keeps storage order
  p.ordered = !first_index && f.ordered && opt(f, OPT_ORDER);
  const bool bounded = p.stage == STAGE_PREP4;
  // The batch sizes of a real run (ndraw 128 ... 65536): per-proposal stage, sweep, re-check and answers in ONE launch
  // (mlf_mid.hip); the exact-scan launch behind it only works if a proposal was routed to it.
  p.mid = bounded && !pregate && !first_index && f.ks <= 4 && mid_usable(r->dp) && nq <= opt(f, OPT_MID_MAX);
  if (p.mid) return p;
  // Phased sweep: the live-point tiles are split into nphase ranges; after each range the queries that are decided
  // (certain hit) leave, the rest is compacted into fresh 32-query groups.  Worth it when the sweep is long compared with
  // one compaction (~25 us + 40 us per 10^6 queries).
  const int want_phases = (int)opt(f, OPT_PHASES);
  const long long phase_min = opt(f, OPT_PHASE_MIN_QUERIES);
  if (want_phases && nq >= phase_min && (phase_min < 32768 || nq * f.ntiles32 >= 30000000ll))
    p.nphase = want_phases >= 2 ? (want_phases <= f.ntiles32 / 4 ? want_phases : (f.ntiles32 >= 16 ? 2 : 1))
                                : (f.ntiles32 >= 16 ? 2 : 1);
  p.narrow = (p.nphase > 1 && f.ks <= 4) ? (int)opt(f, OPT_NARROW_TAIL) : 0;
  const long long ngroups = (nq + 31) / 32;
  p.split = p.nphase == 1 ? filter_tile_split(f.ks, ngroups, f.ntiles32, (int)opt(f, OPT_SPLIT_WAVES)) : 1;
  // mask mode behind the bounded per-proposal stage, single-sweep batches (below ~262144 proposals at N = 4000): the
  // re-check (binary64 whitening of the queries of the uncertain pairs + the reference's distance loop) runs inside the
  // sweep launch, each wave on the segment it has just written, and the ellipsoid band rides in the same launch: three
  // launches per batch instead of four (131072 proposals: 104 -> 96 us).  Phased sweeps keep the separate re-check launch:
  // there the waves' re-check tails cost more than the launch they save (10^6: 0.473 -> 0.51 ms)
  p.own_recheck = bounded && !first_index && p.nphase == 1;
  // two ranges, compaction inside the first, finalise tail in the scan launch: nobody pads the compacted set or publishes
  // its group count (k_phase_finish: a 5 us launch) -- the second range reads the slot counter itself, the tail resets it
  p.fold_finish = bounded && p.nphase == 2;
  // Two ranges in mask mode behind the bounded per-proposal stage: the min-only sweep (mlf_sweepmin.hip).  The two long
  // launches carry the running minimum only; the queries whose minimum ends in the band are swept once more by
  // k_uncertain (band pairs found, queries whitened, pairs decided in one launch), which also carries the ellipsoid band.
  p.min_path = p.fold_finish && !first_index && f.ks <= 4 && opt(f, OPT_SWEEP_MIN);
  // Tile ranges, every range at least 4 tiles.  Two ranges: [0, c1) [c1, ntiles32) with c1 = first_pct of the tiles.  Three
  // (min-only sweep) -- batches of at least min_work (proposals x tiles), where the pairs a third range saves outweigh its
  // launch and its compaction: the last range starts at c2 = second_pct of the tiles and [0, c2) is split at first_pct of
  // c2 (30 % of 50 % = 15 %, 50 %: profiles/r05_three_range_ab.jsonl).
  if (p.nphase == 2) {
    const int nt = f.ntiles32, first_pct = (int)opt(f, OPT_FIRST_RANGE_PCT), second_pct = (int)opt(f, OPT_SECOND_RANGE_PCT);
    const int cut = (int)((long long)nt * first_pct / 100);
    p.cut[0] = cut < 4 ? 4 : (cut > nt - 4 ? nt - 4 : cut);
    if (p.min_path && second_pct > 0 && nq * nt >= opt(f, OPT_THIRD_MIN_WORK)) {
      const int cut2 = (int)((long long)nt * second_pct / 100);
      int a = (int)((long long)cut2 * first_pct / 100);
      a = a < 4 ? 4 : a;
      if (cut2 >= a + 4 && cut2 <= nt - 4) {
        p.cut[0] = a;
        p.cut[1] = cut2;
      }
    }
  }
  // large batches on the min-only path: the per-proposal stage runs inside the first sweep launch (mlf_fused.hip)
  p.defer = p.min_path && opt(f, OPT_FUSED_FIRST) && fused_usable(r->dp);
  if (p.defer) {
    p.fused_waves = (int)opt(f, OPT_FUSED_WAVES);
    p.fused_variant = (unsigned)(opt(f, OPT_FUSED_VARIANT) & 0xff);
    if (!(r->same_matrix && r->same_centres)) p.fused_variant &= ~2u;   // the region does not have the same quadratic form
    if (pregate) p.fused_variant |= 4u;   // the pre-gate is read out of the gate array
  }
  const long long waves = filter_wave_count(f.ks, ngroups);
  if (p.min_path)
    p.nsegs = uncertain_blocks();
  else if (p.split > 1)   // one segment per (wave, range), whole workgroups
    p.nsegs = (waves + 3) / 4 * 4 * p.split;
  else   // a narrow later range has more waves than the first
    p.nsegs = std::max(waves, filter_wave_count(f.ks, ngroups, p.narrow));
  p.seg_room = std::max(p.nsegs, (waves + 3) / 4 * 4 * p.split);   // the padding waves of a grid write (empty) segments too
  return p;
}

// Device buffers of one filtered batch.
int filter_reserve(FilterCtx &f, const BatchPlan &p, long long nq) {
  const long long nqpad = (nq + 31) / 32 * 32;
  CK(f.qF.reserve((size_t)nqpad * f.ks * 16 * 2));
  CK(f.tlo.reserve((size_t)nqpad * sizeof(float)));
  CK(f.thi.reserve((size_t)nqpad * sizeof(float)));
  CK(f.route.reserve((size_t)nq));
  CK(f.best.reserve((size_t)nq * sizeof(int)));
  CK(f.counters.reserve(4 * sizeof(unsigned)));
  CK(f.list.reserve((size_t)p.seg_room * kFilterSegCap * sizeof(unsigned long long)));
  CK(f.segcnt.reserve((size_t)p.seg_room * sizeof(unsigned)));
  CK(f.gate2.reserve((size_t)nq));
  return misc_reserve(f);
}

// exact scan of nq rows (element (j, k) at q[j*ldq + k*ldk]) against the live set
ScanArgs scan_args(const LiveSet &L, const double *q, long long ldq, long long ldk, long long nq, int mode) {
  ScanArgs a{};
  a.refT = L.refT;
  a.n = L.n;
  a.npad = L.npad;
  a.ntiles = L.npad / kWave;
  a.q = q;
  a.ldq = ldq;
  a.ldk = ldk;
  a.nq = nq;
  a.d = L.d;
  a.r2 = L.r2;
  a.mode = mode;
  return a;
}

// The finalise work of a batch behind the bounded stage rides in its exact-scan launch: the gate is the routing itself
// (route 2: proposals the pre-filter cannot take), the launch is idle unless the batch's flag is up, and the (rare)
// workgroups that do scan whiten their own queries
void scan_finalise(ScanArgs &a, const FilterCtx &f, const ExactSrc &xs) {
  a.only_gated = 1;   // leave the outputs of ungated queries alone
  a.raw_ctr = xs.lay_ctr;
  a.raw_T8 = xs.T8;
  a.raw_ldt = xs.ldt;
  a.route = f.route.as<uint8_t>();
  a.counters = f.counters.as<unsigned>();
  a.any_flag = f.misc.as<unsigned>() + 2 + f.batch_parity;
  a.fin_reset = f.misc.as<unsigned>() + 2 + (f.batch_parity ^ 1u);
}

namespace {

// a matrix-kernel launch of a timed call, bracketed by an event pair (mlf_region_timing_filter_launches)
template <class Launch>
int timed_launch(const FilterBatch &b, Launch &&launch) {
  FilterCtx &f = b.f;
  const bool timed = b.ev_after || b.p.time_launches;
  if (timed) {
    while (f.kev.size() < f.kev_used + 2) {
      hipEvent_t e;
      CK(hipEventCreate(&e));
      f.kev.push_back(e);
    }
    CK(hipEventRecord(f.kev[f.kev_used], b.s));
  }
  CK(launch());
  if (timed) {
    CK(hipEventRecord(f.kev[f.kev_used + 1], b.s));
    f.kev_used += 2;
  }
  return 0;
}

// The min-only sweep in two or three ranges, then k_uncertain on the queries whose minimum ended in the band.
// filter_second_range_pct > 0: three ranges (the middle one reads set 0 and writes set 1 with a second array of minima;
// the uncertain set then reuses set 0's arrays, which nobody reads any more)
int filter_sweep_min(const FilterBatch &b) {
  FilterCtx &f = b.f;
  const BatchPlan &p = b.p;
  const ExactSrc &xs = *b.xs;
  const long long nqpad = b.ngroups() * 32;
  const bool min3 = p.cut[1] > 0;
  CK(f.segcnt.reserve((size_t)(p.nsegs + 8) * sizeof(unsigned)));
  CK(f.pmin.reserve((size_t)nqpad * sizeof(int)));
  if (min3) CK(f.pmin2.reserve((size_t)nqpad * sizeof(int)));
  MinArgs m{};
  m.refF = b.opF();
  m.ntiles32 = f.ntiles32;
  m.nq = b.nq;
  m.best = f.best.as<int>();
  m.ngroups = b.ngroups();
  m.ccap = (unsigned)nqpad;
  // first range: slot = query; the queries without a certain hit go to set 0 with their minimum
  m.tile0 = 0;
  m.tile1 = p.cut[0];
  m.qF = f.qF.p;
  m.tlo = f.tlo.as<float>();
  m.thi = f.thi.as<float>();
  m.cq = f.pqF[0].p;
  m.ctlo = f.ptlo[0].as<float>();
  m.cthi = f.pthi[0].as<float>();
  m.cmap = f.pmap[0].as<int>();
  m.cmin = f.pmin.as<int>();
  m.ccount = f.png.as<unsigned>() + 2;
  m.last = 0;
  if (p.defer) {   // per-proposal stage + first range in one launch: the operand never leaves the registers
    FusedArgs fu{};
    fu.p = xs.prep;
    fu.refF = b.opF();
    fu.ntiles32 = f.ntiles32;
    fu.tile0 = 0;
    fu.tile1 = p.cut[0];
    fu.cq = m.cq;
    fu.ctlo = m.ctlo;
    fu.cthi = m.cthi;
    fu.cmap = m.cmap;
    fu.cmin = m.cmin;
    fu.ccount = m.ccount;
    fu.ccap = m.ccap;
    if (f.stamp_block >= 0 && f.stamp_block < 1000000) {   // diagnostics (mlf_region_debug_fused_stamps)
      CK(f.fstamps.reserve(16 * sizeof(unsigned long long)));
      CK(hipMemsetAsync(f.fstamps.p, 0, 16 * sizeof(unsigned long long), b.s));   // (a stage the wave never reaches reads as 0)
      fu.stamps = f.fstamps.as<unsigned long long>();
      fu.stamp_block = (unsigned)f.stamp_block;
    }
    fu.variant = p.fused_variant;
    if (fu.variant & 2u) fu.p.c = xs.same;
    if (int rc = timed_launch(b, [&] { return launch_prep_sweep(fu, b.s, p.fused_waves); })) return rc;
  } else if (int rc = timed_launch(b, [&] { return launch_sweep_min(f.ks, filter_groups_per_wave(f.ks, 0), m, b.s); })) {
    return rc;
  }
  // next range: set 0 with its minima.  Two ranges: this is the last, the uncertain queries go to set 1.  Three: the
  // queries still without a certain hit go to set 1 with their minima, and the last range sweeps those into set 0's arrays
  const int usrc = min3 ? 0 : 1;   // the set that holds the uncertain queries in the end
  m.tile0 = p.cut[0];
  m.tile1 = min3 ? p.cut[1] : f.ntiles32;
  m.qF = f.pqF[0].p;
  m.tlo = f.ptlo[0].as<float>();
  m.thi = f.pthi[0].as<float>();
  m.qmap = f.pmap[0].as<int>();
  m.qmin = f.pmin.as<int>();
  m.nslots_dev = f.png.as<unsigned>() + 2;
  m.cq = f.pqF[1].p;
  m.ctlo = f.ptlo[1].as<float>();
  m.cthi = f.pthi[1].as<float>();
  m.cmap = f.pmap[1].as<int>();
  m.cmin = min3 ? f.pmin2.as<int>() : nullptr;
  m.ccount = f.png.as<unsigned>() + 3;
  m.last = min3 ? 0 : 1;
  // diagnostics: stage stamps of one k_sweep_min workgroup -- block 1 000 000 + b: the launch that follows the first range,
  // 2 000 000 + b: the one after it
  auto sweep_stamps = [&](int which) -> int {
    m.stamps = nullptr;
    if (f.stamp_block >= which * 1000000 && f.stamp_block < (which + 1) * 1000000) {
      CK(f.fstamps.reserve(16 * sizeof(unsigned long long)));
      CK(hipMemsetAsync(f.fstamps.p, 0, 16 * sizeof(unsigned long long), b.s));
      m.stamps = f.fstamps.as<unsigned long long>();
      m.stamp_block = (unsigned)(f.stamp_block - which * 1000000);
    }
    return 0;
  };
  if (int rc = sweep_stamps(1)) return rc;
  if (min3) {
    if (int rc = timed_launch(b, [&] { return launch_sweep_min(f.ks, filter_groups_per_wave(f.ks, 0), m, b.s); })) return rc;
    if (int rc = sweep_stamps(2)) return rc;
    m.tile0 = p.cut[1];
    m.tile1 = f.ntiles32;
    m.qF = f.pqF[1].p;
    m.tlo = f.ptlo[1].as<float>();
    m.thi = f.pthi[1].as<float>();
    m.qmap = f.pmap[1].as<int>();
    m.qmin = f.pmin2.as<int>();
    m.nslots_dev = f.png.as<unsigned>() + 3;
    m.cq = f.pqF[0].p;
    m.ctlo = f.ptlo[0].as<float>();
    m.cthi = f.pthi[0].as<float>();
    m.cmap = f.pmap[0].as<int>();
    m.cmin = nullptr;
    m.ccount = f.png.as<unsigned>() + 4;
    m.last = 1;
  }
  // four query groups per wave here too: with the min-only loop the narrow form (two groups, twice the waves) that paid for
  // k_sweep's second range loses (0.080 against 0.085-0.088 ms; profiles/r04_first_range_ab.jsonl)
  if (int rc = timed_launch(b, [&] { return launch_sweep_min(f.ks, filter_groups_per_wave(f.ks, 0), m, b.s); })) return rc;
  // the uncertain set: band pairs, exact whitening, exact distances -- one launch; the ellipsoid band rides along
  UncertainArgs ua{};
  ua.refF = b.opF();
  ua.ntiles32 = f.ntiles32;
  ua.qF = f.pqF[usrc].p;
  ua.thi = f.pthi[usrc].as<float>();
  ua.qmap = f.pmap[usrc].as<int>();
  ua.nslots_dev = f.png.as<unsigned>() + (min3 ? 4 : 3);
  ua.pts = xs.pts;
  ua.d = b.L.d;
  ua.dp = b.L.dp;
  ua.lay_ctr = xs.lay_ctr;
  ua.T8 = xs.T8;
  ua.ldt8 = xs.ldt;
  ua.refR = b.opR();
  ua.n = b.L.n;
  ua.r2 = b.L.r2;
  ua.best = f.best.as<int>();
  ua.counters = f.counters.as<unsigned>();
  ua.seg_count = f.segcnt.as<unsigned>();
  ua.ell = xs.ell;   // the band proposals of k_prep4: trailing workgroups of this launch
  if (int rc = timed_launch(b, [&] { return launch_uncertain(f.ks, ua, b.s); })) return rc;
  if (b.ev_after) CK(hipEventRecord(b.ev_after, b.s));
  return 0;
}

// Re-check of the uncertain pairs behind the bounded stage: the queries of the pairs are whitened from the proposals, and
// the ellipsoid band of the stage rides in the same launch
RecheckWArgs recheck_w_args(const FilterBatch &b) {
  RecheckWArgs rw{};
  rw.list = b.f.list.as<unsigned long long>();
  rw.seg_cap = kFilterSegCap;
  rw.seg_count = b.f.segcnt.as<unsigned>();
  rw.refR = b.opR();
  rw.n = b.L.n;
  rw.d = b.L.d;
  rw.dp = b.L.dp;
  rw.pts = b.xs->pts;
  rw.nq = b.nq;
  rw.lay_ctr = b.xs->lay_ctr;
  rw.T64 = b.xs->T64;
  rw.r2 = b.L.r2;
  rw.best = b.f.best.as<int>();
  rw.ell = b.xs->ell;
  return rw;
}

// k_sweep (mask mode) / k_filter (first index) over the plan's ranges; every launch is sized for the worst case and reads
// the actual group count from device memory: no host sync
int filter_phases(const FilterBatch &b) {
  FilterCtx &f = b.f;
  const BatchPlan &p = b.p;
  const long long ngroups = b.ngroups();
  FilterArgs fa{};
  fa.refF = b.opF();
  fa.qF = f.qF.p;
  fa.tlo = f.tlo.as<float>();
  fa.thi = f.thi.as<float>();
  fa.ntiles32 = f.ntiles32;
  fa.ngroups = ngroups;
  fa.nq = b.nq;
  fa.best = f.best.as<int>();
  fa.list = f.list.as<unsigned long long>();
  fa.seg_cap = kFilterSegCap;
  fa.seg_count = f.segcnt.as<unsigned>();
  fa.counters = f.counters.as<unsigned>();
  fa.split = p.split;
  if (p.own_recheck) fa.rw = recheck_w_args(b);   // the sweeping waves re-check their own segments
  const bool fused = p.nphase > 1;   // the compaction of the undecided queries rides in the matrix kernel's epilogue
  for (int ph = 0; ph < p.nphase; ++ph) {
    fa.tile0 = (int)((long long)f.ntiles32 * ph / p.nphase);
    fa.tile1 = (int)((long long)f.ntiles32 * (ph + 1) / p.nphase);
    if (p.nphase == 2) {   // two ranges: the first takes filter_first_range_pct per cent of the tiles
      fa.tile0 = ph == 0 ? 0 : p.cut[0];
      fa.tile1 = ph == 0 ? p.cut[0] : f.ntiles32;
    }
    fa.append = ph > 0;
    fa.seg_first_extra = filter_wave_count(f.ks, ngroups);   // segments beyond the first launch's own: for a narrow later range
    fa.seg_extra = p.narrow ? filter_wave_count(f.ks, ngroups, p.narrow) - fa.seg_first_extra : 0;
    if (fa.seg_extra < 0) fa.seg_extra = 0;
    fa.cq = nullptr;
    if (fused && ph > 0) {   // the previous launch compacted its undecided queries into set (ph - 1) & 1
      const int src = (ph - 1) & 1;
      fa.qF = f.pqF[src].p;
      fa.tlo = f.ptlo[src].as<float>();
      fa.thi = f.pthi[src].as<float>();
      fa.qmap = f.pmap[src].as<int>();
      fa.ngroups_dev = f.png.as<unsigned>() + src;
      if (p.fold_finish) {
        fa.ngroups_dev = nullptr;
        fa.nslots_dev = f.png.as<unsigned>() + 2;
      }
    }
    if (fused && ph + 1 < p.nphase) {   // ... and this one compacts into set ph & 1
      const int dst = ph & 1;
      fa.cq = f.pqF[dst].p;
      fa.ctlo = f.ptlo[dst].as<float>();
      fa.cthi = f.pthi[dst].as<float>();
      fa.cmap = f.pmap[dst].as<int>();
      fa.ccount = f.png.as<unsigned>() + 2;
      fa.ccap = (unsigned)(ngroups * 32);
      fa.route = f.route.as<uint8_t>();
    }
    const int narrow = ph > 0 ? p.narrow : 0;
    if (int rc = timed_launch(b, [&] { return launch_filter(f.ks, fa, b.out_idx != nullptr, b.s, narrow); })) return rc;
    if (fa.cq && !p.fold_finish) {
      const int dst = ph & 1;
      launch_phase_finish(fa.cq, fa.ctlo, fa.cthi, fa.cmap, fa.ccount, f.png.as<unsigned>() + dst, f.ks, b.s);
      CK(hipGetLastError());
    }
  }
  if (b.ev_after) CK(hipEventRecord(b.ev_after, b.s));
  return 0;
}

// the separate re-check launch of the uncertain pairs
int filter_recheck(const FilterBatch &b) {
  FilterCtx &f = b.f;
  const BatchPlan &p = b.p;
  if (b.xs) {   // no whitened coordinates were stored: the re-check whitens the queries of its pairs itself
    RecheckWArgs rw = recheck_w_args(b);   // (the band proposals of k_prep4: the last waves of this launch, before the finalise)
    rw.nsegs = p.nsegs;
    rw.unit_cap = (unsigned)(p.nphase * (f.ks <= 4 ? 4 : (f.ks <= 8 ? 2 : 1)) * 32);   // queries per filter wave, all phases (a narrow later range has fewer)
    launch_recheck_whiten(rw, b.s);
  } else {
    RecheckArgs ra{};
    ra.list = f.list.as<unsigned long long>();
    ra.seg_cap = kFilterSegCap;
    ra.seg_count = f.segcnt.as<unsigned>();
    ra.refR = b.opR();
    ra.n = b.L.n;
    ra.d = b.L.d;
    ra.dp = b.L.dp;
    ra.q = b.q;
    ra.ldq = b.ldq;
    ra.ldk = b.ldk;
    ra.nq = b.nq;
    ra.r2 = b.L.r2;
    ra.best = f.best.as<int>();
    launch_recheck(ra, p.nsegs, b.s);
  }
  CK(hipGetLastError());
  return 0;
}

// answers of the filtered queries + the exact scan of the queries the filter did not decide: (a) queries that do not fit
// binary16 and (b) every filtered query if the uncertain-pair list overflowed
int filter_scan_tail(const FilterBatch &b) {
  FilterCtx &f = b.f;
  const BatchPlan &p = b.p;
  const int mode = b.out_idx ? SCAN_FIRST : SCAN_MASK;
  if (!b.xs)
    launch_filter_finalize(f.route.as<uint8_t>(), f.best.as<int>(), f.counters.as<unsigned>(), b.nq, b.out_mask,
                           b.out_idx, f.gate2.as<uint8_t>(), b.s);
  ScanArgs a = b.xs ? scan_args(b.L, b.xs->pts, b.L.d, 1, b.nq, mode) : scan_args(b.L, b.q, b.ldq, b.ldk, b.nq, mode);
  a.gate = f.gate2.as<uint8_t>();
  a.out_idx = b.out_idx;
  a.out_mask = b.out_mask;
  a.only_gated = 1;   // leave the outputs of ungated queries alone
  if (b.xs) {
    scan_finalise(a, f, *b.xs);
    a.fin_best = f.best.as<int>();
    if (p.fold_finish) {
      a.fin_slots = f.png.as<unsigned>() + 2;
      a.fin_groups = f.png.as<unsigned>();   // where k_phase_finish would have left the group count (debug_stats)
      if (p.min_path) a.fin_slots2 = f.png.as<unsigned>() + (p.cut[1] > 0 ? 4 : 3);
      if (p.cut[1] > 0) a.fin_slots3 = f.png.as<unsigned>() + 3;
    }
  }
  CK(launch_scan(b.L.dp, a, b.s));
  CK(hipGetLastError());
  return 0;
}

// 129 ... 1024 dimensions, mask mode (mlf_wide_filter.hip): the whitened rows are quantised and routed, one min-only sweep
// answers every query whose minimum is outside its band, and the exact scan takes what is left (route 2)
int filter_run_wide(const FilterBatch &b) {
  FilterCtx &f = b.f;
  if (b.out_idx || !b.out_mask || b.xs || b.ldk > 1) return fail_arg(MLF_E_STATE, "wide pre-filter: mask mode on row-major whitened rows only");
  const long long nqpad = b.ngroups() * 32;
  f.last = b.p;
  CK(f.qF.reserve((size_t)nqpad * f.ks * 16 * 2));
  CK(f.tlo.reserve((size_t)nqpad * sizeof(float)));
  CK(f.thi.reserve((size_t)nqpad * sizeof(float)));
  CK(f.route.reserve((size_t)b.nq));
  CK(f.best.reserve((size_t)b.nq * sizeof(int)));   // the list of the route-2 queries
  // png[1]: queries whose minimum ended in the band, png[6]: length of the route-2 list (mlf_region_debug_stats reads both).
  // The list counter is cleared in front of every batch: a batch that failed between its quantiser and its tail leaves nothing
  // behind that the next tail could take for query numbers
  if (!f.png.p) {
    CK(f.png.reserve(8 * sizeof(unsigned)));
    CK(hipMemset(f.png.p, 0, 8 * sizeof(unsigned)));
  }
  WideQuantArgs qa{};
  qa.q = b.q;
  qa.ldq = b.ldq;
  qa.nq = b.nq;
  qa.nqpad = nqpad;
  qa.d_src = b.L.d;
  qa.d = b.L.dp;
  qa.ks = f.ks;
  qa.stats = f.stats.as<double>();
  qa.r2 = b.L.r2;
  qa.gate = b.gate;
  qa.qF = f.qF.p;
  qa.tlo = f.tlo.as<float>();
  qa.thi = f.thi.as<float>();
  qa.route = f.route.as<uint8_t>();
  qa.out_mask = b.out_mask;
  unsigned *qcount = f.png.as<unsigned>() + 6;
  CK(hipMemsetAsync(qcount, 0, sizeof(unsigned), b.s));
  qa.band_count = f.png.as<unsigned>() + 1;
  qa.qlist = f.best.as<int>();
  qa.qcount = qcount;
  if (int rc = timed_launch(b, [&] { return launch_wide_quant_queries(qa, b.s); })) return rc;
  WideSweepArgs sa{};
  sa.refF = f.refF.p;
  sa.ntiles32 = f.ntiles32;
  sa.ks = f.ks;
  sa.qF = f.qF.p;
  sa.tlo = f.tlo.as<float>();
  sa.thi = f.thi.as<float>();
  sa.ngroups = b.ngroups();
  sa.nq = b.nq;
  sa.route = f.route.as<uint8_t>();
  sa.out_mask = b.out_mask;
  sa.band_count = f.png.as<unsigned>() + 1;
  sa.qlist = f.best.as<int>();
  sa.qcount = qcount;
  if (int rc = timed_launch(b, [&] { return launch_wide_sweep(sa, b.s); })) return rc;
  if (b.ev_after) CK(hipEventRecord(b.ev_after, b.s));
  ScanArgs a = scan_args(b.L, b.q, b.ldq, b.ldk, b.nq, SCAN_MASK);
  a.out_mask = b.out_mask;
  CK(launch_scan_wide_list(b.L.dp, a, f.best.as<int>(), qcount, b.s));
  return 0;
}

}  // namespace

// Filter pipeline on device data along the plan's route
int filter_run(const FilterBatch &b) {
  FilterCtx &f = b.f;
  const BatchPlan &p = b.p;
  if (p.wide) return filter_run_wide(b);
  const long long nqpad = b.ngroups() * 32;
  f.last = p;
  if (p.min_path) f.last_min = p;
  if (int rc = filter_reserve(f, p, b.nq)) return rc;
  if (p.stage != STAGE_PREP4 && p.stage != STAGE_PREP3)   // the fused per-proposal stage has not quantised this batch
    launch_quant_queries(b.q, b.ldq, b.nq, nqpad, b.L.d, b.L.dp, f.ks, f.stats.as<double>(), b.L.r2, b.gate, f.qF.p,
                         f.tlo.as<float>(), f.thi.as<float>(), f.route.as<uint8_t>(), f.best.as<int>(),
                         f.counters.as<unsigned>(), b.s);
  CK(hipGetLastError());
  if (p.nphase > 1) {   // two compacted query sets (ping-pong)
    for (int i = 0; i < 2; ++i) {
      CK(f.pqF[i].reserve((size_t)nqpad * f.ks * 16 * 2));
      CK(f.ptlo[i].reserve((size_t)nqpad * sizeof(float)));
      CK(f.pthi[i].reserve((size_t)nqpad * sizeof(float)));
      CK(f.pmap[i].reserve((size_t)nqpad * sizeof(int)));
    }
    if (!f.png.p) {   // group counts + the slot counter of the fused compaction (returns to zero by itself: k_phase_finish)
      // words: [0] groups after the first range, [1] size of the uncertain set (statistics of the last batch), [2] [3] [4] slot
      // counters of the compacted sets, [5] groups after the second of three ranges
      CK(f.png.reserve(8 * sizeof(unsigned)));
      CK(hipMemset(f.png.p, 0, 8 * sizeof(unsigned)));
    } else if (f.png_dirty) {   // an earlier phased batch failed between its first compaction and its scan launch
      CK(hipMemsetAsync(f.png.p, 0, 8 * sizeof(unsigned), b.s));
    }
    f.png_dirty = true;   // until the scan launch of this batch is queued
  }
  if (int rc = p.min_path ? filter_sweep_min(b) : filter_phases(b)) return rc;
  // the min-only sweep and the single sweep behind the bounded stage have re-checked every pair in their own launches
  if (!p.min_path && !p.own_recheck)
    if (int rc = filter_recheck(b)) return rc;
  if (int rc = filter_scan_tail(b)) return rc;
  // only a PHASED batch's scan tail (or its k_phase_finish) returns the slot counters to zero: a single-sweep batch that
  // follows a failed phased one must leave the flag standing for the next phased batch
  if (p.nphase > 1) f.png_dirty = false;
  return 0;
}

}  // namespace mlf
