// mlf_host.hpp -- what the host units of the membership / region C ABI (mlf_api.hip, mlf_route.hip, mlf_region.hip,
// mlf_inside.hip, mlf_region_sample.hip, mlf_stateless.hip, mlf_debug.hip) share: the tuning options, the routing plan of
// one batch, the filter and library contexts, the region handle, and the functions that cross a unit boundary.
#pragma once
#include <cmath>
#include <vector>

#include "mlf_ctx.hpp"
#include "mlf_filter.hpp"
#include "mlf_misc.hpp"
#include "mlf_small.hpp"
#include "mlf_wide_filter.hpp"

namespace mlf {

// Buffers and host-side state of the MFMA pre-filter (mlf_filter.hip) for one set of live points.
constexpr unsigned kFilterSegCap = 2048;
constexpr long long kFilterMinQueriesDefault = 257;   // = everything the single-launch path does not take (with the tile
// ranges of filter_tile_split a 1024-query batch takes 33 us through the filter, 175 us through the exact scan)

// ---- tuning options -----------------------------------------------------------------------------------------------
// Every option has a PROCESS default (mlf_set_option) and may be overridden per region handle
// (mlf_region_set_option): two regions of one process can run different routings, and nothing a test or a benchmark
// flips on one handle reaches another.  Results never depend on them.
enum Opt : int {
  OPT_FILTER,              // "filter" 0/1: matrix-core pre-filter in front of the exact scan
  OPT_FIRST_RANGE_PCT,     // "filter_first_range_pct" 10 ... 90: share of the live-point tiles in the first of two ranges
  OPT_SPLIT_WAVES,         // "filter_split_waves": waves a single-sweep launch aims at when it splits the tiles (1 ... 16 ranges)
  OPT_NARROW_TAIL,         // "filter_narrow_tail" 0/1: later ranges of a phased sweep with 2 query groups per wave
  OPT_SMALL_PATH,          // "small_path" 0/1: one launch for up to 256 proposals handed over on the host
  OPT_FUSED_PREP,          // "fused_prep" 0/1: fused per-proposal stage (off: k_prep + separate quantisation)
  OPT_PHASE_MIN_QUERIES,   // "filter_phase_min_queries": smaller batches sweep all tiles in one launch
  OPT_PHASES,              // "filter_phases": 0 single sweep, 1 default phase count, n >= 2 exactly n phases
  OPT_TIME_LAUNCHES,       // "time_filter_launches" 0/1: event pairs around every matrix-kernel launch of every call
  OPT_PREP_BOUNDED,        // "prep_bounded" 0/1: bounded matrix-core per-proposal stage (mlf_prep4.hip) or the binary64 one
  OPT_MIN_QUERIES,         // "filter_min_queries": smaller batches go straight to the exact scan
  OPT_SWEEP_MIN,           // "sweep_min" 0/1: two-range batches through the min-only sweep (mlf_sweepmin.hip) or k_sweep
  OPT_MID_MAX,             // "mid_max_queries": batches up to this size take the one-launch path (mlf_mid.hip); 0 = never
  OPT_FUSED_FIRST,         // "fused_first_range" 0/1: per-proposal stage and first range of the min-only sweep in one launch (mlf_fused.hip)
  OPT_BOOT_SYM,            // "boot_symmetric" 0/1: whole-range bootstrap passes compute every pair distance once (k_boot_sym)
  OPT_ORDER,               // "filter_order" 0/1: mask-mode operand in storage order / nearest to the centre first (k_ref_rank)
  OPT_SECOND_RANGE_PCT,    // "filter_second_range_pct" 0 ... 90: min-only sweep in three ranges, the second ending at this share of the tiles (0: two ranges)
  OPT_THIRD_MIN_WORK,      // "filter_third_range_min_work": three ranges from this many (proposals x 32-row live-point tiles) on
  OPT_FUSED_WAVES,         // "fused_waves" 4 / 8: waves per workgroup of k_prep_sweep (4, default: two workgroups per CU up to d = 50; 8: one)
  OPT_FUSED_VARIANT,       // "fused_variant": bit 0 = k_prep_sweep loads its matrix fragments by LDS-DMA (default) or by a load / store loop;
                           // bit 1 = the ellipsoid form read off the whitening chain where the region allows it (default; region_prep4_setup)
  OPT_COUNT
};

extern long long g_opt[OPT_COUNT];   // the process defaults (mlf_api.hip)

struct OptOverrides {
  long long v[OPT_COUNT] = {};
  bool set[OPT_COUNT] = {};
};

// ---- routing of one batch of rows through the membership / neighbour test -----------------------------------------
enum BatchKind : int {
  BATCH_INSIDE,   // region_inside_enqueue: cube-space proposals, per-proposal stage + neighbour test
  BATCH_TSPACE,   // region_scan_mask: whitened rows, neighbour test only
  BATCH_GATE,     // region_ellipsoid_gate: the wrapping-ellipsoid test only
  BATCH_HOST,     // scan_host: rows against live points handed over with the call (the context's FilterCtx, no region)
};

// the stage that turns the proposals into what the neighbour test reads
enum Stage : int {
  STAGE_NONE,     // the rows arrive whitened
  STAGE_PREP4,    // bounded matrix-core stage (mlf_prep4.hip): ellipsoid test, approximate whitening into the filter operand
  STAGE_PREP3,    // binary64 matrix-core stage (mlf_prep3.hip), quantising for the filter where it applies
  STAGE_PREP64,   // 65 ... 128 dimensions (mlf_prep64.hip)
  STAGE_PREP,     // vector kernel (k_prep), a scaling layer's transform behind it
};

// Every choice the routing of one batch makes.  plan_batch decides them once; the launch sequences only read them.
struct BatchPlan {
  bool filter = false;          // matrix-core pre-filter in front of the exact scan (else the exact scan alone)
  bool host_refs = false;       // BATCH_HOST: quantise the live points for the filter, then plan the batch again
  Stage stage = STAGE_NONE;
  bool mid = false;             // stage, sweep, re-check and answers in one launch (k_inside_mid)
  bool wide = false;            // 129 ... 1024 dimensions: the run-time-dimension pre-filter (mlf_wide_filter.hip), mask mode only
  bool time_launches = false;   // "time_filter_launches": event pairs around the matrix launches, k_inside_mid's stamps
  bool ordered = false;         // sweep the centre-first copy of the live points (refFm / refRm)
  int nphase = 1;               // live-point ranges of the sweep
  int narrow = 0;               // later ranges with two query groups per wave
  int split = 1;                // tile ranges of a single sweep (filter_tile_split)
  bool own_recheck = false;     // the sweeping waves re-check their own segments: no re-check launch
  bool fold_finish = false;     // two ranges, finalise in the scan launch: no k_phase_finish
  bool min_path = false;        // min-only sweep (mlf_sweepmin.hip) + k_uncertain
  int cut[2] = {0, 0};          // tile cuts of two ranges: [0, cut[0]) [cut[0], ntiles32); three: cut[1] starts the last
  bool defer = false;           // the bounded stage runs inside the first sweep launch (k_prep_sweep)
  unsigned fused_variant = 0;   // k_prep_sweep: bit 0 LDS-DMA fragments, bit 1 same quadratic form, bit 2 pre-gated
  int fused_waves = 4;          // waves per workgroup of k_prep_sweep
  long long nsegs = 0;          // list segments the re-check walks
  long long seg_room = 0;       // list segments any launch of the batch writes
};

struct FilterCtx {
  bool refs_ready = false;   // live points quantised
  bool refs_dirty = false;   // a live point was replaced since: requantise before the next batch that uses the operands
  bool usable = false;       // statistics are finite and the dimensionality is covered
  int ks = 0, ntiles32 = 0;
  bool wide = false;         // the operands are those of mlf_wide_filter.hip (ks > 9): mask mode only, storage order only
  double sigma = 1.0, amax = 0.0;
  DevBuf stats, statscratch, refF, qF, tlo, thi, route, best, counters, list, segcnt, gate2;
  // mask-mode operand: the live points nearest to the centre first (launch_ref_order): binary16 fragments, the rows the exact
  // re-check reads (same order), keys and permutation (slot -> storage row).  The first-index operand refF keeps storage order.
  DevBuf refFm, refRm, okeys, operm;
  bool ordered = false;      // refFm / refRm are current
  int order_n = -1;          // the live-set size the permutation was ranked for
  // phased sweep: two compacted query sets (ping-pong)
  DevBuf pqF[2], ptlo[2], pthi[2], pmap[2], png, pmin, pmin2;
  DevBuf mid_rec, mid_meta, mid_arrive;   // one-launch path (mlf_mid.hip): records of the tile ranges, arrival counters
  bool mid_dirty = false;                 // a launch of that path failed: its self-resetting counters are zeroed before the next batch
  DevBuf wstatscratch;                    // statistics scratch of the wide operands (its own layout: 1024 columns)
  DevBuf fstamps;                         // diagnostics: stage stamps of one k_prep_sweep wave
  int stamp_block = -1;
  bool png_dirty = false;                 // a phased batch did not reach its scan launch (whose tail returns the slot counters to zero)
  // bounded per-proposal stage (mlf_prep4.hip): ellipsoid band list, per-call counters
  // misc: [0] band proposals, [1] k_ell_exact workgroups done -- both return to zero by themselves (no memset per batch),
  // zeroed once when the buffer is allocated; [2], [3] "a proposal is routed to the exact scan", used alternately by
  // successive batches (the scan launch of a batch clears the word of the next one); [4] band proposals of the last
  // batch (mlf_region_debug_stats)
  DevBuf ell_list, misc;
  unsigned batch_parity = 0;
  BatchPlan last;             // the route of the last filtered batch (debug_stats) ...
  BatchPlan last_min;         // ... and of the last one that took the min-only sweep
  // (start, stop) event pairs around every k_filter launch of the timed calls
  std::vector<hipEvent_t> kev;
  size_t kev_used = 0;
  OptOverrides ov;            // per-handle tuning (mlf_region_set_option); the stateless calls' context has none
  void release() {
    DevBuf *b[] = {&stats, &statscratch, &refF, &qF, &tlo, &thi, &route, &best, &counters, &list, &segcnt, &gate2, &refFm, &refRm, &okeys, &operm,
                   &pqF[0], &pqF[1], &ptlo[0], &ptlo[1], &pthi[0], &pthi[1], &pmap[0], &pmap[1], &png, &pmin, &pmin2, &mid_rec, &mid_meta, &mid_arrive,
                   &ell_list, &misc, &fstamps, &wstatscratch};
    for (DevBuf *x : b) x->release();
    refs_ready = usable = ordered = wide = false;
    order_n = -1;
  }
};

inline long long opt(const FilterCtx &f, int id) { return f.ov.set[id] ? f.ov.v[id] : g_opt[id]; }

struct Ctx {
  bool ready = false;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copy_stream = nullptr;   // host batches in chunks: copies here, kernels on `stream` (mlf_region_inside)
  hipEvent_t copy_event = nullptr;
  // scratch used by the stateless host-pointer entry points
  unsigned long long *pin_adj = nullptr;   // pinned host copy of the adjacency bits (mlf_cluster_labels)
  size_t pin_adj_cap = 0;
  DevBuf src, refT, refR, q, out, flags, sel, selmask, selbytes, M, small0, small1, small2, small3, mask, tq;
  FilterCtx filter;
  // single-launch path for a handful of proposals (mlf_small.hip): pinned, device-mapped staging + two scratch words
  // per proposal
  double *pin_pts = nullptr, *pin_pts_dev = nullptr;
  uint8_t *pin_mask = nullptr, *pin_mask_dev = nullptr;   // mask bytes, then (at kSmallMaxPoints) the completion word
  unsigned small_seq = 0;
  DevBuf small_words;
};

extern Ctx g_ctx;   // mlf_api.hip

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// Pinned staging for the many small constant uploads of one call (mlf_region_set sends ~14 matrices and fragment sets):
// while an arena is active, a small upload copies its source into the arena and leaves from there -- truly
// asynchronous, so the caller needs no stream synchronisation before its host vectors go out of scope (round 2: nine
// synchronisations and a dozen pageable copies, 0.2 of the call's 0.6 ms).  The arena is rewound by the caller once the
// stream has been synchronised.
struct HostArena {
  unsigned char *p = nullptr;       // pinned host memory ...
  unsigned char *p_dev = nullptr;   // ... as the device sees it
  size_t cap = 0, used = 0;
  ScatterArgs pending{};            // uploads staged but not yet sent (arena_flush)
  int npending = 0;
  void *take(size_t bytes) {
    const size_t at = (used + 63) / 64 * 64;
    if (!p || at + bytes > cap) return nullptr;
    used = at + bytes;
    return p + at;
  }
};
extern HostArena *g_arena;   // mlf_api.hip; mlf_region_set makes the handle's arena the active one for its own duration
constexpr size_t kArenaBytes = 1u << 20, kArenaMaxPiece = 128u << 10;

constexpr size_t kSmallStagingBytes = (size_t)kSmallMaxPoints * kSmallMaxDim * sizeof(double);

inline float f32_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = nextafterf(f, INFINITY);
  return f;
}

inline float f32_dn(double x) {
  float f = (float)x;
  if ((double)f > x) f = nextafterf(f, -INFINITY);
  return f;
}

}  // namespace mlf

// ============================================================================================
struct mlf_region {
  bool ready = false;
  int n = 0, d = 0, dp = 0, npad = 0;
  int layer_kind = 0, use_scan = 1, live_space = 0;
  bool has_wrap = false;
  double enlarge = 0.0, r2 = 0.0;
  double live_extent_hint = -1.0;   // mlf_region_hint_live_extent, consumed by the next mlf_region_set
  mlf::HostArena arena;                  // pinned staging of the constants sent by mlf_region_set
  mlf::DevBuf refT, refR, lay_ctr, lay_mat, lay_T8, wrap, ell_ctr, ell_A, ell_Lt, ell_LtF, lay_TtF;
  bool chol_ready = false, chol_ok = false;
  double ell_eps_scale = 0.0;
  mlf::DevBuf tq, gate, pts, mask, row;
  // bounded per-proposal stage (mlf_prep4.hip): binary32 fragments, chain start values, error constants
  mlf::DevBuf p4_LtF, p4_TtF, p4_y0, lay_T64, ell_L;
  mlf::Prep4Consts p4c{};
  bool p4_ready = false;
  // "same quadratic form": A = T T^T + E with |E|_F measured (same_matrix) and c_lay == c_ell bit for bit (same_centres):
  // k_prep_sweep<.., true> reads delta^T A delta off the whitening chain; p4c_same = the constants of that form
  mlf::Prep4Consts p4c_same{};
  bool same_matrix = false, same_centres = false;
  std::vector<double> h_L, h_lay_ctr, h_ell_ctr;   // host copies: y0 = L^T (c_lay - c_ell) follows the ellipsoid centre
  mlf::FilterCtx filter;
  mlf::DevBuf gen, gen2, cube, smask, blk, sout, ax_zero, ax_mat, ax_pad;   // device-side sampling
  mlf::DevBuf s_invT, s_lo, s_hi, s_thin, s_count, rf_p, rf_L, rf_out, rf_aux, rf_keep;
  mlf::DevBuf s_invT_pad, s_tc, s_wc, s_thc, s_gate;   // t-space sampling: padded invT, survivors of the cheap tests (rows, cube rows, thinning draws)
  bool axes_ready = false, sampling_ready = false;
  // the driver's parameter-space wrapping ellipsoid (mlf_region_set_tregion / _wide): dense tr_w x tr_w matrix, centre, fixed
  // values; the refill calls gate on it while tr_on.  tr_w is d, or d + nderived for the gate over a user model's derived
  // parameters (mlf_region_refill_user_derived_gated alone runs then).  rf_member2: accepted && gate of the batch under evaluation
  mlf::DevBuf tr_A, tr_ctr, tr_fixed, rf_member2;
  mlf::DevBuf rf_wide;   // the kept rows as [p | q] of a refill with derived parameters (mlf_region_refill_user_derived)
  mlf::DevBuf rf_q;      // the q rows of the batch under evaluation (mlf_region_refill_user_derived_gated, direct form)
  bool tr_on = false;
  int tr_w = 0;
  double tr_enlarge = 0.0;
  std::vector<hipEvent_t> events;  // 4 per timed call
  size_t events_used = 0;
};

namespace mlf {

// The live points an exact test runs against: refT / refR as stage_live_points lays them out
struct LiveSet {
  const double *refT, *refR;
  int n, npad, d, dp;
  double r2;
};

inline LiveSet region_live(const mlf_region *r) { return {r->refT.as<double>(), r->refR.as<double>(), r->n, r->npad, r->d, r->dp, r->r2}; }

// Where the exact whitened coordinates come from when the per-proposal stage did not store them (k_prep4): the proposals
// themselves and the layer; the queries that need coordinates are whitened after the sweeps.  Also what the stage hands
// over to the launches behind it.
struct ExactSrc {
  const double *pts;
  const double *lay_ctr;
  const double *T8;   // row-major layer matrix, row stride ldt
  int ldt;
  const double *T64;  // the same as 64 x 64, zero padded (d <= 64)
  Prep4Args prep;     // plan.defer: the per-proposal stage, run inside the first sweep launch
  Prep4Consts same;   // its constants in the "same quadratic form" variant (plan.fused_variant bit 1; region_prep4_setup)
  EllExactArgs ell;   // the ellipsoid band, decided by the trailing waves of a later launch (count == nullptr: none)
};

// One filtered batch: query element (j, k) is q[j*ldq + k*ldk]; answers for all nq queries in out_mask (bytes) and/or out_idx
struct FilterBatch {
  FilterCtx &f;
  const BatchPlan &p;
  LiveSet L;
  const double *q;
  long long ldq, ldk, nq;
  const uint8_t *gate;     // queries not quantised by the per-proposal stage: the gate their quantisation honours
  uint8_t *out_mask;
  long long *out_idx;
  hipStream_t s;
  hipEvent_t ev_after;     // recorded behind the last matrix launch (stage events of a timed call)
  const ExactSrc *xs;      // plan.stage == STAGE_PREP4, else null
  const void *opF() const { return p.ordered ? f.refFm.p : f.refF.p; }
  const double *opR() const { return p.ordered ? f.refRm.as<double>() : L.refR; }
  long long ngroups() const { return (nq + 31) / 32; }
};

// ---- mlf_api.hip: library context, staging ------------------------------------------------------------------------
std::vector<double> pad_matrix(const double *m, int d, int dp, bool transpose);
std::vector<double> pad_vector(const double *v, int d, int dp, double fill = 0.0);
bool arena_active();
int arena_flush(hipStream_t s);
bool is_device_pointer(const void *p);
int upload(DevBuf &b, const void *src, size_t bytes, hipStream_t s);
int upload_any(DevBuf &b, const void *src, size_t bytes, hipStream_t s);
int check_dims(size_t d);
int stage_live_points(const double *pts, size_t n, size_t d, int dp, int npad, bool want_rows);
int prep_consts(DevBuf &ctr_b, DevBuf &mat_b, const double *ctr, const double *mat, int d, int dp, bool transpose, hipStream_t s);

// ---- mlf_route.hip: one membership batch along its plan ------------------------------------------------------------
int filter_prepare_refs(FilterCtx &f, const double *refR, int n, int d, int dp, hipStream_t s, bool host_sync, bool mask_mode = true);
int filter_refresh_refs(FilterCtx &f, const double *refR, int n, int d, int dp, hipStream_t s);
int misc_reserve(FilterCtx &f);
BatchPlan plan_batch(const FilterCtx &f, const mlf_region *r, BatchKind kind, long long nq, double r2, bool first_index = false,
                     bool pregate = false, const void *pts = nullptr, size_t host_nlive = 0);
int filter_reserve(FilterCtx &f, const BatchPlan &p, long long nq);
ScanArgs scan_args(const LiveSet &L, const double *q, long long ldq, long long ldk, long long nq, int mode);
void scan_finalise(ScanArgs &a, const FilterCtx &f, const ExactSrc &xs);
int filter_run(const FilterBatch &b);

// ---- mlf_inside.hip: the region's membership test on device data ---------------------------------------------------
int small_staging(Ctx &c);
int region_ellipsoid_gate(mlf_region *r, const double *d_pts, size_t np, uint8_t *gate, hipStream_t s);
int region_inside_enqueue(mlf_region *r, const double *d_pts, size_t np, uint8_t *d_mask, hipStream_t s,
                          hipEvent_t *ev /* 4 events or null */, long long *d_idx = nullptr, const uint8_t *pregate = nullptr);

}  // namespace mlf
