// mlf_walk_api.hip -- C ABI of the population step-sampler path (include/mlfriends_hip.h, section
// "population step sampler"): argument checks, device buffers, staging, kernel sequencing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/mlfriends_hip.h"
#include "mlf_ctx.hpp"
#include "mlf_misc.hpp"
#include "mlf_rwalk.hpp"
#include "mlf_sample.hpp"
#include "mlf_sslice.hpp"
#include "mlf_walk.hpp"

using namespace mlf;

// (the bound of every wide kernel: the resident slice walkers, k_rwalk_propose_wide, k_sslice_propose_wide)
static_assert(kWideDirMaxDim == MLF_MAX_DIM, "dw_direction_wide stages MLF_MAX_DIM normals in LDS");

// Device copies of what the region and the live points contribute, with the state of their setters: shared by the three
// population handles (mlf_walkers, mlf_rwalk, mlf_sslice)
struct RegionCopies {
  int d = 0;
  DevBuf axes, live, std, lay_ctr, lay_mat, lay_wrap, liveL;
  bool have_liveL = false;
  int nlive = 0;
  bool have_axes = false, have_live = false, have_std = false;
  int layer_kind = -1;
  bool layer_wrap = false;
  double r2 = 1.0;
  void release_copies() {
    for (DevBuf *b : {&axes, &live, &std, &lay_ctr, &lay_mat, &lay_wrap, &liveL}) b->release();
  }
};

// PopulationRandomWalkSampler's population (mlf_rwalk.hip): no chain, a walker is its current (u, p, L)
struct mlf_rwalk : RegionCopies {
  int P = 0, nsteps = 0;
  DevBuf u, p, L, start, ever, last, rej, tl, tr, dist2, unew, pnew, Lnew, inside, aux, parts, out;
  DevBuf *all[17] = {&u, &p, &L, &start, &ever, &last, &rej, &tl, &tr, &dist2, &unew, &pnew, &Lnew, &inside, &aux, &parts, &out};
};

// PopulationSimpleSliceSampler's population (mlf_sslice.hip): points, one iteration's proposals per worker, the control block
struct mlf_sslice : RegionCopies {
  int P = 0, nsteps = 0, max_it = 0;
  DevBuf u, p, L, start, v, tl, tr, status, zlist, taken, taken_it, t, unew, pnew, Lnew, member, widths, iters, dist2, nanrow, ctl,
      dirscale, aux, out;
  DevBuf *all[24] = {&u, &p, &L, &start, &v, &tl, &tr, &status, &zlist, &taken, &taken_it, &t, &unew, &pnew, &Lnew, &member,
                     &widths, &iters, &dist2, &nanrow, &ctl, &dirscale, &aux, &out};
  SsliceCtl *h_ctl = nullptr;      // pinned: the control block as the last poll saw it
  long long last_total_it = 0;     // iterations of the previous refill (batch policy)
};

struct mlf_walkers : RegionCopies {
  int P = 0, nsteps = 0, nparams = 0;
  DevBuf allu, allL, generation, currentt, currentv, left, right, sl, sr, currentp;
  DevBuf unew, movable, acceptable, success, pnew, Lnew, dist2;
  DevBuf gmax, flags, snap, idx, rows, vals, vidx, vrows, unif, blk, compact, pc, Lc, rec, aux;
  DevBuf ring, partials;
  bool proposed = false, compacted = false;
  std::vector<uint8_t> host_snap;
  // one captured launch sequence (replay): the executable graph and everything its captured arguments depend on
  struct GraphCache {
    hipGraphExec_t exec = nullptr;
    std::vector<unsigned long long> key;
    hipError_t release() {
      hipGraphExec_t e = exec;
      exec = nullptr;
      key.clear();
      return e ? hipGraphExecDestroy(e) : hipSuccess;
    }
  };
  // whole-step hipGraph: one launch replays the ~12 kernels + the record copy; the values that change per
  // call travel through a pinned StepParams block
  GraphCache step_graph;
  StepParams *h_sp = nullptr;      // pinned
  double *h_rec = nullptr;         // pinned
  DevBuf d_sp;
  // several rounds per call (mlf_walkers_rounds_dev)
  DevBuf r_ctl, r_flags, r_dist2, r_out, r_sp, r_last, r_parts, live_stage;
  GraphCache rounds_graph;         // the launch sequence of mlf_walkers_rounds_dev (parameter copy, four kernels, record copy) as ONE graph launch
  double *h_live = nullptr;        // pinned staging of mlf_walkers_update_live
  size_t h_live_bytes = 0;
  StepParams *h_rsp = nullptr;     // pinned
  double *h_rout = nullptr;        // pinned: record + per-round statistics
  size_t h_rout_doubles = 0;
};

namespace {

struct Scratch {
  DevBuf a, b, c, d, e, f, g, h, i, j, k, l, m;
};
Scratch g_s;

int upload(DevBuf &b, const void *host, size_t bytes, hipStream_t s) {
  CK(b.reserve(bytes ? bytes : 1));
  if (bytes) CK(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, s));
  return 0;
}

int download(void *host, const DevBuf &b, size_t bytes, hipStream_t s) {
  if (bytes) CK(hipMemcpyAsync(host, b.p, bytes, hipMemcpyDeviceToHost, s));
  return 0;
}

int check_nd(size_t n, size_t d) {
  if (d == 0) return fail_arg(MLF_E_BADARG, "dimensionality must be positive");
  if (n > 0x7fffffffull / (d ? d : 1)) return fail_arg(MLF_E_BADARG, "population too large");
  return 0;
}

WalkState state_of(const mlf_walkers *w) {
  WalkState s{};
  s.P = w->P;
  s.G = w->nsteps + 1;
  s.d = w->d;
  s.nparams = w->nparams;
  s.allu = w->allu.as<double>();
  s.allL = w->allL.as<double>();
  s.generation = w->generation.as<long long>();
  s.currentt = w->currentt.as<double>();
  s.currentv = w->currentv.as<double>();
  s.left = w->left.as<double>();
  s.right = w->right.as<double>();
  s.sl = w->sl.as<uint8_t>();
  s.sr = w->sr.as<uint8_t>();
  s.currentp = w->currentp.as<double>();
  s.unew = w->unew.as<double>();
  s.movable = w->movable.as<uint8_t>();
  s.acceptable = w->acceptable.as<uint8_t>();
  s.success = w->success.as<uint8_t>();
  s.pnew = w->pnew.as<double>();
  s.Lnew = w->Lnew.as<double>();
  s.dist2 = w->dist2.as<double>();
  return s;
}

WalkLayer layer_of(const RegionCopies *w) {
  WalkLayer l{};
  l.kind = w->layer_kind;
  l.ctr = w->lay_ctr.as<double>();
  l.mat = w->lay_mat.as<double>();
  l.wrap = w->layer_wrap ? w->lay_wrap.as<double>() : nullptr;
  l.r2 = w->r2;
  return l;
}

int ensure_params(mlf_walkers *w, size_t nparams) {
  if (nparams == 0) return fail_arg(MLF_E_BADARG, "nparams must be positive");
  if (w->nparams == (int)nparams) return 0;
  if (w->nparams != 0) return fail_arg(MLF_E_STATE, "number of transformed parameters changed between calls");
  w->nparams = (int)nparams;
  CK(w->currentp.reserve((size_t)w->P * nparams * sizeof(double)));
  CK(w->pnew.reserve((size_t)w->P * nparams * sizeof(double)));
  CK(hipMemsetAsync(w->currentp.p, 0xff, (size_t)w->P * nparams * sizeof(double), ctx_stream()));   // NaN
  return 0;
}

// What evaluates the proposals: the built-in pair (prior transform tkind, ta, tb; likelihood lkind, aux, sigma) or a user
// model (mlf_user.hip), whose kernel writes pnew itself and evaluates only the acceptable proposals (dw_update reads Lnew only
// where acceptable, and pnew only after a success, which needs acceptable); with it, tkind -1: a step's prologue proposes
// without a transform.
struct StepEval {
  mlf_usermodel *model = nullptr;
  int tkind = -1;
  double ta = 0.0, tb = 0.0;
  int lkind = 0;
  const double *aux = nullptr;
  double sigma = 0.0;

  int check(const RegionCopies *w) const {
    if (model) {
      if (usermodel_dim(model) != w->d) return fail_arg(MLF_E_BADARG, "user model and walkers differ in dimensionality");
      return 0;
    }
    if (tkind < 0 || tkind > 2 || lkind < 0 || lkind > 3) return fail_arg(MLF_E_BADARG, "unknown transform / likelihood kind");
    if (lkind == 0 && !aux) return fail_arg(MLF_E_BADARG, "the Gaussian likelihood needs its centres");
    return 0;
  }
  // pnew and Lnew on s; transform: the built-in transform has not run yet (a step's prologue runs it)
  int enqueue(mlf_walkers *w, bool transform, hipStream_t s) const {
    const WalkState st = state_of(w);
    if (model) return usermodel_rows(model, st.unew, w->P, st.acceptable, st.pnew, st.Lnew, s);
    if (transform) launch_walk_transform(st, tkind, ta, tb, s);
    launch_loglike(lkind, st.pnew, w->d, w->P, w->aux.as<double>(), sigma, st.Lnew, s);
    return 0;
  }
};

// update + harvest of walker ringindex; ev (mlf_walkers_finish_dev / _finish_user): the device evaluates the proposals first
int finish_common(mlf_walkers *w, double Lmin, const StepEval *ev, int64_t ringindex, double *rec) {
  hipStream_t s = ctx_stream();
  if (ev) {
    if (int rc = ev->check(w)) return rc;
    if (int rc = ensure_params(w, (size_t)w->d)) return rc;
    if (ev->aux)
      if (int rc = upload(w->aux, ev->aux, (size_t)w->d * 8, s)) return rc;
    if (int rc = ev->enqueue(w, true, s)) return rc;
    CK(hipGetLastError());
  }
  if (ringindex < 0 || ringindex >= w->P) return fail_arg(MLF_E_BADARG, "ringindex out of range");
  const size_t nrec = 9 + (size_t)w->d + (size_t)w->nparams;
  CK(w->rec.reserve(nrec * sizeof(double)));
  const WalkState st = state_of(w);
  launch_walk_update(st, Lmin, layer_of(w), s);
  launch_walk_harvest(st, ringindex, nullptr, w->r2, w->rec.as<double>(), w->partials.as<double>(), s);
  CK(hipGetLastError());
  if (int rc = download(rec, w->rec, nrec * sizeof(double), s)) return rc;
  CK(hipStreamSynchronize(s));
  w->proposed = false;
  return 0;
}

WalkDirData dir_data(const RegionCopies *w) {
  WalkDirData dd{};
  dd.axes = w->axes.as<double>();
  dd.live = w->live.as<double>();
  dd.nlive = w->nlive;
  dd.std = w->std.as<double>();
  return dd;
}

int check_direction_data(const RegionCopies *w, int kind) {
  const bool need_axes = kind == DIR_REGION_ORIENTED || kind == DIR_REGION_RANDOM || kind == DIR_MIXTURE;
  const bool need_live = kind == DIR_DIFFERENTIAL || kind == DIR_MIXTURE;
  if ((need_axes && !w->have_axes) || (need_live && !w->have_live) || (kind == DIR_CUBE_ORIENTED_SCALED && !w->have_std))
    return fail_arg(MLF_E_STATE, "mlf_walkers_set_direction_data has not provided what this direction kind needs");
  return 0;
}

// the record of a whole step: that of finish (nparams = d), then the ring index after the step
size_t step_nrec(const mlf_walkers *w) { return 10 + 2 * (size_t)w->d; }

// Philox counters one whole step (one round) consumes
uint64_t philox_per_call(const mlf_walkers *w) {
  const uint64_t per = (uint64_t)((w->d + 1) / 2 + 2);
  return (uint64_t)w->P * (per > 64 ? per : 64);
}

// the checks of every whole-step route, in this order; max_rounds: that of mlf_walkers_rounds_dev, test-hook sign removed
int check_step(const mlf_walkers *w, int dirkind, const StepEval &ev, int max_rounds = 1) {
  if (!w->have_liveL) return fail_arg(MLF_E_STATE, "mlf_walkers_set_live not called");
  if (dirkind < 0 || dirkind > DIR_MIXTURE) return fail_arg(MLF_E_BADARG, "unknown direction kind");
  if (int rc = ev.check(w)) return rc;
  if (max_rounds < 1) return fail_arg(MLF_E_BADARG, "max_rounds must not be 0");
  return check_direction_data(w, dirkind);
}

int prepare_step(mlf_walkers *w, const StepEval &ev, hipStream_t s) {
  if (int rc = ensure_params(w, (size_t)w->d)) return rc;
  if (!w->ring.p) {
    CK(w->ring.reserve(8));
    CK(hipMemsetAsync(w->ring.p, 0, 8, s));
  }
  CK(w->rec.reserve(step_nrec(w) * sizeof(double)));
  CK(w->aux.reserve((size_t)w->d * 8));
  if (ev.aux)
    if (int rc = upload(w->aux, ev.aux, (size_t)w->d * 8, s)) return rc;
  return 0;
}

// One whole step on s: the prologue (step_back, restarts, new slices, proposal, built-in transform), the likelihood, update
// and harvest into w->rec.  The kernels take the per-call scalars from p, or, with dev_params (a graph capture), from there.
int enqueue_step(mlf_walkers *w, int dirkind, const StepEval &ev, const StepParams &p, const StepParams *dev_params,
                 hipStream_t s) {
  const WalkState st = state_of(w);
  launch_walk_prologue(st, w->live.as<double>(), w->liveL.as<double>(), w->nlive, dirkind, dir_data(w), ev.tkind, ev.ta, ev.tb,
                       w->flags.as<uint8_t>(), p, dev_params, s);
  if (int rc = ev.enqueue(w, false, s)) return rc;
  launch_walk_update(st, p.Lmin, layer_of(w), s, dev_params);
  launch_walk_harvest(st, 0, w->ring.as<long long>(), p.r2, w->rec.as<double>(), w->partials.as<double>(), s, dev_params,
                      w->flags.as<uint8_t>());
  return 0;
}

// mlf_walkers_step_dev / _step_user: the kernels of one step launched one by one, one record back
int run_step(mlf_walkers *w, int dirkind, const StepEval &ev, const StepParams &p, double *rec, uint64_t *next_offset) {
  if (int rc = check_step(w, dirkind, ev)) return rc;
  hipStream_t s = ctx_stream();
  if (int rc = prepare_step(w, ev, s)) return rc;
  if (int rc = enqueue_step(w, dirkind, ev, p, nullptr, s)) return rc;
  CK(hipGetLastError());
  if (int rc = download(rec, w->rec, step_nrec(w) * sizeof(double), s)) return rc;
  CK(hipStreamSynchronize(s));
  *next_offset = p.offset + philox_per_call(w);
  return 0;
}

unsigned long long bits(double v) {
  unsigned long long u;
  memcpy(&u, &v, sizeof u);
  return u;
}
unsigned long long addr(const void *p) { return (unsigned long long)(uintptr_t)p; }

// what the captured arguments of a whole step depend on, on both graph routes
std::vector<unsigned long long> step_key(const mlf_walkers *w, int dirkind, const StepEval &ev) {
  return {(unsigned long long)dirkind, (unsigned long long)ev.tkind, bits(ev.ta), bits(ev.tb), (unsigned long long)ev.lkind,
          bits(ev.sigma), (unsigned long long)(w->layer_kind + 1), (unsigned long long)w->layer_wrap, (unsigned long long)w->nlive,
          addr(w->live.p), addr(w->liveL.p), addr(w->axes.p), addr(w->std.p), addr(w->lay_ctr.p), addr(w->lay_mat.p),
          addr(w->lay_wrap.p), addr(w->aux.p), addr(w->pnew.p), addr(w->currentp.p)};
}

// Launch c's graph on s and wait for it.  Without a graph for `key`, the old one goes and capture(s) is captured anew: every
// call in it is checked and the capture is always ended.  A capture that fails leaves no graph (exec null, key empty) and
// returns the first error.
template <class Capture>
int replay(mlf_walkers::GraphCache &c, std::vector<unsigned long long> key, hipStream_t s, Capture &&capture) {
  if (!c.exec || key != c.key) {
    CK(c.release());
    CK(hipStreamSynchronize(s));
    CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    int rc = capture(s);
    hipError_t e = hipGetLastError();
    if (!rc && e != hipSuccess) rc = fail_hip(e, "a launch during the graph capture", "mlf_walk_api.hip", __LINE__);
    hipGraph_t graph = nullptr;
    e = hipStreamEndCapture(s, &graph);
    if (!rc && e != hipSuccess) rc = fail_hip(e, "hipStreamEndCapture", "mlf_walk_api.hip", __LINE__);
    if (!rc) {
      e = hipGraphInstantiate(&c.exec, graph, nullptr, nullptr, 0);
      if (e != hipSuccess) {
        c.exec = nullptr;
        rc = fail_hip(e, "hipGraphInstantiate", "mlf_walk_api.hip", __LINE__);
      }
    }
    if (graph) (void)hipGraphDestroy(graph);
    if (rc) return rc;
    c.key = std::move(key);
  }
  CK(hipGraphLaunch(c.exec, s));
  CK(hipStreamSynchronize(s));
  return 0;
}

// ---- the setters of the region copies: one body for both handles
int set_direction_data(RegionCopies *w, const double *axes, const double *live, size_t nlive, const double *std) {
  hipStream_t s = ctx_stream();
  const size_t d = (size_t)w->d;
  if (axes) {
    if (int rc = upload(w->axes, axes, d * d * 8, s)) return rc;
    w->have_axes = true;
  }
  if (live) {
    if (nlive < 2) return fail_arg(MLF_E_BADARG, "differential directions need at least two live points");
    if (int rc = upload(w->live, live, nlive * d * 8, s)) return rc;
    w->nlive = (int)nlive;
    w->have_live = true;
  }
  if (std) {
    if (int rc = upload(w->std, std, d * 8, s)) return rc;
    w->have_std = true;
  }
  CK(hipStreamSynchronize(s));
  return 0;
}

int set_layer(RegionCopies *w, int kind, const double *ctr, const double *mat, const double *wrap, double maxradiussq) {
  if (kind < 0) {
    w->layer_kind = -1;
    return 0;
  }
  if (kind > 1 || !ctr || !mat) return fail_arg(MLF_E_BADARG, "layer kind must be 0 (affine) or 1 (scaling)");
  hipStream_t s = ctx_stream();
  const size_t d = (size_t)w->d;
  if (int rc = upload(w->lay_ctr, ctr, d * 8, s)) return rc;
  if (int rc = upload(w->lay_mat, mat, (kind == 0 ? d * d : d) * 8, s)) return rc;
  w->layer_wrap = wrap != nullptr;
  if (wrap)
    if (int rc = upload(w->lay_wrap, wrap, d * 8, s)) return rc;
  CK(hipStreamSynchronize(s));
  w->layer_kind = kind;
  w->r2 = maxradiussq;
  return 0;
}

int set_live(RegionCopies *w, const double *us, const double *Ls, size_t nlive) {
  if (nlive < 2) return fail_arg(MLF_E_BADARG, "at least two live points are needed");
  hipStream_t s = ctx_stream();
  if (int rc = upload(w->live, us, nlive * (size_t)w->d * 8, s)) return rc;
  if (int rc = upload(w->liveL, Ls, nlive * 8, s)) return rc;
  w->nlive = (int)nlive;
  w->have_live = true;
  w->have_liveL = true;
  return 0;
}

// ---- mlf_rwalk: one refill = start rows, nsteps moves of every walker, diagnostics and counts, one synchronisation
struct RwalkOut {
  double *u, *p, *L;
  int64_t *start;
  uint8_t *ever, *last;
  double *tleft, *tright, *counts;
};

int rwalk_refill(mlf_rwalk *w, double Lmin, int dirkind, double dirscale, uint64_t seed, uint64_t offset, const StepEval &ev,
                 int form, const RwalkOut &o, uint64_t *next_offset) {
  if (!w || !o.u || !o.p || !o.L || !o.start || !o.ever || !o.last || !o.counts || !next_offset)
    return fail_arg(MLF_E_BADARG, "null pointer");
  if (!w->have_liveL) return fail_arg(MLF_E_STATE, "mlf_rwalk_set_live not called");
  if (dirkind < 0 || dirkind > DIR_MIXTURE) return fail_arg(MLF_E_BADARG, "unknown direction kind");
  if (form < 0 || form > 1) return fail_arg(MLF_E_BADARG, "form must be 0 (chosen by shape) or 1 (chain form)");
  if (int rc = ev.check(w)) return rc;
  if (int rc = check_direction_data(w, dirkind)) return rc;
  hipStream_t s = ctx_stream();
  const size_t P = (size_t)w->P, d = (size_t)w->d;
  if (ev.aux)
    if (int rc = upload(w->aux, ev.aux, d * 8, s)) return rc;
  RwalkArgs a{};
  a.w.P = w->P;
  a.w.nsteps = w->nsteps;
  a.w.d = w->d;
  a.w.u = w->u.as<double>();
  a.w.p = w->p.as<double>();
  a.w.L = w->L.as<double>();
  a.w.start = w->start.as<long long>();
  a.w.ever = w->ever.as<uint8_t>();
  a.w.last = w->last.as<uint8_t>();
  a.w.rej = w->rej.as<int>();
  a.w.tl = w->tl.as<double>();
  a.w.tr = w->tr.as<double>();
  a.w.dist2 = w->dist2.as<double>();
  a.w.unew = w->unew.as<double>();
  a.w.pnew = w->pnew.as<double>();
  a.w.Lnew = w->Lnew.as<double>();
  a.w.inside = w->inside.as<uint8_t>();
  a.live = w->live.as<double>();
  a.Ls = w->liveL.as<double>();
  a.nlive = w->nlive;
  a.dirkind = dirkind;
  a.dirscale = dirscale;
  a.dd = dir_data(w);
  a.tkind = ev.tkind;
  a.ta = ev.ta;
  a.tb = ev.tb;
  a.lkind = ev.lkind;
  a.aux = w->aux.as<double>();
  a.sigma = ev.sigma;
  a.ly = layer_of(w);
  a.Lmin = Lmin;
  a.seed = seed;
  a.offset = offset;
  a.parts = w->parts.as<double>();
  a.out = w->out.as<double>();
  const bool fused = !ev.model && form == 0 && rwalk_fused_covers(w->d, w->layer_kind);
  if (fused) {
    launch_rwalk_fused(a, s);
  } else {   // all nsteps triples queued back to back, no synchronisation in between
    launch_rwalk_start(a, s);
    for (int step = 0; step < w->nsteps; ++step) {
      launch_rwalk_propose(a, step, s);
      if (ev.model) {
        if (int rc = usermodel_rows(ev.model, a.w.unew, w->P, a.w.inside, a.w.pnew, a.w.Lnew, s)) return rc;
      } else {
        launch_loglike(ev.lkind, a.w.pnew, w->d, w->P, a.aux, ev.sigma, a.w.Lnew, s);
      }
      launch_rwalk_accept(a, s);
    }
  }
  launch_rwalk_finish(a, s);
  CK(hipGetLastError());
  if (int rc = download(o.u, w->u, P * d * 8, s)) return rc;
  if (int rc = download(o.p, w->p, P * d * 8, s)) return rc;
  if (int rc = download(o.L, w->L, P * 8, s)) return rc;
  if (int rc = download(o.start, w->start, P * 8, s)) return rc;
  if (int rc = download(o.ever, w->ever, P, s)) return rc;
  if (int rc = download(o.last, w->last, P, s)) return rc;
  if (o.tleft)
    if (int rc = download(o.tleft, w->tl, P * 8, s)) return rc;
  if (o.tright)
    if (int rc = download(o.tright, w->tr, P * 8, s)) return rc;
  if (int rc = download(o.counts, w->out, kRwalkOut * sizeof(double), s)) return rc;
  CK(hipStreamSynchronize(s));
  o.counts[kRwalkOut] = fused ? 0.0 : 1.0;
  *next_offset = offset + rwalk_philox_per_refill(w->P, w->nsteps, w->d);
  return 0;
}

// ---- mlf_sslice: one refill = start rows, nsteps slice steps of the whole population, diagnostics and counts.  The host
// queues slots (propose, evaluation, update, deal) without knowing which step they serve and reads the control block once
// per batch (a pinned copy and one synchronisation) until `finished` is set.
struct SsliceOut {
  double *u, *p, *L;
  int64_t *start;
  double *tleft, *tright;
  int32_t *taken, *taken_it, *iters;
  double *widths, *counts;
};

// Batch policy (slots_per_poll == 0).  A slot past the end costs four launches that exit at their first load (the built-in
// likelihood kernel, which has no such load, evaluates P stale rows), a poll costs one synchronisation.  The first batch is
// the previous refill's iteration count plus an eighth (at least 2) -- refills of one run resemble each other -- or, for a
// handle's first refill, 6 per step; each later batch is the steps still open times the mean iterations per step so far (at
// least 2 per step, at least 4 slots).  Never more than the worst case that is left.
long long sslice_batch(const mlf_sslice *w, const SsliceCtl &c, bool first) {
  const long long left = (long long)(w->nsteps - c.step) * w->max_it - c.it;
  long long n;
  if (first) {
    n = w->last_total_it ? w->last_total_it + std::max(2ll, w->last_total_it / 8) : (long long)w->nsteps * std::min(w->max_it, 6);
  } else {
    const long long per = c.step ? (c.total_it + c.step - 1) / c.step : c.total_it;
    n = std::max(4ll, (long long)(w->nsteps - c.step) * std::min((long long)w->max_it, std::max(2ll, per)));
  }
  return std::min(n, left);
}

int sslice_refill(mlf_sslice *w, double Lmin, int dirkind, const double *dirscale, int limit, double shrink, uint64_t seed,
                  uint64_t offset, const StepEval &ev, int slots_per_poll, const SsliceOut &o, uint64_t *next_offset) {
  if (!w || !dirscale || !o.u || !o.p || !o.L || !o.start || !o.iters || !o.widths || !o.counts || !next_offset)
    return fail_arg(MLF_E_BADARG, "null pointer");
  if (!w->have_liveL) return fail_arg(MLF_E_STATE, "mlf_sslice_set_live not called");
  if (dirkind < 0 || dirkind > DIR_MIXTURE) return fail_arg(MLF_E_BADARG, "unknown direction kind");
  if (limit < 0 || limit > 1) return fail_arg(MLF_E_BADARG, "slice limit must be 0 (unit cube) or 1 (clipped to [-1, 1])");
  if (!(shrink >= 1.0)) return fail_arg(MLF_E_BADARG, "the shrink factor must be at least 1");
  if (slots_per_poll < 0) return fail_arg(MLF_E_BADARG, "slots per poll must not be negative");
  if (int rc = ev.check(w)) return rc;
  if (int rc = check_direction_data(w, dirkind)) return rc;
  hipStream_t s = ctx_stream();
  const size_t P = (size_t)w->P, d = (size_t)w->d, nsteps = (size_t)w->nsteps;
  if (ev.aux)
    if (int rc = upload(w->aux, ev.aux, d * 8, s)) return rc;
  if (int rc = upload(w->dirscale, dirscale, nsteps * 8, s)) return rc;
  CK(hipMemsetAsync(w->ctl.p, 0, sizeof(SsliceCtl), s));
  SsliceArgs a{};
  a.w.P = w->P;
  a.w.nsteps = w->nsteps;
  a.w.d = w->d;
  a.w.max_it = w->max_it;
  a.w.u = w->u.as<double>();
  a.w.p = w->p.as<double>();
  a.w.L = w->L.as<double>();
  a.w.start = w->start.as<long long>();
  a.w.v = w->v.as<double>();
  a.w.tl = w->tl.as<double>();
  a.w.tr = w->tr.as<double>();
  a.w.status = w->status.as<uint8_t>();
  a.w.zlist = w->zlist.as<int>();
  a.w.taken = w->taken.as<int>();
  a.w.taken_it = w->taken_it.as<int>();
  a.w.t = w->t.as<double>();
  a.w.unew = w->unew.as<double>();
  a.w.pnew = w->pnew.as<double>();
  a.w.Lnew = w->Lnew.as<double>();
  a.w.member = w->member.as<uint8_t>();
  a.w.widths = w->widths.as<double>();
  a.w.iters = w->iters.as<int>();
  a.w.dist2 = w->dist2.as<double>();
  a.w.nanrow = w->nanrow.as<uint8_t>();
  a.w.ctl = w->ctl.as<SsliceCtl>();
  a.live = w->live.as<double>();
  a.Ls = w->liveL.as<double>();
  a.nlive = w->nlive;
  a.dirkind = dirkind;
  a.dirscale = w->dirscale.as<double>();
  a.dd = dir_data(w);
  a.limit = limit;
  a.shrink = shrink;
  a.tkind = ev.tkind;
  a.ta = ev.ta;
  a.tb = ev.tb;
  a.ly = layer_of(w);
  a.Lmin = Lmin;
  a.seed = seed;
  a.offset = offset;
  a.out = w->out.as<double>();
  launch_sslice_start(a, s);
  SsliceCtl seen{};
  for (bool first = true; !seen.finished; first = false) {
    const long long left = (long long)(w->nsteps - seen.step) * w->max_it - seen.it;
    const long long nslots = slots_per_poll ? std::min((long long)slots_per_poll, left) : sslice_batch(w, seen, first);
    for (long long slot = 0; slot < nslots; ++slot) {
      launch_sslice_propose(a, s);
      if (ev.model) {
        if (int rc = usermodel_rows(ev.model, a.w.unew, w->P, a.w.member, a.w.pnew, a.w.Lnew, s)) return rc;
      } else {
        launch_loglike(ev.lkind, a.w.pnew, w->d, w->P, w->aux.as<double>(), ev.sigma, a.w.Lnew, s);
      }
      launch_sslice_update(a, s);
      launch_sslice_deal(a, s);
    }
    CK(hipGetLastError());
    CK(hipMemcpyAsync(w->h_ctl, w->ctl.p, sizeof(SsliceCtl), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    const SsliceCtl now = *w->h_ctl;
    // every slot of an unfinished refill is one iteration: anything else means the control block is not ours
    if (!now.finished && now.total_it != seen.total_it + nslots) return fail_arg(MLF_E_STATE, "mlf_sslice: the control block did not advance");
    seen = now;
  }
  launch_sslice_finish(a, s);
  CK(hipGetLastError());
  if (int rc = download(o.u, w->u, P * d * 8, s)) return rc;
  if (int rc = download(o.p, w->p, P * d * 8, s)) return rc;
  if (int rc = download(o.L, w->L, P * 8, s)) return rc;
  if (int rc = download(o.start, w->start, P * 8, s)) return rc;
  if (o.tleft)
    if (int rc = download(o.tleft, w->tl, P * 8, s)) return rc;
  if (o.tright)
    if (int rc = download(o.tright, w->tr, P * 8, s)) return rc;
  if (o.taken)
    if (int rc = download(o.taken, w->taken, P * 4, s)) return rc;
  if (o.taken_it)
    if (int rc = download(o.taken_it, w->taken_it, P * 4, s)) return rc;
  if (int rc = download(o.iters, w->iters, nsteps * 4, s)) return rc;
  if (int rc = download(o.widths, w->widths, nsteps * P * 8, s)) return rc;
  if (int rc = download(o.counts + 2, w->out, kSsliceOut * sizeof(double), s)) return rc;
  CK(hipStreamSynchronize(s));
  o.counts[0] = (double)seen.discarded;
  o.counts[1] = (double)seen.total_it;
  w->last_total_it = seen.total_it;
  *next_offset = offset + sslice_philox_per_refill(w->P, w->nsteps, w->d, w->max_it);
  return 0;
}

}  // namespace

extern "C" {

int mlf_walkers_create(mlf_walkers **out, size_t popsize, size_t nsteps, size_t d) {
  if (!out) return fail_arg(MLF_E_BADARG, "null pointer");
  *out = nullptr;
  if (popsize == 0 || nsteps == 0 || d == 0 || popsize > (1u << 24) || nsteps > 65535)
    return fail_arg(MLF_E_BADARG, "mlf_walkers_create: popsize, nsteps, d must be positive");
  if (d > MLF_MAX_DIM)
    return fail_arg(MLF_E_DIM, "the resident walkers (one wave per walker, the lanes striding over the row) cover up to MLF_MAX_DIM = 1024 dimensions");
  // walker * d + coordinate is an int in the element-per-thread kernels (k_walk_start / points / brackets)
  if (popsize * d > 0x7fffffffull) return fail_arg(MLF_E_BADARG, "mlf_walkers_create: population too large");
  if (int rc = ensure_ctx()) return rc;
  mlf_walkers *w = new mlf_walkers();
  w->P = (int)popsize;
  w->nsteps = (int)nsteps;
  w->d = (int)d;
  const size_t P = popsize, G = nsteps + 1;
  struct {
    DevBuf *b;
    size_t bytes;
  } plan[] = {{&w->allu, P * G * d * 8}, {&w->allL, P * G * 8}, {&w->generation, P * 8}, {&w->currentt, P * 8},
              {&w->currentv, P * d * 8}, {&w->left, P * 8},     {&w->right, P * 8},      {&w->sl, P},
              {&w->sr, P},               {&w->unew, P * d * 8}, {&w->movable, P},        {&w->acceptable, P},
              {&w->success, P},          {&w->Lnew, P * 8},     {&w->dist2, P * 8},      {&w->gmax, 8},
              {&w->flags, P},            {&w->unif, P * 8},     {&w->blk, ((P + 255) / 256 + 1) * 4},
              {&w->compact, P * d * 8}, {&w->partials, ((P + 1023) / 1024) * 6 * 8}};
  for (auto &e : plan) {
    hipError_t err = e.b->reserve(e.bytes);
    if (err != hipSuccess) {
      mlf_walkers_destroy(w);
      return fail_hip(err, "device allocation for the walker population", "mlf_walk_api.hip", __LINE__);
    }
  }
  launch_walk_reset(state_of(w), ctx_stream());
  hipError_t err = hipStreamSynchronize(ctx_stream());
  if (err != hipSuccess) {
    mlf_walkers_destroy(w);
    return fail_hip(err, "walker reset", "mlf_walk_api.hip", __LINE__);
  }
  *out = w;
  return 0;
}

int mlf_walkers_destroy(mlf_walkers *w) {
  if (!w) return 0;
  DevBuf *all[] = {&w->allu, &w->allL, &w->generation, &w->currentt, &w->currentv, &w->left, &w->right, &w->sl,
                   &w->sr, &w->currentp, &w->unew, &w->movable, &w->acceptable, &w->success, &w->pnew, &w->Lnew,
                   &w->dist2, &w->gmax, &w->flags, &w->snap, &w->idx, &w->rows, &w->vals, &w->vidx, &w->vrows, &w->unif, &w->blk, &w->compact,
                   &w->pc, &w->Lc, &w->rec, &w->aux, &w->ring, &w->partials};
  for (DevBuf *b : all) b->release();
  w->release_copies();
  w->d_sp.release();
  for (DevBuf *b : {&w->r_ctl, &w->r_flags, &w->r_dist2, &w->r_out, &w->r_sp, &w->r_last, &w->r_parts, &w->live_stage}) b->release();
  if (w->h_live) (void)hipHostFree(w->h_live);
  (void)w->rounds_graph.release();
  if (w->h_rsp) (void)hipHostFree(w->h_rsp);
  if (w->h_rout) (void)hipHostFree(w->h_rout);
  (void)w->step_graph.release();
  if (w->h_sp) (void)hipHostFree(w->h_sp);
  if (w->h_rec) (void)hipHostFree(w->h_rec);
  delete w;
  return 0;
}

int mlf_walkers_reset(mlf_walkers *w) {
  if (!w) return fail_arg(MLF_E_BADARG, "null pointer");
  launch_walk_reset(state_of(w), ctx_stream());
  if (w->nparams) CK(hipMemsetAsync(w->currentp.p, 0xff, (size_t)w->P * w->nparams * sizeof(double), ctx_stream()));
  if (w->ring.p) CK(hipMemsetAsync(w->ring.p, 0, 8, ctx_stream()));
  CK(hipGetLastError());
  w->proposed = false;
  return 0;
}

int mlf_walkers_begin(mlf_walkers *w, double Lmin, int64_t *generation, uint8_t *flags) {
  if (!w || !generation || !flags) return fail_arg(MLF_E_BADARG, "null pointer");
  hipStream_t s = ctx_stream();
  const size_t P = (size_t)w->P;
  // snapshot = generation (8 P bytes) followed by the flags (P bytes): one device-to-host copy
  CK(w->snap.reserve(9 * P));
  uint8_t *d_flags = w->snap.as<uint8_t>() + 8 * P;
  launch_walk_step_back(state_of(w), Lmin, w->gmax.as<long long>(), d_flags, s);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(w->snap.p, w->generation.p, 8 * P, hipMemcpyDeviceToDevice, s));
  w->host_snap.resize(9 * P);
  CK(hipMemcpyAsync(w->host_snap.data(), w->snap.p, 9 * P, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  memcpy(generation, w->host_snap.data(), 8 * P);
  memcpy(flags, w->host_snap.data() + 8 * P, P);
  return 0;
}

int mlf_walkers_start(mlf_walkers *w, const int64_t *idx, size_t n, const double *u_rows, const double *L) {
  if (!w || (n && (!idx || !u_rows || !L))) return fail_arg(MLF_E_BADARG, "null pointer");
  if (n == 0) return 0;
  for (size_t j = 0; j < n; ++j)
    if (idx[j] < 0 || idx[j] >= w->P) return fail_arg(MLF_E_BADARG, "walker index out of range");
  hipStream_t s = ctx_stream();
  if (int rc = upload(w->idx, idx, n * 8, s)) return rc;
  if (int rc = upload(w->rows, u_rows, n * (size_t)w->d * 8, s)) return rc;
  if (int rc = upload(w->vals, L, n * 8, s)) return rc;
  launch_walk_start(state_of(w), w->idx.as<long long>(), (int)n, w->rows.as<double>(), w->vals.as<double>(), s);
  CK(hipGetLastError());
  return 0;
}

int mlf_walkers_points(mlf_walkers *w, const int64_t *idx, size_t n, double *out_rows) {
  if (!w || (n && (!idx || !out_rows))) return fail_arg(MLF_E_BADARG, "null pointer");
  if (n == 0) return 0;
  for (size_t j = 0; j < n; ++j)
    if (idx[j] < 0 || idx[j] >= w->P) return fail_arg(MLF_E_BADARG, "walker index out of range");
  hipStream_t s = ctx_stream();
  if (int rc = upload(w->idx, idx, n * 8, s)) return rc;
  CK(w->rows.reserve(n * (size_t)w->d * 8));
  launch_walk_points(state_of(w), w->idx.as<long long>(), (int)n, w->rows.as<double>(), s);
  CK(hipGetLastError());
  if (int rc = download(out_rows, w->rows, n * (size_t)w->d * 8, s)) return rc;
  CK(hipStreamSynchronize(s));
  return 0;
}

int mlf_walkers_brackets(mlf_walkers *w, const int64_t *idx, size_t n, double scale, const double *v_rows) {
  if (!w || (n && (!idx || !v_rows))) return fail_arg(MLF_E_BADARG, "null pointer");
  if (n == 0) return 0;
  for (size_t j = 0; j < n; ++j)
    if (idx[j] < 0 || idx[j] >= w->P) return fail_arg(MLF_E_BADARG, "walker index out of range");
  hipStream_t s = ctx_stream();
  if (int rc = upload(w->vidx, idx, n * 8, s)) return rc;
  if (int rc = upload(w->vrows, v_rows, n * (size_t)w->d * 8, s)) return rc;
  launch_walk_brackets(state_of(w), w->vidx.as<long long>(), (int)n, scale, w->vrows.as<double>(), s);
  CK(hipGetLastError());
  return 0;
}

int mlf_walkers_set_direction_data(mlf_walkers *w, const double *axes, const double *live, size_t nlive,
                                   const double *std) {
  if (!w) return fail_arg(MLF_E_BADARG, "null pointer");
  return set_direction_data(w, axes, live, nlive, std);
}

int mlf_walkers_brackets_philox(mlf_walkers *w, double scale, int kind, double dirscale, uint64_t seed,
                                uint64_t offset, uint64_t *next_offset) {
  if (!w || !next_offset) return fail_arg(MLF_E_BADARG, "null pointer");
  if (kind < 0 || kind > DIR_MIXTURE) return fail_arg(MLF_E_BADARG, "unknown direction kind");
  if (int rc = check_direction_data(w, kind)) return rc;
  launch_walk_brackets_philox(state_of(w), scale, kind, dirscale, dir_data(w), seed, offset, ctx_stream());
  CK(hipGetLastError());
  *next_offset = offset + (uint64_t)w->P * (uint64_t)((w->d + 1) / 2 + 2);
  return 0;
}

int mlf_walkers_set_layer(mlf_walkers *w, int kind, const double *ctr, const double *mat, const double *wrap,
                          double maxradiussq) {
  if (!w) return fail_arg(MLF_E_BADARG, "null pointer");
  return set_layer(w, kind, ctr, mat, wrap, maxradiussq);
}

int mlf_walkers_propose(mlf_walkers *w, const double *unif, uint64_t seed, uint64_t offset, double *unew_out,
                        size_t *nacc) {
  if (!w) return fail_arg(MLF_E_BADARG, "null pointer");
  if ((unew_out == nullptr) != (nacc == nullptr)) return fail_arg(MLF_E_BADARG, "unew_out and nacc go together");
  hipStream_t s = ctx_stream();
  const WalkState st = state_of(w);
  const double *d_unif = nullptr;
  if (unif) {
    if (int rc = upload(w->unif, unif, (size_t)w->P * 8, s)) return rc;
    d_unif = w->unif.as<double>();
  }
  launch_walk_propose(st, d_unif, seed, offset, s);
  CK(hipGetLastError());
  w->proposed = true;
  w->compacted = false;
  if (!nacc) return 0;
  // host likelihood: hand back the acceptable rows in walker order
  const Compaction acceptable(st.acceptable, w->P, w->blk.as<unsigned>(), s);
  acceptable.scatter(st.unew, w->d, w->compact.as<double>(), (size_t)w->P);
  size_t count = 0;
  CK(acceptable.count((size_t)w->P, &count));
  if (count) {
    if (int rc = download(unew_out, w->compact, (size_t)count * w->d * 8, s)) return rc;
    CK(hipStreamSynchronize(s));
  }
  *nacc = count;
  w->compacted = true;
  return 0;
}

int mlf_walkers_finish(mlf_walkers *w, double Lmin, const double *pnew, const double *Lnew, size_t nacc,
                       size_t nparams, int64_t ringindex, double *rec) {
  if (!w || !rec || (nacc && (!pnew || !Lnew))) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!w->proposed || !w->compacted)
    return fail_arg(MLF_E_STATE, "mlf_walkers_finish without a preceding mlf_walkers_propose(unew_out != NULL)");
  if (int rc = ensure_params(w, nparams)) return rc;
  hipStream_t s = ctx_stream();
  if (nacc) {
    if (int rc = upload(w->pc, pnew, nacc * nparams * 8, s)) return rc;
    if (int rc = upload(w->Lc, Lnew, nacc * 8, s)) return rc;
    launch_walk_expand(state_of(w), w->blk.as<unsigned>(), w->pc.as<double>(), w->Lc.as<double>(), s);
    CK(hipGetLastError());
  }
  return finish_common(w, Lmin, nullptr, ringindex, rec);
}

int mlf_walkers_finish_dev(mlf_walkers *w, double Lmin, int tkind, double ta, double tb, int lkind,
                           const double *aux, double sigma, int64_t ringindex, double *rec) {
  if (!w || !rec) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!w->proposed) return fail_arg(MLF_E_STATE, "mlf_walkers_finish_dev without a preceding mlf_walkers_propose");
  const StepEval ev{nullptr, tkind, ta, tb, lkind, aux, sigma};
  return finish_common(w, Lmin, &ev, ringindex, rec);
}

int mlf_walkers_finish_user(mlf_walkers *w, double Lmin, mlf_usermodel *model, int64_t ringindex, double *rec) {
  if (!w || !rec || !model) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!w->proposed) return fail_arg(MLF_E_STATE, "mlf_walkers_finish_user without a preceding mlf_walkers_propose");
  const StepEval ev{model};
  return finish_common(w, Lmin, &ev, ringindex, rec);
}

int mlf_walkers_set_live(mlf_walkers *w, const double *us, const double *Ls, size_t nlive) {
  if (!w || !us || !Ls) return fail_arg(MLF_E_BADARG, "null pointer");
  return set_live(w, us, Ls, nlive);
}

int mlf_walkers_update_live(mlf_walkers *w, const int64_t *rows, size_t count, const double *us_rows, const double *Ls_rows) {
  if (!w || (count && (!rows || !us_rows || !Ls_rows))) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!w->have_liveL) return fail_arg(MLF_E_STATE, "mlf_walkers_set_live not called");
  if (count == 0) return 0;
  const size_t d = (size_t)w->d;
  for (size_t j = 0; j < count; ++j)
    if (rows[j] < 0 || rows[j] >= w->nlive) return fail_arg(MLF_E_BADARG, "live point index out of range");
  hipStream_t s = ctx_stream();
  // pinned staging, reused from call to call: every path that reads the device copy ends with a synchronisation of the
  // library's stream, so the copy queued by the previous update has long been made
  const size_t need = count * (d + 2) * sizeof(double);
  if (w->h_live_bytes < need) {
    if (w->h_live) CK(hipHostFree(w->h_live));
    w->h_live = nullptr;
    w->h_live_bytes = 0;
    const size_t cap = need < 4096 ? 4096 : need;
    CK(hipHostMalloc(reinterpret_cast<void **>(&w->h_live), cap, hipHostMallocDefault));
    w->h_live_bytes = cap;
  }
  CK(w->live_stage.reserve(w->h_live_bytes));
  double *hs = w->h_live;
  memcpy(hs, us_rows, count * d * sizeof(double));
  memcpy(hs + count * d, Ls_rows, count * sizeof(double));
  memcpy(hs + count * (d + 1), rows, count * sizeof(int64_t));
  CK(hipMemcpyAsync(w->live_stage.p, hs, need, hipMemcpyHostToDevice, s));
  const double *ds = w->live_stage.as<double>();
  launch_walk_scatter_live(ds, ds + count * d, reinterpret_cast<const long long *>(ds + count * (d + 1)), (int)count, (int)d,
                           w->live.as<double>(), w->liveL.as<double>(), s);
  CK(hipGetLastError());
  return 0;
}

int mlf_walkers_step_dev(mlf_walkers *w, double Lmin, double scale, int dirkind, double dirscale, uint64_t seed,
                         uint64_t offset, int tkind, double ta, double tb, int lkind, const double *aux, double sigma,
                         double *rec, uint64_t *next_offset) {
  if (!w || !rec || !next_offset) return fail_arg(MLF_E_BADARG, "null pointer");
  return run_step(w, dirkind, StepEval{nullptr, tkind, ta, tb, lkind, aux, sigma}, StepParams{Lmin, scale, dirscale, w->r2, seed, offset},
                  rec, next_offset);
}

int mlf_walkers_step_user(mlf_walkers *w, double Lmin, double scale, int dirkind, double dirscale, uint64_t seed,
                          uint64_t offset, mlf_usermodel *model, double *rec, uint64_t *next_offset) {
  if (!w || !rec || !next_offset || !model) return fail_arg(MLF_E_BADARG, "null pointer");
  return run_step(w, dirkind, StepEval{model}, StepParams{Lmin, scale, dirscale, w->r2, seed, offset}, rec, next_offset);
}

int mlf_walkers_step_graph(mlf_walkers *w, double Lmin, double scale, int dirkind, double dirscale, uint64_t seed,
                           uint64_t offset, int tkind, double ta, double tb, int lkind, const double *aux, double sigma,
                           double *rec, uint64_t *next_offset) {
  if (!w || !rec || !next_offset) return fail_arg(MLF_E_BADARG, "null pointer");
  const StepEval ev{nullptr, tkind, ta, tb, lkind, aux, sigma};
  if (int rc = check_step(w, dirkind, ev)) return rc;
  hipStream_t s = ctx_stream();
  if (int rc = prepare_step(w, ev, s)) return rc;
  const size_t nrec = step_nrec(w);
  if (!w->h_sp) {
    CK(hipHostMalloc(reinterpret_cast<void **>(&w->h_sp), sizeof(StepParams), hipHostMallocDefault));
    CK(hipHostMalloc(reinterpret_cast<void **>(&w->h_rec), nrec * sizeof(double), hipHostMallocDefault));
    CK(w->d_sp.reserve(sizeof(StepParams)));
  }
  std::vector<unsigned long long> key = step_key(w, dirkind, ev);
  key.push_back(addr(w->rec.p));
  *w->h_sp = StepParams{Lmin, scale, dirscale, w->r2, seed, offset};
  if (int rc = replay(w->step_graph, std::move(key), s, [&](hipStream_t s) -> int {
        CK(hipMemcpyAsync(w->d_sp.p, w->h_sp, sizeof(StepParams), hipMemcpyHostToDevice, s));
        if (int rc = enqueue_step(w, dirkind, ev, StepParams{}, w->d_sp.as<StepParams>(), s)) return rc;
        CK(hipMemcpyAsync(w->h_rec, w->rec.p, nrec * sizeof(double), hipMemcpyDeviceToHost, s));
        return 0;
      }))
    return rc;
  memcpy(rec, w->h_rec, nrec * sizeof(double));
  *next_offset = offset + philox_per_call(w);
  return 0;
}

int mlf_walkers_rounds_dev(mlf_walkers *w, double Lmin, double scale, int dirkind, double dirscale, uint64_t seed,
                           uint64_t offset, int tkind, double ta, double tb, int lkind, const double *aux, double sigma,
                           int max_rounds, double *rec, double *round_rows, int *rounds, uint64_t *next_offset) {
  if (!w || !rec || !round_rows || !rounds || !next_offset) return fail_arg(MLF_E_BADARG, "null pointer");
  const int force_memory_form = max_rounds < 0;   // test hook: every round through global memory (the first form of this path)
  if (force_memory_form) max_rounds = -max_rounds;
  const StepEval ev{nullptr, tkind, ta, tb, lkind, aux, sigma};
  if (int rc = check_step(w, dirkind, ev, max_rounds)) return rc;
  hipStream_t s = ctx_stream();
  if (int rc = prepare_step(w, ev, s)) return rc;
  // the per-round flag / distance arrays are [max_rounds][P]: keep them within 64 MiB
  const size_t per_round = (size_t)w->P * 9;
  const size_t cap = ((size_t)64 << 20) / per_round;
  if ((size_t)max_rounds > cap) max_rounds = cap < 1 ? 1 : (int)cap;
  if (max_rounds > 4096) max_rounds = 4096;
  const size_t nrec = step_nrec(w);
  const size_t nout = nrec + 5 * (size_t)max_rounds;
  if (!w->h_rsp) CK(hipHostMalloc(reinterpret_cast<void **>(&w->h_rsp), sizeof(StepParams), hipHostMallocDefault));
  if (w->h_rout_doubles < nout) {
    if (w->h_rout) CK(hipHostFree(w->h_rout));
    w->h_rout = nullptr;
    CK(hipHostMalloc(reinterpret_cast<void **>(&w->h_rout), nout * sizeof(double), hipHostMallocDefault));
    w->h_rout_doubles = nout;
  }
  CK(w->r_sp.reserve(sizeof(StepParams)));
  CK(w->r_ctl.reserve(8 * sizeof(int)));
  CK(w->r_flags.reserve((size_t)max_rounds * w->P));
  CK(w->r_dist2.reserve((size_t)max_rounds * w->P * sizeof(double)));
  CK(w->r_out.reserve(nout * sizeof(double)));
  CK(w->r_last.reserve((size_t)w->P * sizeof(int)));
  const size_t nchunks = ((size_t)w->P + 1023) / 1024;
  if (nchunks > 1) CK(w->r_parts.reserve((size_t)max_rounds * nchunks * 5 * sizeof(double)));
  *w->h_rsp = StepParams{Lmin, scale, dirscale, w->r2, seed, offset};
  RoundsArgs a{};
  a.w = state_of(w);
  a.live = w->live.as<double>();
  a.Ls = w->liveL.as<double>();
  a.nlive = w->nlive;
  a.dirkind = dirkind;
  a.dd = dir_data(w);
  a.tkind = tkind;
  a.ta = ta;
  a.tb = tb;
  a.lkind = lkind;
  a.aux = w->aux.as<double>();
  a.sigma = sigma;
  a.ly = layer_of(w);
  a.was_starting = w->flags.as<uint8_t>();
  a.sp = w->r_sp.as<StepParams>();
  a.ring = w->ring.as<long long>();
  a.ctl = w->r_ctl.as<int>();
  a.rflags = w->r_flags.as<uint8_t>();
  a.rdist2 = w->r_dist2.as<double>();
  a.rlast = w->r_last.as<int>();
  a.rparts = nchunks > 1 ? w->r_parts.as<double>() : nullptr;
  a.force_memory_form = force_memory_form;
  a.rec = w->r_out.as<double>();
  a.rows = w->r_out.as<double>() + nrec;
  a.max_rounds = max_rounds;
  a.per_call = philox_per_call(w);
  // the values that change from call to call (threshold, scale, seed, offset) travel through the pinned parameter block
  std::vector<unsigned long long> key = step_key(w, dirkind, ev);
  key.insert(key.end(), {(unsigned long long)max_rounds, (unsigned long long)force_memory_form, (unsigned long long)nout,
                         bits(w->r2), addr(w->r_out.p), addr(w->r_flags.p), addr(w->r_dist2.p), addr(w->r_last.p),
                         addr(w->r_parts.p), addr(w->r_ctl.p), addr(w->r_sp.p), addr(w->h_rout), addr(w->h_rsp),
                         addr(w->flags.p), addr(w->ring.p)});
  if (int rc = replay(w->rounds_graph, std::move(key), s, [&](hipStream_t s) -> int {
        CK(hipMemcpyAsync(w->r_sp.p, w->h_rsp, sizeof(StepParams), hipMemcpyHostToDevice, s));
        launch_walk_rounds(a, s);
        CK(hipMemcpyAsync(w->h_rout, w->r_out.p, nout * sizeof(double), hipMemcpyDeviceToHost, s));
        return 0;
      }))
    return rc;
  const int R = (int)w->h_rout[4];
  if (w->h_rout[5] != 0.0) return fail_arg(MLF_E_STATE, "mlf_walkers_rounds_dev: a walker gave up waiting for the ring walker's rounds");
  if (R < 1 || R > max_rounds) return fail_arg(MLF_E_STATE, "mlf_walkers_rounds_dev: the device reported an impossible round count");
  memcpy(rec, w->h_rout, nrec * sizeof(double));
  memcpy(round_rows, w->h_rout + nrec, (size_t)R * 5 * sizeof(double));
  *rounds = R;
  *next_offset = offset + (uint64_t)R * a.per_call;
  return 0;
}

int mlf_walkers_export(mlf_walkers *w, double *allu, double *allL, int64_t *generation, double *currentt,
                       double *currentv, double *left, double *right, uint8_t *sl, uint8_t *sr) {
  if (!w) return fail_arg(MLF_E_BADARG, "null pointer");
  hipStream_t s = ctx_stream();
  const size_t P = (size_t)w->P, G = (size_t)w->nsteps + 1, d = (size_t)w->d;
  if (allu) CK(hipMemcpyAsync(allu, w->allu.p, P * G * d * 8, hipMemcpyDeviceToHost, s));
  if (allL) CK(hipMemcpyAsync(allL, w->allL.p, P * G * 8, hipMemcpyDeviceToHost, s));
  if (generation) CK(hipMemcpyAsync(generation, w->generation.p, P * 8, hipMemcpyDeviceToHost, s));
  if (currentt) CK(hipMemcpyAsync(currentt, w->currentt.p, P * 8, hipMemcpyDeviceToHost, s));
  if (currentv) CK(hipMemcpyAsync(currentv, w->currentv.p, P * d * 8, hipMemcpyDeviceToHost, s));
  if (left) CK(hipMemcpyAsync(left, w->left.p, P * 8, hipMemcpyDeviceToHost, s));
  if (right) CK(hipMemcpyAsync(right, w->right.p, P * 8, hipMemcpyDeviceToHost, s));
  if (sl) CK(hipMemcpyAsync(sl, w->sl.p, P, hipMemcpyDeviceToHost, s));
  if (sr) CK(hipMemcpyAsync(sr, w->sr.p, P, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return 0;
}

// ---- PopulationRandomWalkSampler's refill -----------------------------------------------------------
int mlf_rwalk_create(mlf_rwalk **out, size_t popsize, size_t nsteps, size_t d) {
  if (!out) return fail_arg(MLF_E_BADARG, "null pointer");
  *out = nullptr;
  if (popsize == 0 || nsteps == 0 || d == 0) return fail_arg(MLF_E_BADARG, "mlf_rwalk_create: popsize, nsteps, d must be positive");
  if (d > MLF_MAX_DIM)
    return fail_arg(MLF_E_DIM, "the random-walk population (one wave per walker, the lanes striding over the row) covers up to MLF_MAX_DIM = 1024 dimensions");
  // walker * nsteps + step and walker * d + coordinate are ints on the device
  if (popsize > (1u << 24) || nsteps > 65535 || popsize * nsteps > 0x7fffffffull || popsize * d > 0x7fffffffull)
    return fail_arg(MLF_E_BADARG, "mlf_rwalk_create: population too large");
  if (int rc = ensure_ctx()) return rc;
  mlf_rwalk *w = new mlf_rwalk();
  w->P = (int)popsize;
  w->nsteps = (int)nsteps;
  w->d = (int)d;
  const size_t P = popsize;
  struct {
    DevBuf *b;
    size_t bytes;
  } plan[] = {{&w->u, P * d * 8},    {&w->p, P * d * 8},    {&w->L, P * 8},      {&w->start, P * 8}, {&w->ever, P},
              {&w->last, P},         {&w->rej, P * 4},      {&w->tl, P * 8},     {&w->tr, P * 8},    {&w->dist2, P * 8},
              {&w->unew, P * d * 8}, {&w->pnew, P * d * 8}, {&w->Lnew, P * 8},   {&w->inside, P},    {&w->aux, d * 8},
              {&w->parts, ((P + 1023) / 1024) * kRwalkOut * 8},                  {&w->out, kRwalkOut * 8}};
  for (auto &e : plan) {
    hipError_t err = e.b->reserve(e.bytes);
    if (err != hipSuccess) {
      mlf_rwalk_destroy(w);
      return fail_hip(err, "device allocation for the random-walk population", "mlf_walk_api.hip", __LINE__);
    }
  }
  *out = w;
  return 0;
}

int mlf_rwalk_destroy(mlf_rwalk *w) {
  if (!w) return 0;
  for (DevBuf *b : w->all) b->release();
  w->release_copies();
  delete w;
  return 0;
}

int mlf_rwalk_set_layer(mlf_rwalk *w, int kind, const double *ctr, const double *mat, const double *wrap, double maxradiussq) {
  if (!w) return fail_arg(MLF_E_BADARG, "null pointer");
  return set_layer(w, kind, ctr, mat, wrap, maxradiussq);
}

int mlf_rwalk_set_direction_data(mlf_rwalk *w, const double *axes, const double *live, size_t nlive, const double *std) {
  if (!w) return fail_arg(MLF_E_BADARG, "null pointer");
  return set_direction_data(w, axes, live, nlive, std);
}

int mlf_rwalk_set_live(mlf_rwalk *w, const double *us, const double *Ls, size_t nlive) {
  if (!w || !us || !Ls) return fail_arg(MLF_E_BADARG, "null pointer");
  return set_live(w, us, Ls, nlive);
}

int mlf_rwalk_refill_dev(mlf_rwalk *w, double Lmin, int dirkind, double dirscale, uint64_t seed, uint64_t offset, int tkind,
                         double ta, double tb, int lkind, const double *aux, double sigma, int form, double *out_u,
                         double *out_p, double *out_L, int64_t *out_start, uint8_t *out_ever, uint8_t *out_last,
                         double *out_tleft, double *out_tright, double *counts, uint64_t *next_offset) {
  return rwalk_refill(w, Lmin, dirkind, dirscale, seed, offset, StepEval{nullptr, tkind, ta, tb, lkind, aux, sigma}, form,
                      RwalkOut{out_u, out_p, out_L, out_start, out_ever, out_last, out_tleft, out_tright, counts}, next_offset);
}

int mlf_rwalk_refill_user(mlf_rwalk *w, double Lmin, int dirkind, double dirscale, uint64_t seed, uint64_t offset,
                          mlf_usermodel *model, double *out_u, double *out_p, double *out_L, int64_t *out_start,
                          uint8_t *out_ever, uint8_t *out_last, double *out_tleft, double *out_tright, double *counts,
                          uint64_t *next_offset) {
  if (!model) return fail_arg(MLF_E_BADARG, "null pointer");
  return rwalk_refill(w, Lmin, dirkind, dirscale, seed, offset, StepEval{model}, 1,
                      RwalkOut{out_u, out_p, out_L, out_start, out_ever, out_last, out_tleft, out_tright, counts}, next_offset);
}

// ---- PopulationSimpleSliceSampler's refill ----------------------------------------------------------
int mlf_sslice_create(mlf_sslice **out, size_t popsize, size_t nsteps, size_t d, size_t max_it) {
  if (!out) return fail_arg(MLF_E_BADARG, "null pointer");
  *out = nullptr;
  if (popsize == 0 || nsteps == 0 || d == 0 || max_it == 0)
    return fail_arg(MLF_E_BADARG, "mlf_sslice_create: popsize, nsteps, d, max_it must be positive");
  if (d > MLF_MAX_DIM)
    return fail_arg(MLF_E_DIM, "the simple slice population (one wave per worker, the lanes striding over the row) covers up to MLF_MAX_DIM = 1024 dimensions");
  // point * nsteps + step, point * d + coordinate and nsteps * max_it are ints on the device or the host
  if (popsize > (1u << 24) || nsteps > 65535 || max_it > 65535 || popsize * nsteps > 0x7fffffffull || popsize * d > 0x7fffffffull ||
      nsteps * max_it > 0x7fffffffull)
    return fail_arg(MLF_E_BADARG, "mlf_sslice_create: population too large");
  if (int rc = ensure_ctx()) return rc;
  mlf_sslice *w = new mlf_sslice();
  w->P = (int)popsize;
  w->nsteps = (int)nsteps;
  w->d = (int)d;
  w->max_it = (int)max_it;
  const size_t P = popsize;
  struct {
    DevBuf *b;
    size_t bytes;
  } plan[] = {{&w->u, P * d * 8},    {&w->p, P * d * 8},      {&w->L, P * 8},          {&w->start, P * 8},
              {&w->v, P * d * 8},    {&w->tl, P * 8},         {&w->tr, P * 8},         {&w->status, P},
              {&w->zlist, P * 4},    {&w->taken, P * 4},      {&w->taken_it, P * 4},   {&w->t, P * 8},
              {&w->unew, P * d * 8}, {&w->pnew, P * d * 8},   {&w->Lnew, P * 8},       {&w->member, P},
              {&w->widths, nsteps * P * 8},                   {&w->iters, nsteps * 4}, {&w->dist2, P * 8},
              {&w->nanrow, P},       {&w->ctl, sizeof(SsliceCtl)},                     {&w->dirscale, nsteps * 8},
              {&w->aux, d * 8},      {&w->out, kSsliceOut * 8}};
  hipError_t err = hipHostMalloc((void **)&w->h_ctl, sizeof(SsliceCtl), hipHostMallocDefault);
  for (auto &e : plan)
    if (err == hipSuccess) err = e.b->reserve(e.bytes);
  if (err != hipSuccess) {
    mlf_sslice_destroy(w);
    return fail_hip(err, "allocation for the simple slice population", "mlf_walk_api.hip", __LINE__);
  }
  *out = w;
  return 0;
}

int mlf_sslice_destroy(mlf_sslice *w) {
  if (!w) return 0;
  for (DevBuf *b : w->all) b->release();
  w->release_copies();
  if (w->h_ctl) (void)hipHostFree(w->h_ctl);
  delete w;
  return 0;
}

int mlf_sslice_set_layer(mlf_sslice *w, int kind, const double *ctr, const double *mat, const double *wrap, double maxradiussq) {
  if (!w) return fail_arg(MLF_E_BADARG, "null pointer");
  return set_layer(w, kind, ctr, mat, wrap, maxradiussq);
}

int mlf_sslice_set_direction_data(mlf_sslice *w, const double *axes, const double *live, size_t nlive, const double *std) {
  if (!w) return fail_arg(MLF_E_BADARG, "null pointer");
  return set_direction_data(w, axes, live, nlive, std);
}

int mlf_sslice_set_live(mlf_sslice *w, const double *us, const double *Ls, size_t nlive) {
  if (!w || !us || !Ls) return fail_arg(MLF_E_BADARG, "null pointer");
  return set_live(w, us, Ls, nlive);
}

int mlf_sslice_refill_dev(mlf_sslice *w, double Lmin, int dirkind, const double *dirscale, int limit, double shrink,
                          uint64_t seed, uint64_t offset, int slots_per_poll, int tkind, double ta, double tb, int lkind,
                          const double *aux, double sigma, double *out_u, double *out_p, double *out_L, int64_t *out_start,
                          double *out_tleft, double *out_tright, int32_t *out_taken, int32_t *out_taken_it, int32_t *out_iters,
                          double *out_widths, double *counts, uint64_t *next_offset) {
  return sslice_refill(w, Lmin, dirkind, dirscale, limit, shrink, seed, offset, StepEval{nullptr, tkind, ta, tb, lkind, aux, sigma},
                       slots_per_poll,
                       SsliceOut{out_u, out_p, out_L, out_start, out_tleft, out_tright, out_taken, out_taken_it, out_iters,
                                 out_widths, counts},
                       next_offset);
}

int mlf_sslice_refill_user(mlf_sslice *w, double Lmin, int dirkind, const double *dirscale, int limit, double shrink,
                           uint64_t seed, uint64_t offset, int slots_per_poll, mlf_usermodel *model, double *out_u,
                           double *out_p, double *out_L, int64_t *out_start, double *out_tleft, double *out_tright,
                           int32_t *out_taken, int32_t *out_taken_it, int32_t *out_iters, double *out_widths, double *counts,
                           uint64_t *next_offset) {
  if (!model) return fail_arg(MLF_E_BADARG, "null pointer");
  return sslice_refill(w, Lmin, dirkind, dirscale, limit, shrink, seed, offset, StepEval{model}, slots_per_poll,
                       SsliceOut{out_u, out_p, out_L, out_start, out_tleft, out_tright, out_taken, out_taken_it, out_iters,
                                 out_widths, counts},
                       next_offset);
}

// ------------------------------------------------------------------ stateless forms ------------
int mlf_within_unit_cube(const double *u, size_t n, size_t d, uint8_t *out) {
  if (n == 0) return 0;
  if (!u || !out) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = check_nd(n, d)) return rc;
  if (int rc = ensure_ctx()) return rc;
  hipStream_t s = ctx_stream();
  if (int rc = upload(g_s.a, u, n * d * 8, s)) return rc;
  CK(g_s.b.reserve(n));
  launch_within_unit_cube(g_s.a.as<double>(), (int)n, (int)d, g_s.b.as<uint8_t>(), s);
  CK(hipGetLastError());
  if (int rc = download(out, g_s.b, n, s)) return rc;
  CK(hipStreamSynchronize(s));
  return 0;
}

int mlf_evolve_propose(const double *currentu, const double *currentv, const double *left, const double *right,
                       const uint8_t *sl, const uint8_t *sr, const double *unif_full, double *currentt, size_t n,
                       size_t d, double *unew, uint8_t *acceptable) {
  if (n == 0) return 0;
  if (!currentu || !currentv || !left || !right || !sl || !sr || !currentt || !unew || !acceptable)
    return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = check_nd(n, d)) return rc;
  if (int rc = ensure_ctx()) return rc;
  hipStream_t s = ctx_stream();
  if (int rc = upload(g_s.a, currentu, n * d * 8, s)) return rc;
  if (int rc = upload(g_s.b, currentv, n * d * 8, s)) return rc;
  if (int rc = upload(g_s.c, left, n * 8, s)) return rc;
  if (int rc = upload(g_s.d, right, n * 8, s)) return rc;
  if (int rc = upload(g_s.e, sl, n, s)) return rc;
  if (int rc = upload(g_s.f, sr, n, s)) return rc;
  if (int rc = upload(g_s.g, currentt, n * 8, s)) return rc;
  if (unif_full) {
    if (int rc = upload(g_s.h, unif_full, n * 8, s)) return rc;
    launch_bisect_draw(g_s.c.as<double>(), g_s.d.as<double>(), g_s.e.as<uint8_t>(), g_s.f.as<uint8_t>(),
                       g_s.h.as<double>(), (int)n, g_s.g.as<double>(), s);
  }
  CK(g_s.i.reserve(n * d * 8));
  CK(g_s.j.reserve(n));
  launch_evolve_propose(g_s.a.as<double>(), g_s.b.as<double>(), g_s.c.as<double>(), g_s.d.as<double>(),
                        g_s.e.as<uint8_t>(), g_s.f.as<uint8_t>(), g_s.g.as<double>(), (int)n, (int)d,
                        g_s.i.as<double>(), s);
  launch_within_unit_cube(g_s.i.as<double>(), (int)n, (int)d, g_s.j.as<uint8_t>(), s);
  CK(hipGetLastError());
  if (int rc = download(currentt, g_s.g, n * 8, s)) return rc;
  if (int rc = download(unew, g_s.i, n * d * 8, s)) return rc;
  if (int rc = download(acceptable, g_s.j, n, s)) return rc;
  CK(hipStreamSynchronize(s));
  return 0;
}

int mlf_evolve_update(const uint8_t *acceptable, const double *Lnew_full, double Lmin, double *currentt, double *left,
                      double *right, uint8_t *sl, uint8_t *sr, uint8_t *success, size_t n) {
  if (n == 0) return 0;
  if (!acceptable || !Lnew_full || !currentt || !left || !right || !sl || !sr || !success)
    return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = check_nd(n, 1)) return rc;
  if (int rc = ensure_ctx()) return rc;
  hipStream_t s = ctx_stream();
  if (int rc = upload(g_s.a, acceptable, n, s)) return rc;
  if (int rc = upload(g_s.b, Lnew_full, n * 8, s)) return rc;
  if (int rc = upload(g_s.c, currentt, n * 8, s)) return rc;
  if (int rc = upload(g_s.d, left, n * 8, s)) return rc;
  if (int rc = upload(g_s.e, right, n * 8, s)) return rc;
  if (int rc = upload(g_s.f, sl, n, s)) return rc;
  if (int rc = upload(g_s.g, sr, n, s)) return rc;
  CK(g_s.h.reserve(n));
  launch_evolve_update(g_s.a.as<uint8_t>(), g_s.b.as<double>(), Lmin, g_s.c.as<double>(), g_s.d.as<double>(),
                       g_s.e.as<double>(), g_s.f.as<uint8_t>(), g_s.g.as<uint8_t>(), g_s.h.as<uint8_t>(), (int)n, s);
  CK(hipGetLastError());
  if (int rc = download(currentt, g_s.c, n * 8, s)) return rc;
  if (int rc = download(left, g_s.d, n * 8, s)) return rc;
  if (int rc = download(right, g_s.e, n * 8, s)) return rc;
  if (int rc = download(sl, g_s.f, n, s)) return rc;
  if (int rc = download(sr, g_s.g, n, s)) return rc;
  if (int rc = download(success, g_s.h, n, s)) return rc;
  CK(hipStreamSynchronize(s));
  return 0;
}

int mlf_step_back(double Lmin, double *allL, size_t n, size_t ngen, int64_t *generation, double *currentt) {
  if (n == 0) return 0;
  if (!allL || !generation || !currentt) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = check_nd(n, ngen)) return rc;
  if (int rc = ensure_ctx()) return rc;
  hipStream_t s = ctx_stream();
  if (int rc = upload(g_s.a, allL, n * ngen * 8, s)) return rc;
  if (int rc = upload(g_s.b, generation, n * 8, s)) return rc;
  if (int rc = upload(g_s.c, currentt, n * 8, s)) return rc;
  CK(g_s.d.reserve(8));
  launch_step_back(Lmin, g_s.a.as<double>(), (int)n, (int)ngen, g_s.b.as<long long>(), g_s.c.as<double>(),
                   g_s.d.as<long long>(), s);
  CK(hipGetLastError());
  if (int rc = download(allL, g_s.a, n * ngen * 8, s)) return rc;
  if (int rc = download(generation, g_s.b, n * 8, s)) return rc;
  if (int rc = download(currentt, g_s.c, n * 8, s)) return rc;
  CK(hipStreamSynchronize(s));
  return 0;
}

int mlf_unitcube_line_intersection(const double *origin, const double *direction, size_t n, size_t d, double *tleft,
                                   double *tright) {
  if (n == 0) return 0;
  if (!origin || !direction || !tleft || !tright) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = check_nd(n, d)) return rc;
  if (int rc = ensure_ctx()) return rc;
  hipStream_t s = ctx_stream();
  if (int rc = upload(g_s.a, origin, n * d * 8, s)) return rc;
  if (int rc = upload(g_s.b, direction, n * d * 8, s)) return rc;
  CK(g_s.c.reserve(n * 8));
  CK(g_s.d.reserve(n * 8));
  launch_line_intersection(g_s.a.as<double>(), g_s.b.as<double>(), (int)n, (int)d, g_s.c.as<double>(),
                           g_s.d.as<double>(), s);
  CK(hipGetLastError());
  if (int rc = download(tleft, g_s.c, n * 8, s)) return rc;
  if (int rc = download(tright, g_s.d, n * 8, s)) return rc;
  CK(hipStreamSynchronize(s));
  return 0;
}

int mlf_update_vectorised_slice_sampler(const double *t, double *tleft, double *tright, const double *proposed_L,
                                        const double *proposed_u, const double *proposed_p, int64_t *worker_running,
                                        int64_t *status, double threshold, double shrink_factor, double *allu,
                                        double *allL, double *allp, size_t popsize, size_t d, size_t nparams,
                                        int64_t *discarded) {
  if (!discarded) return fail_arg(MLF_E_BADARG, "null pointer");
  *discarded = 0;
  if (popsize == 0) return 0;
  if (!t || !tleft || !tright || !proposed_L || !proposed_u || !proposed_p || !worker_running || !status || !allu ||
      !allL || !allp)
    return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = check_nd(popsize, d > nparams ? d : nparams)) return rc;
  for (size_t l = 0; l < popsize; ++l)
    if (worker_running[l] < 0 || (size_t)worker_running[l] >= popsize)
      return fail_arg(MLF_E_BADARG, "worker_running entry out of range");
  if (int rc = ensure_ctx()) return rc;
  hipStream_t s = ctx_stream();
  const size_t P = popsize;
  if (int rc = upload(g_s.a, t, P * 8, s)) return rc;
  if (int rc = upload(g_s.b, tleft, P * 8, s)) return rc;
  if (int rc = upload(g_s.c, tright, P * 8, s)) return rc;
  if (int rc = upload(g_s.d, proposed_L, P * 8, s)) return rc;
  if (int rc = upload(g_s.e, proposed_u, P * d * 8, s)) return rc;
  if (int rc = upload(g_s.f, proposed_p, P * nparams * 8, s)) return rc;
  if (int rc = upload(g_s.g, worker_running, P * 8, s)) return rc;
  if (int rc = upload(g_s.h, status, P * 8, s)) return rc;
  if (int rc = upload(g_s.i, allu, P * d * 8, s)) return rc;
  if (int rc = upload(g_s.j, allL, P * 8, s)) return rc;
  if (int rc = upload(g_s.k, allp, P * nparams * 8, s)) return rc;
  CK(g_s.l.reserve((P + 1) * 8));
  launch_slice_update(g_s.a.as<double>(), g_s.b.as<double>(), g_s.c.as<double>(), g_s.d.as<double>(),
                      g_s.e.as<double>(), g_s.f.as<double>(), g_s.g.as<long long>(), g_s.h.as<long long>(), threshold,
                      shrink_factor, g_s.i.as<double>(), g_s.j.as<double>(), g_s.k.as<double>(), (int)P, (int)d,
                      (int)nparams, g_s.l.as<long long>(), s);
  CK(hipGetLastError());
  if (int rc = download(tleft, g_s.b, P * 8, s)) return rc;
  if (int rc = download(tright, g_s.c, P * 8, s)) return rc;
  if (int rc = download(worker_running, g_s.g, P * 8, s)) return rc;
  if (int rc = download(status, g_s.h, P * 8, s)) return rc;
  if (int rc = download(allu, g_s.i, P * d * 8, s)) return rc;
  if (int rc = download(allL, g_s.j, P * 8, s)) return rc;
  if (int rc = download(allp, g_s.k, P * nparams * 8, s)) return rc;
  if (int rc = download(discarded, g_s.l, 8, s)) return rc;
  CK(hipStreamSynchronize(s));
  return 0;
}

int mlf_row_dist2(const double *a, const double *b, size_t n, size_t d, double *out) {
  if (n == 0) return 0;
  if (!a || !b || !out) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = check_nd(n, d)) return rc;
  if (int rc = ensure_ctx()) return rc;
  hipStream_t s = ctx_stream();
  if (int rc = upload(g_s.a, a, n * d * 8, s)) return rc;
  if (int rc = upload(g_s.b, b, n * d * 8, s)) return rc;
  CK(g_s.c.reserve(n * 8));
  launch_row_dist2(g_s.a.as<double>(), g_s.b.as<double>(), (int)n, (int)d, g_s.c.as<double>(), s);
  CK(hipGetLastError());
  if (int rc = download(out, g_s.c, n * 8, s)) return rc;
  CK(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
