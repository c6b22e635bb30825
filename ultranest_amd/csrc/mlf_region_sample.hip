// mlf_region_sample.hip -- MLFriends.sample and the refill of the live points on the device: draw a batch, run it through
// the region's tests, compact, evaluate, keep what lies above the threshold.  Host code only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/mlfriends_hip.h"
#include "mlf_host.hpp"
#include "mlf_sample.hpp"

namespace {

using namespace mlf;

// neighbour test of t-space points against the resident live points (MFMA pre-filter when it applies)
int region_scan_mask(mlf_region *r, const double *d_t, long long np, uint8_t *d_mask, hipStream_t s) {
  if (int rc = filter_refresh_refs(r->filter, r->refR.as<double>(), r->n, r->d, r->dp, s)) return rc;
  const BatchPlan p = plan_batch(r->filter, r, BATCH_TSPACE, np, r->r2);
  if (p.filter)
    return filter_run({r->filter, p, region_live(r), d_t, (long long)r->d, 1, np, nullptr, d_mask, nullptr, s, nullptr, nullptr});
  ScanArgs a = scan_args(region_live(r), d_t, r->d, 0, np, SCAN_MASK);
  a.out_mask = d_mask;
  CK(launch_scan(r->dp, a, s));
  return 0;
}

// methods 2 and 3 after the draw: w = t . invT + ctr (+ unwrap) of `n` t-space rows, gate = w inside the unit cube and the
// wrapping ellipsoid
int region_cube_gate(mlf_region *r, const double *t, long long n, double *w, uint8_t *gate, hipStream_t s) {
  uint8_t *in_cube = r->cube.as<uint8_t>();
  const double *wrap = r->has_wrap ? r->wrap.as<double>() : nullptr;
  if (r->d <= 128 && r->s_invT_pad.p)
    CK(launch_rows_affine(t, n, r->d, r->s_invT_pad.as<double>(), r->lay_ctr.as<double>(), wrap, w, in_cube, s));
  else
    launch_untransform_rows(t, n, r->d, r->s_invT.as<double>(), r->lay_ctr.as<double>(), wrap, w, in_cube, s);
  CK(hipGetLastError());
  if (int rc = region_ellipsoid_gate(r, w, (size_t)n, gate, s)) return rc;
  launch_mask_and(gate, in_cube, n, s);
  return 0;
}

// what region_draw leaves on the device: n rows of d doubles in cube space, accepted where member[i] != 0 (n = 0: none)
struct Drawn {
  const double *rows = nullptr;
  const uint8_t *member = nullptr;
  long long n = 0;
};

// MLFriends.sample on the device: `nsamples` proposals of `method` (0 cube, 1 wrapping ellipsoid, 2 t-space box, 3 around the live
// points) from Philox counter `offset` on, through the region's tests; *next_offset = the first counter not used.  The batch stays
// on the device as its last stage left it, not compacted; r->blk holds the offsets of any mask of up to nsamples rows.
int region_draw(mlf_region *r, int method, size_t nsamples, uint64_t seed, uint64_t offset, Drawn *b, uint64_t *next_offset) {
  if (!r || !next_offset) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!r->ready) return fail_arg(MLF_E_STATE, "region used before mlf_region_set");
  if (method < 0 || method > 3)
    return fail_arg(MLF_E_BADARG, "method must be 0 (cube), 1 (wrapping ellipsoid), 2 (t-space box) or 3 (live points)");
  if (method == 1 && !r->axes_ready) return fail_arg(MLF_E_STATE, "mlf_region_set_axes not called");
  if (method >= 2 && (!r->use_scan || !r->sampling_ready))
    return fail_arg(MLF_E_STATE, "mlf_region_set_sampling_data not called (or region without live points)");
  *b = Drawn{};
  *next_offset = offset;
  if (nsamples == 0) return 0;
  hipStream_t s = g_ctx.stream;
  const long long n = (long long)nsamples;
  const int d = r->d;
  CK(r->gen.reserve((size_t)n * d * sizeof(double)));
  CK(r->smask.reserve((size_t)n));
  CK(r->blk.reserve(((size_t)(n + 255) / 256 + 1) * sizeof(unsigned)));
  double *gen = r->gen.as<double>();
  uint8_t *mask = r->smask.as<uint8_t>();
  if (method == 0) {
    CK(launch_generate_cube(gen, n * d, seed, offset, s));
    *next_offset = offset + (uint64_t)((n * d + 1) / 2);
    if (int rc = region_inside_enqueue(r, gen, nsamples, mask, s, nullptr, nullptr, nullptr)) return rc;
    *b = {gen, mask, n};
    return 0;
  }
  CK(r->cube.reserve((size_t)n));
  if (method == 1) {
    *next_offset = offset + (uint64_t)n * (uint64_t)((d + 1) / 2 + 1);
    if (d <= 128 && r->ax_pad.p) {   // draws, axes product, centre and cube test in one launch: the batch is written once
      CK(launch_generate_ellipsoid(gen, n, d, r->enlarge, r->ax_pad.as<double>(), r->ell_ctr.as<double>(), r->cube.as<uint8_t>(),
                                   seed, offset, s));
    } else {
      CK(r->gen2.reserve((size_t)n * d * sizeof(double)));
      CK(launch_generate_ball(r->gen2.as<double>(), n, d, r->enlarge, seed, offset, s));
      PrepArgs pa{};
      pa.pts = r->gen2.as<double>();
      pa.np = n;
      pa.d = d;
      pa.do_tr = 1;
      pa.lay_ctr = r->ax_zero.as<double>();
      pa.lay_Tt = r->ax_mat.as<double>();
      pa.t_out = gen;
      pa.ldt = d;
      CK(launch_prep(r->dp, pa, s));
      launch_center_and_cube(gen, n, d, r->ell_ctr.as<double>(), r->cube.as<uint8_t>(), s);
      CK(hipGetLastError());
    }
    if (int rc = region_inside_enqueue(r, gen, nsamples, mask, s, nullptr, nullptr, r->cube.as<uint8_t>())) return rc;
    *b = {gen, mask, n};
    return 0;
  }
  // methods 2 and 3: proposals are born in t-space
  CK(r->gen2.reserve((size_t)n * d * sizeof(double)));
  if (method == 2) {
    CK(launch_generate_tbox(gen, n, d, r->s_lo.as<double>(), r->s_hi.as<double>(), std::sqrt(r->r2), seed, offset, s));
    *next_offset = offset + (uint64_t)((n * d + 1) / 2);
    if (int rc = region_scan_mask(r, gen, n, mask, s)) return rc;
    // survivors of the neighbour test, compacted; everything after works on those rows only
    const Compaction nearby(mask, n, r->blk.as<unsigned>(), s);
    nearby.scatter(gen, d, r->gen2.as<double>(), nsamples);
    size_t k1 = 0;
    CK(nearby.count(nsamples, &k1));
    if (k1 == 0) return 0;
    // the t-space batch is not needed any more: gen takes the cube-space rows
    if (int rc = region_cube_gate(r, r->gen2.as<double>(), (long long)k1, gen, mask, s)) return rc;
    *b = {gen, mask, (long long)k1};
    return 0;
  }
  // Method 3.  Reference order (:1072-1094, :1154-1160): multiplicity of every proposal -> thinning -> untransform -> cube and
  // ellipsoid tests.  Every one of these is a function of the proposal alone (the thinning uniform is drawn with it), so the
  // accepted set does not depend on their order: the cheap tests run FIRST, on the whole batch (untransform + cube 0.2 ms,
  // ellipsoid 0.15 ms per 2^20 x 50), and the multiplicity -- the exact count over all live points, 22 ms for the whole batch, the
  // one stage that cannot stop at the first hit -- is taken of their survivors only (a few per cent at C5).
  CK(r->s_thin.reserve((size_t)n * sizeof(double)));
  CK(r->s_gate.reserve((size_t)n));
  CK(launch_generate_around_points(gen, r->s_thin.as<double>(), n, d, r->refR.as<double>(), r->n, r->dp, r->r2, seed, offset, s));
  *next_offset = offset + (uint64_t)n * (uint64_t)((d + 1) / 2 + 2);
  double *wall = r->gen2.as<double>();
  if (int rc = region_cube_gate(r, gen, n, wall, r->s_gate.as<uint8_t>(), s)) return rc;
  const Compaction cheap(r->s_gate.as<uint8_t>(), n, r->blk.as<unsigned>(), s);
  size_t k0 = 0;
  CK(cheap.count(nsamples, &k0));
  if (k0 == 0) return 0;
  CK(r->s_tc.reserve(k0 * d * sizeof(double)));
  CK(r->s_wc.reserve(k0 * d * sizeof(double)));
  CK(r->s_thc.reserve(k0 * sizeof(double)));
  CK(r->s_count.reserve(k0 * sizeof(long long)));
  cheap.scatter(gen, d, r->s_tc.as<double>(), k0);
  cheap.scatter(wall, d, r->s_wc.as<double>(), k0);
  cheap.scatter(r->s_thin.as<double>(), 1, r->s_thc.as<double>(), k0);
  // multiplicity: how many balls contain the proposal (no early exit, reference :1087-1088)
  ScanArgs a = scan_args(region_live(r), r->s_tc.as<double>(), d, 0, (long long)k0, SCAN_COUNT);
  a.out_idx = r->s_count.as<long long>();
  CK(launch_scan(r->dp, a, s));
  launch_thin_by_multiplicity(r->s_count.as<long long>(), r->s_thc.as<double>(), (long long)k0, mask, s);
  CK(hipGetLastError());
  *b = {r->s_wc.as<double>(), mask, (long long)k0};
  return 0;
}

// the t-region of the handle as a gated launch reads it
TregionGate region_tregion(const mlf_region *r) {
  return {r->tr_A.as<double>(), r->tr_ctr.as<double>(), r->tr_fixed.as<double>(), r->tr_enlarge, r->rf_member2.as<uint8_t>()};
}

// the body of mlf_region_refill / mlf_region_refill_user: `evaluate(rows, member, n, p_buf, L_buf, s, &prow)` enqueues the prior
// transform and the likelihood of the n rows (p into p_buf, or *prow = rows for the identity; L into L_buf).  With a t-region on
// the handle, evaluate also fills r->rf_member2 = member && inside(p) (region_tregion): that mask replaces the membership
// mask from there on and its count is *nevaluated; the choice between the two routes keeps using the region's count.
// derive (a derive handle, or none): out_p receives the kept rows as [p | q], d + nderived wide (mlf_region_refill_user_derived,
// mlf_region_refill_user_derived_gated).
template <class Evaluate>
int region_refill(mlf_region *r, int method, size_t nsamples, uint64_t seed, uint64_t offset, double Lmin, Evaluate evaluate,
                  double *out_u, double *out_p, double *out_L, size_t capacity, size_t *nevaluated, size_t *nkept,
                  uint64_t *next_offset, const mlf_usermodel *derive = nullptr) {
  *nevaluated = 0;
  *nkept = 0;
  Drawn b;
  if (int rc = region_draw(r, method, nsamples, seed, offset, &b, next_offset)) return rc;
  if (b.n == 0) return 0;
  hipStream_t s = g_ctx.stream;
  const int d = r->d;
  // The accepted count first.  A batch drawn in the cube (methods 0 and 1) with at least a quarter of it accepted is evaluated
  // where it was drawn: the prior transform and the likelihood run over all its rows (a rejected row costs a wasted evaluation,
  // no copy) and the threshold cut keeps accepted rows only, so rows, order and values are those of the compacted route.  Any
  // other batch is compacted before the evaluation.
  const Compaction accepted(b.member, b.n, r->blk.as<unsigned>(), s);
  size_t nacc = 0;
  CK(accepted.count(nsamples, &nacc));
  *nevaluated = nacc;
  if (nacc == 0 || capacity == 0) return 0;
  if (method >= 2 || nacc * 4 < nsamples) {
    CK(r->sout.reserve(nsamples * d * sizeof(double)));
    accepted.scatter(b.rows, d, r->sout.as<double>(), nacc);
    b = {r->sout.as<double>(), nullptr, (long long)nacc};
  }
  const long long n = b.n;
  CK(r->rf_p.reserve((size_t)n * d * sizeof(double)));
  CK(r->rf_L.reserve((size_t)n * sizeof(double)));
  CK(r->rf_out.reserve(capacity * (2 * (size_t)d + 1) * sizeof(double)));
  CK(r->rf_keep.reserve((size_t)n));
  if (r->tr_on) CK(r->rf_member2.reserve((size_t)n));
  // prior transform + likelihood on the accepted proposals, where they are (reference _refill_samples,
  // integrator.py:1789-1804); only the points above the threshold travel to the host
  const double *prow = b.rows;   // identity transform: the parameters ARE the cube coordinates, no copy
  if (int rc = evaluate(b.rows, b.member, n, r->rf_p.as<double>(), r->rf_L.as<double>(), s, &prow)) return rc;
  const uint8_t *counted = b.member;
  if (r->tr_on) {
    counted = r->rf_member2.as<uint8_t>();
    const Compaction gated(counted, n, r->blk.as<unsigned>(), s);
    size_t ngated = 0;
    CK(gated.count(nsamples, &ngated));
    *nevaluated = ngated;
    if (ngated == 0) return 0;
  }
  uint8_t *keep = r->rf_keep.as<uint8_t>();
  launch_mask_greater(r->rf_L.as<double>(), n, Lmin, keep, s, counted);
  double *ou = r->rf_out.as<double>(), *op = ou + capacity * (size_t)d, *oL = op + capacity * (size_t)d;
  const Compaction kept(keep, n, r->blk.as<unsigned>(), s);   // one count + scan for the three arrays
  kept.scatter(b.rows, d, ou, capacity);
  kept.scatter(prow, d, op, capacity);
  kept.scatter(r->rf_L.as<double>(), 1, oL, capacity);
  size_t take = 0;
  CK(kept.count(capacity, &take));
  size_t pw = (size_t)d;   // width of a row of out_p
  if (take && derive) {    // derived parameters: [p | q] of the kept rows, the only rows that leave (no row above changes width)
    pw += (size_t)usermodel_nderived(derive);
    CK(r->rf_wide.reserve(take * pw * sizeof(double)));   // (the kept rows alone: capacity may be the whole batch)
    if (int rc = usermodel_derive_rows(derive, op, (long long)take, r->rf_wide.as<double>(), s)) return rc;
    op = r->rf_wide.as<double>();
  }
  if (take) {
    CK(hipMemcpyAsync(out_u, ou, take * (size_t)d * sizeof(double), hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(out_p, op, take * pw * sizeof(double), hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(out_L, oL, take * sizeof(double), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
  }
  *nkept = take;
  return 0;
}

}  // namespace

extern "C" {

int mlf_region_sample(mlf_region *r, int method, size_t nsamples, uint64_t seed, uint64_t offset, double *out,
                      size_t capacity, size_t *naccepted, uint64_t *next_offset) {
  if (!out || !naccepted) return fail_arg(MLF_E_BADARG, "null pointer");
  *naccepted = 0;
  Drawn b;
  // capacity 0 draws nothing: the counter stays at `offset`
  if (int rc = region_draw(r, method, capacity ? nsamples : 0, seed, offset, &b, next_offset)) return rc;
  if (b.n == 0) return 0;
  hipStream_t s = g_ctx.stream;
  const int d = r->d;
  CK(r->sout.reserve(capacity * (size_t)d * sizeof(double)));
  const Compaction accepted(b.member, b.n, r->blk.as<unsigned>(), s);
  accepted.scatter(b.rows, d, r->sout.as<double>(), capacity);
  size_t take = 0;
  CK(accepted.count(capacity, &take));
  if (take) {
    CK(hipMemcpyAsync(out, r->sout.p, take * (size_t)d * sizeof(double), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
  }
  *naccepted = take;
  return 0;
}

int mlf_region_refill(mlf_region *r, int method, size_t nsamples, uint64_t seed, uint64_t offset, double Lmin, int tkind,
                      double ta, double tb, int lkind, const double *aux, double sigma, double *out_u, double *out_p,
                      double *out_L, size_t capacity, size_t *nevaluated, size_t *nkept, uint64_t *next_offset) {
  if (!r || !out_u || !out_p || !out_L || !nevaluated || !nkept || !next_offset)
    return fail_arg(MLF_E_BADARG, "null pointer");
  if (tkind < 0 || tkind > 2 || lkind < 0 || lkind > 3) return fail_arg(MLF_E_BADARG, "unknown transform / likelihood kind");
  if (r->tr_on && r->tr_w != r->d)   // (the gate kernel would read the w x w matrix as d x d)
    return fail_arg(MLF_E_STATE, "the region's t-region spans d + nderived columns: it gates mlf_region_refill_user_derived_gated only");
  if (lkind == 0 && !aux) return fail_arg(MLF_E_BADARG, "the Gaussian likelihood needs its centres");
  auto evaluate = [&](const double *rows, const uint8_t *member, long long n, double *pbuf, double *Lbuf, hipStream_t s,
                      const double **prow) -> int {
    const int d = r->d;
    if (aux)
      if (int rc = upload(r->rf_aux, aux, (size_t)d * sizeof(double), s)) return rc;
    if (r->tr_on) {   // transform and t-region gate in one pass over the batch
      // On the in-place route the gate kernel leaves the p rows of the rows the region rejected unwritten.  launch_loglike below
      // still runs over all n rows of pbuf (allocated for n rows), so it evaluates stale contents there; member2 is 0 for those
      // rows, and the threshold cut and the count read member2, so none of these values is ever used.
      const TregionGate g = region_tregion(r);
      if (tkind != 0) *prow = pbuf;
      CK(launch_transform_gate({rows, n, d, member, tkind, ta, tb, pbuf, g.A, g.ctr, g.fixed_val, g.enlarge, g.member2}, s));
    } else if (tkind != 0) {
      launch_elementwise_affine(rows, n * d, tkind, ta, tb, pbuf, s);
      *prow = pbuf;
    }
    launch_loglike(lkind, *prow, d, n, r->rf_aux.as<double>(), sigma, Lbuf, s);
    return 0;
  };
  return region_refill(r, method, nsamples, seed, offset, Lmin, evaluate, out_u, out_p, out_L, capacity, nevaluated, nkept,
                       next_offset);
}

int mlf_region_set_tregion(mlf_region *r, const double *A, const double *ctr, const double *fixed_val, double enlarge) {
  if (!r || !A || !ctr) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!r->ready) return fail_arg(MLF_E_STATE, "region not set");
  return mlf_region_set_tregion_wide(r, (size_t)r->d, A, ctr, fixed_val, enlarge);
}

int mlf_region_set_tregion_wide(mlf_region *r, size_t w, const double *A, const double *ctr, const double *fixed_val,
                                double enlarge) {
  if (!r || !A || !ctr) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!r->ready) return fail_arg(MLF_E_STATE, "region not set");
  if (w < (size_t)r->d) return fail_arg(MLF_E_BADARG, "a t-region is at least as wide as the region (d <= w)");
  if (w > MLF_MAX_DIM) return fail_arg(MLF_E_DIM, "t-region: width above MLF_MAX_DIM");
  hipStream_t s = g_ctx.stream;
  r->tr_on = false;
  std::vector<double> fixed(w, NAN);
  if (fixed_val) fixed.assign(fixed_val, fixed_val + w);
  if (int rc = upload(r->tr_A, A, w * w * sizeof(double), s)) return rc;
  if (int rc = upload(r->tr_ctr, ctr, w * sizeof(double), s)) return rc;
  if (int rc = upload(r->tr_fixed, fixed.data(), w * sizeof(double), s)) return rc;
  CK(hipStreamSynchronize(s));
  r->tr_enlarge = enlarge;
  r->tr_w = (int)w;
  r->tr_on = true;
  return 0;
}

int mlf_region_set_tregion_center(mlf_region *r, const double *ctr) {
  if (!r || !ctr) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!r->ready || !r->tr_on) return fail_arg(MLF_E_STATE, "no t-region set (mlf_region_set_tregion)");
  hipStream_t s = g_ctx.stream;
  if (int rc = upload(r->tr_ctr, ctr, (size_t)r->tr_w * sizeof(double), s)) return rc;
  CK(hipStreamSynchronize(s));
  return 0;
}

int mlf_region_clear_tregion(mlf_region *r) {
  if (!r) return fail_arg(MLF_E_BADARG, "null pointer");
  r->tr_on = false;
  return 0;
}

// What the three mlf_region_refill_user* entries share.  refill_user_pair: `derive` is a derive handle of the model's dimensionality
// (and, with nq != 0, of that many derived columns), and model and region agree in dimensionality.
static int refill_user_pair(const mlf_region *r, const mlf_usermodel *model, const mlf_usermodel *derive, int nq) {
  if (derive) {
    if (usermodel_nderived(derive) == 0) return fail_arg(MLF_E_STATE, "not a derive handle (mlf_usermodel_create_derived)");
    if (nq && usermodel_nderived(derive) != nq)
      return fail_arg(MLF_E_BADARG, "user model and its derive program differ in the number of derived parameters");
    if (usermodel_dim(derive) != usermodel_dim(model))
      return fail_arg(MLF_E_BADARG, "user model and its derive program differ in dimensionality");
  }
  if (r->ready && usermodel_dim(model) != r->d) return fail_arg(MLF_E_BADARG, "user model and region differ in dimensionality");
  return 0;
}

// refill_user: one mlf_user_rows launch for transform + likelihood; rows outside the membership mask are not evaluated (L = -inf:
// the threshold cut that follows drops them either way).  The gate: none without a t-region on the handle, d wide with nq == 0,
// else d + nq wide -- the same launch computes q before the gate, and r->rf_q holds the direct form's q rows (the staged form keeps
// them in LDS).  The rows stay d wide; with `derive`, region_refill widens the kept rows alone.
static int refill_user(mlf_region *r, int method, size_t nsamples, uint64_t seed, uint64_t offset, double Lmin, mlf_usermodel *model,
                       mlf_usermodel *derive, int nq, double *out_u, double *out_p, double *out_L, size_t capacity,
                       size_t *nevaluated, size_t *nkept, uint64_t *next_offset) {
  auto evaluate = [&](const double *rows, const uint8_t *member, long long n, double *pbuf, double *Lbuf, hipStream_t s,
                      const double **prow) -> int {
    double *p = usermodel_has_transform(model) ? pbuf : nullptr;
    if (p) *prow = p;
    if (!r->tr_on) return usermodel_rows(model, rows, n, member, p, Lbuf, s);
    TregionGate g = region_tregion(r);
    if (nq) {
      CK(r->rf_q.reserve((size_t)n * (size_t)nq * sizeof(double)));
      g.width = r->tr_w;
      g.q_scratch = r->rf_q.as<double>();
    }
    return usermodel_rows(model, rows, n, member, p, Lbuf, s, &g);
  };
  return region_refill(r, method, nsamples, seed, offset, Lmin, evaluate, out_u, out_p, out_L, capacity, nevaluated, nkept,
                       next_offset, derive);
}

int mlf_region_refill_user(mlf_region *r, int method, size_t nsamples, uint64_t seed, uint64_t offset, double Lmin,
                           mlf_usermodel *model, double *out_u, double *out_p, double *out_L, size_t capacity,
                           size_t *nevaluated, size_t *nkept, uint64_t *next_offset) {
  if (!r || !model || !out_u || !out_p || !out_L || !nevaluated || !nkept || !next_offset)
    return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = refill_user_pair(r, model, nullptr, 0)) return rc;
  if (r->tr_on && r->tr_w != r->d)   // (the kernel would read the w x w matrix as d x d)
    return fail_arg(MLF_E_STATE, "the region's t-region spans d + nderived columns: it gates mlf_region_refill_user_derived_gated only");
  if (r->tr_on != usermodel_gated(model))
    return fail_arg(MLF_E_STATE, r->tr_on ? "the region has a t-region: the user model must be loaded as MLF_USERMODEL_TREGION"
                                          : "user model loaded as MLF_USERMODEL_TREGION, but the region has no t-region");
  return refill_user(r, method, nsamples, seed, offset, Lmin, model, nullptr, 0, out_u, out_p, out_L, capacity, nevaluated, nkept,
                     next_offset);
}

int mlf_region_refill_user_derived(mlf_region *r, int method, size_t nsamples, uint64_t seed, uint64_t offset, double Lmin,
                                   mlf_usermodel *model, mlf_usermodel *derive, double *out_u, double *out_p, double *out_L,
                                   size_t capacity, size_t *nevaluated, size_t *nkept, uint64_t *next_offset) {
  if (!r || !model || !derive || !out_u || !out_p || !out_L || !nevaluated || !nkept || !next_offset)
    return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = refill_user_pair(r, model, derive, 0)) return rc;
  // the reference's t-region spans all nparams columns: its gate would need q before the likelihood (such a batch takes the host
  // sequence, or mlf_region_refill_user_derived_gated)
  if (r->tr_on) return fail_arg(MLF_E_STATE, "derived parameters together with a t-region do not run on the device");
  if (usermodel_gated(model)) return fail_arg(MLF_E_STATE, "user model loaded as MLF_USERMODEL_TREGION, but the region has no t-region");
  return refill_user(r, method, nsamples, seed, offset, Lmin, model, derive, 0, out_u, out_p, out_L, capacity, nevaluated, nkept,
                     next_offset);
}

int mlf_region_refill_user_derived_gated(mlf_region *r, int method, size_t nsamples, uint64_t seed, uint64_t offset, double Lmin,
                                         mlf_usermodel *model, mlf_usermodel *derive, double *out_u, double *out_p, double *out_L,
                                         size_t capacity, size_t *nevaluated, size_t *nkept, uint64_t *next_offset) {
  if (!r || !model || !derive || !out_u || !out_p || !out_L || !nevaluated || !nkept || !next_offset)
    return fail_arg(MLF_E_BADARG, "null pointer");
  const int nq = usermodel_gate_nderived(model);
  if (nq == 0)
    return fail_arg(MLF_E_STATE, "the user model is not of a _TREGION_DERIVED variant (mlf_usermodel_create_gate_derived)");
  if (int rc = refill_user_pair(r, model, derive, nq)) return rc;
  if (!r->tr_on) return fail_arg(MLF_E_STATE, "no t-region set: the gated derived refill needs mlf_region_set_tregion_wide");
  if (r->tr_w != r->d + nq)
    return fail_arg(MLF_E_BADARG, "the t-region's width is not d + nderived (mlf_region_set_tregion_wide)");
  return refill_user(r, method, nsamples, seed, offset, Lmin, model, derive, nq, out_u, out_p, out_L, capacity, nevaluated, nkept,
                     next_offset);
}

}  // extern "C"
