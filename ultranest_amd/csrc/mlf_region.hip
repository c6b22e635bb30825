// mlf_region.hip -- the region handle: its constants on the device (ellipsoid, layer, live points, the fragments and error
// constants of the bounded per-proposal stage) and the entry points that set or replace them.  Host code only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mlfriends_hip.h"
#include "mlf_host.hpp"
#include "mlf_prep3.hpp"
#include "mlf_prep64.hpp"
#include "mlf_sample.hpp"

namespace {

using namespace mlf;

// power of two s with s * amax in (2^(e-1), 2^e]
double pow2_scale(double amax, int e) {
  int ex = 0;
  std::frexp(amax, &ex);   // amax = m 2^ex, m in [0.5, 1)
  return std::ldexp(1.0, e - ex);
}

// k_prep4 subtracts the LAYER centre from every proposal; the ellipsoid form then starts its chain at
// y0 = L^T (c_lay - c_ell) (scaled like the accumulator: s_L s_x).  Recomputed whenever one of the two centres changes.
int region_prep4_centres(mlf_region *r, hipStream_t s) {
  const int d = r->d;
  const std::vector<double> &L = r->h_L;
  std::vector<double> s0((size_t)d);
  double s0n2 = 0.0, y0n2 = 0.0;
  for (int k = 0; k < d; ++k) {
    s0[k] = r->h_lay_ctr[k] - r->h_ell_ctr[k];
    s0n2 += s0[k] * s0[k];
  }
  const double acc_scale = 1.0 / (double)r->p4c.inv_sl_sx;
  std::vector<float> y0f((size_t)32 * ((r->dp + 31) / 32), 0.0f);
  for (int i = 0; i < d; ++i) {
    double y = 0.0;
    for (int k = i; k < d; ++k) y += L[(size_t)k * d + i] * s0[k];
    y0n2 += y * y;
    y0f[i] = (float)(y * acc_scale);
  }
  if (!std::isfinite(s0n2) || !std::isfinite(y0n2) || std::sqrt(y0n2) * acc_scale > 1e30) {
    r->p4_ready = false;
    return 0;
  }
  r->same_centres = s0n2 == 0.0;   // every difference an exact zero
  r->p4c.s0n = f32_up(std::sqrt(s0n2) * (1.0 + 1e-12));
  r->p4c.y0n = f32_up(std::sqrt(y0n2) * (1.0 + 1e-12));
  if (int rc = upload(r->p4_y0, y0f.data(), y0f.size() * sizeof(float), s)) return rc;
  if (!arena_active()) CK(hipStreamSynchronize(s));
  return 0;
}

// Fragments and error constants of the bounded per-proposal stage.  L: lower Cholesky factor of the ellipsoid matrix,
// fro2 = |A|_F^2; layer_T / layer_ctr may be null for regions without a neighbour scan; `live` = the cube-space live
// points (n x d) or null: their spread around the layer centre fixes the scale of the binary16 proposal operand.
int region_prep4_setup(mlf_region *r, const std::vector<double> &L, double fro2, const double *ell_center,
                       const double *layer_ctr, const double *layer_T, const double *live, size_t nlive, hipStream_t s,
                       const double *ell_invcov) {
  r->p4_ready = false;
  r->same_matrix = r->same_centres = false;
  const int d = r->d, dp = r->dp;
  if (!prep4_usable(d) || (dp & 1) || dp > 64 || !r->chol_ok || r->has_wrap) return 0;
  if (r->use_scan && (r->layer_kind != 0 || !layer_T || !layer_ctr)) return 0;
  double lf2 = 0.0, lmax = 0.0, dmin = INFINITY;
  for (int i = 0; i < d; ++i)
    for (int k = 0; k <= i; ++k) {
      const double v = L[(size_t)i * d + k];
      lf2 += v * v;
      lmax = std::fmax(lmax, std::fabs(v));
      if (k == i) dmin = std::fmin(dmin, v);
    }
  if (!std::isfinite(lf2) || !(lmax > 0.0) || !(lmax < 1e100) || !(dmin > 0.0)) return 0;
  const int nsteps = 3 * ((dp + 15) / 16);   // matrix instructions per output chain
  const int kdim = 16 * ((dp + 15) / 16);
  const double g = (4.0 * nsteps + 8.0) * std::ldexp(1.0, -24) * (1.0 + std::ldexp(1.0, -8)) + std::pow(2.0, -21.6) +
                   std::pow(2.0, -21.9);
  const double lf = std::sqrt(lf2);
  // share of the proposals near the boundary that the split-binary16 chain cannot decide ~ d g |L|_F / sigma_min(L):
  // beyond a few per cent the binary64 test behind it would dominate, the binary64 stage (k_prep3) is used instead
  if (d * g * lf / dmin > 0.02) return 0;
  // scale of the proposal operand: the live points' largest centred coordinate lands in (16, 32]; a region without
  // live points uses the ellipsoid's extent, 1 / (smallest diagonal entry of L) being a bound on its semi-axes' scale
  const double *ctr = r->use_scan ? layer_ctr : ell_center;
  double amax = 0.0;
  if (live) {   // four running maxima (a NaN never wins a comparison, as with fmax): one chain of dependent maxima cost 0.1 ms at N = 4000, d = 50
    double m[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = 0; i < nlive; ++i) {
      const double *row = live + i * d;
      int k = 0;
      for (; k + 4 <= d; k += 4)
        for (int q = 0; q < 4; ++q) {
          const double v = std::fabs(row[k + q] - ctr[k + q]);
          m[q] = v > m[q] ? v : m[q];
        }
      for (; k < d; ++k) {
        const double v = std::fabs(row[k] - ctr[k]);
        m[0] = v > m[0] ? v : m[0];
      }
    }
    amax = std::fmax(std::fmax(m[0], m[1]), std::fmax(m[2], m[3]));
  }
  if (!(amax > 0.0) || !std::isfinite(amax)) amax = 4.0 / dmin;
  if (!(amax > 1e-60) || !(amax < 1e60)) return 0;
  const double sx = pow2_scale(amax, 5);
  const double sl = pow2_scale(lmax, 8);            // largest |s_L L| entry in (128, 256]
  Prep4Consts &c = r->p4c;
  c = Prep4Consts{};
  c.g_chain = f32_up(g);
  c.lf = f32_up(lf * (1.0 + 1e-12));
  c.eps_scale = f32_up(std::ldexp(1.0, -34) * std::sqrt(fro2) * (1.0 + 1e-12));
  c.s_x = (float)sx;
  c.inv_sx = (float)(1.0 / sx);
  c.inv_sl_sx = (float)(1.0 / (sl * sx));
  c.l_abs = f32_up(lf * std::sqrt((double)kdim) * std::ldexp(1.0, -25) / sx * (1.0 + 1e-12));
  if (!(c.inv_sl_sx > 0.0f) || !std::isfinite(1.0f / c.inv_sl_sx) || !(c.inv_sx > 0.0f)) return 0;
  r->h_L = L;
  r->h_ell_ctr.assign(ell_center, ell_center + d);
  r->h_lay_ctr.assign(ctr, ctr + d);
  {   // the lower factor itself, row-major with stride dp (the wave-per-proposal exact test reads its columns)
    std::vector<double> lrm((size_t)dp * dp, 0.0);
    for (int j = 0; j < d; ++j)
      for (int k = 0; k <= j; ++k) lrm[(size_t)j * dp + k] = L[(size_t)j * d + k];
    if (int rc = upload(r->ell_L, lrm.data(), lrm.size() * sizeof(double), s)) return rc;
    if (!arena_active()) CK(hipStreamSynchronize(s));
  }
  std::vector<uint16_t> ltf(prep4_ltf_count(dp));
  const double el = prep4_lt_fragments(L.data(), d, dp, sl, ltf.data());
  c.el = f32_up(el / sl * (1.0 + 1e-12));
  if (int rc = upload(r->p4_LtF, ltf.data(), ltf.size() * sizeof(uint16_t), s)) return rc;
  if (r->use_scan) {
    double tf2 = 0.0, tmax = 0.0, cmin = INFINITY, cmax = 0.0;
    for (int cc = 0; cc < d; ++cc) {
      double cn = 0.0;
      for (int k = 0; k < d; ++k) {
        const double v = layer_T[(size_t)k * d + cc];
        cn += v * v;
        tmax = std::fmax(tmax, std::fabs(v));
      }
      tf2 += cn;
      cmin = std::fmin(cmin, cn);
      cmax = std::fmax(cmax, cn);
    }
    if (!std::isfinite(tf2) || !(tmax > 0.0) || !(tmax < 1e100) || !(cmin > 0.0)) return 0;
    // zeta against the binary16 term of Delta: g sqrt(d) cond(T) < 2^-11, or the uncertainty band of the filter more than
    // doubles (T = eigenvectors x diag: the column norms are its singular values)
    if (g * std::sqrt((double)d) * std::sqrt(cmax / cmin) * 2048.0 > 1.0) return 0;
    const double st = pow2_scale(tmax, 8);
    const double tf = std::sqrt(tf2);
    std::vector<uint16_t> ttf(prep4_ttf_count(dp));
    const double et = prep4_t_fragments(layer_T, d, dp, st, ttf.data());
    c.zt = f32_up((g * tf + et / st) * (1.0 + 1e-12));
    c.zt_abs = f32_up(tf * std::sqrt((double)kdim) * std::ldexp(1.0, -25) / sx * (1.0 + 1e-12));
    c.inv_st_sx = (float)(1.0 / (st * sx));
    if (!(c.inv_st_sx > 0.0f) || !std::isfinite(1.0f / c.inv_st_sx)) return 0;
    if (int rc = upload(r->p4_TtF, ttf.data(), ttf.size() * sizeof(uint16_t), s)) return rc;
    std::vector<double> t64((size_t)64 * 64, 0.0);   // for the exact whitening inside the re-check
    for (int k = 0; k < d; ++k)
      for (int c2 = 0; c2 < d; ++c2) t64[(size_t)k * 64 + c2] = layer_T[(size_t)k * d + c2];
    if (int rc = upload(r->lay_T64, t64.data(), t64.size() * sizeof(double), s)) return rc;
    // Same quadratic form?  E = sym(A) - T T^T in binary64 (the reference's einsum sees delta^T A delta = delta^T sym(A) delta);
    // |delta^T E delta| <= |E|_F |delta|^2 joins eps.  The residue is computed with rounding errors of its own: every entry of
    // T T^T is a d-term dot product (error <= d 2^-53 (|T| |T|^T)_ij, in the Frobenius norm <= d 2^-53 |T|_F^2), the
    // symmetrisation and the difference add 2^-52 |A|_F.  Accepted while the enlarged eps stays below twice the old one.
    if (ell_invcov) {
      double e2 = 0.0;
      for (int i = 0; i < d; ++i)
        for (int j = 0; j <= i; ++j) {
          double pij = 0.0;
          for (int cc = 0; cc < d; ++cc) pij += layer_T[(size_t)i * d + cc] * layer_T[(size_t)j * d + cc];
          const double e = 0.5 * (ell_invcov[(size_t)i * d + j] + ell_invcov[(size_t)j * d + i]) - pij;
          e2 += (i == j ? 1.0 : 2.0) * e * e;
        }
      const double afro = std::sqrt(fro2);
      const double e_bound = (std::sqrt(e2) + (d + 4.0) * std::ldexp(1.0, -52) * (tf2 + afro)) * (1.0 + 1e-12);
      if (std::isfinite(e_bound) && e_bound <= std::ldexp(1.0, -34) * afro) {
        Prep4Consts &q = r->p4c_same;
        q = c;
        q.y0n = 0.0f;                                   // the whitening chain starts at zero
        q.lf = f32_up(tf * (1.0 + 1e-12));              // eta = g |T|_F |delta| + |E_T|_F |delta| / s_T + |T|_F sqrt(K) 2^-25 / s_x
        q.el = f32_up(et / st * (1.0 + 1e-12));
        q.l_abs = c.zt_abs;
        q.s0n = 0.0f;                                   // (same_centres)
        q.eps_scale = f32_up((std::ldexp(1.0, -34) * afro + e_bound) * (1.0 + 1e-12));
        q.inv_sl_sx = c.inv_st_sx;                      // accumulator of the whitening chain -> T^T delta
        r->same_matrix = true;
      }
    }
  }
  if (!arena_active()) CK(hipStreamSynchronize(s));
  r->p4_ready = true;
  return region_prep4_centres(r, s);
}

// whiten `n` cube-space rows already on the device with the region's own layer (same kernels and
// arithmetic as for proposals, so a live point is at distance exactly 0 from itself)
int region_whiten_rows(mlf_region *r, const double *d_u, size_t n, double *d_t, hipStream_t s) {
  if (r->layer_kind == 0 && r->dp <= 64) {   // a few thousand rows at most: the wave-per-8-rows form of the same chain
    CK(launch_whiten_rows(d_u, (long long)n, r->d, r->dp, r->lay_ctr.as<double>(), r->lay_T8.as<double>(), (r->dp + 7) / 8 * 8,
                          r->has_wrap ? r->wrap.as<double>() : nullptr, d_t, r->d, s));
  } else if (r->layer_kind == 0) {
    PrepArgs pa{};
    pa.pts = d_u;
    pa.np = (long long)n;
    pa.d = r->d;
    pa.do_tr = 1;
    pa.lay_ctr = r->lay_ctr.as<double>();
    pa.lay_Tt = r->lay_mat.as<double>();
    pa.wrap_shift = r->has_wrap ? r->wrap.as<double>() : nullptr;
    pa.t_out = d_t;
    pa.ldt = r->d;
    CK(launch_prep(r->dp, pa, s));
  } else {
    launch_scaling_transform(d_u, (long long)n, r->d, r->lay_ctr.as<double>(), r->lay_mat.as<double>(),
                             r->has_wrap ? r->wrap.as<double>() : nullptr, nullptr, d_t, r->d, s);
    CK(hipGetLastError());
  }
  return 0;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------ region -----
int mlf_region_create(mlf_region **out) {
  if (!out) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  *out = new mlf_region();
  return 0;
}

int mlf_region_destroy(mlf_region *r) {
  if (!r) return 0;
  DevBuf *bufs[] = {&r->refT, &r->refR, &r->lay_ctr, &r->lay_mat, &r->lay_T8, &r->ell_Lt, &r->ell_LtF, &r->lay_TtF, &r->wrap, &r->ell_ctr,
                    &r->ell_A, &r->tq,  &r->gate,    &r->pts,     &r->mask, &r->row, &r->p4_LtF, &r->p4_TtF, &r->p4_y0, &r->lay_T64, &r->ell_L,
                    &r->gen, &r->gen2, &r->cube, &r->smask, &r->blk, &r->sout, &r->ax_zero, &r->ax_mat,
                    &r->s_invT, &r->s_lo, &r->s_hi, &r->s_thin, &r->s_count, &r->rf_p, &r->rf_L, &r->rf_out, &r->rf_aux,
                    &r->rf_keep, &r->ax_pad, &r->s_invT_pad, &r->s_tc, &r->s_wc, &r->s_thc, &r->s_gate,
                    &r->tr_A, &r->tr_ctr, &r->tr_fixed, &r->rf_member2, &r->rf_wide, &r->rf_q};
  for (DevBuf *b : bufs) b->release();
  for (hipEvent_t e : r->events) (void)hipEventDestroy(e);
  r->filter.release();
  if (r->arena.p) (void)hipHostFree(r->arena.p);
  delete r;
  return 0;
}

int mlf_region_set(mlf_region *r, const double *unormed, size_t n, size_t d, int live_space,
                   int layer_kind, const double *layer_ctr, const double *layer_T,
                   const double *wrap_shift, const double *ell_center, const double *ell_invcov,
                   double enlarge, double radiussq, int use_scan) {
  if (!r) return fail_arg(MLF_E_BADARG, "null region");
  if (int rc = check_dims(d)) return rc;
  if (!ell_center || !ell_invcov) return fail_arg(MLF_E_BADARG, "null ellipsoid");
  if (use_scan && (!unormed || !layer_ctr || !layer_T || n == 0))
    return fail_arg(MLF_E_BADARG, "scan regions need live points and a layer");
  if (layer_kind != 0 && layer_kind != 1) return fail_arg(MLF_E_BADARG, "layer_kind must be 0 or 1");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  if (!r->arena.p) {   // pinned staging of the constants (kept with the handle; handles are recycled)
    if (hipHostMalloc(reinterpret_cast<void **>(&r->arena.p), kArenaBytes, hipHostMallocMapped) == hipSuccess &&
        hipHostGetDevicePointer(reinterpret_cast<void **>(&r->arena.p_dev), r->arena.p, 0) == hipSuccess)
      r->arena.cap = kArenaBytes;
    else
      (void)hipGetLastError();
  }
  r->arena.used = 0;
  r->arena.npending = 0;
  struct ArenaScope {   // every exit path of this call drops the arena
    explicit ArenaScope(HostArena *a) { g_arena = a->p ? a : nullptr; }
    ~ArenaScope() { g_arena = nullptr; }
  } arena_scope(&r->arena);
  r->ready = false;
  r->axes_ready = r->sampling_ready = false;   // a handle may be set again for another region (kernels.DeviceRegion recycles them)
  if (r->d != (int)d) r->tr_on = false;   // a t-region belongs to its dimensionality
  r->n = (int)n;
  r->d = (int)d;
  r->dp = pick_dp((int)d);
  r->npad = round_up((int)n, kWave);
  r->layer_kind = layer_kind;
  r->live_space = live_space ? 1 : 0;
  r->use_scan = use_scan ? 1 : 0;
  r->enlarge = enlarge;
  r->r2 = radiussq;
  r->has_wrap = wrap_shift != nullptr;
  const int dp = r->dp;
  if (int rc = prep_consts(r->ell_ctr, r->ell_A, ell_center, ell_invcov, (int)d, dp, false, c.stream))
    return rc;
  std::vector<double> L((size_t)d * d, 0.0);
  double fro_sq = 0.0;
  {  // Cholesky factor + Frobenius norm of the ellipsoid matrix for the bounded H3 evaluation
    std::vector<double> Lt((size_t)dp * dp, 0.0);
    bool ok = true;
    double fro = 0.0;
    for (size_t e = 0; e < d * d; ++e) fro += ell_invcov[e] * ell_invcov[e];
    for (size_t j = 0; j < d && ok; ++j) {
      double diag = ell_invcov[j * d + j];
      for (size_t k = 0; k < j; ++k) diag -= L[j * d + k] * L[j * d + k];
      if (!(diag > 0.0) || !std::isfinite(diag)) {
        ok = false;
        break;
      }
      const double ljj = std::sqrt(diag);
      L[j * d + j] = ljj;
      for (size_t i = j + 1; i < d; ++i) {
        double v = 0.5 * (ell_invcov[i * d + j] + ell_invcov[j * d + i]);
        for (size_t k = 0; k < j; ++k) v -= L[i * d + k] * L[j * d + k];
        L[i * d + j] = v / ljj;
      }
    }
    // the bound assumes a symmetric matrix: an asymmetric one takes the exact path
    for (size_t i = 0; i < d && ok; ++i)
      for (size_t j = 0; j < i; ++j)
        if (std::fabs(ell_invcov[i * d + j] - ell_invcov[j * d + i]) >
            1e-14 * (std::fabs(ell_invcov[i * d + i]) + std::fabs(ell_invcov[j * d + j])))
          ok = false;
    if (ok)
      for (size_t k = 0; k < d; ++k)
        for (size_t j = 0; j < d; ++j) Lt[k * dp + j] = L[j * d + k];
    fro_sq = fro;
    r->chol_ok = ok && std::isfinite(fro);
    r->ell_eps_scale = std::ldexp(1.0, -34) * std::sqrt(fro);
    if (int rc = upload(r->ell_Lt, Lt.data(), Lt.size() * sizeof(double), c.stream)) return rc;
    if ((prep64_usable((int)d) || prep64_wide_usable((int)d)) && ok) {   // 65 ... 1024 dimensions: the factor itself, row-major (mlf_prep64.hip reads its rows)
      std::vector<double> lrm((size_t)dp * dp, 0.0);
      for (size_t j = 0; j < d; ++j)
        for (size_t k = 0; k <= j; ++k) lrm[j * dp + k] = L[j * d + k];
      if (int rc = upload(r->ell_L, lrm.data(), lrm.size() * sizeof(double), c.stream)) return rc;
    }
    if (prep3_usable((int)d)) {   // the same factor as 16 x 4 matrix-core fragments: (row kb, k j) = L[j][kb]
      std::vector<double> frag(prep3_fragment_count((int)d));
      prep3_fragments(L.data(), (int)d, true, true, frag.data());
      if (int rc = upload(r->ell_LtF, frag.data(), frag.size() * sizeof(double), c.stream)) return rc;
    }
    if (!arena_active()) CK(hipStreamSynchronize(c.stream));
    r->chol_ready = true;
  }
  if (use_scan) {
    if (layer_kind == 0) {
      if (int rc = prep_consts(r->lay_ctr, r->lay_mat, layer_ctr, layer_T, (int)d, dp, true, c.stream))
        return rc;
      const int dp8 = (dp + 7) / 8 * 8;
      std::vector<double> t8((size_t)dp * dp8, 0.0);
      for (size_t k = 0; k < d; ++k)
        for (size_t cc = 0; cc < d; ++cc) t8[k * dp8 + cc] = layer_T[k * d + cc];
      if (int rc = upload(r->lay_T8, t8.data(), t8.size() * sizeof(double), c.stream)) return rc;
      if (prep3_usable((int)d)) {   // (row c, k) = T[k][c]
        std::vector<double> frag(prep3_fragment_count((int)d));
        prep3_fragments(layer_T, (int)d, true, false, frag.data());
        if (int rc = upload(r->lay_TtF, frag.data(), frag.size() * sizeof(double), c.stream)) return rc;
      }
      if (!arena_active()) CK(hipStreamSynchronize(c.stream));
    } else {
      if (int rc = upload(r->lay_ctr, layer_ctr, d * sizeof(double), c.stream)) return rc;
      if (int rc = upload(r->lay_mat, layer_T, d * sizeof(double), c.stream)) return rc;
    }
    if (wrap_shift) {
      std::vector<double> w = pad_vector(wrap_shift, (int)d, dp, NAN);
      if (int rc = upload(r->wrap, w.data(), w.size() * sizeof(double), c.stream)) return rc;
      if (!arena_active()) CK(hipStreamSynchronize(c.stream));  // w goes out of scope
    }
    if (int rc = upload(c.src, unormed, n * d * sizeof(double), c.stream)) return rc;
    const double *rows = c.src.as<double>();
    if (int rc = arena_flush(c.stream)) return rc;   // the layer constants, in front of the kernels that read them
    if (r->live_space) {  // rows are cube-space live points: whiten them on the device
      CK(c.tq.reserve(n * d * sizeof(double)));
      if (int rc = region_whiten_rows(r, c.src.as<double>(), n, c.tq.as<double>(), c.stream)) return rc;
      rows = c.tq.as<double>();
    }
    CK(r->refT.reserve((size_t)r->npad * dp * sizeof(double)));
    CK(r->refR.reserve((size_t)r->npad * dp * sizeof(double)));
    launch_build_layouts(rows, (int)n, (int)d, dp, r->npad, r->refT.as<double>(), r->refR.as<double>(),
                         c.stream);
    CK(hipGetLastError());
    if (int rc = filter_prepare_refs(r->filter, r->refR.as<double>(), (int)n, (int)d, dp, c.stream, true))
      return rc;
  }
  {
    size_t n_for_scale = n;
    const double *live_host = (use_scan && live_space) ? unormed : nullptr;
    std::vector<double> back;
    const double hint = r->live_extent_hint;
    r->live_extent_hint = -1.0;
    if (live_host && hint > 0.0 && std::isfinite(hint)) {   // the caller knows the extent: one fictitious row carries it
      back.assign(d, 0.0);
      for (size_t k = 0; k < d; ++k) back[k] = layer_ctr[k];
      back[0] = layer_ctr[0] + hint;
      live_host = back.data();
      n_for_scale = 1;
    } else if (live_host && is_device_pointer(live_host)) {   // the operand scale is found on the host: fetch the rows once
      back.resize(n * d);
      CK(hipMemcpyAsync(back.data(), unormed, n * d * sizeof(double), hipMemcpyDeviceToHost, c.stream));
      CK(hipStreamSynchronize(c.stream));
      live_host = back.data();
    }
    if (int rc = region_prep4_setup(r, L, fro_sq, ell_center, layer_ctr, layer_T, live_host, n_for_scale, c.stream,
                                    ell_invcov))
      return rc;
  }
  if (int rc = arena_flush(c.stream)) return rc;
  CK(hipStreamSynchronize(c.stream));
  r->ready = true;
  return 0;
}

int mlf_region_hint_live_extent(mlf_region *r, double amax) {
  if (!r) return fail_arg(MLF_E_BADARG, "null region");
  r->live_extent_hint = amax;
  return 0;
}

int mlf_region_update_points(mlf_region *r, size_t count, const int64_t *rows, const double *live_rows) {
  if (!r || (count && (!rows || !live_rows))) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!r->ready || !r->use_scan) return fail_arg(MLF_E_STATE, "region has no live points set");
  for (size_t k = 0; k < count; ++k)
    if (rows[k] < 0 || rows[k] >= (int64_t)r->n) return fail_arg(MLF_E_BADARG, "row out of range");
  if (count == 0) return 0;
  Ctx &c = g_ctx;
  // one buffer: [count x d new rows | count x d whitened rows | count indices]
  const size_t block = count * (size_t)r->d;
  CK(r->row.reserve((2 * block + count) * sizeof(double)));
  double *raw = r->row.as<double>(), *white = raw + block;
  long long *index = reinterpret_cast<long long *>(raw + 2 * block);
  const double *src = raw;
  const long long *index_src = index;
  if (int rc = small_staging(c)) return rc;
  if ((block + count) * sizeof(double) <= kSmallStagingBytes) {
    // the usual few rows: no copy on the stream, the kernels read the pinned staging buffer (free: a single-launch
    // membership call has its mask back before it returns, and this call ends with a synchronisation)
    memcpy(c.pin_pts, live_rows, block * sizeof(double));
    memcpy(c.pin_pts + block, rows, count * sizeof(int64_t));
    src = c.pin_pts_dev;
    index_src = reinterpret_cast<const long long *>(c.pin_pts_dev + block);
  } else {
    CK(hipMemcpyAsync(raw, live_rows, block * sizeof(double), hipMemcpyHostToDevice, c.stream));
    CK(hipMemcpyAsync(index, rows, count * sizeof(int64_t), hipMemcpyHostToDevice, c.stream));
  }
  if (r->live_space) {
    if (int rc = region_whiten_rows(r, src, count, white, c.stream)) return rc;
    src = white;
  }
  launch_update_rows(src, (int)count, r->d, r->dp, r->npad, index_src, r->refT.as<double>(), r->refR.as<double>(), c.stream);
  CK(hipGetLastError());
  // centre / scale / norms of the pre-filter operands depend on every row: requantised (four small kernels) by the next
  // batch that uses them -- the 1-10 point calls between two replacements (mlf_small.hip) never do
  if (r->filter.refs_ready) r->filter.refs_dirty = true;
  CK(hipStreamSynchronize(c.stream));
  return 0;
}

int mlf_region_update_point(mlf_region *r, size_t row, const double *unormed_row) {
  if (!unormed_row) return fail_arg(MLF_E_BADARG, "null pointer");
  const int64_t index = (int64_t)row;
  if (r && row >= (size_t)r->n && r->ready && r->use_scan) return fail_arg(MLF_E_BADARG, "row out of range");
  return mlf_region_update_points(r, 1, &index, unormed_row);
}

int mlf_region_set_thresholds(mlf_region *r, double enlarge, double radiussq) {
  if (!r) return fail_arg(MLF_E_BADARG, "null region");
  r->enlarge = enlarge;
  r->r2 = radiussq;
  return 0;
}

int mlf_region_set_ellipsoid_center(mlf_region *r, const double *ell_center) {
  if (!r || !ell_center) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!r->ready) return fail_arg(MLF_E_STATE, "region not set");
  Ctx &c = g_ctx;
  std::vector<double> pc = pad_vector(ell_center, r->d, r->dp);
  if (int rc = upload(r->ell_ctr, pc.data(), pc.size() * sizeof(double), c.stream)) return rc;
  CK(hipStreamSynchronize(c.stream));
  if (r->p4_ready) {
    r->h_ell_ctr.assign(ell_center, ell_center + r->d);
    if (!r->use_scan) r->h_lay_ctr = r->h_ell_ctr;   // no layer: the proposals are centred on the ellipsoid itself
    if (int rc = region_prep4_centres(r, c.stream)) return rc;
  }
  return 0;
}

int mlf_region_set_axes(mlf_region *r, const double *axes_T) {
  if (!r || !axes_T) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!r->ready) return fail_arg(MLF_E_STATE, "region not set");
  Ctx &c = g_ctx;
  const int d = r->d, dp = r->dp;
  std::vector<double> zero((size_t)dp, 0.0);
  // k_prep computes (x - ctr) . T from T^T rows: with T = axes_T the staged matrix is axes itself
  std::vector<double> m = pad_matrix(axes_T, d, dp, true);
  if (int rc = upload(r->ax_zero, zero.data(), zero.size() * sizeof(double), c.stream)) return rc;
  if (int rc = upload(r->ax_mat, m.data(), m.size() * sizeof(double), c.stream)) return rc;
  std::vector<double> ap;   // k_generate_ellipsoid's copy: element (j, k) = axes_T[j][k], rows padded to 4 x chunk outputs
  if (d <= 128) {
    const int ldk = 4 * generate_ellipsoid_chunk(d);
    ap.assign((size_t)d * ldk, 0.0);
    for (int j = 0; j < d; ++j)
      for (int k = 0; k < d; ++k) ap[(size_t)j * ldk + k] = axes_T[(size_t)j * d + k];
    if (int rc = upload(r->ax_pad, ap.data(), ap.size() * sizeof(double), c.stream)) return rc;
  }
  CK(hipStreamSynchronize(c.stream));
  r->axes_ready = true;
  return 0;
}

int mlf_region_set_sampling_data(mlf_region *r, const double *invT, const double *bbox_lo, const double *bbox_hi) {
  if (!r || !invT || !bbox_lo || !bbox_hi) return fail_arg(MLF_E_BADARG, "null pointer");
  if (!r->ready || !r->use_scan) return fail_arg(MLF_E_STATE, "region has no live points set");
  if (r->layer_kind != 0) return fail_arg(MLF_E_STATE, "t-space sampling needs an affine layer");
  Ctx &c = g_ctx;
  const size_t d = (size_t)r->d;
  if (int rc = upload(r->s_invT, invT, d * d * sizeof(double), c.stream)) return rc;
  std::vector<double> ip;   // k_rows_affine's copy: rows padded to 4 x chunk outputs
  if (d <= 128) {
    const size_t ldk = 4 * (size_t)generate_ellipsoid_chunk((int)d);
    ip.assign(d * ldk, 0.0);
    for (size_t j = 0; j < d; ++j)
      for (size_t k = 0; k < d; ++k) ip[j * ldk + k] = invT[j * d + k];
    if (int rc = upload(r->s_invT_pad, ip.data(), ip.size() * sizeof(double), c.stream)) return rc;
  }
  if (int rc = upload(r->s_lo, bbox_lo, d * sizeof(double), c.stream)) return rc;
  if (int rc = upload(r->s_hi, bbox_hi, d * sizeof(double), c.stream)) return rc;
  CK(hipStreamSynchronize(c.stream));
  r->sampling_ready = true;
  return 0;
}

}  // extern "C"
