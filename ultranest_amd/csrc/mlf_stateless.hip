// mlf_stateless.hip -- the entry points without a region handle: live points and queries arrive with the call and are
// staged in the context's scratch (K1-K5, H1, H3 / T1, bootstrap statistics, likelihoods).  Host code only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mlfriends_hip.h"
#include "mlf_host.hpp"

namespace {

using namespace mlf;

int scan_host(const double *apts, size_t na, const double *bpts, size_t nb, size_t d, double r2,
              int mode, int64_t *out) {
  if (int rc = check_dims(d)) return rc;
  if (nb == 0) return 0;
  if (!bpts || !out || (na && !apts)) return fail_arg(MLF_E_BADARG, "null pointer");
  if (na == 0) {  // the reference loops over zero live points
    for (size_t j = 0; j < nb; ++j) out[j] = mode == SCAN_FIRST ? -1 : 0;
    return 0;
  }
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  const int dp = pick_dp((int)d);
  const int npad = round_up((int)na, kWave);
  if (int rc = stage_live_points(apts, na, d, dp, npad, false)) return rc;
  if (int rc = upload(c.q, bpts, nb * d * sizeof(double), c.stream)) return rc;
  CK(c.out.reserve(nb * sizeof(long long)));
  const LiveSet live{c.refT.as<double>(), c.refR.as<double>(), (int)na, npad, (int)d, dp, r2};
  BatchPlan p = plan_batch(c.filter, nullptr, BATCH_HOST, (long long)nb, r2, mode == SCAN_FIRST, false, nullptr, na);
  if (p.host_refs) {   // quantise the live points, then route with their statistics
    if (int rc = filter_prepare_refs(c.filter, c.refR.as<double>(), (int)na, (int)d, dp, c.stream, true, false)) return rc;   // first-index mode only
    p = plan_batch(c.filter, nullptr, BATCH_HOST, (long long)nb, r2, mode == SCAN_FIRST, false, nullptr, na);
  }
  if (p.filter) {
    if (int rc = filter_run({c.filter, p, live, c.q.as<double>(), (long long)d, 1, (long long)nb, nullptr, nullptr,
                             c.out.as<long long>(), c.stream, nullptr, nullptr}))
      return rc;
  } else {
    ScanArgs a = scan_args(live, c.q.as<double>(), (long long)d, 0, (long long)nb, mode);
    a.out_idx = c.out.as<long long>();
    CK(launch_scan(dp, a, c.stream));
  }
  CK(hipMemcpyAsync(out, c.out.p, nb * sizeof(long long), hipMemcpyDefault, c.stream));   // host or device destination
  CK(hipStreamSynchronize(c.stream));
  return 0;
}

// ------------------------------------------------------------------------------ likelihoods -
int loglike_host(int kind, const double *params, size_t d, size_t n, const double *aux,
                        double sigma, double *like) {
  if (d == 0) return fail_arg(MLF_E_BADARG, "dimensionality must be positive");
  if (n == 0) return 0;
  if (!params || !like || (kind == 0 && !aux)) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  if (int rc = upload(c.q, params, n * d * sizeof(double), c.stream)) return rc;
  if (aux)
    if (int rc = upload(c.small0, aux, d * sizeof(double), c.stream)) return rc;
  CK(c.out.reserve(n * sizeof(double)));
  launch_loglike(kind, c.q.as<double>(), (int)d, (long long)n, aux ? c.small0.as<double>() : nullptr,
                 sigma, c.out.as<double>(), c.stream);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(like, c.out.p, n * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  return 0;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------ K1 / K2 ----
int mlf_find_nearby(const double *apts, size_t na, const double *bpts, size_t nb, size_t d,
                    double radiussq, int64_t *out) {
  return scan_host(apts, na, bpts, nb, d, radiussq, SCAN_FIRST, out);
}

int mlf_count_nearby(const double *apts, size_t na, const double *bpts, size_t nb, size_t d,
                     double radiussq, int64_t *out) {
  return scan_host(apts, na, bpts, nb, d, radiussq, SCAN_COUNT, out);
}

// ------------------------------------------------------------------------------ K3 ---------
int mlf_subtract_nearby(const double *pts, size_t n, size_t d, double radiussq, double *out) {
  if (int rc = check_dims(d)) return rc;
  if (n == 0) return 0;
  if (!pts || !out) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  const int dp = pick_dp((int)d);
  const int npad = round_up((int)n, kWave);
  const int ntiles = npad / kWave;
  if (int rc = stage_live_points(pts, n, d, dp, npad, false)) return rc;
  CK(c.flags.reserve(n * (size_t)ntiles * sizeof(unsigned long long)));
  CK(c.out.reserve(n * d * sizeof(double)));
  ScanArgs a{};
  a.refT = c.refT.as<double>();
  a.n = (int)n;
  a.npad = npad;
  a.ntiles = ntiles;
  a.q = c.src.as<double>();
  a.ldq = (long long)d;
  a.nq = (long long)n;
  a.d = (int)d;
  a.r2 = radiussq;
  a.mode = SCAN_FLAGS;
  a.out_flags = c.flags.as<unsigned long long>();
  CK(launch_scan(dp, a, c.stream));
  launch_subtract_accum(c.src.as<double>(), (int)n, (int)d, c.flags.as<unsigned long long>(), ntiles,
                        c.out.as<double>(), c.stream);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(out, c.out.p, n * d * sizeof(double), hipMemcpyDefault, c.stream));   // host or device destination
  CK(hipStreamSynchronize(c.stream));
  return 0;
}

// ------------------------------------------------------------------------------ H1 ---------
// Friends-of-friends labels of update_clusters (mlfriends.pyx:275-343) from ONE all-pairs pass: the hit ballots of
// every point against every point (k_scan, mode FLAGS: the adjacency matrix as n x ntiles 64-bit words) come back to
// the host, where the reference's growth rounds -- members of the current cluster against the unlabelled points, a new
// cluster seeded when nothing joins -- are replayed on the bit rows.  Distances are symmetric bit for bit, so a round
// joins exactly the points the reference's find_nearby call reports; labels, their numbering and the carried-over
// seeds (previous ids) are the reference's.
int mlf_adjacency_bits(const double *pts, size_t n, size_t d, double radiussq, const unsigned long long **adj_out) {
  if (int rc = check_dims(d)) return rc;
  if (!pts || !adj_out || n == 0) return fail_arg(MLF_E_BADARG, "null pointer or no points");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  const int dp = pick_dp((int)d);
  const int npad = round_up((int)n, kWave);
  const int ntiles = npad / kWave;
  if (int rc = stage_live_points(pts, n, d, dp, npad, false)) return rc;
  CK(c.flags.reserve(n * (size_t)ntiles * sizeof(unsigned long long)));
  ScanArgs a{};
  a.refT = c.refT.as<double>();
  a.n = (int)n;
  a.npad = npad;
  a.ntiles = ntiles;
  a.q = c.src.as<double>();
  a.ldq = (long long)d;
  a.nq = (long long)n;
  a.d = (int)d;
  a.r2 = radiussq;
  a.mode = SCAN_FLAGS;
  a.out_flags = c.flags.as<unsigned long long>();
  CK(launch_scan(dp, a, c.stream));
  const size_t nwords = n * (size_t)ntiles;
  if (c.pin_adj_cap < nwords) {   // pinned landing buffer for the bit matrix (2 MB at n = 4000), kept for the next call
    if (c.pin_adj) (void)hipHostFree(c.pin_adj);
    c.pin_adj = nullptr;
    c.pin_adj_cap = 0;
    CK(hipHostMalloc(reinterpret_cast<void **>(&c.pin_adj), nwords * sizeof(unsigned long long), hipHostMallocDefault));
    c.pin_adj_cap = nwords;
  }
  CK(hipMemcpyAsync(c.pin_adj, c.flags.p, nwords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  *adj_out = c.pin_adj;
  return 0;
}

// Host only (no device, no library state: may run on another thread next to device calls).
int mlf_host_cluster_replay(const unsigned long long *adj, size_t n, const int64_t *previous, int64_t *labels,
                            int64_t *nclusters) {
  if (!adj || !labels || !nclusters || n == 0) return fail_arg(MLF_E_BADARG, "null pointer or no points");
  const int ntiles = (int)((n + 63) / 64);
  // reach = union of the adjacency rows of all members of the current cluster (each member's row is OR-ed in once,
  // when it joins): a growth round joins the unlabelled points inside `reach` -- the points the reference's
  // find_nearby(members, unlabelled) call reports -- and then adds their rows
  std::vector<unsigned long long> reach_v((size_t)ntiles, 0ull), unl((size_t)ntiles, 0ull);
  unsigned long long *__restrict__ reach = reach_v.data();
  std::vector<size_t> fresh;
  for (size_t i = 0; i < n; ++i) {
    labels[i] = 0;
    unl[i >> 6] |= 1ull << (i & 63);
  }
  size_t nlabelled = 0;
  auto seed_for = [&](int64_t cid, size_t fallback) {
    if (previous)
      for (size_t i = 0; i < n; ++i)
        if (previous[i] == cid) return i;
    return fallback;
  };
  auto add_member = [&](size_t i) {
    const unsigned long long *__restrict__ row = adj + i * (size_t)ntiles;
#pragma clang loop vectorize(enable)
    for (int t = 0; t < ntiles; ++t) reach[t] |= row[t];
  };
  int64_t current = 1;
  auto plant = [&](size_t i) {   // a carried-over seed may already wear an earlier label: it is re-labelled, as in the reference
    if (labels[i] == 0) {
      ++nlabelled;
      unl[i >> 6] &= ~(1ull << (i & 63));
    }
    labels[i] = current;
    for (int t = 0; t < ntiles; ++t) reach[t] = 0ull;
    add_member(i);
  };
  plant(seed_for(current, 0));
  while (nlabelled < n) {
    fresh.clear();
    for (int t = 0; t < ntiles; ++t) {
      unsigned long long w = reach[t] & unl[t];
      while (w) {
        const int b = __builtin_ctzll(w);
        w &= w - 1ull;
        fresh.push_back((size_t)t * 64 + (size_t)b);
      }
    }
    if (!fresh.empty()) {
      for (size_t j : fresh) {
        labels[j] = current;
        unl[j >> 6] &= ~(1ull << (j & 63));
      }
      nlabelled += fresh.size();
      for (size_t j : fresh) add_member(j);
    } else {
      ++current;
      size_t first = 0;
      while (first < n && labels[first] != 0) ++first;
      plant(seed_for(current, first));
    }
  }
  std::vector<char> seen((size_t)current + 1, 0);   // number of DISTINCT labels (a re-labelled seed can empty a cluster)
  int64_t distinct = 0;
  for (size_t i = 0; i < n; ++i)
    if (!seen[(size_t)labels[i]]) {
      seen[(size_t)labels[i]] = 1;
      ++distinct;
    }
  *nclusters = distinct;
  return 0;
}

int mlf_cluster_labels(const double *tpts, size_t n, size_t d, double radiussq, const int64_t *previous, int64_t *labels,
                       int64_t *nclusters) {
  const unsigned long long *adj = nullptr;
  if (int rc = mlf_adjacency_bits(tpts, n, d, radiussq, &adj)) return rc;
  return mlf_host_cluster_replay(adj, n, previous, labels, nclusters);
}

// ------------------------------------------------------------------------------ K4 ---------
int mlf_maxradiussq_bootstrap(const double *pts, size_t n, size_t d, const uint8_t *selected,
                              size_t B, double *maxd_out, uint8_t *skipped_out) {
  return mlf_maxradiussq_bootstrap_rows(pts, n, d, selected, B, 0, n, maxd_out, skipped_out);
}

// One rank's share of K4 under ROW-BLOCK sharding: all B rounds, every live point i, but only the rows j in
// [row_lo, row_hi) as the left-out point -- the rank does 1/W of the pair distances (sharding by rounds would repeat all
// of them on every rank: k_boot computes a distance once for all 32 rounds of a pass).
int mlf_maxradiussq_bootstrap_rows(const double *pts, size_t n, size_t d, const uint8_t *selected, size_t B,
                                   size_t row_lo, size_t row_hi, double *maxd_out, uint8_t *skipped_out) {
  if (int rc = check_dims(d)) return rc;
  if (B == 0) return 0;
  if (!pts || !selected || !maxd_out || n == 0) return fail_arg(MLF_E_BADARG, "null pointer or no points");
  if (row_lo > row_hi || row_hi > n) return fail_arg(MLF_E_BADARG, "row range outside [0, n]");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  const int dp = pick_dp((int)d);
  const int npad = round_up((int)n, kWave);
  if (int rc = stage_live_points(pts, n, d, dp, npad, true)) return rc;
  if (int rc = upload_any(c.selbytes, selected, B * n, c.stream)) return rc;
  CK(c.sel.reserve((size_t)npad * sizeof(unsigned)));
  CK(c.selmask.reserve((size_t)(npad + 1) * kBootGroup * sizeof(unsigned)));   // k_boot requests one row past its last
  CK(c.M.reserve((size_t)kBootGroup * npad * sizeof(unsigned long long)));
  CK(c.small0.reserve(B * sizeof(double)));
  CK(c.small1.reserve(B));
  // live-point chunks: one round of the 2048 waves the chip holds at two per SIMD (k_boot's register budget), equal shares
  // (a wave pays ~1 us of set-up for its own 64 rows: no chunk below 8 live points)
  const int blk0 = (int)(row_lo / kWave);
  const int rowblocks = row_hi > row_lo ? (int)((row_hi + kWave - 1) / kWave) - blk0 : 0;
  // a rank's share of a sharded pass is short: one wave per SIMD runs this kernel as fast as two, and half the
  // waves means half the atomicMin traffic on M, which does not shrink with the shard
  const int target_waves = 2 * rowblocks <= npad / kWave ? 1024 : 2048;
  int want_chunks = rowblocks ? target_waves / rowblocks : 1;
  if (want_chunks < 1) want_chunks = 1;
  int chunk = ((int)n + want_chunks - 1) / want_chunks;
  if (chunk < 8) chunk = 8;
  const int nchunks = ((int)n + chunk - 1) / chunk;
  const double init = 1e300;
  unsigned long long init_bits;
  memcpy(&init_bits, &init, sizeof init_bits);
  for (size_t b0 = 0; b0 < B; b0 += kBootGroup) {
    const int nb = (int)((B - b0) < (size_t)kBootGroup ? (B - b0) : (size_t)kBootGroup);
    launch_pack_selection(c.selbytes.as<uint8_t>(), (int)n, npad, (int)b0, nb, c.sel.as<unsigned>(),
                          c.stream, c.selmask.as<unsigned>());
    launch_fill_u64(c.M.as<unsigned long long>(), (long long)kBootGroup * npad, init_bits, c.stream);
    BootArgs a{};
    a.refT = c.refT.as<double>();
    a.refR = c.refR.as<double>();
    a.sel = c.sel.as<unsigned>();
    a.selmask = c.selmask.as<unsigned>();
    a.n = (int)n;
    a.npad = npad;
    a.chunk = chunk;
    a.M = c.M.as<unsigned long long>();
    a.blk0 = blk0;
    if (row_lo == 0 && row_hi == n && dp <= 64 && (g_opt[OPT_BOOT_SYM] == 2 || (g_opt[OPT_BOOT_SYM] == 1 && boot_sym_usable(dp, npad)))) {
      CK(launch_boot_sym(dp, a, c.stream));   // every pair distance once (a rank's row share keeps k_boot: its minima must be complete)
    } else {
      CK(launch_boot(dp, a, nchunks, c.stream, rowblocks));
    }
    launch_boot_final(c.M.as<unsigned long long>(), c.sel.as<unsigned>(), (int)n, npad, nb,
                      c.small0.as<double>() + b0, c.small1.as<uint8_t>() + b0, c.stream, (int)row_lo, (int)row_hi);
    CK(hipGetLastError());
  }
  CK(hipMemcpyAsync(maxd_out, c.small0.p, B * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  std::vector<uint8_t> sk(B);
  CK(hipMemcpyAsync(sk.data(), c.small1.p, B, hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  if (skipped_out) memcpy(skipped_out, sk.data(), B);
  return 0;
}

// ------------------------------------------------------------------------------ K5 ---------
int mlf_pair_dist2_lower(const double *pts, size_t n, size_t d, double *dist2_out) {
  if (int rc = check_dims(d)) return rc;
  if (n < 2) return 0;
  if (!pts || !dist2_out) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  const size_t npairs = n * (n - 1) / 2;
  if (int rc = upload(c.src, pts, n * d * sizeof(double), c.stream)) return rc;
  CK(c.out.reserve(npairs * sizeof(double)));
  launch_pair_dist2_lower(c.src.as<double>(), (int)n, (int)d, c.out.as<double>(), c.stream);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(dist2_out, c.out.p, npairs * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  return 0;
}

// ------------------------------------------------------------------------------ H3 / T1 ----
int mlf_inside_ellipsoid(const double *pts, size_t np, size_t d, const double *ctr,
                         const double *invcov, double sqradius, uint8_t *mask, double *q_out) {
  if (int rc = check_dims(d)) return rc;
  if (np == 0) return 0;
  if (!pts || !ctr || !invcov || !mask) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  const int dp = pick_dp((int)d);
  if (int rc = prep_consts(c.small0, c.small1, ctr, invcov, (int)d, dp, false, c.stream)) return rc;
  if (int rc = upload(c.q, pts, np * d * sizeof(double), c.stream)) return rc;
  CK(c.mask.reserve(np));
  CK(c.out.reserve(np * sizeof(double)));
  PrepArgs a{};
  a.pts = c.q.as<double>();
  a.np = (long long)np;
  a.d = (int)d;
  a.do_ell = 1;
  a.ell_ctr = c.small0.as<double>();
  a.ell_A = c.small1.as<double>();
  a.enlarge = sqradius;
  a.mask = c.mask.as<uint8_t>();
  a.q_out = c.out.as<double>();
  CK(launch_prep(dp, a, c.stream));
  CK(hipMemcpyAsync(mask, c.mask.p, np, hipMemcpyDeviceToHost, c.stream));
  if (q_out) CK(hipMemcpyAsync(q_out, c.out.p, np * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  return 0;
}

int mlf_affine_transform(const double *pts, size_t np, size_t d, const double *ctr, const double *T,
                         const double *wrap_shift, double *out) {
  if (int rc = check_dims(d)) return rc;
  if (np == 0) return 0;
  if (!pts || !ctr || !T || !out) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  const int dp = pick_dp((int)d);
  if (int rc = prep_consts(c.small0, c.small1, ctr, T, (int)d, dp, true, c.stream)) return rc;
  if (wrap_shift) {
    std::vector<double> w = pad_vector(wrap_shift, (int)d, dp, NAN);
    if (int rc = upload(c.small2, w.data(), w.size() * sizeof(double), c.stream)) return rc;
    CK(hipStreamSynchronize(c.stream));
  }
  // device in: read in place; device out: written in place (the device-resident rebuild whitens its live points twice)
  const bool in_dev = is_device_pointer(pts), out_dev = is_device_pointer(out);
  const double *src = pts;
  if (!in_dev) {
    if (int rc = upload(c.q, pts, np * d * sizeof(double), c.stream)) return rc;
    src = c.q.as<double>();
  }
  double *dst = out;
  if (!out_dev) {
    CK(c.out.reserve(np * d * sizeof(double)));
    dst = c.out.as<double>();
  }
  if (dp <= 64) {
    // wave-per-8-rows form of the same chain (k_whiten_rows: bit for bit what k_prep computes, 36 -> 5 us for 4000 rows)
    const int dp8 = (dp + 7) / 8 * 8;
    std::vector<double> t8((size_t)dp * dp8, 0.0);
    for (size_t k = 0; k < d; ++k)
      for (size_t cc = 0; cc < d; ++cc) t8[k * dp8 + cc] = T[k * d + cc];
    if (int rc = upload(c.small3, t8.data(), t8.size() * sizeof(double), c.stream)) return rc;
    CK(launch_whiten_rows(src, (long long)np, (int)d, dp, c.small0.as<double>(), c.small3.as<double>(), dp8,
                          wrap_shift ? c.small2.as<double>() : nullptr, dst, (long long)d, c.stream));
  } else {
    PrepArgs a{};
    a.pts = src;
    a.np = (long long)np;
    a.d = (int)d;
    a.do_tr = 1;
    a.lay_ctr = c.small0.as<double>();
    a.lay_Tt = c.small1.as<double>();
    a.wrap_shift = wrap_shift ? c.small2.as<double>() : nullptr;
    a.t_out = dst;
    a.ldt = (long long)d;
    CK(launch_prep(dp, a, c.stream));
  }
  if (!out_dev) CK(hipMemcpyAsync(out, c.out.p, np * d * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));   // the host vectors above leave scope; a host destination is read next
  return 0;
}

// ------------------------------------------------------------- bootstrap ellipsoid stats ----
int mlf_bootstrap_moments(const double *u, size_t n, size_t d, const uint8_t *selected, size_t B,
                          double *mean_out, double *cov_out) {
  if (int rc = check_dims(d)) return rc;
  if (B == 0) return 0;
  if (!u || !selected || !mean_out || !cov_out || n == 0) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  if (int rc = upload(c.src, u, n * d * sizeof(double), c.stream)) return rc;
  if (int rc = upload(c.selbytes, selected, B * n, c.stream)) return rc;
  CK(c.small0.reserve(B * d * sizeof(double)));
  CK(c.small1.reserve(B * sizeof(int)));
  CK(c.out.reserve(B * d * d * sizeof(double)));
  CK(c.small2.reserve(B * n * sizeof(int)));
  launch_boot_moments(c.src.as<double>(), (int)n, (int)d, c.selbytes.as<uint8_t>(), (int)B,
                      c.small0.as<double>(), c.small1.as<int>(), c.out.as<double>(), c.small2.as<int>(), c.stream);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(mean_out, c.small0.p, B * d * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  CK(hipMemcpyAsync(cov_out, c.out.p, B * d * d * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  return 0;
}

int mlf_bootstrap_factor(const double *u, size_t n, size_t d, const uint8_t *selected, size_t B, double scale,
                         double *f_out) {
  if (int rc = check_dims(d)) return rc;
  if (B == 0) return 0;
  if (!u || !selected || !f_out || n == 0) return fail_arg(MLF_E_BADARG, "null pointer");
  if (d > 64) return fail_arg(MLF_E_DIM, "mlf_bootstrap_factor covers d <= 64 (use the moments + quadratic-form calls above that)");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  if (int rc = upload(c.src, u, n * d * sizeof(double), c.stream)) return rc;
  if (int rc = upload_any(c.selbytes, selected, B * n, c.stream)) return rc;
  CK(c.small0.reserve(B * d * sizeof(double)));
  CK(c.small1.reserve(B * sizeof(int)));
  CK(c.out.reserve(B * d * d * sizeof(double)));
  CK(c.small2.reserve(B * n * sizeof(int)));
  CK(c.small3.reserve(B * sizeof(unsigned long long)));
  launch_boot_moments(c.src.as<double>(), (int)n, (int)d, c.selbytes.as<uint8_t>(), (int)B, c.small0.as<double>(),
                      c.small1.as<int>(), c.out.as<double>(), c.small2.as<int>(), c.stream);
  CK(hipGetLastError());
  CK(hipMemsetAsync(c.small3.p, 0, B * sizeof(unsigned long long), c.stream));
  CK(c.M.reserve(boot_cholmax_scratch_bytes((int)d, (int)B)));
  CK(launch_boot_cholmax(c.src.as<double>(), (int)n, (int)d, c.selbytes.as<uint8_t>(), (int)B, c.small0.as<double>(),
                         c.out.as<double>(), scale, c.small3.as<unsigned long long>(), c.M.p, c.stream));
  std::vector<unsigned long long> bits(B);
  CK(hipMemcpyAsync(bits.data(), c.small3.p, B * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  for (size_t b = 0; b < B; ++b) {
    double v;
    if (bits[b] == ~0ull) {
      v = std::numeric_limits<double>::quiet_NaN();
    } else {
      memcpy(&v, &bits[b], sizeof v);
    }
    f_out[b] = v;
  }
  return 0;
}

int mlf_bootstrap_quadform_max(const double *u, size_t n, size_t d, const uint8_t *selected,
                               size_t B, const double *ctr, const double *invcov, double *f_out) {
  if (int rc = check_dims(d)) return rc;
  if (B == 0) return 0;
  if (!u || !selected || !ctr || !invcov || !f_out || n == 0) return fail_arg(MLF_E_BADARG, "null pointer");
  if (int rc = ensure_ctx()) return rc;
  Ctx &c = g_ctx;
  const int dp = pick_dp((int)d);
  if (int rc = upload(c.src, u, n * d * sizeof(double), c.stream)) return rc;
  if (int rc = upload(c.selbytes, selected, B * n, c.stream)) return rc;
  // all B padded centres / matrices in one upload
  std::vector<double> pc((size_t)B * dp, 0.0), pm((size_t)B * d * dp, 0.0);
  for (size_t b = 0; b < B; ++b) {
    for (size_t k = 0; k < d; ++k) pc[b * dp + k] = ctr[b * d + k];
    for (size_t r = 0; r < d; ++r)
      for (size_t k = 0; k < d; ++k) pm[(b * d + r) * dp + k] = invcov[(b * d + r) * d + k];
  }
  if (int rc = upload(c.small0, pc.data(), pc.size() * sizeof(double), c.stream)) return rc;
  if (int rc = upload(c.small1, pm.data(), pm.size() * sizeof(double), c.stream)) return rc;
  const size_t nblk = wide_dims(dp) ? (size_t)quadmax_blocks_wide((int)n, (int)d) : (n + 255) / 256;
  CK(c.small2.reserve(B * nblk * sizeof(double)));
  QuadMaxArgs qa{};
  qa.u = c.src.as<double>();
  qa.n = (int)n;
  qa.d = (int)d;
  qa.selected = c.selbytes.as<uint8_t>();
  qa.ctr = c.small0.as<double>();
  qa.invcov = c.small1.as<double>();
  qa.part = c.small2.as<double>();
  CK(launch_boot_quadmax(dp, qa, (int)B, c.stream));
  std::vector<double> part(B * nblk);
  CK(hipMemcpyAsync(part.data(), c.small2.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  CK(hipStreamSynchronize(c.stream));
  for (size_t b = 0; b < B; ++b) {
    double m = -INFINITY;
    for (size_t k = 0; k < nblk; ++k) {
      const double o = part[b * nblk + k];
      m = (o > m || o != o) ? o : m;
    }
    f_out[b] = m;
  }
  return 0;
}

int mlf_loglike_gauss(const double *params, size_t d, size_t n, const double *centers, double sigma,
                      double *like) {
  return loglike_host(0, params, d, n, centers, sigma, like);
}
int mlf_loglike_eggbox(const double *params, size_t d, size_t n, double *like) {
  return loglike_host(1, params, d, n, nullptr, 0.0, like);
}
int mlf_loglike_eggbox2(const double *params, size_t d, size_t n, double *like) {
  return loglike_host(2, params, d, n, nullptr, 0.0, like);
}
int mlf_loglike_rosenbrock(const double *params, size_t d, size_t n, double *like) {
  return loglike_host(3, params, d, n, nullptr, 0.0, like);
}

int mlf_loglike_dev(int kind, const double *d_params, size_t d, size_t n, const double *d_aux,
                    double sigma, double *d_like, void *stream) {
  if (kind < 0 || kind > 3 || d == 0) return fail_arg(MLF_E_BADARG, "bad likelihood kind / dimension");
  if (n == 0) return 0;
  if (!d_params || !d_like || (kind == 0 && !d_aux)) return fail_arg(MLF_E_BADARG, "null pointer");
  launch_loglike(kind, d_params, (int)d, (long long)n, d_aux, sigma, d_like, (hipStream_t)stream);
  CK(hipGetLastError());
  return 0;
}

}  // extern "C"
