"""The covariance form of a user model (DeviceModel(..., ncov=n)) on the GPU: the factor bit for bit against the numpy restatement of
the arithmetic contract (cov_reference.restate), the likelihood against an mpmath reference within the derived bound, the failure
rule, independence of position and mask, every device route against the default-form twin (usermodels.gp_sqexp_twin: the same
arithmetic in one thread, so the two agree bit for bit), and ln Z of gp_sqexp(20) against a quadrature.

The bit-for-bit cases use a model whose entries numpy reproduces exactly (`TABLE`: products, sums and differences of table values
and parameters; no exp); square root and division are IEEE operations on both sides."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cov_reference as R  # noqa: E402
import test_devicemodel_gpu as G  # noqa: E402   (its MLFriends region of a live set and its run comparison)
import test_summed_model_gpu as S  # noqa: E402   (eval_dev on torch tensors, the whole-refill comparisons)
import test_tregion_refill_gpu as TR  # noqa: E402   (the gated refill against the host sequence)
from ultranest_amd import devicemodel as dm  # noqa: E402
from ultranest_amd import usermodels  # noqa: E402

# aux = the packed lower triangle of K0, then r0.  p = (scale, jitter, mean, kbad, bump):
# K_ij = K0_ij * scale (+ jitter on the diagonal, + bump at the diagonal entry kbad), r_i = r0_i - mean
TABLE = r"""
#define MLF_TABLE_N %d
__device__ double mlf_user_cov(const double *p, int d, const double *aux, long long naux, int i, int j) {
  double v = aux[i * (i + 1) / 2 + j] * p[0];
  if (i == j) {
    v = v + p[1];
    if (i == (int)p[3]) v = v + p[4];
  }
  return v;
}
__device__ double mlf_user_resid(const double *p, int d, const double *aux, long long naux, int i) {
  return aux[MLF_TABLE_N * (MLF_TABLE_N + 1) / 2 + i] - p[2];
}
"""
TABLE_TRANSFORM = r"""
__device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux) {
  p[0] = u[0] * 2.0 + 0.5;
  p[1] = u[1] * 0.5 + 0.25;
  p[2] = u[2] * 4.0 + -2.0;
  p[3] = u[3] * 1.0 + -1.0;
  p[4] = u[4] * 1.0 + 0.0;
}
"""
NMAX = dm.max_ncov(5, True)


@functools.lru_cache(maxsize=None)
def _table(n, transform=False):
    rs = np.random.RandomState(100 + n)
    B = rs.normal(size=(n, n))
    K0 = B.dot(B.T) / n + np.eye(n)
    r0 = rs.normal(size=n)
    rows, cols = np.tril_indices(n)
    model = dm.DeviceModel(5, TABLE % n, TABLE_TRANSFORM if transform else None, aux=np.concatenate([K0[rows, cols], r0]),
                           name="table%d" % n, ncov=n)
    return model, np.tril(K0), r0


def _table_transform(u):
    return u * np.array([2.0, 0.5, 4.0, 1.0, 1.0]) + np.array([0.5, 0.25, -2.0, -1.0, 0.0])


def _table_matrices(p, K0, r0):
    n = len(r0)
    Ks = K0[None] * p[:, 0, None, None]
    Ks = Ks + np.eye(n)[None] * p[:, 1, None, None]
    for m, row in enumerate(p):
        if 0 <= row[3] < n:
            Ks[m, int(row[3]), int(row[3])] += row[4]
    return Ks, r0[None, :] - p[:, 2:3]


def _table_params(m, seed):
    rs = np.random.RandomState(seed)
    return np.column_stack([rs.uniform(0.5, 2.5, m), rs.uniform(0.25, 0.75, m), rs.uniform(-2, 2, m), np.full(m, -1.0), np.zeros(m)])


# ---- the factor ----------------------------------------------------------------------------------------------------------------------

def test_the_python_lds_size_is_the_librarys():
    from ultranest_amd import _lib
    for n in (1, 2, 64, 65, NMAX, NMAX + 1, 300):
        assert dm.cov_lds_bytes(n) == _lib.lib().mlf_covmodel_lds_bytes(n), n
    assert dm.cov_lds_bytes(NMAX) + 2 * 5 * 8 <= dm.COV_LDS_CAP < dm.cov_lds_bytes(NMAX + 1) + 2 * 5 * 8


@pytest.mark.parametrize("transform", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 128, NMAX])
def test_cov_factor_bit_for_bit(n, transform):
    model, K0, r0 = _table(n, transform)
    if transform:
        u = np.random.RandomState(n).uniform(size=(3, 5)) * np.array([1, 1, 1, 0, 0])      # kbad = -1, bump = 0
        p = _table_transform(u)
        assert np.array_equal(model.transform(u), p)
        Lfac, z, L = model.cov_factor(u, with_transform=True)
    else:
        p = _table_params(3, n)
        Lfac, z, L = model.cov_factor(p)
    tri, Lw = R.restate_rows(*_table_matrices(p, K0, r0))
    Lfac_w, z_w = R.unpack(tri, n)
    assert Lfac.shape == (3, n, n) and z.shape == (3, n) and L.shape == (3,)
    assert np.array_equal(Lfac, Lfac_w), np.abs(Lfac - Lfac_w).max()
    assert np.array_equal(z, z_w), np.abs(z - z_w).max()
    # L from the device's own factor: the device's logarithm against numpy's, each within one ulp of the true value, so two ulps
    # apart per term (eps = 2 u each); the two sequential sums of n such terms then round differently by at most
    # 2 gamma_n sum |log L_kk|, and the two final operations on either side by 4 u |L|
    logs = np.abs(np.log(np.diagonal(Lfac, axis1=1, axis2=2))).sum(axis=1)
    tol = (4 * R.U + 2 * R.gamma(n)) * logs + 4 * R.U * np.abs(Lw)
    print("n = %d: max |L - finish(device factor)| / tolerance = %.3g" % (n, (np.abs(L - Lw) / tol).max()))
    assert (np.abs(L - Lw) <= tol).all(), (L, Lw, tol)
    assert np.array_equal(model.loglike(p), L)      # eval computes what cov_factor computed


@pytest.mark.parametrize("kappa", [1e1, 1e6, 1e10])
def test_loglike_against_mpmath_within_the_derived_bound(kappa):
    n = 24
    model = usermodels.gp_sqexp(n)
    x, y = usermodels.gp_data(n)
    lam = np.linalg.eigvalsh(R.gp_matrices([[0.0, 0.0, -50.0, 0.0]], x, y)[0][0]).max()      # (a = l = 1, no jitter)
    p = np.array([[0.0, 0.0, 0.5 * np.log(lam / kappa), 0.1], [0.0, 0.0, 0.5 * np.log(lam / kappa), -0.3]])
    K, r = R.gp_matrices(p, x, y)
    got_kappa = np.linalg.cond(K[0], 2)
    assert 0.3 * kappa < got_kappa < 3 * kappa, got_kappa      # the case is what it says
    L = model.loglike(p)
    worst = 0.0
    for k in range(len(p)):
        want = R.gp_mp_loglike(p[k], x, y)
        b = R.bound(K[k], r[k], entry_eps=R.GP_ENTRY_EPS)
        err = abs(float(want - R.mp_mpf(L[k])))
        worst = max(worst, err / b)
        assert err <= b, (kappa, k, L[k], float(want), err, b)
    print("kappa_2 = %.3g: largest error / bound = %.3g" % (got_kappa, worst))


# ---- failure ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 9, 65])
def test_failure_paths(n):
    model, K0, r0 = _table(n)
    p = _table_params(7, 7 * n)
    good = model.loglike(p)
    assert np.isfinite(good).all()
    ks = sorted({0, n // 2, n - 1})
    q = p.copy()
    for row, k in zip((1, 3, 5), ks):
        q[row, 3], q[row, 4] = k, -1e6            # this pivot is not > 0
    q[6, 3], q[6, 4] = ks[len(ks) // 2], np.nan   # a NaN entry
    bad = [1, 3, 5][:len(ks)]
    L = model.loglike(q)
    assert np.isneginf(L[bad]).all() and np.isnan(L[6]), L
    rest = [k for k in range(7) if k not in bad + [6]]
    assert np.array_equal(L[rest], good[rest])      # the rows after (and before) a failed row are unaffected
    Lfac, z, Lf = model.cov_factor(q)
    assert np.array_equal(Lf, L, equal_nan=True)
    lower = np.tril(np.ones((n, n), dtype=bool))
    for row in bad + [6]:
        assert np.isnan(Lfac[row][lower]).all() and np.isnan(z[row]).all()
    tri, Lw = R.restate_rows(*_table_matrices(q, K0, r0))
    assert np.array_equal(np.isneginf(Lw), np.isneginf(L)) and np.array_equal(np.isnan(Lw), np.isnan(L))
    assert np.array_equal(Lfac[rest], R.unpack(tri, n)[0][rest])


# ---- position and mask ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _pair(n=8):
    return usermodels.gp_sqexp(n, affine=True), usermodels.gp_sqexp_twin(n, affine=True)


def _gp_transform(u):
    return u * np.array(usermodels.GP_PRIOR_WIDTH) + np.array(usermodels.GP_PRIOR_LO)


@pytest.mark.parametrize("mask", ["members_first", "members_last", "alternating"])
def test_position_and_mask_do_not_matter(mask):
    model, twin = _pair()
    rs = np.random.RandomState(31)
    rows = rs.uniform(size=(5, 4))
    want = model.loglike(model.transform(rows))
    assert np.isfinite(want).all() and np.array_equal(model.transform(rows), _gp_transform(rows))
    for nb in (1, 5, 70):
        k = min(nb, 5)
        batch = rs.uniform(size=(nb, 4))
        member = dict(members_first=np.arange(nb) < k, members_last=np.arange(nb) >= nb - k,
                      alternating=np.arange(nb) % 2 == 0)[mask]
        at = np.flatnonzero(member)[:k]
        batch[at] = rows[:len(at)]
        p, L = S._eval_dev(model, batch, want_p=True, member=member)
        assert np.array_equal(L[at], want[:len(at)]), (nb, mask)
        assert np.isneginf(L[~member]).all() and (p[~member] == S.SENTINEL).all()      # non-members: p untouched
        assert np.array_equal(p[member], _gp_transform(batch[member]))
        # without a mask, and through eval: the same bits
        assert np.array_equal(S._eval_dev(model, batch)[1][at], model.loglike(batch[at]))
        assert np.array_equal(model.loglike(model.transform(batch))[at], want[:len(at)])


# ---- the routes at n = 8, against the default-form twin -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _live(n=60):
    u = np.clip(0.5 + 0.12 * np.random.RandomState(21).normal(size=(n, 4)), 0.01, 0.99)
    twin = _pair()[1]
    return u, twin.loglike(twin.transform(u))


def test_eval_and_eval_dev_equal_the_twin():
    model, twin = _pair()
    u = np.random.RandomState(22).uniform(size=(130, 4))
    p = model.transform(u)
    assert np.array_equal(p, twin.transform(u))
    a, b = model.loglike(p), twin.loglike(p)
    assert np.array_equal(a, b) and len(np.unique(a)) == 130 and np.isfinite(a).all()
    pa, La = S._eval_dev(model, u, want_p=True)
    pb, Lb = S._eval_dev(twin, u, want_p=True)
    assert np.array_equal(pa, pb) and np.array_equal(La, Lb) and np.array_equal(La, a)


@pytest.mark.parametrize("method", ["sample_from_boundingbox", "sample_from_points"])
def test_region_refill_equals_the_twin(method):
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = TR._gap_threshold(Ls)
    out = []
    for model in _pair():
        region = G._region(u)
        region.device_rng = DeviceRNG(seed=11)
        region.current_sampling_method = getattr(region, method)
        got = region.refill(2048, Lmin, model.transform, model.loglike)
        assert got is not None
        out.append(got + (region.device_rng.offset,))
    (ua, pa, La, nca, oa), (ub, pb, Lb, ncb, ob) = out
    assert nca == ncb > 0 and oa == ob and len(ua) > 10
    assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and np.array_equal(La, Lb) and (La > Lmin).all()


def test_gated_region_refill_equals_the_twin_and_the_host_sequence():
    """the gated program (mlf_user_rows_cov_tregion): against the host sequence on the same draws (TR._check), and bit for bit
    against the twin's gated refill"""
    u, _ = _live()
    out = []
    for model in _pair():
        region = G._region(u)
        got, host, tregion, Lmin = TR._check(region, "sample_from_boundingbox", model.transform, model.loglike, n=2048)
        out.append(got)
    (ua, pa, La, nca, oa), (ub, pb, Lb, ncb, ob) = out
    assert nca == ncb > 0 and oa == ob and len(ua) > 10
    assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and np.array_equal(La, Lb)


@pytest.mark.parametrize("philox", [False, True])
def test_population_slice_sampler_equals_the_twin(philox):
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = np.sort(Ls)[3]
    region = G._region(u)
    model, twin = _pair()
    a = S._slice_runs(twin, region, u, Ls, Lmin, DeviceRNG(5) if philox else None)
    b = S._slice_runs(model, region, u, Ls, Lmin, DeviceRNG(5) if philox else None)
    assert G._same_run(a, b) >= 1
    assert sum(x[3] for x in a) == sum(x[3] for x in b) > 0


def test_random_walk_refill_equals_the_twin():
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = Ls.min() - 0.5
    region = S._host_region(u)
    done = []
    for model in _pair():
        s = pop.PopulationRandomWalkSampler(64, 4, pop.generate_mixture_random_direction, 0.05, device_rng=DeviceRNG(6))
        first = s.__next__(region, Lmin, u, Ls, model.transform, model.loglike)
        done.append((s, first))
    (sa, fa), (sb, fb) = done
    assert fa[3] == fb[3] == 64 * 4 and np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]) and fa[2] == fb[2]
    S._same_refill(sa.last_refill, sb.last_refill)
    assert (sa.last_refill["L"] > Lmin).all()
    S._same_prepared(sa.prepared_samples, sb.prepared_samples)
    assert sa.device_rng.offset == sb.device_rng.offset > 0


def test_simple_slice_refill_equals_the_twin():
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = Ls.min() - 0.5
    region = S._host_region(u)
    done = []
    for model in _pair():
        s = pop.PopulationSimpleSliceSampler(64, 4, pop.generate_mixture_random_direction, scale_adapt_factor=0.8, max_it=20,
                                             device_rng=DeviceRNG(7))
        first = s.__next__(region, Lmin, u, Ls, model.transform, model.loglike)
        done.append((s, first))
    (sa, fa), (sb, fb) = done
    assert fa[3] == fb[3] > 0 and np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]) and fa[2] == fb[2]
    S._same_refill(sa.last_refill, sb.last_refill)
    assert (sa.last_refill["L"] > Lmin).all()
    S._same_prepared(sa.prepared_samples, sb.prepared_samples)
    assert sa.device_rng.offset == sb.device_rng.offset > 0


def test_a_covariance_model_of_the_other_gating_is_refused():
    model = _pair()[0]
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(model.code, 4, True, model.aux, gated=True, ncov=8)
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(model.code, 4, True, model.aux)      # a covariance program as a default model
    with pytest.raises(ValueError, match="compiled with"):
        dm._Handle(model.code, 4, True, model.aux, ncov=9)      # ncov sizes the factor rows: it must be the program's
    with pytest.raises(ValueError, match="ncov"):
        _pair()[1].cov_factor(np.zeros((1, 4)))


# ---- ln Z ------------------------------------------------------------------------------------------------------------------------------

def test_lnz_of_gp_sqexp_against_the_quadrature():
    from ultranest_amd.harness import StaticNestedSampler
    n = 20
    model = usermodels.gp_sqexp(n, affine=True)
    x, y = usermodels.gp_data(n)
    lo, width = usermodels.GP_PRIOR_LO, usermodels.GP_PRIOR_WIDTH
    fine, coarse = R.gp_lnz_quadrature(x, y, lo, width, 40), R.gp_lnz_quadrature(x, y, lo, width, 28)
    quad_err = abs(fine - coarse)
    s = StaticNestedSampler(4, model.loglike, transform=model.transform, num_live_points=200, ndraw=2048, seed=3)
    res = s.run(dlogz=0.2)
    print("ln Z = %.4f +- %.4f, quadrature %.4f (28 against 40 nodes: %.2g)" % (res["logz"], res["logzerr"], fine, quad_err))
    assert quad_err < 0.01
    assert abs(res["logz"] - fine) <= 3 * res["logzerr"] + quad_err, (res["logz"], res["logzerr"], fine, quad_err)
