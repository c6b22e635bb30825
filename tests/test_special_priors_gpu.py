"""The iterative prior families (ultranest_amd.priors: Gamma, ChiSquared, InverseGamma, Beta, StudentT, Dirichlet) on the GPU:
every setting of the golden fixture (tests/golden/g17_special_priors.npz, 60-digit mpmath roots) inside its bound from
u = 2^-1022 to 1 - 2^-53, monotone and finite columns, the Student-t quantile odd bit for bit, a row's bits independent of
batch size, position and model form, the Dirichlet block against its numpy restatement, every device route with a six-column
model, and an evidence with an analytic value.

The bounds are special_prior_reference's; the largest error / bound per family that the first test prints is the "device"
column of the table in DESIGN.md 7f."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import special_prior_reference as SR  # noqa: E402
from ultranest_amd import priors as P  # noqa: E402
from ultranest_amd import usermodels  # noqa: E402

GAUSS = usermodels.GAUSS_LOGLIKE % 0.5
ONE_COLUMN = ("Gamma", "ChiSquared", "InverseGamma", "Beta", "StudentT")


def _columns(priors, u):
    """every prior of the list evaluated on the same 1-d u: an (len(u), len(priors)) array from one model"""
    pt = P.PriorTransform(priors)
    return pt.transform(np.repeat(u[:, None], pt.ndim, axis=1))


_cache = {}


def _family(family):
    """(names, priors, u, columns on the device) of one family's fixture settings, computed once"""
    if family not in _cache:
        names = SR.settings(family)
        loaded = [SR.load(n) for n in names]
        u = loaded[0][1]
        assert all(np.array_equal(u, ld[1]) for ld in loaded) and len(u) <= 1024
        _cache[family] = (names, [ld[0] for ld in loaded], u, _columns([ld[0] for ld in loaded], u))
    return _cache[family]


@pytest.mark.parametrize("family", ONE_COLUMN)
def test_every_setting_is_inside_its_bound(family):
    names, priors, u, got = _family(family)
    worst = 0.0
    for k, name in enumerate(names):
        e = SR.excess(priors[k], u, got[:, k], SR.load(name)[2])
        print("%s %r: largest error %.3g of the bound at u = %r" % (name, priors[k].consts, e.max(), u[np.argmax(e)]))
        worst = max(worst, e.max())
    print("MEASURED %s %.3g" % (family, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("family", ONE_COLUMN)
def test_columns_are_monotone_and_finite(family):
    names, priors, u, got = _family(family)
    assert (np.diff(u) > 0).all() and np.isfinite(got).all()
    for k, name in enumerate(names):
        assert (np.diff(got[:, k]) >= 0).all(), (name, u[1:][np.diff(got[:, k]) < 0])
    if family in ("Gamma", "ChiSquared", "InverseGamma"):
        assert (got >= 0).all()
    if family == "Beta":
        assert (got >= 0).all() and (got <= 1).all()


@pytest.mark.parametrize("nu", [1.0, 30.0])
def test_student_t_is_odd_bit_for_bit(nu):
    """u = k 2^-10: 1 - u is exact, so StudentT(nu, 0, 1) at u and at 1 - u are one iteration and its negation"""
    u = np.arange(1, 1024) * 2.0 ** -10
    t = _columns([P.StudentT(nu)], u)[:, 0]
    tr = _columns([P.StudentT(nu)], 1.0 - u)[:, 0]
    assert np.array_equal(t, -tr) and t[511] == 0.0 and (t[:511] < 0).all() and (np.diff(t) > 0).all()


def _mixed():
    from test_special_priors_compile import special_mixed
    from test_priors_compile import SUMMED
    pt = P.PriorTransform(special_mixed())
    return pt, pt.model(GAUSS, aux=np.zeros(9), name="special9"), pt.model(SUMMED, aux=np.zeros(18), nterms=18, name="special9_sum")


def test_position_and_form_independence():
    """the same u row gives the same p bits at every batch size (1: one lane; 63 / 64 / 65: a wave's edge; 1024: sixteen waves,
    whose lanes end their iterations at different counts), at another position in the batch, from the stand-alone callback and
    in the summed form, where the transform runs on one lane of the row's wave.  (The gated form is held to the same bits by
    test_gated_refill_equals_the_host_sequence.)"""
    pt, m, s = _mixed()
    rs = np.random.RandomState(12)
    u = rs.uniform(size=(1024, 9))
    g = SR.grid()
    u[:20, :] = g[:20, None]          # both tails in every column
    u[20:40, :] = g[-20:, None]
    full = m.transform(u)
    assert np.isfinite(full).all()
    for n in (1, 63, 64, 65, 1024):
        assert np.array_equal(m.transform(u[:n]), full[:n]), n
        assert np.array_equal(m.transform(u[-n:]), full[-n:]), n
    perm = rs.permutation(1024)
    assert np.array_equal(m.transform(u[perm]), full[perm])
    assert np.array_equal(s.transform(u), full) and np.array_equal(s.transform(u[perm][:65]), full[perm][:65])
    assert np.array_equal(pt.transform(u), full)
    # and the columns are those of one-family models: a column does not depend on its neighbours
    assert np.array_equal(full[:, 0], _columns([P.Gamma(2.5, 3.0)], u[:, 0])[:, 0])
    assert np.array_equal(full[:, 4], _columns([P.Beta(2.0, 3.0)], u[:, 4])[:, 0])
    assert np.array_equal(full[:, 6], _columns([P.StudentT(5.0, 1.0, 0.5)], u[:, 6])[:, 0])
    assert np.array_equal(full[:, 2], _columns([P.Gamma(2.5, 2.0)], u[:, 2])[:, 0])          # ChiSquared(5) is Gamma(5/2, 2)


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_dirichlet_block(n):
    name = "Dirichlet_%d" % n
    prior, u, ref = SR.load(name)
    g = P.PriorTransform(prior.gammas()).transform(u)          # the device's own g rows
    e = SR.excess(prior, u, g, ref)
    print("MEASURED Dirichlet%d %.3g" % (n, e.max()))
    assert e.max() <= 1.0
    got = P.PriorTransform([prior]).transform(u)
    assert np.array_equal(got, SR.dirichlet_restatement(g))
    assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
    for row in got:
        assert abs(math.fsum(row) - 1.0) <= n * 2.0 ** -52


@pytest.mark.parametrize("n", [1, 3])
def test_dirichlet_block_whose_gammas_all_underflow(n):
    """alpha = 0.1 and u = 1e-300 throughout: every g is 1e-3000 in exact arithmetic, 0 in binary64; the sum is 0 and the
    row is 1 / n"""
    prior = P.Dirichlet([0.1] * n)
    u = np.full((2, n), 1e-300)
    u[1] = 0.5
    assert np.array_equal(P.PriorTransform(prior.gammas()).transform(u)[0], np.zeros(n))
    got = P.PriorTransform([prior]).transform(u)
    assert np.array_equal(got[0], np.full(n, 1.0 / n))
    assert np.array_equal(got[1], np.full(n, got[1][0])) and abs(got[1].sum() - 1.0) <= n * 2.0 ** -52


# ---- routes ----------------------------------------------------------------------------------------------------------

NLIVE = 100


def _route_priors(simplex=True):
    """six columns.  The two columns of Dirichlet(2) sum to 1, so no ellipsoid in parameter space has a volume: with
    `simplex` False the block is Dirichlet(1) (the constant 1, which a t-region leaves out as a fixed column) and a
    ChiSquared column takes the sixth place"""
    head = [P.Gamma(2.5, 1.0), P.Beta(2.0, 3.0), P.StudentT(5.0, 0.0, 1.0), P.InverseGamma(3.0, 2.0)]
    return head + ([P.Dirichlet([1.5, 2.5])] if simplex else [P.Dirichlet([2.0]), P.ChiSquared(5.0)])


_route = {}


def _route_model(simplex=True):
    if simplex not in _route:
        pt = P.PriorTransform(_route_priors(simplex))
        assert pt.ndim == 6
        centers = pt.transform(np.full((1, 6), 0.5))[0]          # the likelihood peaks at u = 0.5
        _route[simplex] = pt.model(GAUSS, aux=centers, name="special_route6_%d" % simplex)
    return _route[simplex]


def _live(seed=77):
    import test_tregion_refill_gpu as T
    u = T._blob(4 * NLIVE, 6, seed)[:NLIVE]
    assert len(u) == NLIVE
    return u


def test_refill_equals_the_host_sequence():
    import test_tregion_refill_gpu as T
    from ultranest_amd.regions import DeviceRNG
    M = _route_model()
    region = T._region_of("MLFriends", _live())
    method = "sample_from_wrapping_ellipsoid"
    region.current_sampling_method = getattr(region, method)
    region.device_rng = DeviceRNG(41)
    pts = region.sample(T.N)
    nxt = region.device_rng.offset
    p_host = M.transform(pts)
    L_host = M.loglike(p_host)
    Lmin = T._gap_threshold(L_host)
    u, p, L, nc, offset = T._gated(region, method, T.N, Lmin, M.transform, M.loglike, None)
    keep = L_host > Lmin
    assert nc == len(pts) and offset == nxt and 10 < keep.sum() < len(pts)
    assert np.array_equal(u, pts[keep]) and np.array_equal(p, p_host[keep]) and np.array_equal(L, L_host[keep])


def test_a_dirichlet_block_has_no_tregion():
    """p_4 + p_5 = 1 on every row: the parameter rows span five dimensions and the wrapping ellipsoid's bootstrap meets a
    singular matrix, as in the reference; the drivers catch it and run without a t-region (harness.py), which is why the
    evidence run below and a run with a Dirichlet prior need no special care, and why the gated refill is checked with
    Dirichlet(1) in the block's place"""
    import test_tregion_refill_gpu as T
    M = _route_model()
    p = M.transform(_live())
    assert np.abs(p[:, 4] + p[:, 5] - 1.0).max() <= 2.0 ** -52
    with pytest.raises(np.linalg.LinAlgError):
        T._tregion(p)


def test_gated_refill_equals_the_host_sequence():
    import test_tregion_refill_gpu as T
    M = _route_model(simplex=False)
    region = T._region_of("MLFriends", _live())
    got, host, tregion, Lmin = T._check(region, "sample_from_wrapping_ellipsoid", M.transform, M.loglike)
    keep = host[3] > Lmin
    assert keep.sum() > 10 and np.array_equal(got[2], host[3][keep])


def _walk_problem():
    import test_tregion_refill_gpu as T
    M = _route_model()
    u = _live()
    region = T._region_of("MLFriends", u)
    Ls = M.loglike(M.transform(u))
    return M, u, region, Ls, Ls.min() - 0.5        # every live point lies above the threshold, as in a run


def _rows_are_the_models(M, rows, Lmin):
    found = [(u, p, L) for u, p, L, nc in rows if u is not None]
    u, p, L = np.array([f[0] for f in found]), np.array([f[1] for f in found]), np.array([f[2] for f in found])
    want_p = M.transform(u)
    assert np.array_equal(p, want_p) and np.array_equal(L, M.loglike(want_p)) and (L > Lmin).all()
    return len(found)


@pytest.mark.parametrize("which", ["randomwalk", "simpleslice"])
def test_whole_refill_samplers_hand_out_the_models_rows(which):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    M, u, region, Ls, Lmin = _walk_problem()
    if which == "randomwalk":
        s = pop.PopulationRandomWalkSampler(popsize=64, nsteps=6, generate_direction=pop.generate_random_direction, scale=0.3,
                                            device_rng=DeviceRNG(6))
    else:
        s = pop.PopulationSimpleSliceSampler(64, 4, pop.generate_random_direction, device_rng=DeviceRNG(6))
    assert s._device_route(M.transform, M.loglike) is not None
    rows = [s.__next__(region, Lmin, u, Ls, M.transform, M.loglike) for _ in range(64)]
    assert rows[0][3] > 0 and all(r[3] == 0 for r in rows[1:]) and not s.prepared_samples        # one refill, on the device
    assert s.last_refill is not None and _rows_are_the_models(M, rows, Lmin) == 64


@pytest.mark.parametrize("philox", [False, True])
def test_population_slice_sampler_hands_out_the_models_rows(philox):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    M, u, region, Ls, Lmin = _walk_problem()
    np.random.seed(8)
    s = pop.PopulationSliceSampler(popsize=32, nsteps=6, generate_direction=pop.generate_mixture_random_direction, scale=0.5,
                                   device_rng=DeviceRNG(5) if philox else None)
    rows = [s.__next__(region, Lmin, u, Ls, M.transform, M.loglike) for _ in range(120)]
    assert _rows_are_the_models(M, rows, Lmin) > 5


# ---- evidence --------------------------------------------------------------------------------------------------------

CONJUGATE_LOGLIKE = r"""
__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {
  // two binomial observations (k of n successes) of p[0], p[1]; two Poisson counts y of p[2], p[3]; aux[6]: the constants
  double s = aux[6];
  s += aux[0] * log(p[0]) + (aux[1] - aux[0]) * log1p(-p[0]);
  s += aux[2] * log(p[1]) + (aux[3] - aux[2]) * log1p(-p[1]);
  s += aux[4] * log(p[2]) - p[2];
  s += aux[5] * log(p[3]) - p[3];
  return s;
}
"""


def _lbeta(a, b):
    return math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)


def _lchoose(n, k):
    return math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)


def test_nested_sampling_evidence_of_a_conjugate_model():
    """Beta(2, 3) priors under binomial likelihoods: ln Z = ln B(a + k, b + n - k) - ln B(a, b) + ln C(n, k) each; Gamma(3, 1)
    priors under Poisson likelihoods: the negative-binomial marginal, ln Z = lgamma(a + y) - lgamma(y + 1) - lgamma(a)
    - (a + y) ln 2 each.  The data (4 of 10 and 5 of 12 successes against a prior mean of 0.4; counts 3 and 2 against a prior
    mean of 3) put every posterior in its prior's bulk, so the run is short: batches of 512 draws make it more than a handful
    of refills.  Every refill is a user refill on the device."""
    from ultranest_amd import kernels
    from ultranest_amd.harness import StaticNestedSampler
    from ultranest_amd.regions import DeviceRNG
    a, b, ga = 2.0, 3.0, 3.0
    binom, counts = [(4.0, 10.0), (5.0, 12.0)], [3.0, 2.0]
    const = sum(_lchoose(n, k) for k, n in binom) - sum(math.lgamma(y + 1.0) for y in counts)
    want = sum(_lbeta(a + k, b + n - k) - _lbeta(a, b) + _lchoose(n, k) for k, n in binom)
    want += sum(math.lgamma(ga + y) - math.lgamma(y + 1.0) - math.lgamma(ga) - (ga + y) * math.log(2.0) for y in counts)
    pt = P.PriorTransform([P.Beta(a, b, name="p0"), P.Beta(a, b, name="p1"), P.Gamma(ga, 1.0, name="l0"), P.Gamma(ga, 1.0, name="l1")])
    aux = np.array([binom[0][0], binom[0][1], binom[1][0], binom[1][1], counts[0], counts[1], const])
    G = pt.model(CONJUGATE_LOGLIKE, aux=aux, name="conjugate4")
    calls = []
    orig = kernels.DeviceRegion.refill_user

    def counting(self, *args, **kw):
        calls.append(1)
        return orig(self, *args, **kw)

    kernels.DeviceRegion.refill_user = counting
    try:
        s = StaticNestedSampler(4, G.loglike, transform=G.transform, build_tregion=True, num_live_points=200, ndraw=512,
                                seed=2, device_rng=DeviceRNG(21))
        res = s.run(dlogz=0.5)
    finally:
        kernels.DeviceRegion.refill_user = orig
    print(res["logz"], res["logzerr"], want, len(calls))
    assert abs(res["logz"] - want) < 4 * res["logzerr"] + 0.15, (res, want)
    assert len(calls) > 5 and s.phases["refills"] == len(calls)
