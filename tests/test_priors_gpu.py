"""Prior library (ultranest_amd.priors) on the GPU: every family against the mpmath reference of prior_reference over a grid
that reaches into both tails, seams between branches, bit patterns that must be exact, independence of the row's position and of
the model form, the two block priors, every device route with a mixed model, and an evidence.

Measured on the MI355X (largest |error| / (1e-12 S) per family over its three settings; bound and S: prior_reference):
see DESIGN.md 7f for the table this test prints."""
import mpmath as mp
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import prior_reference as PR  # noqa: E402
from ultranest_amd import priors as P  # noqa: E402
from ultranest_amd import usermodels  # noqa: E402

U = PR.grid()
GAUSS = usermodels.GAUSS_LOGLIKE % 0.5


def _columns(priors, u):
    """every prior of the list evaluated on the same 1-d u: an (len(u), len(priors)) array from one model"""
    pt = P.PriorTransform(priors)
    return pt.transform(np.repeat(u[:, None], pt.ndim, axis=1))


@pytest.mark.parametrize("name", sorted(PR.FAMILIES))
def test_family_against_the_reference(name):
    priors = PR.family(name)
    got = _columns(priors, U)
    assert got.shape == (len(U), 3)
    inner = (U >= 2.0 ** -53) & (U <= 1 - 2.0 ** -53)
    worst = 0.0
    for k, prior in enumerate(priors):
        col = got[:, k]
        e = PR.excess(prior, U, col)
        print("%s %r: largest error %.3g of the bound at u = %r" % (name, {a: b for a, b in vars(prior).items() if a != "name"},
                                                                     e.max(), U[np.argmax(e)]))
        worst = max(worst, e.max())
        assert np.isfinite(col[inner]).all()
        assert e.max() <= 1.0, (name, k, U[np.argmax(e)])
        assert (np.diff(col) >= 0).all(), (name, k, U[1:][np.diff(col) < 0])        # no seam between branches
        if name == "Uniform":
            assert np.array_equal(col, prior.lo + U * prior.w)
        if name == "Fixed":
            assert np.array_equal(col, np.full(len(U), prior.v))
    print("MEASURED %s %.3g" % (name, worst))


def test_standard_normal_is_odd_bit_for_bit():
    """u = k 2^-10: 1 - u is exact, so Normal(0, 1) at u and at 1 - u are one normcdfinv call and its negation"""
    u = np.arange(1, 1024) * 2.0 ** -10
    z = _columns([P.Normal(0.0, 1.0)], u)[:, 0]
    zr = _columns([P.Normal(0.0, 1.0)], 1.0 - u)[:, 0]
    assert np.array_equal(z, -zr) and z[511] == 0.0 and (z[:511] < 0).all() and (np.diff(z) > 0).all()


def _mixed():
    from test_priors_compile import SUMMED, mixed_priors
    pt = P.PriorTransform(mixed_priors())
    return pt, pt.model(GAUSS, aux=np.zeros(12), name="mixed12"), pt.model(SUMMED, aux=np.zeros(24), nterms=24, name="mixed12_sum")


def test_position_independence():
    """the same u row gives the same p bits at every batch size (1: one lane; 63 / 64 / 65: a wave's edge; 257: five waves), at
    another position in the batch, from the stand-alone callback and in the summed form, where the transform runs on one lane
    of the row's wave"""
    pt, m, s = _mixed()
    rs = np.random.RandomState(12)
    u = rs.uniform(size=(257, 12))
    u[:20, 3] = U[:20]          # both tails, in the truncated normal's and the normal's column
    u[:20, 2] = U[-20:]
    full = m.transform(u)
    assert np.isfinite(full).all()
    for n in (1, 63, 64, 65, 257):
        assert np.array_equal(m.transform(u[:n]), full[:n]), n
        assert np.array_equal(m.transform(u[-n:]), full[-n:]), n
    perm = rs.permutation(257)
    assert np.array_equal(m.transform(u[perm]), full[perm])
    assert np.array_equal(s.transform(u), full) and np.array_equal(s.transform(u[perm][:65]), full[perm][:65])
    assert np.array_equal(pt.transform(u), full)
    # and the columns are those of one-family models: a column does not depend on its neighbours
    assert np.array_equal(full[:, 2], _columns([P.Normal(0.0, 2.0)], u[:, 2])[:, 0])
    assert np.array_equal(full[:, 6], np.full(257, 0.25))


def _block_rows(n, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.uniform(size=(40, n)), rs.choice(U[:8], size=(8, n)), rs.choice(U[-8:], size=(8, n))])


@pytest.mark.parametrize("n", [1, 2, 8])
def test_multivariate_normal_block(n):
    from test_prior_reference import _mvn
    prior = _mvn(n)
    u = _block_rows(n, 20 + n)
    z = P.PriorTransform([P.Normal(0.0, 1.0)] * n).transform(u)
    got = P.PriorTransform([prior]).transform(u)
    assert np.array_equal(got, PR.mvn_restatement(prior.mean, prior.L, z))
    ref, S = PR.reference(prior, u), PR.mvn_scale(prior, z)
    worst = max(float(abs(mp.mpf(float(got[r, i])) - ref[r][i]) / (PR.RTOL * S[r, i])) for r in range(len(u)) for i in range(n))
    print("MEASURED MultivariateNormal%d %.3g" % (n, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("n", [1, 2, 5])
def test_ordered_uniform_block(n):
    """seeded draws: t_k = t_(k+1) exp(log(u_k) / (k + 1)) equals t_(k+1) only where u_k lies within (k + 1) 2^-53 of 1, so on
    draws the vector is strictly ascending; class A with loc = lo and scale = hi - lo"""
    prior = P.OrderedUniform(-2.0, 5.0, n)
    u = np.random.RandomState(30 + n).uniform(size=(64, n))
    got = P.PriorTransform([prior]).transform(u)
    assert (np.diff(got, axis=1) > 0).all() and (got >= -2.0).all() and (got <= 5.0).all()
    ref = PR.reference(prior, u)
    worst = 0.0
    with mp.workdps(PR.DPS):
        for r in range(len(u)):
            for k in range(n):
                S = PR.scale(prior, u[r, k], ref[r][k])
                worst = max(worst, float(abs(mp.mpf(float(got[r, k])) - ref[r][k]) / (PR.RTOL * S)))
    print("MEASURED OrderedUniform%d %.3g" % (n, worst))
    assert worst <= 1.0


# ---- routes ----------------------------------------------------------------------------------------------------------

NLIVE = 100


def _route_model():
    priors = [P.Uniform(-1.0, 1.0), P.LogUniform(0.1, 10.0), P.Normal(0.0, 1.0), P.TruncatedNormal(0.0, 1.0, -1.0, 2.0),
              P.Exponential(1.0)]
    pt = P.PriorTransform(priors)
    centers = np.array([PR.standin(p, np.array([0.5]))[0] for p in priors])       # the likelihood peaks at u = 0.5
    return pt.model(GAUSS, aux=centers, name="route5")


def _live(seed=77):
    import test_tregion_refill_gpu as T
    u = T._blob(4 * NLIVE, 5, seed)[:NLIVE]
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


def test_gated_refill_equals_the_host_sequence():
    import test_tregion_refill_gpu as T
    M = _route_model()
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


def test_nested_sampling_evidence_under_normal_priors():
    """gauss_normal_prior(4): sigma 0.1 under Normal(0.5, 0.5) priors, analytic ln Z = sum_k ln N(c_k; 0.5, sqrt(0.26)); the
    centres lie within half a prior sigma of the prior's mean and the posterior is a fifth of the prior wide: well inside the
    bulk (and a shorter run than under the default prior_sigma = 1).  Every refill is a user refill on the device (gated: the
    priors are not affine, so the driver keeps its t-region)"""
    from ultranest_amd import kernels
    from ultranest_amd.harness import StaticNestedSampler
    from ultranest_amd.regions import DeviceRNG
    G, want = usermodels.gauss_normal_prior(4, prior_sigma=0.5)
    assert np.abs(usermodels.gauss_centers(4) - 0.5).max() < 0.5 * 0.5
    calls = []
    orig = kernels.DeviceRegion.refill_user

    def counting(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    kernels.DeviceRegion.refill_user = counting
    try:
        s = StaticNestedSampler(4, G.loglike, transform=G.transform, build_tregion=True, num_live_points=400, ndraw=4096,
                                seed=2, device_rng=DeviceRNG(21))
        res = s.run(dlogz=0.5)
    finally:
        kernels.DeviceRegion.refill_user = orig
    print(res["logz"], res["logzerr"], want, len(calls))
    assert abs(res["logz"] - want) < 4 * res["logzerr"] + 0.15, (res, want)
    assert len(calls) > 10 and s.phases["refills"] == len(calls)
