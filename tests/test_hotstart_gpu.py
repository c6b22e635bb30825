"""Warm start on the GPU (ultranest_amd/hotstart.py): forms (a) and (b) as ordinary DeviceModels, at d = 1, 2, 5 on 257 rows.

Form (a): the umod-derived columns against the numpy restatement bit for bit (tests/hotstart_reference.py), the weight
within its derived bound of the exact sum; L equal to the inner model's own L plus p[d], bit for bit, for default, single-sum
and three-sum inner models.  Form (b) against a 40-digit restatement within 1e-12 * scale, where per row

    scale = 1 + |L_inner| + sum_i |logpdf_i| + sum_i (|dL_inner/dx_i| + |dlogpdf_i/dx_i|) * (|ctr_i| + err_i |t_i|)

(the magnitudes of the terms that make L, and the device quantile's own bound of 1e-12 times the magnitude of x_i carried
through the slopes of the inner likelihood and of the log-density, which the device takes from its x).  Then position and batch-size independence, rows with a NaN or -inf weight (never
kept), every device route against the model's own callbacks on the same draws, and nested-sampling runs of a separable
d = 3 Gaussian (sigma = 0.01) with 200 live points: form (b)'s ``logz + logz_offset`` against the analytic evidence, form (a)'s
``logz`` against ``ln integral Z_box(t) dt``, both with fewer iterations than the plain run."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hotstart_reference as HR  # noqa: E402
from ultranest_amd import devicemodel as dm  # noqa: E402
from ultranest_amd import hotstart as hs  # noqa: E402
from ultranest_amd import usermodels as um  # noqa: E402

DIMS = (1, 2, 5)
ROWS = 257
_cache = {}


def tables(d):
    if d not in _cache:
        up, w = HR.samples(d, 400)
        _cache[d] = (up, w) + tuple(hs.compute_quantile_intervals_refined(HR.STEPS, up, w))
    return _cache[d]


def cube_rows(d):
    """257 rows, d + 1 wide: t on every knot and on both neighbours of every inner knot, u within 2^-53 of both ends"""
    xp = tables(d)[4]
    rs = np.random.RandomState(50 + d)
    u = rs.uniform(size=(ROWS, d + 1))
    ts = list(xp[1:-1]) + [np.nextafter(x, 2.0) for x in xp[1:-1]] + [np.nextafter(x, -1.0) for x in xp[1:-1]] + [HR.EPS, 1.0 - HR.EPS]
    u[:len(ts), d] = ts
    u[0, :d] = HR.EPS
    u[1, :d] = 1.0 - HR.EPS
    u[len(ts), :d] = HR.EPS
    u[len(ts) + 1, :d] = 1.0 - HR.EPS
    return u


def contbox_of(inner, d):
    up, w = tables(d)[:2]
    names, L, T, vec = hs.get_auxiliary_contbox_parameterization(["x%d" % k for k in range(d)], inner.loglike, inner.transform, up, w)
    return L.model


# ---- form (a) ----

@pytest.mark.parametrize("d", DIMS)
def test_contbox_transform_against_the_restatement(d):
    up, w, ulos, uhis, xp = tables(d)
    u = cube_rows(d)
    umod, weight, j, decided = HR.contbox_restated(u, ulos, uhis, xp)
    assert decided.all() and set(j) == set(range(len(xp) - 1))
    plain = contbox_of(um.gauss(d), d)
    p = plain.transform(u)
    assert p.shape == (ROWS, d + 1) and np.array_equal(p[:, :d], umod)
    affine = contbox_of(um.gauss(d, affine=True), d)
    q = affine.transform(u)
    assert np.array_equal(q[:, :d], umod * 20.0 + -10.0) and np.array_equal(q[:, d], p[:, d])
    exact, bound = HR.weight_exact_and_bound(u, ulos, uhis, xp)
    e = HR.weight_excess(p[:, d], exact, bound)
    print("MEASURED device weight d=%d: largest error %.3g of the bound" % (d, e.max()))
    assert e.max() <= 1.0
    # the host form of the same problem returns these rows
    host = hs.get_auxiliary_contbox_parameterization(["a"] * d, HR.host_loglike, HR.host_transform, up, w, vectorized=True)[2](u)
    assert np.array_equal(host[:, :d], q[:, :d])


@pytest.mark.parametrize("kind", ["default", "nterms", "nsums3", "nderived"])
@pytest.mark.parametrize("d", DIMS)
def test_contbox_loglike_is_the_inner_loglike_plus_the_weight(d, kind):
    inner = {"default": lambda: um.gauss(d, affine=True), "nterms": lambda: um.linear_sum(d, 130, affine=True),
             "nsums3": lambda: um.amplitude_sum(d, 130, affine=True),
             "nderived": lambda: um.gauss_derived(max(d, 2), affine=True)}[kind]()
    d = inner.ndim
    aux = contbox_of(inner, d)
    u = cube_rows(d)
    p = aux.transform(u)
    L = aux.loglike(p)
    assert np.isfinite(L).all()
    pin = p[:, :d]
    assert np.array_equal(L, inner.loglike(pin) + p[:, d])
    if kind == "nderived":
        assert p.shape == (ROWS, d + 1 + 3) and np.array_equal(p[:, d + 1:], um.gauss_derived_columns(pin))
        assert np.array_equal(aux.loglike(p[:, :d + 1]), L)
    else:
        assert p.shape == (ROWS, d + 1)
    for n in (1, 63, 64, 65):
        assert np.array_equal(aux.transform(u[:n]), p[:n]) and np.array_equal(aux.transform(u[-n:]), p[-n:])
        assert np.array_equal(aux.loglike(p[:n]), L[:n]) and np.array_equal(aux.loglike(p[-n:]), L[-n:])
    perm = np.random.RandomState(3).permutation(ROWS)
    assert np.array_equal(aux.transform(u[perm]), p[perm]) and np.array_equal(aux.loglike(p[perm]), L[perm])


def _degenerate(d=2):
    """a contbox model whose boxes have a negative width for t < 0.5 (NaN weight), zero width at t = 0.5 (-inf) and grow to
    the cube above"""
    inner = um.gauss(d)
    xp = np.array([0.0, 0.5, 1.0])
    ulos = np.array([[0.6] * d, [0.5] * d, [0.0] * d])
    uhis = np.array([[0.4] * d, [0.5] * d, [1.0] * d])
    return hs._contbox_device(inner, True, ulos, uhis, xp)


def test_nan_and_minus_infinite_weights_are_never_kept():
    import test_tregion_refill_gpu as T
    d = 2
    aux = _degenerate(d)
    u = np.array([[0.3, 0.6, 0.25], [0.3, 0.6, 0.5], [0.3, 0.6, 0.75]])
    p = aux.transform(u)
    L = aux.loglike(p)
    assert np.isnan(p[0, d]) and p[1, d] == -np.inf and np.isfinite(p[2, d])
    assert np.isnan(L[0]) and L[1] == -np.inf and np.isfinite(L[2])
    live = T._blob(400, d + 1, 5, width=0.1)[:100]
    region = T._region_of("MLFriends", live)
    method = "sample_from_wrapping_ellipsoid"
    region.current_sampling_method = getattr(region, method)
    from ultranest_amd.regions import DeviceRNG
    region.device_rng = DeviceRNG(41)
    pts = region.sample(T.N)
    p_host = aux.transform(pts)
    L_host = aux.loglike(p_host)
    bad = ~np.isfinite(p_host[:, d])
    assert 100 < bad.sum() < len(pts) - 100 and np.array_equal(bad, pts[:, d] <= 0.5) and not np.isfinite(L_host[bad]).any()
    got_u, got_p, got_L, nc, offset = T._gated(region, method, T.N, -1e300, aux.transform, aux.loglike, None)
    assert np.array_equal(got_u, pts[~bad]) and np.array_equal(got_p, p_host[~bad]) and np.array_equal(got_L, L_host[~bad])
    assert np.isfinite(got_L).all() and (got_u[:, d] > 0.5).all()


# ---- form (b) ----

def _independent_case(d, df):
    up, w = tables(d)[:2]
    ctr, err, invcov = HR.moments(up, w)
    inner = um.gauss(d, sigma=0.1)
    L, T = hs.get_extended_auxiliary_independent_problem(inner.loglike, inner.transform, ctr, 2.0 * err, df=df)
    rs = np.random.RandomState(70 + d)
    u = rs.uniform(size=(ROWS, d))
    u[0], u[1] = HR.EPS, 1.0 - HR.EPS
    u[2] = 0.5
    return inner, L.model, ctr, 2.0 * err, u


@pytest.mark.parametrize("df", [1, 4.5])
@pytest.mark.parametrize("d", DIMS)
def test_independent_form_against_the_high_precision_restatement(d, df):
    inner, aux, ctr, err, u = _independent_case(d, df)
    centers, sigma = um.gauss_centers(d, 0.1), 0.1

    def inner_L(x):
        return -0.5 * (((x - centers) / sigma) ** 2).sum(axis=1) - 0.5 * math.log(2.0 * math.pi * sigma * sigma) * d

    x, s, L_want = HR.independent_exact(u, ctr, err, df, inner_L)
    assert (x > -1e-9).all() and (x < 1 + 1e-9).all()      # (w and lo are rounded: the ends may pass the cube's by an ulp)
    got = aux.transform(u)             # [x | p | logweight]; this inner model has no transform, so p is x
    assert got.shape == (ROWS, 2 * d + 1) and np.array_equal(got[:, d:2 * d], got[:, :d])
    L = aux.loglike(got)
    assert np.array_equal(aux.loglike(got[:, :d]), L)
    t = (x - ctr) / err
    xmag = np.abs(ctr) + err * np.abs(t)
    logpdf_abs = np.abs(np.log(err)).sum() + np.abs(0.5 * (df + 1) * np.log1p(t * t / df)).sum(axis=1) + d * abs(math.lgamma(0.5 * (df + 1)) - math.lgamma(0.5 * df) - 0.5 * math.log(df * math.pi))
    logpdf_slope = ((df + 1) * np.abs(t) / (df + t * t) / err * xmag).sum(axis=1)
    scale = 1.0 + np.abs(inner_L(x)) + logpdf_abs + logpdf_slope + (np.abs(x - centers) / sigma ** 2 * xmag).sum(axis=1)
    eL = np.abs(L - L_want) / (1e-12 * scale)
    ex = np.abs(got[:, :d] - x) / (1e-12 * xmag)
    weight_ref = hs.independent_tables(ctr, err, float(df))[5][6]
    ew = np.abs(got[:, 2 * d] - (-s + weight_ref)) / (1e-12 * (1.0 + logpdf_abs + logpdf_slope))
    print("MEASURED form (b) d=%d df=%g: L %.3g, x %.3g, logweight %.3g of 1e-12 * scale" % (d, df, eL.max(), ex.max(), ew.max()))
    assert eL.max() <= 1.0 and ex.max() <= 1.0 and ew.max() <= 1.0
    for n in (1, 64, 65):
        assert np.array_equal(aux.loglike(got[:n]), L[:n]) and np.array_equal(aux.transform(u[-n:]), got[-n:])
    perm = np.random.RandomState(4).permutation(ROWS)
    assert np.array_equal(aux.loglike(got[perm]), L[perm]) and np.array_equal(aux.transform(u[perm]), got[perm])
    assert aux.logz_offset == float(np.log(hs.independent_tables(ctr, err, float(df))[2]).sum())
    # the same problem over an inner model WITH a transform (the likelihood then holds the transformed row in a private array):
    # the same x and logweight bit for bit, p the affine map of x in numpy's bits, L the inner L of that p minus the same sum
    inner2 = um.gauss(d, sigma=0.1, affine=True)
    aux2 = hs.get_extended_auxiliary_independent_problem(inner2.loglike, inner2.transform, ctr, err, df=df)[0].model
    got2 = aux2.transform(u)
    assert np.array_equal(got2[:, :d], got[:, :d]) and np.array_equal(got2[:, 2 * d], got[:, 2 * d])
    assert np.array_equal(got2[:, d:2 * d], got[:, :d] * 20.0 + -10.0)
    L2 = aux2.loglike(got2)
    want2 = inner2.loglike(got2[:, d:2 * d]) + (got[:, 2 * d] - weight_ref)
    assert (np.abs(L2 - want2) <= 1e-12 * (scale + np.abs(want2))).all()
    assert np.array_equal(aux2.loglike(got2[perm][:65]), L2[perm][:65])


# ---- routes ----

def _route_problem(form):
    import test_tregion_refill_gpu as T
    d = 5
    if form == "a":
        aux = contbox_of(um.gauss(d, affine=True), d)
    else:
        aux = _independent_case(d, 1)[1]
    live = T._blob(400, aux.ndim, 77)[:100]
    if form == "a":
        # t below the first inner knot, where the box still grows with t: over [0.25, 0.75] the boxes of 400 equally weighted
        # samples coincide, the weight column is constant there and no ellipsoid in parameter space has a volume
        live[:, d] = 0.03 + 0.2 * np.random.RandomState(78).uniform(size=len(live))
    region = T._region_of("MLFriends", live)
    Ls = aux.loglike(aux.transform(live))
    assert np.isfinite(Ls).all()
    return aux, live, region, Ls


@pytest.mark.parametrize("form", ["a", "b"])
def test_refill_equals_the_host_sequence(form):
    import test_tregion_refill_gpu as T
    from ultranest_amd.regions import DeviceRNG
    aux, live, region, Ls = _route_problem(form)
    assert dm.device_route(aux.transform, aux.loglike) == (aux, True)
    method = "sample_from_wrapping_ellipsoid"
    region.current_sampling_method = getattr(region, method)
    region.device_rng = DeviceRNG(41)
    pts = region.sample(T.N)
    nxt = region.device_rng.offset
    p_host = aux.transform(pts)
    L_host = aux.loglike(p_host)
    Lmin = T._gap_threshold(L_host[np.isfinite(L_host)])
    u, p, L, nc, offset = T._gated(region, method, T.N, Lmin, aux.transform, aux.loglike, None)
    keep = L_host > Lmin
    assert nc == len(pts) and offset == nxt and 10 < keep.sum() < len(pts)
    assert np.array_equal(u, pts[keep]) and np.array_equal(p, p_host[keep]) and np.array_equal(L, L_host[keep])


def test_gated_refill_equals_the_host_sequence():
    import test_tregion_refill_gpu as T
    aux, live, region, Ls = _route_problem("a")
    got, host, tregion, Lmin = T._check(region, "sample_from_wrapping_ellipsoid", aux.transform, aux.loglike)
    keep = host[3] > Lmin
    assert keep.sum() > 10 and np.array_equal(got[2], host[3][keep])


def test_form_b_refill_with_a_tregion_takes_the_host_sequence():
    """form (b) has derived columns and no gate_derived: with a t-region (here over all 2 d + 1 output columns, as the driver
    builds it) `refill` returns None and `harness.refill_samples` runs the host sequence through the model's callbacks -- the
    same draws, gated by the t-region, the rows the callbacks give.  The inner transform is nonlinear (Normal priors), so
    that [x | p | logweight] spans an ellipsoid with a volume."""
    import test_tregion_refill_gpu as T
    from ultranest_amd import harness
    from ultranest_amd.mlfriends import WrappingEllipsoid
    from ultranest_amd.regions import DeviceRNG
    d = 3
    inner = um.gauss_normal_prior(d, sigma=0.1, prior_sigma=0.2)[0]
    aux = hs.get_extended_auxiliary_independent_problem(inner.loglike, inner.transform, np.full(d, 0.5), np.full(d, 0.2))[0].model
    live = T._blob(400, d, 77, width=0.15)[:100]
    region = T._region_of("MLFriends", live)
    p_live = aux.transform(live)
    assert p_live.shape == (100, 2 * d + 1) and np.isfinite(p_live).all()
    t = WrappingEllipsoid.__new__(WrappingEllipsoid)          # built on the host from the live rows' moments (no bootstrap)
    WrappingEllipsoid.__init__(t, p_live)
    v = p_live[:, t.variable_dims]
    t.enlarge = 1.0
    t.ellipsoid_center = v.mean(axis=0)
    t.ellipsoid_cov = np.cov(v, rowvar=0) * (v.shape[1] + 2)
    t.ellipsoid_invcov = np.linalg.inv(t.ellipsoid_cov)
    assert np.isfinite(t.ellipsoid_invcov).all()
    method = "sample_from_wrapping_ellipsoid"
    region.current_sampling_method = getattr(region, method)
    region.device_rng = DeviceRNG(41)
    pts = region.sample(T.N)
    p_host = aux.transform(pts)
    t.enlarge = float(np.median(T._quadratic_form(t, p_host)))          # the gate decides something: about half the draws pass
    acc = t.inside(p_host)
    assert 0.2 < acc.mean() < 0.8
    L_host = aux.loglike(p_host[acc])
    Lmin = T._gap_threshold(L_host[np.isfinite(L_host)])
    region.device_rng = DeviceRNG(41)
    assert region.refill(T.N, Lmin, aux.transform, aux.loglike, tregion=t) is None
    region.device_rng = DeviceRNG(41)
    u, p, L, nc = harness.refill_samples(region, t, aux.transform, aux.loglike, Lmin, T.N)
    keep = L_host > Lmin
    assert nc == acc.sum() and 10 < keep.sum() < acc.sum()
    assert np.array_equal(u, pts[acc][keep]) and np.array_equal(p, p_host[acc][keep]) and np.array_equal(L, L_host[keep])


def _rows_are_the_models(M, rows, Lmin):
    found = [(u, p, L) for u, p, L, nc in rows if u is not None]
    u, p, L = np.array([f[0] for f in found]), np.array([f[1] for f in found]), np.array([f[2] for f in found])
    want_p = M.transform(u)
    assert np.isfinite(p).all() and np.isfinite(L).all()
    assert np.array_equal(p, want_p) and np.array_equal(L, M.loglike(want_p)) and (L > Lmin).all()
    return len(found)


@pytest.mark.parametrize("form", ["a", "b"])
@pytest.mark.parametrize("which", ["randomwalk", "simpleslice", "slice"])
def test_population_samplers_hand_out_the_models_rows(which, form):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    aux, live, region, Ls = _route_problem(form)
    Lmin = Ls.min() - 0.5
    if which == "randomwalk":
        s = pop.PopulationRandomWalkSampler(popsize=64, nsteps=6, generate_direction=pop.generate_random_direction, scale=0.3,
                                            device_rng=DeviceRNG(6))
    elif which == "simpleslice":
        s = pop.PopulationSimpleSliceSampler(64, 4, pop.generate_random_direction, device_rng=DeviceRNG(6))
    else:
        np.random.seed(8)
        s = pop.PopulationSliceSampler(popsize=32, nsteps=6, generate_direction=pop.generate_mixture_random_direction, scale=0.5,
                                       device_rng=DeviceRNG(5))
    rows = [s.__next__(region, Lmin, live, Ls, aux.transform, aux.loglike) for _ in range(120 if which == "slice" else 64)]
    if which != "slice":
        assert s._device_route(aux.transform, aux.loglike) is not None
        assert rows[0][3] > 0 and all(r[3] == 0 for r in rows[1:]) and s.last_refill is not None        # one refill, on the device
    assert _rows_are_the_models(aux, rows, Lmin) > 5


# ---- nested sampling ----

SIGMA = 0.01
_runs = {}


def _gauss3():
    return um.gauss(3, sigma=SIGMA)


def _posterior_samples():
    rs = np.random.RandomState(11)
    c = um.gauss_centers(3, SIGMA)
    return c + SIGMA * rs.normal(size=(400, 3)), np.full(400, 1.0 / 400)


def _run(which):
    from ultranest_amd.harness import StaticNestedSampler
    from ultranest_amd.regions import DeviceRNG
    if which not in _runs:
        inner = _gauss3()
        up, w = _posterior_samples()
        if which == "plain":
            model = inner
        elif which == "a":
            model = hs.from_results(inner, {"weighted_samples": {"upoints": up, "weights": w}})[1].model
        else:
            model = hs.get_extended_auxiliary_independent_problem(inner.loglike, inner.transform, up.mean(axis=0), up.std(axis=0))[0].model
        s = StaticNestedSampler(model.ndim, model.loglike, transform=model.transform, num_live_points=200, ndraw=4096, seed=2,
                                device_rng=DeviceRNG(21))
        _runs[which] = (model, s.run(dlogz=0.5), s)
    return _runs[which]


def _analytic_logz():
    c = um.gauss_centers(3, SIGMA)
    return math.log(HR.gauss_box_evidence(np.zeros(3), np.ones(3), c, SIGMA))


def test_nested_sampling_with_the_independent_form():
    plain = _run("plain")[1]
    model, res, s = _run("b")
    want = _analytic_logz()
    print("MEASURED form (b): logz %.4f + offset %.4f, analytic %.4f, logzerr %.4f, niter %d of the plain run's %d (ratio %.3f)" % (
        res["logz"], model.logz_offset, want, res["logzerr"], res["niter"], plain["niter"], res["niter"] / plain["niter"]))
    assert abs(plain["logz"] - want) < 4 * plain["logzerr"] + 0.15
    assert abs(res["logz"] + model.logz_offset - want) < 4 * res["logzerr"] + 0.15, (res, want)
    assert res["niter"] < plain["niter"] and s.phases["refills"] > 0


def test_nested_sampling_with_the_contbox_form():
    plain = _run("plain")[1]
    model, res, s = _run("a")
    up, w = _posterior_samples()
    ulos, uhis, xp = hs.compute_quantile_intervals_refined(HR.STEPS, up, w)
    want = HR.contbox_log_evidence(ulos, uhis, xp, um.gauss_centers(3, SIGMA), SIGMA)
    assert abs(want - HR.contbox_log_evidence(ulos, uhis, xp, um.gauss_centers(3, SIGMA), SIGMA, order=32)) < 1e-6
    print("MEASURED form (a): logz %.4f, ln int Z_box dt %.4f (ln Z %.4f), logzerr %.4f, niter %d of the plain run's %d (ratio %.3f)" % (
        res["logz"], want, _analytic_logz(), res["logzerr"], res["niter"], plain["niter"], res["niter"] / plain["niter"]))
    assert model.ndim == 4 and abs(res["logz"] - want) < 4 * res["logzerr"] + 0.15, (res, want)
    assert res["niter"] < plain["niter"] and s.phases["refills"] > 0
