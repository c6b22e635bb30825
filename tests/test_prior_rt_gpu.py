"""Run-time priors (``priors.Ref``, ``priors.Tabulated``) on the GPU: every Ref-capable family read from Fixed parents
against the bound of the constant-parameter family (pass-through families bit for bit the constant column), varying parents
judged row by row, the evaluation order, the run-time contract (point mass, NaN and its propagation), tables bit for bit
against their numpy restatement, independence of the row's position and of the model form, every device route with a
hierarchical model (and one whose rows are NaN now and then), and an evidence.

Measured on the MI355X: see DESIGN.md 7f for the table this test prints (lines MEASURED)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import prior_reference as PR  # noqa: E402
import prior_rt_reference as RT  # noqa: E402
from ultranest_amd import priors as P  # noqa: E402
from ultranest_amd import usermodels  # noqa: E402
from ultranest_amd.priors import Ref  # noqa: E402

U = PR.grid()
GAUSS = usermodels.GAUSS_LOGLIKE % 0.5
BATCH = 530
assert len(U) <= BATCH


def _transform(pt, u):
    """pt.transform in batches of at most BATCH rows"""
    return np.concatenate([pt.transform(u[i:i + BATCH]) for i in range(0, len(u), BATCH)])


def _columns(priors, u):
    """every column of the list evaluated on the same 1-d u"""
    pt = P.PriorTransform(priors)
    return _transform(pt, np.repeat(u[:, None], pt.ndim, axis=1))


_unit = {}


def _unit_column(prior, u):
    """the device's column of a parameter-free or unit-parameter prior (Normal(0, 1): z itself, 0 + 1 * z), computed once"""
    key = (type(prior).__name__, u.tobytes())
    if key not in _unit:
        _unit[key] = _columns([prior], u)[:, 0]
    return _unit[key]


# ---- families ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(RT.REF_FAMILIES))
def test_family_with_fixed_parents(name):
    """one model per family: per setting the Fixed parents, the child that reads them and the constant-parameter twin"""
    priors, where = [], []
    for lead, args in [((), RT.REF_FAMILIES[name](prior)) for prior in PR.family(name)]:
        first = len(priors)
        priors += [P.Fixed(a) for a in args]
        priors.append(getattr(P, name)(*(tuple(lead) + tuple(Ref(first + k) for k in range(len(args))))))
        priors.append(RT.constant_prior(name, args, lead))
        where.append((len(priors) - 2, len(priors) - 1, args))
    got = _columns(priors, U)
    worst = 0.0
    for child, twin, args in where:
        col, const = got[:, child], got[:, twin]
        assert np.isfinite(col[(U >= 2.0 ** -53) & (U <= 1 - 2.0 ** -53)]).all()
        assert (np.diff(col) >= 0).all(), (name, args, U[1:][np.diff(col) < 0])
        if name in RT.RUN_TIME_FORMS:
            e = PR.excess(priors[twin], U, col)
            worst = max(worst, e.max())
            assert e.max() <= 1.0, (name, args, U[np.argmax(e)], e.max())
        else:           # pass-through: the constant column's bits
            assert np.array_equal(col, const, equal_nan=True), (name, args)
            e = PR.excess(priors[twin], U, col)
            worst = max(worst, e.max())
            assert e.max() <= 1.0, (name, args, U[np.argmax(e)], e.max())
        if name == "Uniform":
            assert np.array_equal(col, args[0] + U * (args[1] - args[0]))
    print("MEASURED rt %s %.3g" % (name, worst))


@pytest.mark.parametrize("name", sorted(RT.SPECIAL_REF_FAMILIES))
def test_iterative_family_with_fixed_parents(name):
    """the Gamma / InverseGamma scale and the StudentT loc and scale read from Fixed parents, at the settings and over the grid
    of the golden fixture of the iterative families, against its 60-digit references and its bound"""
    import special_prior_reference as SR
    loaded = [SR.load(n) for n in SR.settings(name)]
    u = loaded[0][1]
    assert all(np.array_equal(u, ld[1]) for ld in loaded) and (np.diff(u) > 0).all()
    priors, where = [], []
    for prior, _, ref in loaded:
        lead, args = ((prior.nu,), (prior.loc, prior.scale)) if name == "StudentT" else ((prior.shape,), (prior.scale,))
        first = len(priors)
        priors += [P.Fixed(a) for a in args]
        priors.append(getattr(P, name)(*(lead + tuple(Ref(first + k) for k in range(len(args))))))
        priors.append(prior)
        where.append((len(priors) - 2, len(priors) - 1, prior, ref))
    got = _columns(priors, u)
    worst = 0.0
    for child, twin, prior, ref in where:
        col = got[:, child]
        assert np.array_equal(col, got[:, twin]) and np.isfinite(col).all() and (np.diff(col) >= 0).all(), (name, prior.consts)
        e = SR.excess(prior, u, col, ref)
        worst = max(worst, e.max())
        assert e.max() <= 1.0, (name, prior.consts, u[np.argmax(e)], e.max())
    print("MEASURED rt %s %.3g" % (name, worst))


def test_varying_parents_row_by_row():
    rs = np.random.RandomState(31)
    priors = [P.Uniform(0.5, 2.0, name="a"), P.LogUniform(0.1, 10.0, name="b"),
              P.Uniform(Ref("a", scale=-1.0), Ref("b")), P.LogUniform(Ref("a", scale=0.01), Ref("b")),
              P.TruncatedNormal(Ref("a"), Ref("b"), Ref("a", offset=-3.0), Ref("b", offset=2.5)),
              P.Triangular(Ref("a", scale=-1.0), Ref("a", scale=0.25), Ref("b", offset=0.5)),
              P.Normal(Ref("a"), Ref("b")), P.Weibull(Ref("b"), Ref("a"))]
    pt = P.PriorTransform(priors)
    u = rs.uniform(size=(257, pt.ndim))
    got = pt.transform(u)
    assert np.isfinite(got).all()
    names = ["Uniform", "LogUniform", "TruncatedNormal", "Triangular", "Normal", "Weibull"]
    order = {"Uniform": ("lo", "hi"), "LogUniform": ("lo", "hi"), "TruncatedNormal": ("mu", "sigma", "lo", "hi"),
             "Triangular": ("lo", "mode", "hi"), "Normal": ("mu", "sigma"), "Weibull": ("scale", "shape")}
    for j, name in zip(range(2, 8), names):
        prior = priors[j]
        params = np.stack([prior.refs[a][0].value(got[:, pt.paramnames.index(prior.refs[a][0].target)]) for a in order[name]], axis=1)
        e = RT.ref_excess(name, params, u[:, j], got[:, j])
        print("MEASURED rt varying %s %.3g" % (name, e.max()))
        assert e.max() <= 1.0, (name, params[np.argmax(e)], u[np.argmax(e), j])
    lo, hi = -1.0 * got[:, 0], got[:, 1]
    assert np.array_equal(got[:, 2], lo + u[:, 2] * (hi - lo))


def test_columns_are_written_in_dependency_order():
    from test_prior_rt_reference import chain5, diamond
    rs = np.random.RandomState(32)
    u = rs.uniform(size=(65, 6))
    z = np.stack([_unit_column(P.Normal(0.0, 1.0), np.ascontiguousarray(u[:, k])) for k in range(6)], axis=1)
    got = P.PriorTransform(chain5()).transform(u)
    assert np.array_equal(got[:, 5], z[:, 5])
    for k in range(4, -1, -1):
        assert np.array_equal(got[:, k], got[:, k + 1] + 1.0 * z[:, k]), k
    got = P.PriorTransform(diamond()).transform(u[:, :5])
    top = _columns([P.LogUniform(0.1, 10.0)], np.ascontiguousarray(u[:, 1]))[:, 0]
    e1 = _unit_column(P.Exponential(1.0), np.ascontiguousarray(u[:, 3]))
    assert np.array_equal(got[:, 1], top) and np.array_equal(got[:, 2], top + 1.0 * z[:, 2])
    assert np.array_equal(got[:, 3], top * e1) and np.array_equal(got[:, 0], got[:, 2] + got[:, 3] * z[:, 0])
    assert np.array_equal(got[:, 4], 0.0 + u[:, 4] * 1.0)
    later = P.PriorTransform([P.Uniform(0.0, 1.0), P.Normal(Ref(3), 1.0), P.Uniform(0.0, 1.0), P.Normal(0.0, 1.0), P.Sine()])
    got = later.transform(u[:, :5])
    assert np.array_equal(got[:, 3], z[:, 3]) and np.array_equal(got[:, 1], z[:, 3] + 1.0 * z[:, 1])


def test_run_time_contract():
    """a scale of 0 is the point mass at loc; a strictly positive parameter of 0 and a scale that overflowed give NaN, in the
    column and in every column that reads it, and nowhere else.  LogNormal(700, 1) itself stays finite over (0, 1) (it would
    need z > 9.78); its multiple by 1e4 overflows for z > 0.57"""
    with np.errstate(over="ignore"):
        return _run_time_contract()


def _run_time_contract():
    priors = [P.Fixed(0.0, name="zero"), P.Fixed(1.5, name="loc"), P.Uniform(0.0, 1.0, name="free"),
              P.Normal(Ref("loc"), Ref("zero"), name="point"), P.Cauchy(Ref("loc"), Ref("zero"), name="point2"),
              P.Weibull(1.0, Ref("zero"), name="bad"), P.Pareto(Ref("zero"), 2.0, name="bad2"),
              P.Normal(0.0, Ref("bad"), name="child"), P.Laplace(Ref("child"), 1.0, name="grandchild"),
              P.LogNormal(700.0, 1.0, name="big"), P.Exponential(Ref("big", scale=1e4), name="over"),
              P.Logistic(Ref("over"), 1.0, name="overchild"), P.LogUniform(Ref("zero"), 1.0, name="bad3"),
              P.TruncatedNormal(0.0, Ref("zero"), -1.0, 1.0, name="bad4"), P.Normal(Ref("point"), 1.0, name="good")]
    pt = P.PriorTransform(priors)
    got = _columns(priors, U)
    col = {n: got[:, k] for k, n in enumerate(pt.paramnames)}
    assert np.array_equal(col["free"], U) and np.array_equal(col["point"], np.full(len(U), 1.5))
    assert np.array_equal(col["point2"], np.full(len(U), 1.5))
    for n in ("bad", "bad2", "child", "grandchild", "bad3", "bad4"):
        assert np.isnan(col[n]).all(), n
    assert np.isfinite(col["big"]).all()
    over = 1e4 * col["big"] == np.inf
    assert 100 < over.sum() < len(U) - 100
    assert np.isnan(col["over"][over]).all() and np.isnan(col["overchild"][over]).all()
    # a finite scale near the top of the range may still overflow in the family's own product: inf, not NaN; as a location of
    # the next column that inf is refused in turn
    assert not np.isnan(col["over"][~over]).any() and (col["over"][~over] > 0).all()
    assert np.array_equal(np.isnan(col["overchild"]), ~np.isfinite(col["over"]))
    assert np.array_equal(col["good"], _columns([P.Normal(1.5, 1.0)], U)[:, 0])


# ---- tables ----------------------------------------------------------------------------------------------------------------

def _check_tables(tabs):
    """all tables in one model, each column fed its own u values (padded with 0.5)"""
    us = [RT.table_u(t) for t in tabs]
    rows = max(len(v) for v in us)
    u = np.full((rows, len(tabs)), 0.5)
    for k, v in enumerate(us):
        u[:len(v), k] = v
    got = _transform(P.PriorTransform(tabs), u)
    worst = 0.0
    for k, (tab, v) in enumerate(zip(tabs, us)):
        col = got[:len(v), k]
        assert np.array_equal(col, RT.table_restatement(tab, v)), (k, tab.n)
        assert (np.diff(col) >= 0).all() and col[0] >= tab.x[0] and col[-1] <= tab.x[-1], (k, tab.n)
        if tab.n <= 1025:
            worst = max(worst, RT.table_excess(tab, v, col).max())
    return worst


def test_tables_of_every_size_are_the_numpy_restatement_bit_for_bit():
    worst = _check_tables([RT.make_table(n, 1) for n in RT.TABLE_SIZES] + [RT.make_table(1025, 2, "steps")])
    print("MEASURED rt table %.3g" % worst)
    assert worst <= 1.0


def test_the_three_table_constructors():
    from test_prior_rt_reference import _histogram18
    rs = np.random.RandomState(9)
    samples = np.round(rs.normal(size=300), 1)              # many duplicates
    tabs = [P.Tabulated([0.5, 0.5, 2.0], [0.0, 0.25, 1.0]), _histogram18(), P.Tabulated.from_samples(samples),
            RT.make_table(1000, 3, "heavy")]
    worst = _check_tables(tabs)
    print("MEASURED rt table constructors %.3g" % worst)
    assert worst <= 1.0
    tab = tabs[2]
    u = np.sort(rs.uniform(size=500))
    got = P.PriorTransform([tab]).transform(u[:, None])[:, 0]
    ref = RT.table_reference(tab, u)
    k = RT.table_index(tab.cdf, u)
    bound = 2.0 ** -52 * np.abs(tab.slopes[k]) + np.array([float(2 * RT.EPS * abs(r) + 3 * RT.EPS * w) for r, w in zip(*ref)])
    assert (np.abs(got - np.quantile(samples, u)) <= bound).all()


# ---- position and form ---------------------------------------------------------------------------------------------------

def test_position_and_form_independence():
    from test_prior_rt_compile import mixed_rt_priors
    from test_priors_compile import SUMMED
    pt = P.PriorTransform(mixed_rt_priors())
    m = pt.model(GAUSS, aux=np.zeros(12), name="mixed_rt12")
    s = pt.model(SUMMED, aux=np.zeros(24), nterms=24, name="mixed_rt12_sum")
    rs = np.random.RandomState(12)
    u = rs.uniform(size=(257, 12))
    u[:20, 6] = U[:20]
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
    # a child of a table column is the constant family at the table's value: Exponential(scale) = scale * E1
    e1 = _unit_column(P.Exponential(1.0), np.ascontiguousarray(u[:, 4]))
    assert np.array_equal(full[:, 3], RT.table_restatement(pt.priors[3], u[:, 3])) and np.array_equal(full[:, 4], full[:, 3] * e1)


# ---- routes ----------------------------------------------------------------------------------------------------------------

NLIVE = 100
_models = {}


def _route_model(nan=False):
    """five columns: mu, tau, two groups and a bounded column between -tau and tau.  With `nan` the last column is a
    Weibull whose shape is a table column that is 0 for u <= 0.36: one draw in six of a region around live points that lie
    above 0.37 in that column (measured: 5231 of 29256)"""
    if nan not in _models:
        priors = [P.Normal(0.0, 1.0, name="mu"), P.LogUniform(0.1, 1.0, name="tau"), P.Normal(Ref("mu"), Ref("tau"), name="theta0"),
                  P.Normal(Ref("mu"), Ref("tau", scale=2.0, offset=0.1), name="theta1")]
        if nan:
            priors[3] = P.Tabulated([0.0, 0.0, 2.0], [0.0, 0.36, 1.0], name="k")
            priors.append(P.Weibull(Ref("tau"), Ref("k"), name="w"))
        else:
            priors.append(P.Uniform(Ref("tau", scale=-1.0), Ref("tau"), name="between"))
        pt = P.PriorTransform(priors)
        centers = pt.transform(np.full((1, 5), 0.5))[0]
        assert np.isfinite(centers).all()
        _models[nan] = pt.model(GAUSS, aux=centers, name="hier5_nan" if nan else "hier5")
    return _models[nan]


def _live(nan=False, seed=77):
    import test_tregion_refill_gpu as T
    u = T._blob(4 * NLIVE, 5, seed)[:NLIVE]
    assert len(u) == NLIVE
    if nan:
        u[:, 3] = np.where(u[:, 3] <= 0.37, 0.74 - u[:, 3], u[:, 3])        # every live point has a shape above 0
    return u


@pytest.mark.parametrize("nan", [False, True])
def test_refill_equals_the_host_sequence(nan):
    import test_tregion_refill_gpu as T
    from ultranest_amd.regions import DeviceRNG
    M = _route_model(nan)
    region = T._region_of("MLFriends", _live(nan))
    method = "sample_from_wrapping_ellipsoid"
    region.current_sampling_method = getattr(region, method)
    region.device_rng = DeviceRNG(41)
    pts = region.sample(T.N)
    nxt = region.device_rng.offset
    p_host = M.transform(pts)
    L_host = M.loglike(p_host)
    bad = np.isnan(p_host).any(axis=1)
    print("rows with a NaN: %d of %d" % (bad.sum(), len(pts)))
    # (a shape just above 0 overflows the Weibull quantile itself: p = inf and L = -inf, which is not kept either)
    assert np.isnan(L_host[bad]).all() and not np.isnan(L_host[~bad]).any()
    assert (50 < bad.sum() < 0.5 * len(pts)) if nan else (not bad.any() and np.isfinite(L_host).all())
    Lmin = T._gap_threshold(L_host[np.isfinite(L_host)])
    u, p, L, nc, offset = T._gated(region, method, T.N, Lmin, M.transform, M.loglike, None)
    with np.errstate(invalid="ignore"):
        keep = L_host > Lmin
    assert nc == len(pts) and offset == nxt and 10 < keep.sum() < len(pts) and not (keep & bad).any()
    assert np.array_equal(u, pts[keep]) and np.array_equal(p, p_host[keep]) and np.array_equal(L, L_host[keep])
    assert np.isfinite(p).all() and np.isfinite(L).all()


def test_gated_refill_equals_the_host_sequence():
    import test_tregion_refill_gpu as T
    M = _route_model()
    region = T._region_of("MLFriends", _live())
    got, host, tregion, Lmin = T._check(region, "sample_from_wrapping_ellipsoid", M.transform, M.loglike)
    keep = host[3] > Lmin
    assert keep.sum() > 10 and np.array_equal(got[2], host[3][keep])


def _walk_problem(nan):
    import test_tregion_refill_gpu as T
    M = _route_model(nan)
    u = _live(nan)
    region = T._region_of("MLFriends", u)
    Ls = M.loglike(M.transform(u))
    assert np.isfinite(Ls).all()
    return M, u, region, Ls, Ls.min() - 0.5


def _rows_are_the_models(M, rows, Lmin):
    found = [(u, p, L) for u, p, L, nc in rows if u is not None]
    u, p, L = np.array([f[0] for f in found]), np.array([f[1] for f in found]), np.array([f[2] for f in found])
    want_p = M.transform(u)
    assert np.isfinite(p).all() and np.isfinite(L).all()
    assert np.array_equal(p, want_p) and np.array_equal(L, M.loglike(want_p)) and (L > Lmin).all()
    return len(found)


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("which", ["randomwalk", "simpleslice"])
def test_whole_refill_samplers_hand_out_the_models_rows(which, nan):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    M, u, region, Ls, Lmin = _walk_problem(nan)
    if which == "randomwalk":
        s = pop.PopulationRandomWalkSampler(popsize=64, nsteps=6, generate_direction=pop.generate_random_direction, scale=0.3,
                                            device_rng=DeviceRNG(6))
    else:
        s = pop.PopulationSimpleSliceSampler(64, 4, pop.generate_random_direction, device_rng=DeviceRNG(6))
    assert s._device_route(M.transform, M.loglike) is not None
    rows = [s.__next__(region, Lmin, u, Ls, M.transform, M.loglike) for _ in range(64)]
    assert rows[0][3] > 0 and all(r[3] == 0 for r in rows[1:]) and not s.prepared_samples        # one refill, on the device
    assert s.last_refill is not None and _rows_are_the_models(M, rows, Lmin) == 64


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("philox", [False, True])
def test_population_slice_sampler_hands_out_the_models_rows(philox, nan):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    M, u, region, Ls, Lmin = _walk_problem(nan)
    np.random.seed(8)
    s = pop.PopulationSliceSampler(popsize=32, nsteps=6, generate_direction=pop.generate_mixture_random_direction, scale=0.5,
                                   device_rng=DeviceRNG(5) if philox else None)
    rows = [s.__next__(region, Lmin, u, Ls, M.transform, M.loglike) for _ in range(120)]
    assert _rows_are_the_models(M, rows, Lmin) > 5


def test_nested_sampling_evidence_of_the_hierarchical_model():
    """usermodels.hierarchical_gauss(3): four columns, analytic ln Z; every refill is a user refill on the device (gated: the
    priors are not affine, so the driver keeps its t-region)"""
    from ultranest_amd import kernels
    from ultranest_amd.harness import StaticNestedSampler
    from ultranest_amd.regions import DeviceRNG
    G, want = usermodels.hierarchical_gauss(3)
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
    assert len(calls) >= 5 and s.phases["refills"] == len(calls)
