"""Run-time priors (``priors.Ref``, ``priors.Tabulated``), CPU side: the references of
prior_rt_reference accept the numpy stand-ins of every run-time formula and of the table formula and reject five seeded
defects; support propagation, every ValueError (before any compile), the evaluation order, the three table constructors and the
analytic evidence of usermodels.hierarchical_gauss."""
import math

import numpy as np
import pytest

import prior_reference as PR
import prior_rt_reference as RT
from ultranest_amd import devicemodel as dm
from ultranest_amd import priors as P
from ultranest_amd import usermodels
from ultranest_amd.priors import Ref

U = PR.grid()
INF = math.inf


# ---- stand-ins and seeded defects ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RT.RUN_TIME_FORMS)
def test_run_time_standins_are_accepted(name):
    for prior in PR.family(name):
        got = RT.rt_standin(name, U, *RT.REF_FAMILIES[name](prior))
        assert PR.accepts(prior, U, got), (name, PR.excess(prior, U, got).max())


def test_ref_excess_judges_each_row_by_its_own_parameters():
    rs = np.random.RandomState(3)
    u, mu, sigma = rs.uniform(size=40), rs.normal(size=40), rs.uniform(0.5, 2.0, size=40)
    got = PR.standin(P.Normal(0.0, 1.0), u) * sigma + mu
    assert RT.ref_excess("Normal", np.stack([mu, sigma], axis=1), u, got).max() <= 1.0
    assert RT.ref_excess("Normal", np.stack([mu, sigma[::-1]], axis=1), u, got).max() > 1e6


def _histogram18():
    """17 bins, five of them empty (flat CDF segments, among them two in a row)"""
    rs = np.random.RandomState(18)
    h = rs.uniform(0.1, 2.0, size=17)
    h[[2, 7, 8, 12, 15]] = 0.0
    return P.Tabulated.from_histogram(np.cumsum(rs.uniform(0.2, 1.5, size=18)) - 4.0, h)


def _tables():
    return {"two": P.Tabulated([-1.0, 3.0], [0.0, 1.0]), "three_dup": P.Tabulated([0.5, 0.5, 2.0], [0.0, 0.25, 1.0]),
            "hist18": _histogram18(), "heavy1000": RT.make_table(1000, 3, "heavy"), "smooth1025": RT.make_table(1025, 1),
            "steps1025": RT.make_table(1025, 2, "steps")}


@pytest.mark.parametrize("which", sorted(_tables()))
def test_table_restatement_is_accepted(which):
    tab = _tables()[which]
    u = RT.table_u(tab)
    got = RT.table_restatement(tab, u)
    e = RT.table_excess(tab, u, got)
    print("MEASURED numpy table %s: largest error %.3g of the bound" % (which, e.max()))
    assert e.max() <= 1.0 and RT.slopes_follow_the_rule(tab)
    assert (np.diff(got) >= 0).all() and got[0] >= tab.x[0] and got[-1] <= tab.x[-1]
    # the knots themselves are met exactly (the last knot of a run of equal c is the one u = c reaches)
    k = RT.table_index(tab.cdf, tab.cdf[1:-1])
    assert np.array_equal(RT.table_restatement(tab, tab.cdf[1:-1]), tab.x[k])


def test_defect_wrong_k_at_a_knot_is_rejected():
    """side="left" puts u = c_k into the segment below: the same value on a strictly increasing CDF (both segments meet the
    knot exactly), the wrong end of the gap where the CDF is flat"""
    tab = _histogram18()
    u = RT.table_u(tab)
    k = np.clip(np.searchsorted(tab.cdf, u, side="left") - 1, 0, tab.n - 2)
    got = RT.table_restatement(tab, u, k=k)
    assert not np.array_equal(got, RT.table_restatement(tab, u)) and not RT.table_accepts(tab, u, got)


def test_defect_wrong_side_of_the_seam_is_rejected():
    """from the farther knot the value is the same line with up to twice the rounding error: not the stated bits, which is what
    the device is held to"""
    tab = RT.make_table(1025, 1)
    rs = np.random.RandomState(4)
    u = np.sort(rs.uniform(size=20000))
    c, x, s = tab.cdf, tab.x, tab.slopes
    k = RT.table_index(c, u)
    dl, dr = u - c[k], c[k + 1] - u
    got = np.where(dl > dr, x[k] + dl * s[k], x[k + 1] - dr * s[k])
    good = RT.table_restatement(tab, u)
    assert RT.table_accepts(tab, u, good)
    assert not np.array_equal(got, good)


def test_defect_hi_taken_for_the_width_is_rejected():
    prior = PR.family("Uniform")[1]
    assert not PR.accepts(prior, U, prior.lo + U * prior.hi)


def test_defect_fa_and_qa_swapped_is_rejected():
    from scipy.special import erfc, ndtri
    prior = PR.family("TruncatedNormal")[0]
    mu, sigma, lo, hi = RT.REF_FAMILIES["TruncatedNormal"](prior)
    r2 = np.sqrt(2.0)
    a, b = (lo - mu) / sigma, (hi - mu) / sigma
    Qa, Fb, Fa, Qb = 0.5 * erfc(-a / r2), 0.5 * erfc(-b / r2), 0.5 * erfc(a / r2), 0.5 * erfc(b / r2)     # Fa <-> Qa
    q, qq = Fa + U * (Fb - Fa), Qb + (1.0 - U) * (Qa - Qb)
    with np.errstate(all="ignore"):
        z = np.where(q <= 0.5, ndtri(np.clip(q, 0, 0.5)), -ndtri(np.clip(qq, 0, 0.5)))
    assert not PR.accepts(prior, U, mu + sigma * np.minimum(np.maximum(z, a), b))


def test_defect_nonzero_slope_of_a_flat_segment_is_rejected():
    tab = _histogram18()
    flat = np.flatnonzero(np.diff(tab.cdf) == 0)
    assert len(flat) == 5 and (tab.slopes[flat] == 0).all() and RT.slopes_follow_the_rule(tab)
    tab.slopes = tab.slopes.copy()
    tab.slopes[flat[0]] = 1.0
    assert not RT.slopes_follow_the_rule(tab)


# ---- the three constructors --------------------------------------------------------------------------------------------

def test_from_samples_is_the_linear_rule_of_np_quantile():
    rs = np.random.RandomState(9)
    samples = np.round(rs.normal(size=300), 1)          # many duplicates
    tab = P.Tabulated.from_samples(samples)
    assert tab.n == 300 and np.array_equal(tab.x, np.sort(samples)) and np.array_equal(tab.cdf, np.arange(300) / 299.0)
    u = np.sort(rs.uniform(size=500))
    got, want = RT.table_restatement(tab, u), np.quantile(samples, u)
    ref = RT.table_reference(tab, u)
    k = RT.table_index(tab.cdf, u)
    bound = 2.0 ** -52 * np.abs(tab.slopes[k]) + np.array([float(2 * RT.EPS * abs(r) + 3 * RT.EPS * w) for r, w in zip(*ref)])
    assert (np.abs(got - want) <= bound).all()


def test_from_histogram_pins_the_ends_and_keeps_empty_bins_flat():
    tab = _histogram18()
    assert tab.n == 18 and tab.cdf[0] == 0.0 and tab.cdf[-1] == 1.0 and (np.diff(tab.cdf) >= 0).all()
    assert tab.support() == (tab.x[0], tab.x[-1]) and tab.steps == 5
    assert [P.Tabulated(np.arange(n), np.linspace(0, 1, n)).steps for n in (2, 3, 4, 5, 6, 1024, 1025, 1026, 4096)] == \
        [0, 1, 2, 2, 3, 10, 10, 11, 12]


BAD_TABLES = [
    lambda: P.Tabulated([0.0], [0.0]), lambda: P.Tabulated(np.arange(4097), np.linspace(0, 1, 4097)),
    lambda: P.Tabulated([0.0, 1.0], [0.0, 0.5, 1.0]), lambda: P.Tabulated([[0.0, 1.0]], [[0.0, 1.0]]),
    lambda: P.Tabulated([0.0, float("nan")], [0.0, 1.0]), lambda: P.Tabulated([0.0, float("inf")], [0.0, 1.0]),
    lambda: P.Tabulated([0.0, 2.0, 1.0], [0.0, 0.5, 1.0]), lambda: P.Tabulated([1.0, 1.0], [0.0, 1.0]),
    lambda: P.Tabulated([0.0, 1.0, 2.0], [0.0, 0.6, 0.5]), lambda: P.Tabulated([0.0, 1.0], [1e-300, 1.0]),
    lambda: P.Tabulated([0.0, 1.0], [0.0, np.nextafter(1.0, 0.0)]), lambda: P.Tabulated([0.0, 1.0, 2.0], [0.0, 1.5, 1.0]),
    lambda: P.Tabulated([-1e308, 0.0, 1e308], [0.0, 5e-324, 1.0]),                 # a slope overflows
    lambda: P.Tabulated("ab", [0.0, 1.0]), lambda: P.Tabulated([0.0, Ref(0)], [0.0, 1.0]),
    lambda: P.Tabulated.from_samples(np.arange(4097.0)), lambda: P.Tabulated.from_samples([1.0]),
    lambda: P.Tabulated.from_samples([2.0, 2.0, 2.0]), lambda: P.Tabulated.from_samples([0.0, float("nan")]),
    lambda: P.Tabulated.from_histogram([0.0, 1.0, 2.0], [1.0]), lambda: P.Tabulated.from_histogram([0.0, 1.0], [0.0]),
    lambda: P.Tabulated.from_histogram([0.0, 1.0, 1.0], [1.0, 1.0]), lambda: P.Tabulated.from_histogram([0.0, 1.0], [-1.0]),
    lambda: P.Tabulated.from_histogram([0.0, 1.0], [float("inf")]),
    lambda: P.PriorTransform([RT.make_table(4096, s) for s in range(4)] + [P.Tabulated([0.0, 1.0], [0.0, 1.0])]),      # 16 386 knots
]


def test_from_samples_above_the_cap_says_what_to_do():
    with pytest.raises(ValueError, match="quantile knots"):
        P.Tabulated.from_samples(np.arange(5000.0))


# ---- argument checks -----------------------------------------------------------------------------------------------------

def _mu_tau():
    return [P.Normal(0.0, 10.0, name="mu"), P.LogUniform(0.01, 10.0, name="tau")]


BAD_REFS = [
    lambda: Ref(None), lambda: Ref(1.5), lambda: Ref(True), lambda: Ref("a", scale=float("nan")), lambda: Ref("a", offset=float("inf")),
    lambda: Ref("a", scale=0.0),
    # parameters that stay constants
    lambda: P.Fixed(Ref(0)), lambda: P.Gamma(Ref(0), 1.0), lambda: P.InverseGamma(Ref(0)), lambda: P.ChiSquared(Ref(0)),
    lambda: P.Beta(Ref(0), 1.0), lambda: P.Beta(1.0, Ref(0)), lambda: P.StudentT(Ref(0)), lambda: P.Dirichlet([1.0, Ref(0)]),
    lambda: P.MultivariateNormal([Ref(0), 0.0], np.eye(2)), lambda: P.OrderedUniform(Ref(0), 1.0, 2),
    lambda: P.OrderedUniform(0.0, 1.0, Ref(0)), lambda: P.Uniform(Ref(0), 1.0, circular=True),
    # constants beside a Ref are still checked
    lambda: P.Normal(Ref(0), -1.0), lambda: P.Normal(float("nan"), Ref(0)), lambda: P.TruncatedNormal(Ref(0), 1.0, 2.0, 1.0),
    lambda: P.Triangular(2.0, Ref(0), 1.0), lambda: P.Weibull(Ref(0), 0.0), lambda: P.Uniform(Ref(0), float("inf")),
    # resolution
    lambda: P.PriorTransform(_mu_tau() + [P.Normal(Ref("nu"), 1.0)]),                       # unknown name
    lambda: P.PriorTransform(_mu_tau() + [P.Normal(Ref(3), 1.0)]), lambda: P.PriorTransform(_mu_tau() + [P.Normal(Ref(-1), 1.0)]),
    lambda: P.PriorTransform(_mu_tau() + [P.Normal(Ref(2), 1.0)]),                          # itself
    lambda: P.PriorTransform(_mu_tau() + [P.Normal(Ref("x"), 1.0, name="x")]),
    lambda: P.PriorTransform([P.Normal(0.0, 1.0, name="a"), P.Normal(1.0, 1.0, name="a"), P.Normal(Ref("a"), 1.0)]),      # twice
    lambda: P.PriorTransform([P.Normal(Ref(1), 1.0), P.Normal(Ref(0), 1.0)]),               # a cycle of two
    lambda: P.PriorTransform([P.Normal(Ref(2), 1.0), P.Normal(Ref(0), 1.0), P.Normal(Ref(1), 1.0), P.Fixed(0.0)]),
    # supports
    lambda: P.PriorTransform(_mu_tau() + [P.Normal(0.0, Ref("mu"))]),
    lambda: P.PriorTransform(_mu_tau() + [P.Normal(0.0, Ref("tau", scale=-1.0))]),
    lambda: P.PriorTransform(_mu_tau() + [P.Normal(0.0, Ref("tau", offset=-0.02))]),
    lambda: P.PriorTransform(_mu_tau() + [P.Exponential(Ref("mu"))]), lambda: P.PriorTransform(_mu_tau() + [P.Pareto(Ref("mu"), 2.0)]),
    lambda: P.PriorTransform(_mu_tau() + [P.Weibull(1.0, Ref("mu"))]), lambda: P.PriorTransform(_mu_tau() + [P.Gamma(2.0, Ref("mu"))]),
    lambda: P.PriorTransform(_mu_tau() + [P.StudentT(2.0, 0.0, Ref("mu"))]),
    lambda: P.PriorTransform(_mu_tau() + [P.LogUniform(Ref("mu"), 100.0)]),
    lambda: P.PriorTransform(_mu_tau() + [P.LogUniform(Ref("tau"), 5.0)]),                  # sup 10 > 5
    lambda: P.PriorTransform(_mu_tau() + [P.Uniform(Ref("mu"), 20.0)]),                     # mu is unbounded
    lambda: P.PriorTransform(_mu_tau() + [P.Uniform(0.02, Ref("tau"))]),                    # inf 0.01 < 0.02
    lambda: P.PriorTransform(_mu_tau() + [P.TruncatedNormal(0.0, 1.0, Ref("tau"), 9.0)]),
    lambda: P.PriorTransform(_mu_tau() + [P.Triangular(0.0, Ref("tau"), 9.0)]),
    lambda: P.PriorTransform(_mu_tau() + [P.Triangular(Ref("tau"), 10.0, Ref("tau", offset=9.0))]),
    lambda: P.PriorTransform([P.Sine(name="s"), P.Cosine(name="c"), P.Normal(0.0, Ref("c"))]),
    lambda: P.PriorTransform([P.MultivariateNormal([0.0, 0.0], np.eye(2), name="m"), P.HalfNormal(Ref("m_1"))]),
    lambda: P.PriorTransform([P.Tabulated([-1.0, 1.0], [0.0, 1.0], name="t"), P.HalfNormal(Ref("t"))]),
    lambda: P.PriorTransform([P.Fixed(-1.0), P.Rayleigh(Ref(0))]),
    # a child's support is computed from its parents': Normal(mu, .) is unbounded, whatever tau is
    lambda: P.PriorTransform(_mu_tau() + [P.Normal(Ref("tau"), Ref("tau"), name="th"), P.HalfCauchy(Ref("th"))]),
]


@pytest.mark.parametrize("k", range(len(BAD_REFS) + len(BAD_TABLES)))
def test_argument_checks_come_before_any_compile(k, monkeypatch):
    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)
    with pytest.raises(ValueError):
        (BAD_REFS + BAD_TABLES)[k]()


def test_the_refusal_names_the_parameter_and_the_targets_support():
    with pytest.raises(ValueError, match=r"sigma.*mu.*\[-inf, inf\]"):
        P.PriorTransform(_mu_tau() + [P.Normal(0.0, Ref("mu"))])
    with pytest.raises(ValueError, match=r"lo.*hi.*tau.*\[0\.01, 10\.0\]"):
        P.PriorTransform(_mu_tau() + [P.LogUniform(Ref("tau"), 5.0)])


def test_supports_propagate_by_interval_arithmetic():
    pt = P.PriorTransform([
        P.Fixed(2.0), P.Uniform(-1.0, 3.0, name="a"), P.LogUniform(0.01, 10.0, name="tau"), P.Sine(), P.Cosine(),
        P.Beta(2.0, 3.0), P.Pareto(1.5, 2.0), P.Exponential(1.0), P.Normal(0.0, 1.0), P.OrderedUniform(-2.0, 5.0, 2),
        P.Dirichlet([1.0, 2.0]), P.Tabulated([-3.0, 0.0, 4.0], [0.0, 0.5, 1.0], name="tab"), P.Triangular(0.0, 1.0, 2.0),
        P.TruncatedNormal(0.0, 1.0, -1.0, 2.0), P.StudentT(3.0),
        P.Uniform(Ref("a"), Ref("tab", scale=0.5, offset=10.0), name="u"),         # [-1, 3] .. [8.5, 12]
        P.Pareto(Ref("tau", scale=2.0, offset=0.1), 3.0, name="par"),              # xm in [0.12, 20.1]
        P.TruncatedNormal(Ref("a"), Ref("tau"), Ref("a", offset=-5.0), 7.0),        # lo in [-6, -2]
        P.Exponential(Ref("par")), P.Normal(Ref("u"), Ref("tau")),
        P.Uniform(Ref("tau", scale=-1.0), 0.0),                                     # lo in [-10, -0.01]
        P.LogUniform(Ref("tau", scale=0.001), Ref("tau", offset=10.0)),
    ])
    s = pt.supports
    assert s[:9] == [(2.0, 2.0), (-1.0, 3.0), (0.01, 10.0), (0.0, math.pi), (-0.5 * math.pi, 0.5 * math.pi), (0.0, 1.0),
                     (1.5, INF), (0.0, INF), (-INF, INF)]
    assert s[9:14] == [(-2.0, 5.0)] * 2 + [(0.0, 1.0)] * 2 + [(-3.0, 4.0)]
    assert s[14:17] == [(0.0, 2.0), (-1.0, 2.0), (-INF, INF)]
    assert s[17] == (-1.0, 12.0) and s[18] == (2.0 * 0.01 + 0.1, INF) and s[19] == (-6.0, 7.0)
    assert s[20] == (0.0, INF) and s[21] == (-INF, INF) and s[22] == (-10.0, 0.0) and s[23] == (0.001 * 0.01, 20.0)
    assert not pt.is_affine and pt.parents[17] == (1, 13) and pt.parents[19] == (1, 2) and pt.parents[0] == ()
    # an affine list stops being affine with a Ref, and a Ref with scale 1 and offset 0 is written as the bare column
    assert not P.PriorTransform([P.Fixed(1.0), P.Uniform(0.0, Ref(0))]).is_affine
    assert P.PriorTransform([P.Fixed(1.0), P.Uniform(0.0, 2.0)]).is_affine
    assert Ref(3).expr(3) == "p[3]" and Ref(3, scale=2.0, offset=0.5).expr(3) == "(0x1.0000000000000p+1 * p[3] + 0x1.0000000000000p-1)"


# ---- evaluation order ------------------------------------------------------------------------------------------------------

def _order(pt):
    return [[id(q) for q in pt.priors].index(id(p)) for p in pt.order]


def _written(pt):
    """the columns in the order the generated function assigns them for the first time"""
    import re
    seen = []
    for j in re.findall(r"^\s+p\[(\d+)\] = ", pt.source.split("mlf_user_transform")[1], flags=re.M):
        if int(j) not in seen:
            seen.append(int(j))
    return seen


def chain5():
    """a chain of depth 5 written backwards: column k reads column k + 1"""
    return [P.Normal(Ref(k + 1), 1.0, name="c%d" % k) for k in range(5)] + [P.Normal(0.0, 1.0, name="c5")]


def diamond():
    return [P.Normal(Ref("left"), Ref("right"), name="bottom"), P.LogUniform(0.1, 10.0, name="top"),
            P.Normal(Ref("top"), 1.0, name="left"), P.Exponential(Ref("top"), name="right"), P.Uniform(0.0, 1.0, name="free")]


def test_chain_diamond_later_column_and_block_target_are_ordered():
    pt = P.PriorTransform(chain5())
    assert _order(pt) == [5, 4, 3, 2, 1, 0] == _written(pt) and pt.parents == [(1,), (2,), (3,), (4,), (5,), ()]
    pt = P.PriorTransform(diamond())
    assert _order(pt) == [1, 2, 3, 0, 4] == _written(pt) and pt.parents[0] == (2, 3) and pt.parents[2] == (1,)
    # a Ref to a later column moves only what has to move: ties stay in list order
    pt = P.PriorTransform([P.Uniform(0.0, 1.0), P.Normal(Ref(3), 1.0), P.Uniform(0.0, 1.0), P.Normal(0.0, 1.0), P.Sine()])
    assert _order(pt) == [0, 2, 3, 1, 4] == _written(pt)
    # a block is one unit, its columns are targets by name_k or by index
    pt = P.PriorTransform([P.Normal(Ref("o_1"), Ref("d_0")), P.OrderedUniform(0.0, 1.0, 3, name="o"), P.Dirichlet([1.0, 2.0], name="d"),
                           P.Normal(Ref(2), 1.0)])
    assert _order(pt) == [1, 2, 0, 3] and pt.parents[0] == (2, 4) and pt.parents[6] == (2,)
    assert _written(pt)[-2:] == [0, 6] and pt.paramnames[1:6] == ["o_0", "o_1", "o_2", "d_0", "d_1"]
    # without a Ref the order is the list's
    pt = P.PriorTransform([P.Normal(0.0, 1.0), P.Tabulated([0.0, 1.0], [0.0, 1.0]), P.Sine()])
    assert _order(pt) == [0, 1, 2] and pt.parents == [(), (), ()]


def test_column_j_still_consumes_u_j():
    import re
    pt = P.PriorTransform(diamond())
    body = pt.source.split("mlf_user_transform")[1]
    assert re.findall(r"p\[(\d+)\] = \w+\(u\[(\d+)\]", body) == [(str(j), str(j)) for j in (1, 2, 3, 0, 4)]


# ---- the example model -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 6])
def test_hierarchical_gauss_evidence_is_the_marginal_normal_density(n):
    model, lnz = usermodels.hierarchical_gauss(n)
    y = usermodels.hierarchical_gauss_data(n)
    assert model.ndim == n + 1 and model.has_transform and np.array_equal(model.aux, y)
    cov = 0.34 * np.eye(n) + np.ones((n, n))
    want = -0.5 * y.dot(np.linalg.solve(cov, y)) - 0.5 * np.linalg.slogdet(2 * np.pi * cov)[1]
    assert abs(lnz - want) < 1e-12 * (1 + abs(want)), (lnz, want)
    assert np.abs(y).max() < 1.0
