"""The yardstick of the prior library's tests, checked on the CPU: the mpmath quantiles of prior_reference against
scipy.stats, the comparison function against deliberately wrong formulas (it must reject each) and against numpy stand-ins of
the stated device formulas (it must accept each), and the numpy restatement of the MultivariateNormal block against mpmath."""
import mpmath as mp
import numpy as np
import pytest

import prior_reference as PR
from ultranest_amd import priors as P

U = PR.grid()
# where scipy's own ppf can serve as a yardstick: its Cauchy (tan(pi q - pi/2)), half-normal (ndtri((1 + q) / 2)) and others lose
# their tails exactly as the seeded defects below do, so the two references are compared on the bulk of the grid -- the draws and
# the three doubles around the quartiles -- and the tails are left to the defects test, which shows that the mpmath side has them
BULK = U[(U >= 1e-3) & (U <= 1 - 1e-3)]


def _scipy_ppf(prior, u):
    st = pytest.importorskip("scipy.stats")
    t = type(prior).__name__
    if t == "Uniform":
        return st.uniform(prior.lo, prior.hi - prior.lo).ppf(u)
    if t == "LogUniform":
        return st.loguniform(prior.lo, prior.hi).ppf(u)
    if t == "Normal":
        return st.norm(prior.mu, prior.sigma).ppf(u)
    if t == "TruncatedNormal":
        return st.truncnorm(prior.a, prior.b, loc=prior.mu, scale=prior.sigma).ppf(u)
    if t == "LogNormal":
        return st.lognorm(prior.sigma, scale=np.exp(prior.mu)).ppf(u)
    if t == "HalfNormal":
        return st.halfnorm(scale=prior.scale).ppf(u)
    if t == "Exponential":
        return st.expon(scale=prior.scale).ppf(u)
    if t == "Rayleigh":
        return st.rayleigh(scale=prior.scale).ppf(u)
    if t == "Weibull":
        return st.weibull_min(prior.shape, scale=prior.scale).ppf(u)
    if t == "Pareto":
        return st.pareto(prior.shape, scale=prior.scale).ppf(u)
    if t == "Cauchy":
        return st.cauchy(prior.loc, prior.scale).ppf(u)
    if t == "HalfCauchy":
        return st.halfcauchy(scale=prior.scale).ppf(u)
    if t == "Laplace":
        return st.laplace(prior.loc, prior.scale).ppf(u)
    if t == "Logistic":
        return st.logistic(prior.loc, prior.scale).ppf(u)
    if t == "Gumbel":
        return st.gumbel_r(prior.loc, prior.scale).ppf(u)
    if t == "Triangular":
        return st.triang(prior.c, loc=prior.lo, scale=prior.hi - prior.lo).ppf(u)
    pytest.skip("scipy.stats has no %s distribution" % t)


SCIPY_FAMILIES = [f for f in sorted(PR.FAMILIES) if f not in ("Fixed", "Sine", "Cosine")]


@pytest.mark.parametrize("name", SCIPY_FAMILIES)
def test_reference_against_scipy(name):
    """1e-13 * S: ten times tighter than the tolerance the reference serves"""
    for prior in PR.family(name):
        got = _scipy_ppf(prior, BULK)
        e = PR.excess(prior, BULK, got) * (PR.RTOL / 1e-13)
        print(name, vars(prior), "largest error %.3g of the 1e-13 bound at u = %r" % (e.max(), BULK[np.argmax(e)]))
        assert e.max() <= 1.0


@pytest.mark.parametrize("name,cdf", [("Sine", lambda p: (1 - mp.cos(p)) / 2), ("Cosine", lambda p: (1 + mp.sin(p)) / 2)])
def test_sine_and_cosine_references_invert_their_cdf(name, cdf):
    """scipy.stats has neither density: the reference quantile is put back through the closed-form CDF at 60 digits.  Sine is
    judged relatively (class R): relative to u, and at the smallest u, where 1 - cos(p) cancels, through its leading term
    2 sqrt(u).  Cosine is judged absolutely (class A with scale 1): the CDF's slope is at most 1/2, so 1e-50 in the CDF is
    what 1e-50 in the quantile amounts to or more."""
    prior = PR.family(name)[0]
    ref = PR.reference(prior, U)
    with mp.workdps(PR.DPS):
        for u, p in zip(U, ref):
            um = mp.mpf(float(u))
            if name == "Cosine":
                assert abs(cdf(p) - um) <= mp.mpf(10) ** -50
            elif u > 1e-20:
                assert abs(cdf(p) - um) <= mp.mpf(10) ** -40 * um
            else:
                assert abs(p / (2 * mp.sqrt(um)) - 1) <= um


def _ndtri(x):
    from scipy.special import ndtri
    return ndtri(x)


def _erfinv(x):
    from scipy.special import erfinv
    return erfinv(x)


DEFECTS = {
    "Exponential with log(1 - u)": (lambda: P.Exponential(1.0), lambda u: -np.log(1.0 - u)),
    "Cauchy with tan(pi (u - 0.5))": (lambda: P.Cauchy(0.0, 1.0), lambda u: np.tan(np.pi * (u - 0.5))),
    "Sine with arccos(1 - 2 u)": (lambda: P.Sine(), lambda u: np.arccos(1.0 - 2.0 * u)),
    "HalfNormal with ndtri(0.5 + 0.5 u)": (lambda: P.HalfNormal(1.0), lambda u: _ndtri(0.5 + 0.5 * u)),
    "Normal without the flip at u > 0.5": (lambda: P.Normal(0.0, 1.0), lambda u: np.sqrt(2.0) * _erfinv(2.0 * u - 1.0)),
}


@pytest.mark.parametrize("which", sorted(DEFECTS))
def test_seeded_defects_are_rejected(which):
    pytest.importorskip("scipy.special")
    make, wrong = DEFECTS[which]
    prior = make()
    with np.errstate(all="ignore"):
        got = wrong(U)
    e = PR.excess(prior, U, got)
    print(which, "largest error %.3g of the bound at u = %r" % (e.max(), U[np.argmax(e)]))
    assert not PR.accepts(prior, U, got)
    # the same family's stated formula passes on the same grid: it is the defect that is rejected, not the family
    assert PR.accepts(prior, U, PR.standin(prior, U))


@pytest.mark.parametrize("name", sorted(PR.FAMILIES))
def test_standins_of_the_stated_formulas_pass(name):
    pytest.importorskip("scipy.special")
    for prior in PR.family(name):
        got = PR.standin(prior, U)
        e = PR.excess(prior, U, got)
        print(name, vars(prior), "largest error %.3g of the bound at u = %r" % (e.max(), U[np.argmax(e)]))
        assert np.isfinite(got).all() and e.max() <= 1.0
        assert (np.diff(got) >= 0).all()


def _mvn(n, seed=3):
    rs = np.random.RandomState(seed + n)
    A = rs.normal(size=(n, n))
    cov = A.dot(A.T) + n * np.eye(n)
    cov = 0.5 * (cov + cov.T)
    return P.MultivariateNormal(rs.normal(size=n) * 3, cov)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_multivariate_normal_restatement_against_mpmath(n):
    pytest.importorskip("scipy.special")
    prior = _mvn(n)
    assert np.allclose(prior.L.dot(prior.L.T), prior.cov, rtol=1e-13, atol=0) and np.array_equal(prior.L, np.tril(prior.L))
    rs = np.random.RandomState(5)
    u = np.concatenate([rs.uniform(size=(40, n)), rs.choice(U[:8], size=(8, n)), rs.choice(U[-8:], size=(8, n))])
    z = PR.standin(P.Normal(0.0, 1.0), u.ravel()).reshape(u.shape)
    p = PR.mvn_restatement(prior.mean, prior.L, z)
    # the restatement is the triangular product: a plain loop over rows in float agrees to rounding, and row 0 is one product
    assert np.array_equal(p[:, 0], prior.mean[0] + prior.L[0, 0] * z[:, 0])
    ref = PR.reference(prior, u)
    S = PR.mvn_scale(prior, z)
    worst = 0.0
    for r in range(len(u)):
        for i in range(n):
            err = abs(mp.mpf(float(p[r, i])) - ref[r][i])
            worst = max(worst, float(err / (PR.RTOL * S[r, i])))
    print("n = %d: largest error %.3g of the bound" % (n, worst))
    assert worst <= 1.0
