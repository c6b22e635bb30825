"""Reference of the run-time part of the prior library (``priors.Ref``, ``priors.Tabulated``,
csrc/mlf_priors_rt_dev.hpp), used by the CPU and the GPU tests.

A ``Ref`` column.  Its reference is ``prior_reference.reference`` of the same family constructed from the row's realised
parameter bits (``constant_prior``), its bound that family's 1e-12 * S (``ref_excess``): no new tolerance.  ``rt_standin`` restates
the four run-time forms in numpy (scipy.special supplies erfc and ndtri), ``Ref.value`` the affine map.

A table.  ``table_restatement`` is the device formula in numpy, bit for bit: k = the largest index <= n - 2 with c_k <= u,
dl = u - c_k, dr = c_(k+1) - u, p = dl <= dr ? x_k + dl * s_k : x_(k+1) - dr * s_k.  ``table_reference`` is the exact
piecewise-linear inverse of the binary64 table (c, x) in mpmath, p_ref = x_k + (u - c_k) (x_(k+1) - x_k) / (c_(k+1) - c_k).

The bound B = 2^-52 |p_ref| + 3 * 2^-53 |x_(k+1) - x_k|, from the operation count with eps = 2^-53 per rounding: the host's slope
s_k carries three roundings (the two differences and the quotient), the device's dl (or dr) one and the product one more: the
term dl * s_k has a relative error of at most 5 eps (1 + O(eps)).  The form is chosen from the nearer knot, dl <= dr, so
|dl| <= (c_(k+1) - c_k) / 2 up to a rounding and the term is at most |x_(k+1) - x_k| / 2 (1 + O(eps)): its absolute error is
at most 2.5 eps |x_(k+1) - x_k| (1 + O(eps)) < 3 eps |x_(k+1) - x_k|.  The final sum rounds once, eps |p| <= eps |p_ref| (1 +
O(eps)), which the bound carries with a factor of two.  On a point mass (x_k = x_(k+1), slope 0) and at a knot (dl = 0 or
dr = 0) the result is the knot itself.  A product that underflows adds at most 2^-1075, below every term unless
|x_(k+1) - x_k| < 2^-1020; no test table goes there.
"""
import mpmath as mp
import numpy as np

import prior_reference as PR
from ultranest_amd import priors as P

EPS = 2.0 ** -53


# ---- Ref columns ------------------------------------------------------------------------------------------------------

# family -> (constructor arguments that take a Ref, how to read them off a constant prior of prior_reference.family(name))
REF_FAMILIES = {
    "Uniform": lambda p: (p.lo, p.hi), "LogUniform": lambda p: (p.lo, p.hi), "Normal": lambda p: (p.mu, p.sigma),
    "TruncatedNormal": lambda p: (p.mu, p.sigma, p.lo, p.hi), "LogNormal": lambda p: (p.mu, p.sigma),
    "HalfNormal": lambda p: (p.scale,), "Exponential": lambda p: (p.scale,), "Rayleigh": lambda p: (p.scale,),
    "HalfCauchy": lambda p: (p.scale,), "Weibull": lambda p: (p.scale, p.shape), "Pareto": lambda p: (p.scale, p.shape),
    "Cauchy": lambda p: (p.loc, p.scale), "Laplace": lambda p: (p.loc, p.scale), "Logistic": lambda p: (p.loc, p.scale),
    "Gumbel": lambda p: (p.loc, p.scale), "Triangular": lambda p: (p.lo, p.mode, p.hi),
}
RUN_TIME_FORMS = ("Uniform", "LogUniform", "TruncatedNormal", "Triangular")        # the rest pass through
# the iterative families: (constant leading arguments, Ref arguments) of three settings each
SPECIAL_REF_FAMILIES = {
    "Gamma": [((2.5,), (3.0,)), ((0.1,), (0.01,)), ((1000.0,), (70.0,))],
    "InverseGamma": [((2.5,), (3.0,)), ((0.1,), (0.01,)), ((1000.0,), (70.0,))],
    "StudentT": [((3.0,), (0.0, 1.0)), ((1.0,), (100.0, 0.5)), ((1000.0,), (-3.0, 20.0))],
}


def constant_prior(name, args, lead=()):
    """the constant-parameter prior of one family from realised parameter values"""
    return getattr(P, name)(*(tuple(lead) + tuple(float(a) for a in args)))


def ref_list(name, args, lead=()):
    """[Fixed(a), Fixed(b), ..., Family(lead..., Ref(0), Ref(1), ...)]: the child is the last column"""
    fixed = [P.Fixed(a) for a in args]
    return fixed + [getattr(P, name)(*(tuple(lead) + tuple(P.Ref(k) for k in range(len(args)))))]


def ref_excess(name, params, u, got):
    """|got - reference| / (1e-12 S) per row, the reference and S those of the constant prior built from the row's realised
    parameters `params` (rows, nparams)"""
    params, u, got = np.atleast_2d(params), np.ravel(u), np.ravel(got)
    out = np.empty(len(u))
    for r in range(len(u)):
        out[r] = PR.excess(constant_prior(name, params[r]), u[r:r + 1], got[r:r + 1])[0]
    return out


def rt_standin(name, u, *par):
    """the four run-time forms of csrc/mlf_priors_rt_dev.hpp in numpy (valid parameters)"""
    from scipy.special import erfc, ndtri
    u = np.asarray(u, dtype=float)
    par = [np.asarray(x, dtype=float) for x in par]
    with np.errstate(all="ignore"):
        if name == "Uniform":
            lo, hi = par
            return lo + u * (hi - lo)
        if name == "LogUniform":
            lo, hi = par
            a = np.log(lo)
            return np.exp(a + u * (np.log(hi) - a))
        if name == "TruncatedNormal":
            mu, sigma, lo, hi = par
            r2 = np.sqrt(2.0)
            a, b = (lo - mu) / sigma, (hi - mu) / sigma
            Fa, Fb, Qa, Qb = 0.5 * erfc(-a / r2), 0.5 * erfc(-b / r2), 0.5 * erfc(a / r2), 0.5 * erfc(b / r2)
            q = Fa + u * (Fb - Fa)
            qq = Qb + (1.0 - u) * (Qa - Qb)
            z = np.where(q <= 0.5, ndtri(np.minimum(q, 0.5)), -ndtri(np.minimum(qq, 0.5)))
            return mu + sigma * np.minimum(np.maximum(z, a), b)
        if name == "Triangular":
            lo, mode, hi = par
            w = hi - lo
            c, c1, c2 = (mode - lo) / w, w * (mode - lo), w * (hi - mode)
            return np.where(u <= c, lo + np.sqrt(u * c1), hi - np.sqrt((1.0 - u) * c2))
    raise ValueError("no run-time form for %s" % name)


# ---- tables -----------------------------------------------------------------------------------------------------------

def table_index(c, u):
    """the largest k <= n - 2 with c_k <= u"""
    return np.minimum(np.searchsorted(c, u, side="right") - 1, len(c) - 2)


def table_restatement(tab, u, k=None):
    """the device formula in numpy, bit for bit; `tab` has .cdf, .x and .slopes"""
    u = np.asarray(u, dtype=float)
    c, x, s = tab.cdf, tab.x, tab.slopes
    k = table_index(c, u) if k is None else k
    dl, dr = u - c[k], c[k + 1] - u
    return np.where(dl <= dr, x[k] + dl * s[k], x[k + 1] - dr * s[k])


def table_reference(tab, u):
    """([exact piecewise-linear inverse of the binary64 table as mpf], [|x_(k+1) - x_k| as mpf]) for the 1-d u"""
    c, x = tab.cdf, tab.x
    ref, width = [], []
    with mp.workdps(50):
        for ui, k in zip(np.ravel(u), table_index(c, np.ravel(u))):
            ck, ck1, xk, xk1 = mp.mpf(float(c[k])), mp.mpf(float(c[k + 1])), mp.mpf(float(x[k])), mp.mpf(float(x[k + 1]))
            assert ck <= ui < ck1
            ref.append(xk + (mp.mpf(float(ui)) - ck) * (xk1 - xk) / (ck1 - ck))
            width.append(xk1 - xk)
    return ref, width


def table_excess(tab, u, got, ref=None):
    """|got - p_ref| / B per value (module docstring); a non-finite value gives inf"""
    ref, width = table_reference(tab, u) if ref is None else ref
    got = np.ravel(got)
    out = np.empty(len(got))
    with mp.workdps(50):
        for i in range(len(got)):
            if not np.isfinite(got[i]):
                out[i] = np.inf
                continue
            B = 2 * EPS * abs(ref[i]) + 3 * EPS * width[i]
            err = abs(mp.mpf(float(got[i])) - ref[i])
            out[i] = float(err / B) if B > 0 else (0.0 if err == 0 else np.inf)
    return out


def table_accepts(tab, u, got, ref=None):
    return bool(table_excess(tab, u, got, ref).max() <= 1.0)


def slopes_follow_the_rule(tab):
    """the host's slopes: (x_(k+1) - x_k) / (c_(k+1) - c_k) in binary64, exactly 0 on a flat CDF segment"""
    dx, dc = tab.x[1:] - tab.x[:-1], tab.cdf[1:] - tab.cdf[:-1]
    want = np.zeros(len(dx))
    want[dc > 0] = dx[dc > 0] / dc[dc > 0]
    return bool(np.array_equal(want, tab.slopes) and np.array_equal(tab.table, np.concatenate([tab.cdf, tab.x, tab.slopes])))


def table_u(tab):
    """the u values of the table tests: every knot, both neighbours of every knot, 2^-1022 and 1 - 2^-53, inside (0, 1), sorted"""
    c = tab.cdf
    u = np.concatenate([c, np.nextafter(c, -1.0), np.nextafter(c, 2.0), [2.0 ** -1022, 1 - 2.0 ** -53]])
    return np.unique(u[(u > 0) & (u < 1)])


def make_table(n, seed=0, kind="smooth"):
    """the tables of the tests, a function of (n, seed, kind) alone:
    smooth   seeded knots of a skewed distribution, strictly increasing
    steps    as smooth with every fifth CDF segment flat (a gap in the support) and every seventh x repeated (a point mass)
    heavy    heavy-tailed x of scale 1e6"""
    rs = np.random.RandomState(1000 * seed + n)
    c = np.concatenate([[0.0], np.sort(rs.uniform(size=n - 2)), [1.0]]) if n > 2 else np.array([0.0, 1.0])
    x = np.cumsum(rs.exponential(size=n)) - 3.0
    if kind == "heavy":
        x = 1e6 * np.sort(rs.standard_cauchy(size=n))
    if kind == "steps" and n >= 4:
        for k in range(1, n - 2, 5):
            c[k + 1] = c[k]
        for k in range(2, n - 2, 7):
            if c[k + 1] > c[k]:
                x[k + 1] = x[k]
    return P.Tabulated(x, c)


TABLE_SIZES = (2, 3, 4, 5, 1023, 1024, 1025, 4096)
