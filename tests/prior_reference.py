"""High-precision reference of the prior library (ultranest_amd.priors): the exact quantile of every family from the binary64
u and the binary64 parameters, in mpmath at 60 digits, the scale S against which an error is judged, and the comparison both
the CPU and the GPU tests use.

S classes (the tolerance is the project's class for device libm results against mpmath, 1e-12 * S, tests/test_loglike_forms.py):

  R  |p_ref|                                         where the formula should be relatively accurate
  A  |loc| + scale * (1 + |z_ref|), z_ref = (p_ref - loc) / scale
  E  |p_ref| * (1 + |ln p_ref - ln unit|), unit = lo (LogUniform), 1 (LogNormal), scale (Weibull), xm (Pareto)

so a wrong tail costs a relative error of order 1, not 1e-12.

Every quantile is evaluated from the side that keeps the information of u at 60 digits: ``log1p(-u)`` and ``erf(y) = u`` for
small u (1 - u has 1022 leading nines at u = 2^-1022), the upper-tail equation Q(x) = 1 - u for u > 0.5 (1 - u is exact there).
"""
import statistics

import mpmath as mp
import numpy as np

from ultranest_amd import priors as P

DPS = 60
RTOL = 1e-12
_ND = statistics.NormalDist()


def grid(seed=1):
    """the u values of the tests, sorted: the extremes of (0, 1), the three doubles around 0.25, 0.5 and 0.75, 512 seeded draws"""
    edge = [2.0 ** -1022, 1e-300, 1e-100, 1e-17, 2.0 ** -53, 1e-8, 0.01, 1 - 1e-8, 1 - 2.0 ** -53]
    for c in (0.25, 0.5, 0.75):
        edge += [np.nextafter(c, 0.0), c, np.nextafter(c, 1.0)]
    u = np.concatenate([np.array(edge), np.random.RandomState(seed).uniform(size=512)])
    u = np.unique(u)
    assert u[0] > 0 and u[-1] < 1
    return u


def _upper_x(q):
    """x >= 0 with Q(x) = 0.5 erfc(x / sqrt 2) = q for 0 < q <= 0.5 (Newton on ln Q from a binary64 start)"""
    q = mp.mpf(q)
    if q == mp.mpf(0.5):
        return mp.mpf(0)
    x = mp.mpf(-_ND.inv_cdf(float(q))) if float(q) > 0 else mp.sqrt(-2 * mp.log(q))
    r2 = mp.sqrt(2)
    lq = mp.log(q)
    for _ in range(60):
        Q = mp.erfc(x / r2) / 2
        phi = mp.exp(-x * x / 2) / mp.sqrt(2 * mp.pi)
        step = (mp.log(Q) - lq) * Q / phi
        x = x + step
        if abs(step) <= mp.mpf(10) ** (-DPS + 8) * (1 + abs(x)):
            return x
    raise RuntimeError("no convergence for Q(x) = %s" % q)


def _z(u):
    """standard normal quantile of the binary64 u (mpf)"""
    u = mp.mpf(u)
    return -_upper_x(u) if u <= mp.mpf(0.5) else _upper_x(1 - u)


def _z_of_cdf(q_lower, q_upper):
    """quantile from both tails' probabilities: the smaller one decides"""
    return -_upper_x(q_lower) if q_lower <= q_upper else _upper_x(q_upper)


def _erfinv_small(u):
    """y with erf(y) = u for 0 < u <= 0.5 (Newton; relatively accurate down to the smallest u)"""
    u = mp.mpf(u)
    y = u * mp.sqrt(mp.pi) / 2 if u < mp.mpf("1e-8") else mp.mpf(_ND.inv_cdf(0.5 + 0.5 * float(u))) / mp.sqrt(2)
    for _ in range(60):
        step = (mp.erf(y) - u) / (2 / mp.sqrt(mp.pi) * mp.exp(-y * y))
        y = y - step
        if abs(step) <= mp.mpf(10) ** (-DPS + 8) * abs(y):
            return y
    raise RuntimeError("no convergence for erf(y) = %s" % u)


def _Phi(x):
    return mp.erfc(-x / mp.sqrt(2)) / 2


def _one(prior, u):
    """the exact quantile of a one-column prior at the binary64 u, as an mpf"""
    m = mp.mpf
    u = m(float(u))
    t = type(prior).__name__
    if t == "Fixed":
        return m(prior.v)
    if t == "Uniform":
        return m(prior.lo) + u * (m(prior.hi) - m(prior.lo))
    if t == "LogUniform":
        return mp.exp(mp.log(m(prior.lo)) + u * (mp.log(m(prior.hi)) - mp.log(m(prior.lo))))
    if t == "Normal":
        return m(prior.mu) + m(prior.sigma) * _z(u)
    if t == "LogNormal":
        return mp.exp(m(prior.mu) + m(prior.sigma) * _z(u))
    if t == "TruncatedNormal":
        a, b = (m(prior.lo) - m(prior.mu)) / m(prior.sigma), (m(prior.hi) - m(prior.mu)) / m(prior.sigma)
        Fa, Fb, Qa, Qb = _Phi(a), _Phi(b), _Phi(-a), _Phi(-b)
        z = _z_of_cdf(Fa + u * (Fb - Fa), Qb + (1 - u) * (Qa - Qb))
        return m(prior.mu) + m(prior.sigma) * z
    if t == "HalfNormal":
        x = mp.sqrt(2) * _erfinv_small(u) if u <= m(0.5) else _upper_x((1 - u) / 2)
        return m(prior.scale) * x
    if t == "Exponential":
        return m(prior.scale) * -mp.log1p(-u)
    if t == "Rayleigh":
        return m(prior.scale) * mp.sqrt(-2 * mp.log1p(-u))
    if t == "Weibull":
        return m(prior.scale) * mp.exp(mp.log(-mp.log1p(-u)) / m(prior.shape))
    if t == "Pareto":
        return m(prior.scale) * mp.exp(-mp.log1p(-u) / m(prior.shape))
    if t == "Cauchy":
        return m(prior.loc) - m(prior.scale) * mp.cos(mp.pi * u) / mp.sin(mp.pi * u)
    if t == "HalfCauchy":
        return m(prior.scale) * mp.tan(mp.pi * u / 2)
    if t == "Laplace":
        return m(prior.loc) + m(prior.scale) * (mp.log(2 * u) if u <= m(0.5) else -mp.log(2 * (1 - u)))
    if t == "Logistic":
        return m(prior.loc) + m(prior.scale) * (mp.log(u) - mp.log1p(-u))
    if t == "Gumbel":
        return m(prior.loc) - m(prior.scale) * mp.log(-mp.log(u))
    if t == "Triangular":
        lo, mode, hi = m(prior.lo), m(prior.mode), m(prior.hi)
        if u <= (mode - lo) / (hi - lo):
            return lo + mp.sqrt(u * (hi - lo) * (mode - lo))
        return hi - mp.sqrt((1 - u) * (hi - lo) * (hi - mode))
    if t == "Sine":
        return 2 * mp.asin(mp.sqrt(u))
    if t == "Cosine":
        return 2 * mp.asin(mp.sqrt(u)) - mp.pi / 2
    raise ValueError("no reference for %s" % t)


def reference(prior, u):
    """exact quantiles: a list of mpf for the 1-d array `u` of a one-column prior; for a block prior `u` is (rows, size) and
    the result a list of rows"""
    with mp.workdps(DPS):
        if isinstance(prior, P.MultivariateNormal):
            out = []
            for row in np.atleast_2d(u):
                z = [_z(x) for x in row]
                out.append([mp.mpf(prior.mean[i]) + mp.fsum(mp.mpf(prior.L[i, j]) * z[j] for j in range(i + 1))
                            for i in range(prior.size)])
            return out
        if isinstance(prior, P.OrderedUniform):
            out = []
            n = prior.size
            for row in np.atleast_2d(u):
                t, vals = mp.mpf(1), [None] * n
                for k in range(n - 1, -1, -1):
                    t = t * mp.exp(mp.log(mp.mpf(float(row[k]))) / (k + 1))
                    vals[k] = mp.mpf(prior.lo) + t * (mp.mpf(prior.hi) - mp.mpf(prior.lo))
                out.append(vals)
            return out
        return [_one(prior, x) for x in np.ravel(u)]


_CLASS_R = ("HalfNormal", "Exponential", "Rayleigh", "HalfCauchy", "Sine")
_CLASS_E = {"LogUniform": lambda p: p.lo, "LogNormal": lambda p: 1.0, "Weibull": lambda p: p.scale, "Pareto": lambda p: p.scale}


def _loc_scale(prior, u):
    t = type(prior).__name__
    if t in ("Normal", "TruncatedNormal"):
        return prior.mu, prior.sigma
    if t in ("Cauchy", "Laplace", "Logistic", "Gumbel"):
        return prior.loc, prior.scale
    if t == "Triangular":
        lower = mp.mpf(float(u)) <= (mp.mpf(prior.mode) - mp.mpf(prior.lo)) / (mp.mpf(prior.hi) - mp.mpf(prior.lo))
        return (prior.lo if lower else prior.hi), prior.hi - prior.lo
    if t == "Cosine":
        return 0.0, 1.0
    if t in ("Uniform", "OrderedUniform"):
        return prior.lo, prior.hi - prior.lo
    if t == "Fixed":
        return prior.v, 0.0
    raise ValueError("no scale class for %s" % t)


def scale(prior, u, p_ref):
    """S of one value (mpf): class R, E or A of the module docstring"""
    t = type(prior).__name__
    with mp.workdps(DPS):
        if t in _CLASS_R:
            return abs(p_ref)
        if t in _CLASS_E:
            return abs(p_ref) * (1 + abs(mp.log(p_ref) - mp.log(mp.mpf(_CLASS_E[t](prior)))))
        loc, sc = _loc_scale(prior, u)
        loc, sc = mp.mpf(loc), mp.mpf(sc)
        if sc == 0:
            return abs(loc)
        return abs(loc) + sc * (1 + abs((p_ref - loc) / sc))


def excess(prior, u, got, ref=None):
    """|got - reference| / (1e-12 * S) per value of a one-column prior, as a float array (a non-finite `got` gives inf)"""
    u, got = np.ravel(u), np.ravel(got)
    ref = reference(prior, u) if ref is None else ref
    out = np.empty(len(u))
    with mp.workdps(DPS):
        for i in range(len(u)):
            if not np.isfinite(got[i]):
                out[i] = np.inf
                continue
            S = scale(prior, u[i], ref[i])
            err = abs(mp.mpf(float(got[i])) - ref[i])
            out[i] = float(err / (RTOL * S)) if S > 0 else (0.0 if err == 0 else np.inf)
    return out


def accepts(prior, u, got, ref=None):
    """the comparison of the tests: every value within 1e-12 * S of the reference"""
    return bool(excess(prior, u, got, ref).max() <= 1.0)


def mvn_restatement(mean, L, z):
    """the MultivariateNormal block in numpy, bit for bit, from the z rows (n_rows, n): descending rows, ascending j, plain *
    and +, each product rounded before it is added (what -ffp-contract=off leaves of the generated code)"""
    p = np.array(z, dtype=float)
    n = p.shape[1]
    for i in range(n - 1, -1, -1):
        s = L[i, 0] * p[:, 0]
        for j in range(1, i + 1):
            s = s + L[i, j] * p[:, j]
        p[:, i] = mean[i] + s
    return p


def mvn_scale(prior, z):
    """S_i = |mean_i| + sum_j |L_ij z_j| for the z rows (floats are enough for a scale)"""
    return np.abs(prior.mean)[None, :] + np.abs(z[:, None, :] * prior.L[None, :, :]).sum(axis=2)


# ---- numpy stand-ins of the stated formulas (CPU restatements; scipy.special supplies ndtri and erfinv) ---------------

def _sinpi(x):
    """sin(pi x) for x in [0, 1] from an exactly reduced argument"""
    x = np.asarray(x, dtype=float)
    return np.where(x <= 0.25, np.sin(np.pi * x), np.where(x < 0.75, np.cos(np.pi * (0.5 - x)), np.sin(np.pi * (1.0 - x))))


def _cospi(x):
    """cos(pi x) for x in [0, 1]"""
    x = np.asarray(x, dtype=float)
    return np.where(x <= 0.25, np.cos(np.pi * x), np.where(x < 0.75, np.sin(np.pi * (0.5 - x)), -np.cos(np.pi * (1.0 - x))))


def standin(prior, u):
    """the stated device formula of a one-column prior in numpy"""
    from scipy.special import erfinv, ndtri
    u = np.asarray(u, dtype=float)
    t = type(prior).__name__
    lower = u <= 0.5
    um = np.where(lower, u, 0.5)          # arguments of the branch not taken, kept inside the domain
    tm = np.where(lower, 0.5, 1.0 - u)
    z = np.where(lower, ndtri(um), -ndtri(tm))
    with np.errstate(all="ignore"):
        if t == "Fixed":
            return np.full_like(u, prior.v)
        if t == "Uniform":
            return prior.lo + u * prior.w
        if t == "LogUniform":
            return np.exp(prior.a + u * prior.w)
        if t == "Normal":
            return prior.mu + prior.sigma * z
        if t == "LogNormal":
            return np.exp(prior.mu + prior.sigma * z)
        if t == "TruncatedNormal":
            q = prior.Fa + u * (prior.Fb - prior.Fa)
            qq = prior.Qb + (1.0 - u) * (prior.Qa - prior.Qb)
            zz = np.where(q <= 0.5, ndtri(np.minimum(q, 0.5)), -ndtri(np.minimum(qq, 0.5)))
            return prior.mu + prior.sigma * np.minimum(np.maximum(zz, prior.a), prior.b)
        if t == "HalfNormal":
            return np.where(lower, prior.scale * (np.sqrt(2.0) * erfinv(um)), prior.scale * -ndtri(0.5 * tm))
        if t == "Exponential":
            return prior.scale * -np.log1p(-u)
        if t == "Rayleigh":
            return prior.scale * np.sqrt(-2.0 * np.log1p(-u))
        if t == "Weibull":
            return prior.scale * np.exp(np.log(-np.log1p(-u)) / prior.shape)
        if t == "Pareto":
            return prior.scale * np.exp(-np.log1p(-u) / prior.shape)
        if t == "Cauchy":
            return prior.loc + prior.scale * (-_cospi(u) / _sinpi(u))
        if t == "HalfCauchy":
            return prior.scale * (_sinpi(0.5 * u) / _cospi(0.5 * u))
        if t == "Laplace":
            return np.where(lower, prior.loc + prior.scale * np.log(2.0 * um), prior.loc - prior.scale * np.log(2.0 * tm))
        if t == "Logistic":
            return prior.loc + prior.scale * (np.log(u) - np.log1p(-u))
        if t == "Gumbel":
            return prior.loc - prior.scale * np.log(-np.log(u))
        if t == "Triangular":
            return np.where(u <= prior.c, prior.lo + np.sqrt(u * prior.c1), prior.hi - np.sqrt((1.0 - u) * prior.c2))
        if t == "Sine":
            return 2.0 * np.arctan2(np.sqrt(u), np.sqrt(1.0 - u))
        if t == "Cosine":
            return np.arctan2(2.0 * u - 1.0, 2.0 * np.sqrt(u * (1.0 - u)))
    raise ValueError("no stand-in for %s" % t)


# three parameter settings per family (the tests' cases): a plain one, one with a large offset against its scale or a small
# scale, one with an extreme shape or a truncation in a tail.  Every setting keeps the exact quantile a normal or subnormal
# binary64 number over the whole grid (a Weibull shape k < 1 puts p(2^-1022) = scale * 2^(-1022 / k) below the smallest
# subnormal, a Pareto alpha < 0.05 puts p(1 - 2^-53) above the largest double, a Cauchy scale above 12 does so with
# |p(2^-1022)| = scale / (pi 2^-1022): range limits of the format, not of the formula)
FAMILIES = {
    "Fixed": [lambda: P.Fixed(0.0), lambda: P.Fixed(-3.25), lambda: P.Fixed(1e300)],
    "Uniform": [lambda: P.Uniform(0.0, 1.0), lambda: P.Uniform(-10.0, 10.0), lambda: P.Uniform(1e3, 1e3 + 0.1)],
    "LogUniform": [lambda: P.LogUniform(1e-3, 10.0), lambda: P.LogUniform(1.0, 2.0), lambda: P.LogUniform(1e-10, 1e10)],
    "Normal": [lambda: P.Normal(0.0, 1.0), lambda: P.Normal(100.0, 0.5), lambda: P.Normal(-3.0, 20.0)],
    "TruncatedNormal": [lambda: P.TruncatedNormal(0.0, 1.0, -1.0, 2.0), lambda: P.TruncatedNormal(1.0, 2.0, 7.0, 11.0),
                        lambda: P.TruncatedNormal(0.5, 0.3, -3.0, 0.0)],
    "LogNormal": [lambda: P.LogNormal(0.0, 1.0), lambda: P.LogNormal(3.0, 0.25), lambda: P.LogNormal(-2.0, 2.0)],
    "HalfNormal": [lambda: P.HalfNormal(1.0), lambda: P.HalfNormal(0.01), lambda: P.HalfNormal(300.0)],
    "Exponential": [lambda: P.Exponential(1.0), lambda: P.Exponential(0.03), lambda: P.Exponential(70.0)],
    "Rayleigh": [lambda: P.Rayleigh(1.0), lambda: P.Rayleigh(0.03), lambda: P.Rayleigh(70.0)],
    "Weibull": [lambda: P.Weibull(1.0, 1.5), lambda: P.Weibull(3.0, 1.0), lambda: P.Weibull(0.1, 8.0)],
    "Pareto": [lambda: P.Pareto(1.0, 3.0), lambda: P.Pareto(0.2, 0.7), lambda: P.Pareto(50.0, 12.0)],
    "Cauchy": [lambda: P.Cauchy(0.0, 1.0), lambda: P.Cauchy(100.0, 0.5), lambda: P.Cauchy(-3.0, 5.0)],
    "HalfCauchy": [lambda: P.HalfCauchy(1.0), lambda: P.HalfCauchy(0.01), lambda: P.HalfCauchy(300.0)],
    "Laplace": [lambda: P.Laplace(0.0, 1.0), lambda: P.Laplace(100.0, 0.5), lambda: P.Laplace(-3.0, 20.0)],
    "Logistic": [lambda: P.Logistic(0.0, 1.0), lambda: P.Logistic(100.0, 0.5), lambda: P.Logistic(-3.0, 20.0)],
    "Gumbel": [lambda: P.Gumbel(0.0, 1.0), lambda: P.Gumbel(100.0, 0.5), lambda: P.Gumbel(-3.0, 20.0)],
    "Triangular": [lambda: P.Triangular(0.0, 0.3, 1.0), lambda: P.Triangular(-5.0, -5.0, 2.0), lambda: P.Triangular(10.0, 13.0, 13.0)],
    "Sine": [lambda: P.Sine(), lambda: P.Sine(), lambda: P.Sine()],
    "Cosine": [lambda: P.Cosine(), lambda: P.Cosine(), lambda: P.Cosine()],
}


def family(name):
    return [make() for make in FAMILIES[name]]
