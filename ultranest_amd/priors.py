"""Prior library for device models: closed-form quantile transforms.

A prior transform maps the unit cube to the parameters, column by column, through each prior's quantile function (inverse
CDF).  In the reference users write it with ``scipy.stats.*.ppf`` inside ``transform``; a host callback keeps a model off every
device route.  Here a list of priors becomes an ordinary ``transform_source`` of ``ultranest_amd.devicemodel``, so every route
that serves a user model serves it unchanged::

    pt = PriorTransform([Uniform(-1, 1, name="x"), LogUniform(1e-3, 10, name="scale"), Normal(0, 2, name="offset"),
                         Sine(name="inclination")])
    model = pt.model(loglike_source)                  # a DeviceModel: model.transform / model.loglike on every device route
    StaticNestedSampler(pt.ndim, model.loglike, transform=model.transform, ...)
    p = pt.transform(u)                                # or the transform alone, for a likelihood that stays a host function

The device functions live in ``csrc/mlf_priors_dev.hpp`` (one ``__device__ __noinline__`` function per family); ``source`` is
that header's text followed by one generated call or statement per column, every constant a hexadecimal floating literal.  The
formulas are the interface.  ``u`` lies in the open interval (0, 1); ``1 - u`` is exact for ``u >= 0.5``::

    Fixed(v)                            v
    Uniform(lo, hi)                     lo + u * w,  w = hi - lo computed on the host in binary64
    LogUniform(lo, hi), 0 < lo < hi     exp(a + u * w),  a = log(lo), w = log(hi) - log(lo) from the host
    Normal(mu, sigma)                   z = u <= 0.5 ? normcdfinv(u) : -normcdfinv(1 - u);  mu + sigma * z
    TruncatedNormal(mu, sigma, lo, hi)  a, b = (lo - mu) / sigma, (hi - mu) / sigma;  Fa, Fb, Qa, Qb = Phi(a), Phi(b), Phi(-a),
                                        Phi(-b) from the host (0.5 * math.erfc(-+x / sqrt 2));  q = Fa + u * (Fb - Fa);
                                        q <= 0.5: z = normcdfinv(q), else z = -normcdfinv(Qb + (1 - u) * (Qa - Qb));
                                        z clamped to [a, b];  mu + sigma * z
    LogNormal(mu, sigma)                exp(mu + sigma * z), z as for Normal
    HalfNormal(sigma)                   u <= 0.5: sigma * (sqrt2 * erfinv(u)), else sigma * -normcdfinv(0.5 * (1 - u))
    Exponential(scale)                  scale * -log1p(-u)
    Rayleigh(sigma)                     sigma * sqrt(-2 * log1p(-u))
    Weibull(scale, k)                   scale * exp(log(-log1p(-u)) / k)
    Pareto(xm, alpha)                   xm * exp(-log1p(-u) / alpha)
    Cauchy(loc, scale)                  loc + scale * (-cospi(u) / sinpi(u))
    HalfCauchy(scale)                   scale * (sinpi(0.5 * u) / cospi(0.5 * u))
    Laplace(loc, b)                     u <= 0.5: loc + b * log(2 u), else loc - b * log(2 * (1 - u))
    Logistic(loc, s)                    loc + s * (log(u) - log1p(-u))
    Gumbel(loc, s)                      loc - s * log(-log(u))
    Triangular(lo, mode, hi)            u <= c: lo + sqrt(u * c1), else hi - sqrt((1 - u) * c2);  c = (mode - lo) / (hi - lo),
                                        c1 = (hi - lo) * (mode - lo), c2 = (hi - lo) * (hi - mode) from the host
    Sine()    density ~ sin on [0, pi]           2 * atan2(sqrt(u), sqrt(1 - u))           (= 2 asin(sqrt u))
    Cosine()  density ~ cos on [-pi/2, pi/2]     atan2(2 u - 1, 2 * sqrt(u * (1 - u)))     (= asin(2 u - 1))

(Sine and Cosine go through atan2 because asin has an infinite slope at +-1, exactly where ``sqrt(u)`` for u -> 1 and
``2 u - 1`` for u -> 0 have rounded away their distance from +-1; the atan2 arguments keep their relative accuracy in both
tails.)

Two block priors span several consecutive columns:

``MultivariateNormal(mean, cov)``, block size n <= 64: ``L = np.linalg.cholesky(cov)`` on the host; the generated code writes
``z_k`` (the Normal(0, 1) form) into ``p[k]`` for every column of the block, then for i = n-1 down to 0
``p[i] = mean_i + (((L_i0 * p[0]) + L_i1 * p[1]) + ... + L_ii * p[i])``: straight-line code in ascending j with plain ``*``
and ``+`` (no FMA is formed), so numpy restates it bit for bit from the z row; no table lives in the program's data section.

``OrderedUniform(lo, hi, n)``, an ascending vector (the order statistics of n uniform draws):
``t_(n-1) = exp(log(u_(n-1)) / n)``, ``t_k = t_(k+1) * exp(log(u_k) / (k + 1))`` for k = n-2 down to 0, ``p_k = lo + t_k * w``.

Gamma, beta, Student-t and Dirichlet priors need inverse incomplete gamma / beta functions, which have no closed form.  Their
device functions are iterative and live in a second header, ``csrc/mlf_priors_special_dev.hpp``, whose text follows the first
one's in ``source`` only when the list holds one of these families (a closed-form list gives exactly the text it always gave).
Every function works from the smaller tail q = min(u, 1 - u) and runs Newton's iteration on ln(tail) in the logarithm of the
unknown, with a compile-time cap on every loop (48 steps, 3000 terms); P, Q are the regularized incomplete gamma functions,
I_x(a, b) the regularized incomplete beta function::

    Gamma(shape, scale=1)               scale * x;  P(shape, x) = u for u <= 0.5, Q(shape, x) = 1 - u otherwise
    ChiSquared(k)                       Gamma(k / 2, 2): the same device function
    InverseGamma(shape, scale=1)        scale / x;  Q(shape, x) = u for u <= 0.5, P(shape, x) = 1 - u otherwise
    Beta(a, b)  on (0, 1)               x with I_x(a, b) = u, solved for the smaller of x and y = 1 - x, returned as x or 1 - y
    StudentT(nu, loc=0, scale=1)        loc + scale * t;  t = -sqrt(nu y / x) from x = nu / (nu + t^2) with I_x(nu/2, 1/2) = 2 q,
                                        carried as ln x and ln y; the sign is flipped for u > 0.5 (StudentT(nu, 0, 1) is odd bit
                                        for bit), t = 0 at u = 0.5
    Dirichlet(alpha), block n <= 64     g_k = the Gamma(alpha_k, 1) quantile of u_k into p[k];  s = ((g_0 + g_1) + ...) + g_(n-1)
                                        in ascending order with plain +;  p[k] = g_k / s, or 1 / n for every k if s == 0

Accepted ranges (the ranges over which each quantile is held to 1e-12 * S against 60-digit references from u = 2^-1022 to
1 - 2^-53; outside them the constructor raises ``ValueError``): shape, a, b and every alpha_k in [0.1, 1000], k in [0.2, 2000],
nu in [1, 1000]; scale > 0, loc finite.  ``lgamma(shape + 1)``, ``ln B(a, b)``, ``1 / shape`` and the logarithms of the
parameters are computed here in binary64 and passed as hexadecimal literals.  The columns of a Dirichlet block sum to 1, so no
ellipsoid in parameter space has a volume: a driver's t-region cannot be built over it and the drivers run without one, as the
reference does.  An iterative quantile costs several times a ``normcdfinv`` (DESIGN.md 7f has the measurement).

Every prior validates its parameters at construction (``ValueError`` before anything is compiled) and takes an optional
``name``.  ``Uniform(..., circular=True)`` marks a periodic parameter (``PriorTransform.wrapped_dims``).
"""
import math
import os

import numpy as np

from . import devicemodel
from .devicemodel import DeviceModel

HEADER = os.path.join(devicemodel.INCLUDE_DIR, "mlf_priors_dev.hpp")
SPECIAL_HEADER = os.path.join(devicemodel.INCLUDE_DIR, "mlf_priors_special_dev.hpp")
MAX_BLOCK = 64          # largest MultivariateNormal or Dirichlet block (straight-line code)
SHAPE_MIN, SHAPE_MAX = 0.1, 1000.0      # Gamma / InverseGamma shape, Beta a and b, Dirichlet alpha_k; ChiSquared k is twice it
NU_MIN, NU_MAX = 1.0, 1000.0            # StudentT degrees of freedom

CONSTANT_LOGLIKE = r"""
__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {
  return 0.0;
}
"""


def _hex(x):
    """a binary64 value as a C++17 hexadecimal floating literal (exact, and a function of the value's bits alone)"""
    return float(x).hex()


def _finite(owner, **values):
    out = []
    for key, v in values.items():
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s: %s must be a number, got %r" % (owner, key, v))
        if not math.isfinite(v):
            raise ValueError("%s: %s must be finite, got %r" % (owner, key, v))
        out.append(v)
    return out


def _positive(owner, **values):
    out = _finite(owner, **values)
    for (key, _), v in zip(values.items(), out):
        if v <= 0:
            raise ValueError("%s: %s must be positive, got %r" % (owner, key, v))
    return out


def _ordered(owner, lo, hi):
    if hi <= lo:
        raise ValueError("%s: hi must be larger than lo, got lo = %r, hi = %r" % (owner, lo, hi))


class Prior(object):
    """One column (``size == 1``) or one block of consecutive columns of a prior transform."""
    size = 1
    affine = False
    circular = False

    def __init__(self, name=None):
        self.name = name

    def names(self, first):
        base = self.name or "p%d" % first
        return [base] if self.size == 1 else ["%s_%d" % (base, k) for k in range(self.size)]

    def call(self, u):
        """the C++ expression of a one-column prior from the expression `u`"""
        raise NotImplementedError

    def statements(self, first):
        """the C++ statements that write p[first .. first + size)"""
        return ["p[%d] = %s;" % (first, self.call("u[%d]" % first))]

    def _call(self, fn, u, *consts):
        return "%s(%s)" % (fn, ", ".join((u,) + tuple(_hex(c) for c in consts)))


class Fixed(Prior):
    affine = True

    def __init__(self, v, name=None):
        Prior.__init__(self, name)
        self.v, = _finite("Fixed", v=v)

    def call(self, u):
        return _hex(self.v)


class Uniform(Prior):
    affine = True

    def __init__(self, lo, hi, circular=False, name=None):
        Prior.__init__(self, name)
        self.lo, self.hi = _finite("Uniform", lo=lo, hi=hi)
        _ordered("Uniform", self.lo, self.hi)
        self.w, = _finite("Uniform", width=self.hi - self.lo)
        self.circular = bool(circular)

    def call(self, u):
        return self._call("mlf_prior_uniform", u, self.lo, self.w)


class LogUniform(Prior):
    def __init__(self, lo, hi, name=None):
        Prior.__init__(self, name)
        self.lo, self.hi = _positive("LogUniform", lo=lo, hi=hi)
        _ordered("LogUniform", self.lo, self.hi)
        self.a = math.log(self.lo)
        self.w = math.log(self.hi) - math.log(self.lo)

    def call(self, u):
        return self._call("mlf_prior_loguniform", u, self.a, self.w)


class Normal(Prior):
    def __init__(self, mu, sigma, name=None):
        Prior.__init__(self, name)
        self.mu, = _finite("Normal", mu=mu)
        self.sigma, = _positive("Normal", sigma=sigma)

    def call(self, u):
        return self._call("mlf_prior_normal", u, self.mu, self.sigma)


class TruncatedNormal(Prior):
    def __init__(self, mu, sigma, lo, hi, name=None):
        Prior.__init__(self, name)
        self.mu, self.lo, self.hi = _finite("TruncatedNormal", mu=mu, lo=lo, hi=hi)
        self.sigma, = _positive("TruncatedNormal", sigma=sigma)
        _ordered("TruncatedNormal", self.lo, self.hi)
        self.a, self.b = (self.lo - self.mu) / self.sigma, (self.hi - self.mu) / self.sigma
        r2 = math.sqrt(2.0)
        self.Fa, self.Fb = 0.5 * math.erfc(-self.a / r2), 0.5 * math.erfc(-self.b / r2)
        self.Qa, self.Qb = 0.5 * math.erfc(self.a / r2), 0.5 * math.erfc(self.b / r2)
        if not (self.Fb > self.Fa or self.Qa > self.Qb):
            raise ValueError("TruncatedNormal: no probability between lo = %r and hi = %r in binary64" % (self.lo, self.hi))

    def call(self, u):
        return self._call("mlf_prior_truncnormal", u, self.mu, self.sigma, self.a, self.b, self.Fa, self.Fb, self.Qa, self.Qb)


class LogNormal(Prior):
    def __init__(self, mu, sigma, name=None):
        Prior.__init__(self, name)
        self.mu, = _finite("LogNormal", mu=mu)
        self.sigma, = _positive("LogNormal", sigma=sigma)

    def call(self, u):
        return self._call("mlf_prior_lognormal", u, self.mu, self.sigma)


class _OneScale(Prior):
    fn, key = None, "scale"

    def __init__(self, scale, name=None):
        Prior.__init__(self, name)
        self.scale, = _positive(type(self).__name__, **{self.key: scale})

    def call(self, u):
        return self._call(self.fn, u, self.scale)


class HalfNormal(_OneScale):
    fn, key = "mlf_prior_halfnormal", "sigma"


class Exponential(_OneScale):
    fn = "mlf_prior_exponential"


class Rayleigh(_OneScale):
    fn, key = "mlf_prior_rayleigh", "sigma"


class HalfCauchy(_OneScale):
    fn = "mlf_prior_halfcauchy"


class _ScaleShape(Prior):
    fn, keys = None, ("scale", "shape")

    def __init__(self, scale, shape, name=None):
        Prior.__init__(self, name)
        self.scale, self.shape = _positive(type(self).__name__, **{self.keys[0]: scale, self.keys[1]: shape})

    def call(self, u):
        return self._call(self.fn, u, self.scale, self.shape)


class Weibull(_ScaleShape):
    fn, keys = "mlf_prior_weibull", ("scale", "k")


class Pareto(_ScaleShape):
    fn, keys = "mlf_prior_pareto", ("xm", "alpha")


class _LocScale(Prior):
    fn, key = None, "scale"

    def __init__(self, loc, scale, name=None):
        Prior.__init__(self, name)
        self.loc, = _finite(type(self).__name__, loc=loc)
        self.scale, = _positive(type(self).__name__, **{self.key: scale})

    def call(self, u):
        return self._call(self.fn, u, self.loc, self.scale)


class Cauchy(_LocScale):
    fn = "mlf_prior_cauchy"


class Laplace(_LocScale):
    fn, key = "mlf_prior_laplace", "b"


class Logistic(_LocScale):
    fn, key = "mlf_prior_logistic", "s"


class Gumbel(_LocScale):
    fn, key = "mlf_prior_gumbel", "s"


class Triangular(Prior):
    def __init__(self, lo, mode, hi, name=None):
        Prior.__init__(self, name)
        self.lo, self.mode, self.hi = _finite("Triangular", lo=lo, mode=mode, hi=hi)
        _ordered("Triangular", self.lo, self.hi)
        if not self.lo <= self.mode <= self.hi:
            raise ValueError("Triangular: mode must lie in [lo, hi], got %r" % (self.mode,))
        w = self.hi - self.lo
        self.c = (self.mode - self.lo) / w
        self.c1, self.c2 = _finite("Triangular", c1=w * (self.mode - self.lo), c2=w * (self.hi - self.mode))

    def call(self, u):
        return self._call("mlf_prior_triangular", u, self.lo, self.hi, self.c, self.c1, self.c2)


class Sine(Prior):
    def call(self, u):
        return "mlf_prior_sine(%s)" % u


class Cosine(Prior):
    def call(self, u):
        return "mlf_prior_cosine(%s)" % u


class MultivariateNormal(Prior):
    def __init__(self, mean, cov, name=None):
        Prior.__init__(self, name)
        try:
            mean, cov = np.array(mean, dtype=float), np.array(cov, dtype=float)
        except (TypeError, ValueError):
            raise ValueError("MultivariateNormal: mean and cov must be arrays of numbers")
        if mean.ndim != 1 or not 1 <= len(mean) <= MAX_BLOCK:
            raise ValueError("MultivariateNormal: mean must be a vector of 1 to %d entries, got shape %s" % (MAX_BLOCK, mean.shape))
        if cov.shape != (len(mean), len(mean)):
            raise ValueError("MultivariateNormal: cov must be %d x %d, got shape %s" % (len(mean), len(mean), cov.shape))
        if not (np.isfinite(mean).all() and np.isfinite(cov).all()):
            raise ValueError("MultivariateNormal: mean and cov must be finite")
        if not np.array_equal(cov, cov.T):
            raise ValueError("MultivariateNormal: cov must be symmetric")
        try:
            L = np.linalg.cholesky(cov)
        except np.linalg.LinAlgError:
            raise ValueError("MultivariateNormal: cov is not positive definite")
        if not (np.isfinite(L).all() and (np.diag(L) > 0).all()):
            raise ValueError("MultivariateNormal: cov is not positive definite")
        self.mean, self.cov, self.L = mean, cov, np.tril(L)
        self.size = len(mean)

    def statements(self, first):
        n = self.size
        out = ["p[%d] = mlf_prior_z(u[%d]);" % (first + k, first + k) for k in range(n)]
        for i in range(n - 1, -1, -1):      # row i reads z_0 .. z_i only: descending rows may overwrite in place
            s = "%s * p[%d]" % (_hex(self.L[i, 0]), first)
            for j in range(1, i + 1):
                s = "(%s) + %s * p[%d]" % (s, _hex(self.L[i, j]), first + j)
            out.append("p[%d] = %s + (%s);" % (first + i, _hex(self.mean[i]), s))
        return out


class OrderedUniform(Prior):
    def __init__(self, lo, hi, n, name=None):
        Prior.__init__(self, name)
        self.lo, self.hi = _finite("OrderedUniform", lo=lo, hi=hi)
        _ordered("OrderedUniform", self.lo, self.hi)
        self.w, = _finite("OrderedUniform", width=self.hi - self.lo)
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError("OrderedUniform: n must be a positive integer, got %r" % (n,))
        self.size = int(n)

    def statements(self, first):
        n = self.size
        out = ["{", "  double t = mlf_prior_ordered_factor(u[%d], %s);" % (first + n - 1, _hex(n)),
               "  p[%d] = %s + t * %s;" % (first + n - 1, _hex(self.lo), _hex(self.w))]
        for k in range(n - 2, -1, -1):
            out.append("  t = t * mlf_prior_ordered_factor(u[%d], %s);" % (first + k, _hex(k + 1)))
            out.append("  p[%d] = %s + t * %s;" % (first + k, _hex(self.lo), _hex(self.w)))
        out.append("}")
        return out


def _in_range(owner, lo, hi, **values):
    out = _finite(owner, **values)
    for (key, _), v in zip(values.items(), out):
        if not lo <= v <= hi:
            raise ValueError("%s: %s must lie in [%g, %g] (the range over which the device quantile holds its error bound), "
                             "got %r" % (owner, key, lo, hi, v))
    return out


def _lbeta(a, b):
    return math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)


class _Special(Prior):
    """a family whose quantile is iterative (``csrc/mlf_priors_special_dev.hpp``): ``fn`` and ``consts``, the device function
    and the constants it takes after u"""
    special = True
    fn, consts = None, ()

    def call(self, u):
        return self._call(self.fn, u, *self.consts)


def _gamma_consts(scale, a):
    return (scale, a, 1.0 / a, math.log(a), math.lgamma(a + 1.0))


class Gamma(_Special):
    fn = "mlf_prior_gamma"

    def __init__(self, shape, scale=1.0, name=None):
        Prior.__init__(self, name)
        self.shape, = _in_range("Gamma", SHAPE_MIN, SHAPE_MAX, shape=shape)
        self.scale, = _positive("Gamma", scale=scale)
        self.consts = _gamma_consts(self.scale, self.shape)


class ChiSquared(_Special):
    fn = "mlf_prior_gamma"

    def __init__(self, k, name=None):
        Prior.__init__(self, name)
        self.k, = _in_range("ChiSquared", 2.0 * SHAPE_MIN, 2.0 * SHAPE_MAX, k=k)
        self.shape, self.scale = 0.5 * self.k, 2.0
        self.consts = _gamma_consts(self.scale, self.shape)


class InverseGamma(_Special):
    fn = "mlf_prior_invgamma"

    def __init__(self, shape, scale=1.0, name=None):
        Prior.__init__(self, name)
        self.shape, = _in_range("InverseGamma", SHAPE_MIN, SHAPE_MAX, shape=shape)
        self.scale, = _positive("InverseGamma", scale=scale)
        self.consts = _gamma_consts(self.scale, self.shape)


class Beta(_Special):
    fn = "mlf_prior_beta"

    def __init__(self, a, b, name=None):
        Prior.__init__(self, name)
        self.a, self.b = _in_range("Beta", SHAPE_MIN, SHAPE_MAX, a=a, b=b)
        self.consts = (self.a, self.b, _lbeta(self.a, self.b), math.log(self.a), math.log(self.b))


class StudentT(_Special):
    fn = "mlf_prior_studentt"

    def __init__(self, nu, loc=0.0, scale=1.0, name=None):
        Prior.__init__(self, name)
        self.nu, = _in_range("StudentT", NU_MIN, NU_MAX, nu=nu)
        self.loc, = _finite("StudentT", loc=loc)
        self.scale, = _positive("StudentT", scale=scale)
        ha = 0.5 * self.nu
        self.consts = (self.loc, self.scale, ha, _lbeta(ha, 0.5), math.log(ha), math.log(self.nu))


class Dirichlet(_Special):
    def __init__(self, alpha, name=None):
        Prior.__init__(self, name)
        try:
            alpha = np.array(alpha, dtype=float)
        except (TypeError, ValueError):
            raise ValueError("Dirichlet: alpha must be a vector of numbers")
        if alpha.ndim != 1 or not 1 <= len(alpha) <= MAX_BLOCK:
            raise ValueError("Dirichlet: alpha must be a vector of 1 to %d entries, got shape %s" % (MAX_BLOCK, alpha.shape))
        for k, v in enumerate(alpha):
            _in_range("Dirichlet", SHAPE_MIN, SHAPE_MAX, **{"alpha[%d]" % k: v})
        self.alpha = alpha
        self.size = len(alpha)

    def gammas(self):
        """the block's Gamma(alpha_k, 1) columns: the g row of the module docstring"""
        return [Gamma(a, 1.0) for a in self.alpha]

    def statements(self, first):
        n = self.size
        out = ["p[%d] = %s;" % (first + k, g.call("u[%d]" % (first + k))) for k, g in enumerate(self.gammas())]
        out += ["{", "  double s = p[%d];" % first]
        out += ["  s = s + p[%d];" % (first + k) for k in range(1, n)]
        out.append("  if (s == %s) {" % _hex(0.0))
        out += ["    p[%d] = %s;" % (first + k, _hex(1.0 / n)) for k in range(n)]
        out.append("  } else {")
        out += ["    p[%d] = p[%d] / s;" % (first + k, first + k) for k in range(n)]
        out += ["  }", "}"]
        return out


def header_text():
    """the text of ``csrc/mlf_priors_dev.hpp``"""
    with open(HEADER) as fh:
        return fh.read()


def special_header_text():
    """the text of ``csrc/mlf_priors_special_dev.hpp``"""
    with open(SPECIAL_HEADER) as fh:
        return fh.read()


class PriorTransform(object):
    """The prior transform of a list of priors (module docstring): ``ndim``, ``paramnames``, ``wrapped_dims`` (the circular
    columns, for the transform layer's ``wrapped_dims=``), ``is_affine`` (every prior ``Fixed`` or ``Uniform``: what the
    reference's ``is_affine_transform`` would find, and with it whether a driver needs a t-region), ``source`` (a
    self-contained HIP text defining ``mlf_user_transform``, a deterministic function of the priors' parameter bits),
    ``model(loglike_source, ...)`` and the vectorized callback ``transform``."""

    def __init__(self, priors):
        self.priors = list(priors)
        if not self.priors:
            raise ValueError("PriorTransform needs at least one prior")
        for p in self.priors:
            if not isinstance(p, Prior):
                raise ValueError("PriorTransform takes Prior objects, got %r" % (p,))
        self.ndim = sum(p.size for p in self.priors)
        if self.ndim > devicemodel.MAX_DIM:
            raise ValueError("the priors span %d columns, above MLF_MAX_DIM = %d" % (self.ndim, devicemodel.MAX_DIM))
        self.paramnames, self.wrapped_dims, body = [], [], []
        first = 0
        for p in self.priors:
            self.paramnames += p.names(first)
            if p.circular:
                self.wrapped_dims.append(first)
            body += p.statements(first)
            first += p.size
        self.is_affine = all(p.affine for p in self.priors)
        special = special_header_text() if any(getattr(p, "special", False) for p in self.priors) else ""
        self.source = (header_text() + special + "\n__device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, "
                       "long long naux) {\n" + "".join("  %s\n" % s for s in body) + "}\n")
        self._model = None

    def model(self, loglike_source, aux=None, **kw):
        """``DeviceModel(ndim, loglike_source, transform_source=self.source, aux=aux, **kw)``: name, nterms, nsums, nderived,
        derived_source and gate_derived pass through"""
        return DeviceModel(self.ndim, loglike_source, transform_source=self.source, aux=aux, **kw)

    def transform(self, u):
        """vectorized callback (n, ndim) -> (n, ndim), evaluated on the GPU (a lazily built model with a constant likelihood;
        no CPU fallback), for a likelihood that stays a host function"""
        if self._model is None:
            self._model = self.model(CONSTANT_LOGLIKE, name="PriorTransform%d" % self.ndim)
        return self._model.transform(u)


__all__ = ["Prior", "Fixed", "Uniform", "LogUniform", "Normal", "TruncatedNormal", "LogNormal", "HalfNormal", "Exponential",
           "Rayleigh", "Weibull", "Pareto", "Cauchy", "HalfCauchy", "Laplace", "Logistic", "Gumbel", "Triangular", "Sine",
           "Cosine", "MultivariateNormal", "OrderedUniform", "Gamma", "ChiSquared", "InverseGamma", "Beta", "StudentT",
           "Dirichlet", "PriorTransform"]
