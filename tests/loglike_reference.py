"""High-precision references, error scales and input makers for the batch likelihoods (shared by test_loglike_forms.py,
test_devicemodel_gpu.py).  A plain module, not a conftest.

The four formulas are restated from the docstrings of ultranest_amd/likelihoods.py:

    gauss       -0.5*sum(((theta-centers)/sigma)**2, axis=1) - 0.5*log(2*pi*sigma**2)*ndim
    eggbox      (2 + prod(cos(z/2), axis=1))**5
    eggbox2     prod(cos(theta), axis=1)**2
    rosenbrock  -2 * sum(100*(b - a**2)**2 + (1 - a)**2, axis=1) over consecutive pairs (a, b)

(and "funnel", the user model of ultranest_amd/usermodels.py: the Gaussian of theta[1:] about the data with sigma =
10**theta[0], `centers` being the data)

twice: vectorised in np.longdouble (64-bit mantissa where the platform has one) and row by row in mpmath at 50 digits.
Where only one of the two exists, that one is the reference; neither is a reason to skip.

Tolerance: |got - ref| <= 1e-12 * scale, `scale` being the same formula with every subtraction replaced by a sum of
magnitudes and every term taken positive -- the size of the numbers whose rounding the result inherits.  A plain relative
bound is unsound where the result cancels: the Gaussian at sigma = 0.01 passes through L = 0, and a Rosenbrock point in the
valley b = a**2 cancels inside t = b - a**2, where FMA contraction alone moves L by more than 1e-12 |L|.  Two correct binary64
evaluations (sequential order, pair layout with the xor tree) stay below 8e-15 * scale for d <= 257, so 1e-12 leaves more
than 100x for summation order and cos; test_loglike_forms.py asserts 1e-13 * scale for both on the CPU.
"""
import numpy as np

try:
    import mpmath
    HAVE_MPMATH = True
except ImportError:   # pragma: no cover
    mpmath = None
    HAVE_MPMATH = False

LD = np.longdouble
HAVE_LONGDOUBLE = bool(np.finfo(LD).eps < 1e-18)
assert HAVE_LONGDOUBLE or HAVE_MPMATH, "neither an extended-precision long double nor mpmath: no reference for the likelihoods"

KINDS = ("gauss", "eggbox", "eggbox2", "rosenbrock")
KIND_ID = {"gauss": 0, "eggbox": 1, "eggbox2": 2, "rosenbrock": 3}
RTOL = 1e-12
ATOL = {"gauss": 0.0, "eggbox": 0.0, "eggbox2": 1e-300, "rosenbrock": 0.0, "funnel": 0.0}

_CHUNK = 1 << 21   # elements per piece of the long double evaluation (32 MiB of long doubles)


# ------------------------------------------------------------------------------------------------ kernel forms
def rows_form(d):
    """launch_loglike takes k_loglike_rows for even d <= 128 (16-byte aligned batch)"""
    return d % 2 == 0 and d <= 128


def hw_of(d):
    """lanes per row of k_loglike_rows: the smallest power of two with 2 hw >= d, at least 2"""
    hw = 2
    while 2 * hw < d:
        hw *= 2
    return hw


def rpw_of(d):
    """rows per wave-wide load of k_loglike_rows"""
    return 64 // hw_of(d)


# ------------------------------------------------------------------------------------------------ references
def _ld_rows(kind, x, centers, sigma):
    x = x.astype(LD)
    d = x.shape[1]
    if kind == "gauss":
        s = LD(sigma)
        pi = 4 * np.arctan(LD(1))
        z = (x - np.asarray(centers, dtype=np.float64).astype(LD)) / s
        return -(z * z).sum(axis=1) / 2 - np.log(2 * pi * s * s) / 2 * d
    if kind == "funnel":
        s = np.power(LD(10), x[:, :1])
        pi = 4 * np.arctan(LD(1))
        z = (x[:, 1:] - np.asarray(centers, dtype=np.float64).astype(LD)) / s
        return -(z * z).sum(axis=1) / 2 - np.log(2 * pi * s[:, 0] * s[:, 0]) / 2 * (d - 1)
    if kind == "eggbox":
        return (2 + np.cos(x / 2).prod(axis=1)) ** 5
    if kind == "eggbox2":
        return np.cos(x).prod(axis=1) ** 2
    a, b = x[:, :-1], x[:, 1:]
    t, w = b - a * a, 1 - a
    return -2 * (100 * (t * t) + w * w).sum(axis=1)


def ref_longdouble(kind, x, centers=None, sigma=None):
    """(n,) long double values of the formula, evaluated in pieces of at most _CHUNK elements"""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    step = max(1, _CHUNK // d)
    out = np.empty(n, dtype=LD)
    for i in range(0, n, step):
        out[i:i + step] = _ld_rows(kind, x[i:i + step], centers, sigma)
    return out


def ref_mpmath(kind, x, centers=None, sigma=None):
    """list of mpf values (50 digits), one per row of x, each term written out"""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[1]
    out = []
    with mpmath.workdps(50):
        if kind == "gauss":
            c = [mpmath.mpf(float(v)) for v in np.broadcast_to(np.asarray(centers, dtype=np.float64), (d,))]
            s = mpmath.mpf(float(sigma))
            norm = mpmath.log(2 * mpmath.pi * s * s) / 2 * d
        elif kind == "funnel":
            c = [mpmath.mpf(float(v)) for v in centers]
        for row in x:
            r = [mpmath.mpf(float(v)) for v in row]
            if kind == "gauss":
                out.append(-mpmath.fsum(((r[k] - c[k]) / s) ** 2 for k in range(d)) / 2 - norm)
            elif kind == "funnel":
                s = mpmath.mpf(10) ** r[0]
                out.append(-mpmath.fsum(((r[k + 1] - c[k]) / s) ** 2 for k in range(d - 1)) / 2
                           - mpmath.log(2 * mpmath.pi * s * s) / 2 * (d - 1))
            elif kind == "eggbox":
                out.append((2 + mpmath.fprod(mpmath.cos(v / 2) for v in r)) ** 5)
            elif kind == "eggbox2":
                out.append(mpmath.fprod(mpmath.cos(v) for v in r) ** 2)
            else:
                out.append(-2 * mpmath.fsum(100 * (r[k + 1] - r[k] ** 2) ** 2 + (1 - r[k]) ** 2 for k in range(d - 1)))
    return out


def mp_minus(values, other):
    """|values[i] - other[i]| for a list of mpf and an array (long double or binary64), as binary64: the subtraction is done
    at 50 digits (a long double is split into two binary64 parts, which represent it exactly)"""
    other = np.asarray(other)
    hi = other.astype(np.float64)
    lo = (other - hi.astype(other.dtype)).astype(np.float64)
    with mpmath.workdps(50):
        return np.array([float(abs(v - mpmath.mpf(float(h)) - mpmath.mpf(float(l)))) for v, h, l in zip(values, hi, lo)])


def scale(kind, x, centers=None, sigma=None, ref=None):
    """(n,) binary64: the formula with every subtraction replaced by a sum of magnitudes and every term positive;
    eggbox, eggbox2: |ref|"""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[1]
    if kind == "gauss":
        z = (np.abs(x) + np.abs(np.asarray(centers, dtype=np.float64))) / sigma
        return 0.5 * (z * z).sum(axis=1) + abs(0.5 * np.log(2 * np.pi * sigma ** 2) * d)
    if kind == "funnel":
        sig = 10.0 ** x[:, :1]
        z = (np.abs(x[:, 1:]) + np.abs(np.asarray(centers, dtype=np.float64))) / sig
        return 0.5 * (z * z).sum(axis=1) + np.abs(0.5 * np.log(2 * np.pi * sig[:, 0] ** 2) * (d - 1))
    if kind == "rosenbrock":
        a, b = np.abs(x[:, :-1]), np.abs(x[:, 1:])
        return 2 * (100 * (b + a * a) ** 2 + (1 + a) ** 2).sum(axis=1)
    return np.abs(np.asarray(ref)).astype(np.float64)


def subsample(n, marks=(), every_64=None):
    """sorted row indices for the mpmath restatement: the first two rows, the last two, the rows on either side of every
    multiple of 64 (all of them when mpmath is the only reference, else the first four and the last one), and the rows
    m - 2 ... m of every mark m (batch lengths whose prefixes are evaluated; trip boundaries)"""
    if every_64 is None:
        every_64 = not HAVE_LONGDOUBLE
    rows = {0, 1, n - 2, n - 1}
    mult = list(range(64, n + 1, 64))
    if not every_64:
        mult = mult[:4] + mult[-1:]
    for m in mult:
        rows.update((m - 1, m))
    for m in marks:
        rows.update((m - 2, m - 1, m))
    return np.array(sorted(r for r in rows if 0 <= r < n), dtype=np.int64)


def _ratio(err, bound):
    """err / bound, where 0 / 0 is 0 (0 <= 0 holds: the empty Rosenbrock sum of d = 1) and a NaN is never close"""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio[np.isnan(ratio)] = np.inf
    return ratio


class Reference(object):
    """The reference of one batch.  rows: the rows it holds (all of them with a long double, else the mpmath subsample);
    ref, scale: aligned with rows; mp_rows, mp: the mpmath subsample (None without mpmath, or with with_mpmath=False where
    the long double reference exists)."""

    def __init__(self, kind, x, centers=None, sigma=None, marks=(), with_mpmath=True):
        x = np.asarray(x, dtype=np.float64)
        n = len(x)
        self.kind, self.n = kind, n
        self.mp_rows = self.mp = None
        if HAVE_MPMATH and (with_mpmath or not HAVE_LONGDOUBLE):
            self.mp_rows = subsample(n, marks)
            self.mp = ref_mpmath(kind, x[self.mp_rows], centers, sigma)
        if HAVE_LONGDOUBLE:
            self.rows = np.arange(n)
            self.ref = ref_longdouble(kind, x, centers, sigma)
        else:
            self.rows = self.mp_rows
            self.ref = np.array([float(v) for v in self.mp])   # binary64 rounding of the 50-digit value: 1.1e-16 |ref|
        self.scale = scale(kind, x[self.rows], centers, sigma, self.ref)

    def excess(self, got, rtol=RTOL, first=0):
        """max over the rows of got (the values of rows first ... first + len(got) - 1 of the batch) of
        |got - ref| / (rtol scale + atol), and the row where it is reached: <= 1 passes"""
        got = np.asarray(got, dtype=np.float64)
        sel = (self.rows >= first) & (self.rows < first + len(got))
        rows = self.rows[sel]
        err = np.abs(got[rows - first].astype(self.ref.dtype) - self.ref[sel]).astype(np.float64)
        ratio = _ratio(err, rtol * self.scale[sel] + ATOL[self.kind])
        worst = int(np.argmax(ratio))
        return float(ratio[worst]), int(rows[worst])

    def references_disagree_by(self):
        """max over the mpmath subsample of |long double - mpmath| / scale (both references present)"""
        sel = np.searchsorted(self.rows, self.mp_rows)
        diff = mp_minus(self.mp, self.ref[sel])
        return float(_ratio(diff, self.scale[sel] + ATOL[self.kind] / RTOL).max())


# ------------------------------------------------------------------------------------------------ binary64 restatements
def pair_tree(kind, x, centers=None, sigma=None):
    """k_loglike_rows in numpy (binary64, no FMA): lane l of a row holds coordinates 2 l, 2 l + 1; the per-lane terms are
    combined by the xor tree over hw lanes; lane 0 finishes.  Even d <= 128."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    assert rows_form(d)
    hw = hw_of(d)
    pad = np.zeros((n, 2 * hw + 2))
    pad[:, :d] = x
    x0, x1, nx = pad[:, 0:2 * hw:2], pad[:, 1:2 * hw:2], pad[:, 2:2 * hw + 2:2]
    k0 = 2 * np.arange(hw)
    active = k0 < d
    if kind == "gauss":
        c = np.zeros(2 * hw)
        c[:d] = np.broadcast_to(np.asarray(centers, dtype=np.float64), (d,))
        z0, z1 = (x0 - c[0::2]) / sigma, (x1 - c[1::2]) / sigma
        acc = np.where(active, z0 * z0 + z1 * z1, 0.0)
    elif kind == "eggbox":
        acc = np.where(active, np.cos(x0 / 2.0) * np.cos(x1 / 2.0), 1.0)
    elif kind == "eggbox2":
        acc = np.where(active, np.cos(x0) * np.cos(x1), 1.0)
    else:
        t0, w0 = x1 - x0 * x0, 1.0 - x0
        t1, w1 = nx - x1 * x1, 1.0 - x1
        acc = np.where(k0 + 1 < d, 100.0 * (t0 * t0) + w0 * w0, 0.0)
        acc = np.where(k0 + 2 < d, acc + (100.0 * (t1 * t1) + w1 * w1), acc)
    lanes = np.arange(hw)
    o = hw // 2
    while o > 0:
        other = acc[:, lanes ^ o]
        acc = acc * other if kind in ("eggbox", "eggbox2") else acc + other
        o >>= 1
    acc = acc[:, 0]
    if kind == "gauss":
        return -0.5 * acc + (-0.5 * np.log(2.0 * np.pi * sigma * sigma) * float(d))
    if kind == "eggbox":
        b1 = 2.0 + acc
        b2 = b1 * b1
        return b2 * b2 * b1
    if kind == "eggbox2":
        return acc * acc
    return -2.0 * acc


def plain_numpy(kind, x, centers=None, sigma=None):
    """the docstring formulas in binary64 numpy, as written: what a non-finite row has to give"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == "gauss":
            return -0.5 * (((x - centers) / sigma) ** 2).sum(axis=1) - 0.5 * np.log(2 * np.pi * sigma ** 2) * x.shape[1]
        if kind == "eggbox":
            return (2 + np.cos(x / 2).prod(axis=1)) ** 5
        if kind == "eggbox2":
            return np.cos(x).prod(axis=1) ** 2
        a, b = x[:, :-1], x[:, 1:]
        return -2 * (100 * (b - a ** 2) ** 2 + (1 - a) ** 2).sum(axis=1)


# ------------------------------------------------------------------------------------------------ inputs
def docs_gauss_centers(d, sigma):
    from ultranest_amd.likelihoods import GaussLikelihood
    return GaussLikelihood.docs_gauss(d, sigma).centers


def rosenbrock_valley(rs, n, d):
    """rows along the valley b = a**2: x[k + 1] = x[k]**2 (1 + 1e-9 N(0, 1)), x[0] uniform in [0.5, 1.5].  Repeated squaring
    leaves every finite range within a dozen steps, so where x[k]**2 is outside [0.1, 10] (the transform's domain ends at
    10) the chain starts again: x[k + 1] is a fresh uniform [0.5, 1.5] value.  Every lane of a wide row then holds valley
    pairs, not only the first few."""
    x = np.empty((n, d))
    x[:, 0] = rs.uniform(0.5, 1.5, size=n)
    for k in range(d - 1):
        sq = x[:, k] ** 2
        nxt = sq * (1 + 1e-9 * rs.normal(size=n))
        fresh = rs.uniform(0.5, 1.5, size=n)
        x[:, k + 1] = np.where((sq < 0.1) | (sq > 10), fresh, nxt)
    return x


# two input batches per kind: (name, maker(rs, n, d) -> (x, centers, sigma))
INPUTS = {
    "gauss": (("peak", lambda rs, n, d: (0.5 + 0.1 * rs.normal(size=(n, d)), docs_gauss_centers(d, 0.1), 0.1)),
              ("narrow", lambda rs, n, d: (rs.uniform(size=(n, d)), 0.5, 0.01))),
    "eggbox": (("domain", lambda rs, n, d: (rs.uniform(0, 10 * np.pi, size=(n, d)), None, None)),
               ("margin", lambda rs, n, d: (rs.uniform(-100, 100, size=(n, d)), None, None))),
    "eggbox2": (("domain", lambda rs, n, d: (rs.uniform(0, 10 * np.pi, size=(n, d)), None, None)),
                ("margin", lambda rs, n, d: (rs.uniform(-100, 100, size=(n, d)), None, None))),
    "rosenbrock": (("domain", lambda rs, n, d: (rs.uniform(-10, 10, size=(n, d)), None, None)),
                   ("valley", lambda rs, n, d: (rosenbrock_valley(rs, n, d), None, None))),
}


def make_inputs(kind, which, seed, n, d):
    """(x, centers, sigma) of input batch `which` (0 or 1) of `kind`"""
    name, maker = INPUTS[kind][which]
    return maker(np.random.RandomState(seed), n, d)
