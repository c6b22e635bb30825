"""What the tests of DeviceModel(..., nterms=K, nsums=M) share: a generated M-sum source of + - * / only with its numpy
restatement, the order contract in numpy, and usermodels.amplitude_sum restated in numpy and in long double with its error
bound.  No GPU and no library call here."""
import functools

import numpy as np

from ultranest_amd import usermodels


def contract(t):
    """the M sums of the order contract for the terms t (n, M, K): per accumulator and lane sequential additions from 0.0
    (lane l takes k = l, l + 64, ...), then the six exchange steps s = s + s[lane ^ m], m = 32 ... 1.  Returns (n, M)."""
    n, M, K = t.shape
    s = np.zeros((n, M, 64))
    for k0 in range(0, K, 64):          # one addition per lane and pass, k ascending
        w = min(64, K - k0)
        s[:, :, :w] = s[:, :, :w] + t[:, :, k0:k0 + w]
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lanes ^ m]
    assert ((s == s[:, :, :1]) | np.isnan(s)).all()
    return s[:, :, 0]


# ---- a generated source with M sums ----------------------------------------------------------------------------------------

def _c(j):
    return 0.375 * (j + 1)


def generated_source(M):
    """M sums whose terms and finish use only + - * /: with x = aux[k] and q = p[k % d], t_j = (x + c_j) * q - x * c_j,
    c_j = 0.375 * (j + 1); finish = s_0 - (s_1 * 0.5 + s_2 * 1.0 + ...) / (2 + s_last^2) (the numerator is s_0 for M = 1)"""
    terms = "\n".join("  t[%d] = (x + %r) * q - x * %r;" % (j, _c(j), _c(j)) for j in range(M))
    num = "s[0]" if M == 1 else " + ".join("s[%d] * %r" % (j, 0.5 * j) for j in range(1, M))
    return r"""
__device__ void mlf_user_loglike_terms(const double *p, int d, const double *aux, long long naux, long long k, double *t) {
  const double x = aux[k], q = p[(int)(k %% d)];
%s
}
__device__ double mlf_user_loglike_finish(const double *s, int nsums, const double *p, int d, const double *aux, long long naux) {
  const double num = %s;
  return s[0] - num / (2.0 + s[nsums - 1] * s[nsums - 1]);
}
""" % (terms, num)


def generated_data(K):
    return np.random.RandomState(K).normal(size=K)


def generated_terms(M, p, x):
    """t (n, M, K) of generated_source(M) for the rows p (n, d) and the data x (K), bit for bit"""
    K, d = len(x), p.shape[1]
    q = p[:, np.arange(K) % d]
    return np.stack([(x + _c(j)) * q - x * _c(j) for j in range(M)], axis=1)


def generated_finish(s):
    """finish of generated_source for the sums s (n, M): the numerator added left to right as the C expression is"""
    M = s.shape[1]
    if M == 1:
        num = s[:, 0]
    else:
        num = s[:, 1] * 0.5
        for j in range(2, M):
            num = num + s[:, j] * (0.5 * j)
    last = s[:, M - 1]
    return s[:, 0] - num / (2.0 + last * last)


def generated_L(M, p, x):
    return generated_finish(contract(generated_terms(M, p, x)))


# ---- usermodels.amplitude_sum ----------------------------------------------------------------------------------------------

AMPLITUDE_SHAPES = [(3, 200), (10, 1000)]


def amplitude_terms(p, X, y, w):
    """t (n, 3, K) of amplitude_sum, bit for bit: f from 0.0 in ascending j, a = w y, b = w f, terms a a, a b, b b"""
    f = np.zeros((p.shape[0], X.shape[0]))
    for j in range(X.shape[1]):
        f = f + p[:, j:j + 1] * X[:, j]
    a = np.broadcast_to(w * y, f.shape)
    b = w * f
    return np.stack([a * a, a * b, b * b], axis=1)


def amplitude_finish(s):
    return -0.5 * (s[:, 0] - s[:, 1] * s[:, 1] / s[:, 2]) - 0.5 * np.log(s[:, 2])


@functools.lru_cache(maxsize=None)
def amplitude_rows(d, K):
    """the rows p (130, d) and the data of the amplitude checks at this shape: parameters of order 1, so that
    s2 = sum w^2 f^2 is of the order of K |p|^2 (rows with |p|^2 < 0.5 are pushed out to keep s2 well above K / 10)"""
    p = np.random.RandomState(7 * d + K).normal(size=(130, d))
    r2 = (p * p).sum(axis=1)
    p[r2 < 0.5] *= 2.0 / np.sqrt(r2[r2 < 0.5])[:, None]
    return p, usermodels.linear_data(d, K, seed=d + K)


def amplitude_reference(p, X, y, w):
    """(reference L, tolerance, s2) per row.  Reference: everything in long double (64-bit significand: each operation is
    2^11 times more accurate than binary64, K = 1000 sequential additions included).  Tolerance: the project's 1e-12 class
    propagated through the finish L = -0.5 (s0 - s1^2 / s2) - 0.5 log s2,

        dL/ds0 = -0.5,   dL/ds1 = s1 / s2,   dL/ds2 = -0.5 s1^2 / s2^2 - 0.5 / s2,

    tol = 1e-12 * (sum_j |dL/ds_j| * sum_k |t_jk| + |L|)."""
    ld = np.longdouble
    pl, Xl, yl, wl = (np.asarray(v, dtype=ld) for v in (p, X, y, w))
    f = np.zeros((p.shape[0], X.shape[0]), dtype=ld)
    for j in range(X.shape[1]):
        f = f + pl[:, j:j + 1] * Xl[:, j]
    a, b = wl * yl, wl * f
    t = [np.broadcast_to(a * a, f.shape), a * b, b * b]
    s = []
    for tj in t:
        acc = np.zeros(p.shape[0], dtype=ld)
        for k in range(X.shape[0]):
            acc = acc + tj[:, k]
        s.append(acc)
    s0, s1, s2 = s
    L = ld(-0.5) * (s0 - s1 * s1 / s2) - ld(0.5) * np.log(s2)
    mags = [np.abs(tj).sum(axis=1) for tj in t]
    derivs = [0.5 + 0 * s0, np.abs(s1 / s2), np.abs(ld(-0.5) * s1 * s1 / (s2 * s2) - ld(0.5) / s2)]
    tol = 1e-12 * (sum(dj * mj for dj, mj in zip(derivs, mags)) + np.abs(L))
    return L.astype(float), tol.astype(float), s2.astype(float)
