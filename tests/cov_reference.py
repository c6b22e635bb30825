"""References for the covariance form of a user model (ultranest_amd/csrc/mlf_user_cov.hpp, "THE ARITHMETIC CONTRACT").

restate(K, r)      the contract in numpy, binary64: the packed augmented triangle, the right-looking factor (one rounded
                   multiplication and one rounded subtraction per update, ascending k), the two sequential sums, the likelihood and
                   the failure rule.  numpy's sqrt, division, product and difference are IEEE operations, as the device's are: the
                   device's factor is compared with this one bit for bit.  A column's update is one numpy expression over the
                   trailing block: every element still receives its subtractions in ascending k, which is all the contract fixes.
                   `defect` seeds one of the mistakes the tests must be able to see.
finish(tri, n)     the contract's sums and likelihood from a packed factor (the device's own, to separate the logarithm's error).
mp_loglike(K, r)   the likelihood from an mpmath Cholesky at 60 digits.
bound(...)         the derived error bound of restate's (or the device's) L against the exact value; derivation below.
gp_*               the model of usermodels.gp_sqexp in numpy and in mpmath, and its evidence over the prior box by Gauss-Legendre
                   quadrature.

THE BOUND.  u = 2^-53, gamma_k = k u / (1 - k u).  Computed: quad^ = sum z^_k^2, h^ = sum log(L^_kk), L^ = ((-quad^/2) - h^) - n c.
 (1) Factor and solve.  For every order of the rounded multiply-subtract updates the computed factor and the computed z satisfy
     (K + dK) x = r with |dK| <= gamma_(3n+1) |L^||L^|^T and || |L^||L^|^T ||_2 <= n / (1 - n gamma_(n+1)) ||K||_2 (Higham, Accuracy
     and Stability of Numerical Algorithms, Theorems 10.3, 10.4 and (10.7)): ||dK||_2 <= n gamma_(3n+1) / (1 - n gamma_(3n+1)) ||K||_2.
 (2) Entries.  Where the reference is the exact model and not the rounded matrix, every K_ij carries an absolute error of at most
     entry_eps * max|K| (given by the caller from the model's own operations; 0 when the reference reads the same binary64 matrix):
     ||dK_e||_2 <= n entry_eps ||K||_2.  A residual carries one rounding (y_i - mean): ||dr|| <= u ||r||, which changes quad by at
     most 2 u kappa quad (quad >= ||r||^2 / ||K||).  Together x = kappa_2(K) (n gamma_(3n+1) / (1 - n gamma_(3n+1)) + n entry_eps + 2 u).
 (3) quad = r^T K^-1 r changes by at most quad x / (1 - x) under (1) and (2); its sequential sum of n rounded squares adds
     gamma_(n+1) quad.
 (4) ln det: the eigenvalues of K^-1/2 dK K^-1/2 lie within x, so |d ln det| <= -n log(1 - x), and h is half of it.
 (5) each logarithm is within one ulp (2 u relative) of its value, and the sequential sum of n of them adds gamma_n sum |log L_kk|.
 (6) the three final operations: 3 u (quad / 2 + |h| + n c).
 bound = quad/2 (x / (1 - x) + gamma_(n+1)) - (n/2) log(1 - x) + (2 u + gamma_n) sum |log L_kk| + 3 u (quad/2 + |h| + n c); x < 1 required.
"""
import numpy as np

U = 2.0 ** -53
HALF_LOG_2PI = 0.91893853320467274178
DEFECTS = ("descending", "unrounded", "skip_aug", "bad_index", "no_sqrt")


def tri_size(n):
    return (n + 1) * (n + 2) // 2


def pack(full):
    """the packed lower triangle (row-major) of the last two axes"""
    rows, cols = np.tril_indices(full.shape[-1])
    return np.ascontiguousarray(full[..., rows, cols])


def unpack(tri, n):
    """packed augmented triangle -> (Lfac (n, n) with zeros above the diagonal, z (n,))"""
    rows, cols = np.tril_indices(n + 1)
    full = np.zeros(np.shape(tri)[:-1] + (n + 1, n + 1))
    full[..., rows, cols] = tri
    return full[..., :n, :n], full[..., n, :n]


def finish(tri, n, log=np.log, descending=False):
    """the contract's sums and likelihood from one packed factor"""
    Lfac, z = unpack(np.asarray(tri, dtype=float), n)
    order = range(n - 1, -1, -1) if descending else range(n)
    quad = h = 0.0
    for k in order:
        quad = quad + z[k] * z[k]
    logs = log(np.diagonal(Lfac).copy())
    for k in order:
        h = h + logs[k]
    return ((-0.5 * quad) - h) - float(n) * HALF_LOG_2PI


def restate(K, r, defect=None):
    """(tri packed (n+1)(n+2)/2, L) of one row.  K: (n, n), only its lower triangle is read; r: (n,)."""
    assert defect is None or defect in DEFECTS
    K, r = np.asarray(K, dtype=float), np.asarray(r, dtype=float)
    n = len(r)
    A = np.zeros((n + 1, n + 1))
    A[:n, :n] = np.tril(K)
    A[n, :n] = np.roll(r, -1) if defect == "bad_index" else r      # (the residual row read one packed word too far)
    with np.errstate(all="ignore"):
        if defect == "descending":
            return _left_looking_descending(A, n)
        for k in range(n):
            piv = A[k, k]
            if not piv > 0:
                return np.full(tri_size(n), np.nan), (np.nan if piv != piv else -np.inf)
            lkk = np.sqrt(piv)
            A[k, k] = lkk
            A[k + 1:, k] = A[k + 1:, k] / lkk
            c = A[k + 1:, k]
            rows = slice(k + 1, n if defect == "skip_aug" and k == n // 2 else n + 1)
            cr = A[rows, k]
            if defect == "unrounded":      # the product kept to 64 bits before the subtraction, which is then the only rounding
                m = cr[:, None].astype(np.longdouble) * c[None, :n - k - 1].astype(np.longdouble)
                A[rows, k + 1:n] = (A[rows, k + 1:n].astype(np.longdouble) - m).astype(float)
            else:
                m = cr[:, None] * c[None, :n - k - 1]
                A[rows, k + 1:n] = A[rows, k + 1:n] - m
        A = np.tril(A)
        tri = pack(A)
        if defect == "no_sqrt":
            return tri, finish(tri, n, log=lambda dg: np.log(dg * dg))
        return tri, finish(tri, n)


def _left_looking_descending(A, n):
    """the same factorisation with every element's subtractions in DESCENDING k, and descending sums"""
    for j in range(n):
        for k in range(j - 1, -1, -1):
            A[j:, j] = A[j:, j] - A[j:, k] * A[j, k]
        if not A[j, j] > 0:
            return np.full(tri_size(n), np.nan), (np.nan if A[j, j] != A[j, j] else -np.inf)
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] = A[j + 1:, j] / A[j, j]
    tri = pack(np.tril(A))
    return tri, finish(tri, n, descending=True)


def restate_rows(Ks, rs):
    out = [restate(K, r) for K, r in zip(Ks, rs)]
    return np.array([t for t, _ in out]), np.array([L for _, L in out])


def mp_loglike(K, r, dps=60):
    """L of exactly these binary64 entries (or mpmath entries) by an mpmath Cholesky at `dps` digits"""
    import mpmath as mp
    with mp.workdps(dps):
        n = len(r)
        A = mp.matrix(n, n)
        for i in range(n):
            for j in range(i + 1):
                A[i, j] = A[j, i] = mp.mpf(K[i][j])
        Lc = mp.cholesky(A)
        z = mp.lu_solve(Lc, mp.matrix([mp.mpf(v) for v in r]))      # (Lc is triangular: the elimination is a forward substitution)
        quad = mp.fsum(v * v for v in z)
        h = mp.fsum(mp.log(Lc[k, k]) for k in range(n))
        return mp.mpf(-0.5) * quad - h - n * mp.log(2 * mp.pi) / 2


def mp_mpf(v):
    import mpmath as mp
    return mp.mpf(float(v))


def gamma(k):
    return k * U / (1 - k * U)


def bound(K, r, entry_eps=0.0):
    """the bound of the module docstring for one row (float; inf where x >= 1)"""
    K = np.asarray(K, dtype=float)
    K = np.tril(K) + np.tril(K, -1).T
    n = len(r)
    kappa = np.linalg.cond(K, 2)
    g3 = n * gamma(3 * n + 1)
    x = kappa * (g3 / (1 - g3) + n * entry_eps + 2 * U)
    if not x < 1:
        return np.inf
    Lc = np.linalg.cholesky(K)
    z = np.linalg.solve(Lc, np.asarray(r, dtype=float))
    quad = float(z.dot(z))
    logs = np.log(np.diagonal(Lc))
    h = float(logs.sum())
    return (0.5 * quad * (x / (1 - x) + gamma(n + 1)) - 0.5 * n * np.log1p(-x) + (2 * U + gamma(n)) * float(np.abs(logs).sum())
            + 3 * U * (0.5 * quad + abs(h) + n * HALF_LOG_2PI))


# ---- usermodels.gp_sqexp -----------------------------------------------------------------------------------------------------------

# absolute error of a computed K_ij over max|K|, from the model's operations (eps = 2 u; exp within one ulp = eps): a * a carries
# 2.5 eps, t = dx^2 / (2 l^2) carries 4.5 eps so exp(-t) carries (1 + 4.5 t) eps, the product (4 + 4.5 t) eps of a^2 e^-t, and
# t e^-t <= 1 / e: at most 5.7 eps a^2; the diagonal adds s^2 with 3 eps of itself.  9 eps covers both.
GP_ENTRY_EPS = 9 * 2 * U


def gp_matrices(p, x, y):
    """(K (m, n, n), r (m, n)) of parameter rows p (m, 4) in numpy (its exp: for the bound and the quadrature, not for bits)"""
    p = np.atleast_2d(np.asarray(p, dtype=float))
    a, l, s = np.exp(p[:, 0]), np.exp(p[:, 1]), np.exp(p[:, 2])
    dx = x[:, None] - x[None, :]
    K = (a * a)[:, None, None] * np.exp(-(dx * dx)[None] / (2.0 * (l * l))[:, None, None])
    K = K + (s * s)[:, None, None] * np.eye(len(x))[None]
    return K, y[None, :] - p[:, 3:4]


def gp_mp_loglike(p, x, y, dps=60):
    """L of the exact model at the binary64 parameters p (4,) and data"""
    import mpmath as mp
    with mp.workdps(dps):
        a, l, s, mean = (mp.exp(mp.mpf(float(p[0]))), mp.exp(mp.mpf(float(p[1]))), mp.exp(mp.mpf(float(p[2]))), mp.mpf(float(p[3])))
        n = len(x)
        xs = [mp.mpf(float(v)) for v in x]
        K = [[a * a * mp.exp(-(xs[i] - xs[j]) ** 2 / (2 * l * l)) + (s * s if i == j else 0) for j in range(n)] for i in range(n)]
        return mp_loglike(K, [mp.mpf(float(v)) - mean for v in y], dps)


def _logsumexp(v, w):
    m = np.max(v)
    return m + np.log(np.sum(w * np.exp(v - m)))


def gp_lnz_quadrature(x, y, lo, width, nodes):
    """ln of the integral of the gp_sqexp likelihood over the unit cube under p = lo + width * u, by a tensor Gauss-Legendre rule
    with `nodes` points per axis.  One factorisation per (a, l, s) node: with c = K^-1 y and e = K^-1 1 the quadratic form is
    y.c - 2 m 1.c + m^2 1.e in the mean m."""
    t, w = np.polynomial.legendre.leggauss(nodes)
    t, w = 0.5 * (t + 1.0), 0.5 * w
    g = np.array(np.meshgrid(t, t, t, indexing="ij")).reshape(3, -1).T
    wg = np.array(np.meshgrid(w, w, w, indexing="ij")).reshape(3, -1).prod(axis=0)
    p = np.column_stack([lo[k] + width[k] * g[:, k] for k in range(3)] + [np.zeros(len(g))])
    K, _ = gp_matrices(p, x, y)
    Lc = np.linalg.cholesky(K)
    sol = np.linalg.solve(Lc, np.broadcast_to(np.column_stack([y, np.ones_like(y)]), (len(p),) + (len(y), 2)))
    yy, y1, oo = (sol[:, :, 0] ** 2).sum(1), (sol[:, :, 0] * sol[:, :, 1]).sum(1), (sol[:, :, 1] ** 2).sum(1)
    h = np.log(np.diagonal(Lc, axis1=1, axis2=2)).sum(1)
    m = lo[3] + width[3] * t
    like = -0.5 * (yy[:, None] - 2 * m[None, :] * y1[:, None] + m[None, :] ** 2 * oo[:, None]) - h[:, None] - len(y) * HALF_LOG_2PI
    return float(_logsumexp(like.ravel(), (wg[:, None] * w[None, :]).ravel()))
