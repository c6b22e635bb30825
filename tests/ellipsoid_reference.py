"""High-precision references, derived error bounds, binary64 stand-ins, input families and masks for the bootstrap
wrapping-ellipsoid kernels (shared by test_ellipsoid_reference.py and test_ellipsoid_forms_gpu.py).  A plain module, not a
conftest.

What is computed how.  All references take their binary64 inputs as exact.

    ref_mean(u, sel)                   sum of the selected rows / cnt                       np.longdouble, vectorised
    ref_cov(u, sel, mean)              sum (u_i - mean)(u_i - mean)^T / (cnt - 1)           np.longdouble; `mean` is GIVEN
    ref_quadform(y, P)                 y^T P y per row                                      np.longdouble
    ref_factor(u, sel, mean, cov, s)   max over the left-out rows of y^T (s cov)^-1 y       mpmath, 60 digits (below)
    ref_factor_exact(u, sel, s)        the same with mean and covariance in 60 digits       mpmath

ref_factor: A = s cov is factorised A = L L^T in mpmath at 60 digits and y^T A^-1 y = |L^-1 y|^2 comes from a forward
substitution in mpmath -- the quadratic form with the inverse, without forming it (mpmath's explicit inverse of a 64 x 64
matrix takes 3 s, the factor 0.3 s; test_ellipsoid_reference.py holds the two against each other on small cases).  All
left-out rows are ranked with the same substitution vectorised in long double, and every row within `window` relative of the
top is evaluated again in mpmath; the mpmath maximum is returned.  window = max(1e-12, 2 * 2^-11 * bound_factor_given_moments):
the long double ranking obeys the bound of the binary64 chain with the unit roundoff 2^-64 instead of 2^-53, so a row outside
the window cannot be the true maximum.

Without an extended long double (np.longdouble == binary64) every function falls back to mpmath throughout
(HAVE_LONGDOUBLE False; slow, same values, except that the y = u - ctr a caller hands to ref_quadform is then formed in
binary64 and carries two of the four roundings per term that bound_quadform allows); neither is a reason to skip.

Bounds: functions returning an array of the result's shape, each derived in its docstring from the summation order the kernel
documents (ultranest_amd/csrc/mlf_misc.hip, mlf_wide.hip, mlf_prep.hip).  u = 2^-53, gamma(k) = k u / (1 - k u).

Stand-ins: the kernels' orders restated in plain binary64 numpy (standin_*), with seeded defects (`defect=`) for the CPU
suite: the bounds must admit the stand-ins and reject the defects.
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
assert HAVE_MPMATH, "mpmath is needed for the reference of the bootstrap factor"

MP_DPS = 60
U = 2.0 ** -53
U_LD_OVER_U = 2.0 ** -11   # unit roundoff of the x87 long double over binary64's


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u), u = 2^-53"""
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------ kernel forms
def mean_form(d):
    """launch_boot_moments: k_boot_mean<1> / <2> up to 128 dimensions ("h16"), k_boot_mean_wide above ("wide")"""
    return "h16" if d <= 128 else "wide"


def cov_form(d):
    """launch_boot_moments: k_boot_cov16<NCH> up to 64 dimensions, k_boot_cov<2> up to 128, k_boot_cov_wide above"""
    return "cov16" if d <= 64 else ("cov8" if d <= 128 else "wide")


_DPS = (2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32, 36, 40, 44, 48, 50, 52, 56, 60, 64, 80, 96, 112, 128)


def pick_dp(d):
    """padded width of the quadratic-form kernels (MLF_FOR_EACH_DP of mlf_common.hpp; multiples of 16 above 128)"""
    for dp in _DPS:
        if d <= dp:
            return dp
    return (d + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ mpmath helpers
def _mp():
    mpmath.mp.dps = MP_DPS
    return mpmath


def _mpf_rows(a):
    mp = _mp()
    return [[mp.mpf(float(x)) for x in row] for row in np.atleast_2d(np.asarray(a, dtype=np.float64))]


def _ld_of_mpf(x):
    hi = float(x)
    lo = float(x - _mp().mpf(hi))
    return LD(hi) + LD(lo)


def _mpf_of_ld(v):
    mp = _mp()
    hi = float(v)
    lo = float(v - LD(hi))
    return mp.mpf(hi) + mp.mpf(lo)


def mp_mean(u, sel):
    """list of d mpf: mean of the selected rows"""
    mp = _mp()
    rows = _mpf_rows(np.asarray(u, dtype=np.float64)[np.asarray(sel, dtype=bool)])
    d = len(rows[0])
    return [mp.fsum(r[k] for r in rows) / len(rows) for k in range(d)]


def mp_cov(u, sel, mean):
    """d x d list of mpf: sum (u_i - mean)(u_i - mean)^T / (cnt - 1); `mean`: floats or mpf"""
    mp = _mp()
    rows = _mpf_rows(np.asarray(u, dtype=np.float64)[np.asarray(sel, dtype=bool)])
    d = len(rows[0])
    m = [x if isinstance(x, mp.mpf) else mp.mpf(float(x)) for x in mean]
    xs = [[r[k] - m[k] for k in range(d)] for r in rows]
    out = [[None] * d for _ in range(d)]
    for k in range(d):
        for l in range(k, d):
            out[k][l] = out[l][k] = mp.fsum(x[k] * x[l] for x in xs) / (len(rows) - 1)
    return out


def mp_quadform(y_rows, P):
    """list of mpf: y^T P y per row; y_rows: rows of mpf, P: floats"""
    mp = _mp()
    Pm = _mpf_rows(P)
    d = len(Pm)
    return [mp.fsum(y[j] * Pm[j][k] * y[k] for j in range(d) for k in range(d)) for y in y_rows]


def _mp_cholesky(A):
    """lower factor (list of rows of mpf) of the symmetric positive definite A (rows of mpf)"""
    mp = _mp()
    d = len(A)
    L = [[mp.mpf(0)] * d for _ in range(d)]
    for j in range(d):
        s = A[j][j] - mp.fsum(L[j][k] * L[j][k] for k in range(j))
        if not s > 0:
            raise ValueError("matrix not positive definite at column %d" % j)
        L[j][j] = mp.sqrt(s)
        for i in range(j + 1, d):
            L[i][j] = (A[i][j] - mp.fsum(L[i][k] * L[j][k] for k in range(j))) / L[j][j]
    return L


def _mp_solve_sq(L, y):
    """|L^-1 y|^2 in mpmath"""
    mp = _mp()
    d = len(L)
    z = []
    for i in range(d):
        z.append((y[i] - mp.fsum(L[i][k] * z[k] for k in range(i))) / L[i][i])
    return mp.fsum(v * v for v in z)


# ------------------------------------------------------------------------------------------------ references
def ref_mean(u, sel):
    """(d,) long double"""
    u = np.asarray(u, dtype=np.float64)
    sel = np.asarray(sel, dtype=bool)
    if not HAVE_LONGDOUBLE:
        return np.array([float(x) for x in mp_mean(u, sel)], dtype=LD)
    s = u[sel].astype(LD)
    return s.sum(axis=0) / LD(len(s))


def ref_cov(u, sel, mean):
    """(d, d) long double; `mean` (binary64 or long double) is taken as given"""
    u = np.asarray(u, dtype=np.float64)
    sel = np.asarray(sel, dtype=bool)
    if not HAVE_LONGDOUBLE:
        return np.array([[float(x) for x in row] for row in mp_cov(u, sel, [float(v) for v in mean])], dtype=LD)
    x = u[sel].astype(LD) - np.asarray(mean).astype(LD)
    return (x.T @ x) / LD(len(x) - 1)


def ref_quadform(y_rows, P):
    """(n,) long double: y^T P y per row; y_rows in long double (the caller forms u - ctr there), P binary64"""
    y = np.atleast_2d(np.asarray(y_rows, dtype=LD))
    if not HAVE_LONGDOUBLE:
        return np.array([float(q) for q in mp_quadform(_mpf_rows(y), P)], dtype=LD)
    Pl = np.asarray(P, dtype=np.float64).astype(LD)
    return ((y @ Pl) * y).sum(axis=1)


def _ld_solve_sq(L, Y):
    """|L^-1 y|^2 per row of Y, forward substitution in long double (column by column)"""
    acc = Y.copy()
    d = L.shape[0]
    ss = np.zeros(len(Y), dtype=LD)
    for k in range(d):
        yk = acc[:, k] / L[k, k]
        ss += yk * yk
        if k + 1 < d:
            acc[:, k + 1:] -= yk[:, None] * L[k + 1:, k][None, :]
    return ss


def _factor_from_mp(u, sel, m_mp, A_mp, window):
    mp = _mp()
    u = np.asarray(u, dtype=np.float64)
    sel = np.asarray(sel, dtype=bool)
    d = u.shape[1]
    L = _mp_cholesky(A_mp)
    out = u[~sel]
    assert len(out), "no left-out row"
    if HAVE_LONGDOUBLE:
        L_ld = np.array([[_ld_of_mpf(L[i][j]) for j in range(d)] for i in range(d)], dtype=LD)
        m_ld = np.array([_ld_of_mpf(x) for x in m_mp], dtype=LD)
        q = _ld_solve_sq(L_ld, out.astype(LD) - m_ld)
        cand = np.nonzero(q >= q.max() * LD(1.0 - window))[0]
    else:
        cand = np.arange(len(out))
    best = None
    for i in cand:
        y = [mp.mpf(float(out[i, k])) - m_mp[k] for k in range(d)]
        v = _mp_solve_sq(L, y)
        best = v if best is None or v > best else best
    return best


def ref_factor(u, sel, mean, cov, scale):
    """mpf: max over the left-out rows of (u_i - mean)^T (scale cov)^-1 (u_i - mean), mean and cov (binary64) given"""
    mp = _mp()
    cov = np.atleast_2d(np.asarray(cov, dtype=np.float64))
    d = cov.shape[0]
    A_mp = [[mp.mpf(float(cov[i, j])) * mp.mpf(float(scale)) for j in range(d)] for i in range(d)]
    m_mp = [mp.mpf(float(x)) for x in np.asarray(mean, dtype=np.float64).reshape(-1)]
    window = max(1e-12, 2.0 * U_LD_OVER_U * float(bound_factor_given_moments(cov * float(scale), d)))
    return _factor_from_mp(u, sel, m_mp, A_mp, window)


def ref_factor_exact(u, sel, scale):
    """mpf: the same with mean and covariance of the selected rows computed in mpmath themselves"""
    mp = _mp()
    m_mp = mp_mean(u, sel)
    C = mp_cov(u, sel, m_mp)
    d = len(m_mp)
    A_mp = [[C[i][j] * mp.mpf(float(scale)) for j in range(d)] for i in range(d)]
    A64 = np.array([[float(x) for x in row] for row in A_mp])
    window = max(1e-12, 2.0 * U_LD_OVER_U * float(bound_factor_given_moments(A64, d)))
    return _factor_from_mp(u, sel, m_mp, A_mp, window)


# ------------------------------------------------------------------------------------------------ bounds
def mean_chain(cnt, form):
    """h16: 16 waves, wave g adds the list entries j = g (mod 16) in ascending order (at most ceil(cnt/16) of them, the
    first one to 0.0: ceil(cnt/16) - 1 roundings); thread k adds the 16 partial sums in order (15 roundings, the first
    addition is to 0.0) and divides once: every term passes through at most ceil(cnt/16) + 15 roundings <= L = ceil(cnt/16) + 16.
    wide: one thread adds all cnt entries in list order and divides: cnt roundings <= L = cnt + 1."""
    if form == "h16":
        return -(-cnt // 16) + 16
    assert form == "wide", form
    return cnt + 1


def bound_mean(u, sel, form):
    """(d,) bound on |mean_device - mean|.  A recursive sum of terms t_i in which every term passes through at most L
    roundings (additions and the final division) equals sum t_i (1 + theta_i), |theta_i| <= gamma_L (Higham, Accuracy and
    Stability, Lemma 3.1 and section 4.2), so the error is at most gamma_L sum |u_ik| / cnt.  L: mean_chain."""
    u = np.asarray(u, dtype=np.float64)
    sel = np.asarray(sel, dtype=bool)
    cnt = int(sel.sum())
    return (gamma(mean_chain(cnt, form)) * np.abs(u[sel]).astype(LD).sum(axis=0) / cnt).astype(np.float64)


def cov_chain(cnt, form):
    """cov16 (cov_block): list entry e goes to wave g = (e / 4) mod 8, lane group grp = e mod 4, i.e. a 16-lane group takes
    every 32nd entry, T = ceil(cnt / 32) of them at most, each one fused multiply-add (one rounding; steps past the list add
    exact zeros); then two shuffle additions (the four groups), the eight waves' sums added in order to 0.0 (7 roundings,
    counted as 8) and one division.  With the two roundings of x_k = fl(u_ik - m_k) and x_l: L = T + 2 + 8 + 3.
    cov8 (k_boot_cov<2>): wave g takes the entries j = g (mod 8), T = ceil(cnt / 8) fused multiply-adds, the eight partial
    sums in order, one division, two roundings in x: L = T + 8 + 3.
    wide (k_boot_cov_wide): one thread, cnt fused multiply-adds in list order, one division, two roundings in x: L = cnt + 3."""
    if form == "cov16":
        return -(-cnt // 32) + 2 + 8 + 3
    if form == "cov8":
        return -(-cnt // 8) + 8 + 3
    assert form == "wide", form
    return cnt + 3


def bound_cov(u, sel, mean, form):
    """(d, d) bound on |cov_device - ref_cov(u, sel, mean)| for the SAME mean.  The device forms x_ik = fl(u_ik - m_k)
    = (u_ik - m_k)(1 + delta), |delta| <= u, once per element, and adds the products x_ik x_il through a chain in which
    every product meets at most L - 2 roundings (cov_chain); with the two deltas of its factors the computed value is
    sum_i (u_ik - m_k)(u_il - m_l)(1 + theta_i) / (cnt - 1), |theta_i| <= gamma_L, hence the error is at most
    gamma_L sum_i |x_ik x_il| / (cnt - 1).  (The sum is evaluated with x rounded once; that differs from the exact
    differences by a factor 1 + 2u, far inside the slack between L and the roundings actually met.)"""
    u = np.asarray(u, dtype=np.float64)
    sel = np.asarray(sel, dtype=bool)
    cnt = int(sel.sum())
    x = np.abs(u[sel] - np.asarray(mean, dtype=np.float64)).astype(LD)
    return (gamma(cov_chain(cnt, form)) * (x.T @ x) / max(cnt - 1, 1)).astype(np.float64)


def bound_quadform(y, P, dp=None):
    """(n,) bound on |q_device - y^T P y|, y = u_i - ctr exact.  k_boot_quadmax / k_prep / k_quadmax_wide / k_prep_wide:
    one accumulator, j outer, k inner, term = fl(fl(dl_j P_jk) dl_k) with dl = fl(u - ctr): four roundings per term (two
    differences, two products), and the d * dp terms (dp: padded width, the padding adds exact zeros) are added one by one:
    at most d * dp - 1 further roundings.  Every term therefore carries (1 + theta), |theta| <= gamma_{d dp + 4}:
    error <= gamma_{d dp + 4} sum_jk |y_j P_jk y_k|."""
    y = np.abs(np.atleast_2d(np.asarray(y, dtype=LD)))
    d = y.shape[1]
    dp = pick_dp(d) if dp is None else dp
    Pa = np.abs(np.asarray(P, dtype=np.float64)).astype(LD)
    return (gamma(d * dp + 4) * ((y @ Pa) * y).sum(axis=1)).astype(np.float64)


def cond2(A):
    """kappa_2 of a symmetric positive definite matrix (binary64 eigenvalues; NaN / not positive definite -> inf)"""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    if not np.isfinite(A).all():
        return np.inf
    w = np.linalg.eigvalsh(A)
    return float(w[-1] / w[0]) if w[0] > 0 else np.inf


def bound_factor_given_moments(A, d):
    """Relative bound on the error of f = y^T A^-1 y = |L^-1 y|^2 as k_boot_chol + k_boot_solvemax compute it from the exact
    product A = scale cov and the exact y = u_i - mean; first order in u, valid for every row, hence for the maximum.

    The roundings of the device, in order:
      1. A^ = fl(cov * scale):                         |A^ - A| <= u |A| <= u |L||L^T|
      2. right-looking Cholesky of A^ (k_boot_chol; L_rj = a_rj * fl(1 / sqrt(a_jj)), one rounding more per element than the
         division of Higham's Algorithm 10.2, updates by fma):   L^ L^^T = A^ + dA,  |dA| <= gamma_{d+2} |L^||L^^T|
         (Higham, Thm 10.3, with d + 2 for d + 1); with 1.:      L^ L^^T = A + E,    |E| <= gamma_{d+3} |L||L^T|
         and || |L||L^T| ||_2 <= || |L| ||_2^2 <= d ||L||_2^2 = d ||A||_2 (Higham (10.7)), so ||E||_2 <= d gamma_{d+3} ||A||_2.
         df = -w^T E w with w = A^-1 y and |w|^2 = y^T A^-2 y <= f / lambda_min:   |df| / f <= d gamma_{d+3} kappa_2(A)
      3. y^ = fl(u_i - mean) = y + dy, |dy| <= u |y|:  df = 2 w^T dy,  |df| <= 2 u |w| |y| <= 2 u f sqrt(kappa_2)
         (|w| <= sqrt(f / lambda_min), |y| <= sqrt(f lambda_max))
      4. forward substitution, column by column, y_k = acc_k * fl(1 / L_kk) (again one rounding more than a division),
         updates by fma: (L^ + dL) z^ = y^, |dL| <= gamma_{d+1} |L^| (Higham, Thm 8.5 with d + 1 for d), so
         z^ = z - L^-1 dL z and d|z|^2 = -2 z^T L^-1 dL z:   |df| / f <= 2 ||L^-1||_2 || |L| ||_2 gamma_{d+1}
         <= 2 sqrt(d) gamma_{d+1} sqrt(kappa_2)
      5. ss = fma(y_k, y_k, ss), d roundings:         |df| / f <= gamma_d

    Sum:  d gamma_{d+3} kappa_2 + (2 sqrt(d) gamma_{d+1} + 2u) sqrt(kappa_2) + gamma_d.
    (Bounding sqrt(kappa_2) by kappa_2 and every gamma by (d + 3) u gives the cruder (d + 3)(d + 2 sqrt(d) + 3) u kappa_2.)
    The second-order terms are of the size of the square of the result; the tests assert the result <= 1e-6."""
    k2 = cond2(A)
    return float(d * gamma(d + 3) * k2 + (2.0 * np.sqrt(d) * gamma(d + 1) + 2.0 * U) * np.sqrt(k2) + gamma(d))


def _ld_cholesky(A):
    A = np.array(A, dtype=LD)
    d = A.shape[0]
    L = np.zeros((d, d), dtype=LD)
    for j in range(d):
        L[j, j] = np.sqrt(A[j, j])
        L[j + 1:, j] = A[j + 1:, j] / L[j, j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L


def _ld_lower_inverse(L):
    d = L.shape[0]
    X = np.zeros((d, d), dtype=LD)
    for c in range(d):
        X[c, c] = 1 / L[c, c]
        for r in range(c + 1, d):
            X[r, c] = -(L[r, c:r] @ X[c:r, c]) / L[r, r]
    return X


def bound_factor_composite(u, sel, scale, f=None):
    """Relative bound on |f_device - ref_factor_exact| (first order): the device's mean m^ = m + dm, |dm| <= b_m
    (bound_mean); its covariance C^ = C(m^) + dC, |dC| <= E (bound_cov; C(m^) - C(m) = cnt / (cnt - 1) dm dm^T is second
    order); then the chain of bound_factor_given_moments.  With A = scale C = L L^T, z = L^-1 y, f = |z|^2:
      mean:        df = -2 z^T L^-1 dm,          |df| <= 2 sqrt(f) || |L^-1| b_m ||_2
      covariance:  df = -z^T L^-1 (scale dC) L^-T z,   |df| <= f || |L^-1| (scale E) |L^-T| ||_F
    (|df| of the maximum is at most the largest |df| of a row, and sqrt(f_row) <= sqrt(f)).
    Returned: 2 || |L^-1| b_m ||_2 / sqrt(f) + || |L^-1| scale E |L^-T| ||_F + bound_factor_given_moments(A, d), the first
    two evaluated in long double.  `f`: the exact factor if the caller has it already."""
    u = np.asarray(u, dtype=np.float64)
    sel = np.asarray(sel, dtype=bool)
    d = u.shape[1]
    m = ref_mean(u, sel)
    C = ref_cov(u, sel, m)
    A = C * LD(scale)
    if f is None:
        f = ref_factor_exact(u, sel, scale)
    f = LD(float(f))
    Li = np.abs(_ld_lower_inverse(_ld_cholesky(A)))
    b_m = bound_mean(u, sel, mean_form(d)).astype(LD)
    E = bound_cov(u, sel, m.astype(np.float64), cov_form(d)).astype(LD) * LD(scale)
    t_mean = 2 * np.sqrt(((Li @ b_m) ** 2).sum()) / np.sqrt(f)
    t_cov = np.sqrt(((Li @ E @ Li.T) ** 2).sum())
    return float(t_mean + t_cov) + bound_factor_given_moments(A.astype(np.float64), d)


# ------------------------------------------------------------------------------------------------ error / bound
def ratio(err, bound):
    """largest |err| / bound (0 where both vanish, inf where only the bound does or the error is not finite)"""
    err = np.abs(np.asarray(err, dtype=LD)).reshape(-1)
    bound = np.asarray(bound, dtype=LD).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bound)
    r = np.where(np.isfinite(r), r, LD(np.inf))
    return float(r.max())


def moments_ratios(u, sel, mean, cov):
    """(error / bound of the mean, error / bound of the covariance against ref_cov with THIS mean), as Stage A asserts"""
    d = np.asarray(u).shape[1]
    r_mean = ratio(np.asarray(mean).astype(LD) - ref_mean(u, sel), bound_mean(u, sel, mean_form(d)))
    r_cov = ratio(np.asarray(cov).astype(LD) - ref_cov(u, sel, mean), bound_cov(u, sel, mean, cov_form(d)))
    return r_mean, r_cov


def factor_ratio(f, u, sel, mean, cov, scale):
    """(|f - ref_factor| / (bound_factor_given_moments * ref), the bound), as Stage B asserts"""
    d = np.asarray(u).shape[1]
    b = bound_factor_given_moments(np.asarray(cov, dtype=np.float64) * float(scale), d)
    ref = ref_factor(u, sel, mean, cov, scale)
    if not np.isfinite(f):
        return np.inf, b
    return float(abs(_mp().mpf(float(f)) - ref) / ref) / b, b


# ------------------------------------------------------------------------------------------------ inputs
def family(kind, seed, n, d):
    """(W) uniform in the cube times per-column scales in 0.2 ... 1;  (C) 0.3 + 1e-6 (normal @ A^T), A = orthogonal times
    logspace(0, -1.5, d);  (I) 0.3 + 0.1 (normal @ A^T) with logspace(0, -3, d): kappa_2 of the covariance about 1e6"""
    rs = np.random.RandomState(seed)
    if kind == "W":
        return rs.uniform(size=(n, d)) * rs.uniform(0.2, 1.0, size=d)
    Q, _ = np.linalg.qr(rs.normal(size=(d, d)))
    expo, spread = {"C": (-1.5, 1e-6), "I": (-3.0, 0.1)}[kind]
    A = Q * np.logspace(0, expo, d)[None, :]
    return 0.3 + spread * (rs.normal(size=(n, d)) @ A.T)


def symmetric_matrix(rs, d, kappa):
    """symmetric positive definite, kappa_2 = kappa, eigenvectors at random: no structure to see in its entries"""
    Q, _ = np.linalg.qr(rs.normal(size=(d, d)))
    P = (Q * np.logspace(0, -np.log10(kappa), d)[None, :]) @ Q.T
    return (P + P.T) / 2


def mask_with(n, cnt):
    """(n,) bool with exactly cnt ones: the n - cnt left-out rows are spread evenly over 1 ... n - 2, so rows 0 and n - 1
    are always selected (for cnt >= 2) and the selected ones sit at scattered positions"""
    nout = n - cnt
    sel = np.ones(n, dtype=bool)
    if nout:
        assert cnt >= 2 and nout <= n - 2, (n, cnt)
        sel[1 + (np.arange(nout) * (n - 2)) // nout] = False
    assert int(sel.sum()) == cnt
    return sel


# ------------------------------------------------------------------------------------------------ stand-ins (binary64)
def _grouped_sum(terms, groups):
    """terms[e] added within group e mod `groups` in ascending order; (groups, ...) partial sums"""
    cnt = len(terms)
    steps = -(-cnt // groups)
    pad = np.zeros((steps * groups,) + terms.shape[1:], dtype=terms.dtype)
    pad[:cnt] = terms
    pad = pad.reshape((steps, groups) + terms.shape[1:])
    acc = np.zeros((groups,) + terms.shape[1:], dtype=terms.dtype)
    for t in range(steps):
        acc = acc + pad[t]          # the padding adds exact zeros
    return acc


def standin_mean(u, sel, form=None, defect=None):
    """k_boot_mean<H> (16 interleaved partial sums, added in order, one division) / k_boot_mean_wide (one chain)"""
    u = np.asarray(u, dtype=np.float64)
    rows = u[np.asarray(sel, dtype=bool)]
    cnt = len(rows)
    form = mean_form(u.shape[1]) if form is None else form
    if defect == "drop_last":
        rows = rows[:-1]
    if defect == "mean_f32":
        rows = rows.astype(np.float32)
    part = _grouped_sum(rows, 16 if form == "h16" else 1)
    tot = np.zeros(u.shape[1], dtype=rows.dtype)
    for p in part:
        tot = tot + p
    return (tot / rows.dtype.type(cnt)).astype(np.float64)


def standin_cov(u, sel, mean, form=None, defect=None):
    """k_boot_cov16 (32 chains, the four groups of a wave by two shuffle additions, the eight waves in order),
    k_boot_cov<2> (8 chains, in order), k_boot_cov_wide (one chain); products rounded, then added (no fma in numpy: one more
    rounding per product than the device, still within cov_chain)"""
    u = np.asarray(u, dtype=np.float64)
    rows = u[np.asarray(sel, dtype=bool)]
    cnt, d = rows.shape
    form = cov_form(d) if form is None else form
    mean = np.asarray(mean, dtype=np.float64)
    if defect == "drop_last":
        rows = rows[:-1]
    if defect == "one_pass":
        prod = rows[:, :, None] * rows[:, None, :]
    else:
        x = rows - mean
        prod = x[:, :, None] * x[:, None, :]
    if form == "cov16":
        acc = _grouped_sum(prod, 32).reshape(8, 4, d, d)          # entry e: wave (e / 4) mod 8, group e mod 4
        waves = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])  # xor 16, then xor 32, as lane group 0 sees them
    elif form == "cov8":
        waves = _grouped_sum(prod, 8)
    else:
        waves = _grouped_sum(prod, 1)
    tot = np.zeros((d, d))
    for w in waves:
        tot = tot + w
    if defect == "one_pass":
        tot = tot - cnt * np.outer(mean, mean)
    cov = tot / float(cnt if defect == "divisor_cnt" else cnt - 1)
    if defect == "mirror_missing":
        assert d > 16
        cov[16:min(32, d), 0:16] = 0.0       # the lower image of block (0, 1) stays what the buffer held
    return cov


def standin_chol(A, defect=None):
    """right-looking Cholesky of k_boot_chol: per column the pivot, sp = sqrt, ip = 1 / sp, L_rj = a_rj * ip, then the
    trailing update a_rc -= L_rj L_cj.  Returns (L, 1 / diag, bad)."""
    a = np.array(A, dtype=np.float64)
    d = a.shape[0]
    L = np.zeros((d, d))
    inv = np.ones(d)
    bad = False
    for j in range(d):
        p = a[j, j]
        if not (p > 0.0) or not (p < 1e300):
            bad = True
        sp = np.sqrt(p if p > 0.0 else 1.0)
        ip = 1.0 / sp
        L[j, j] = sp
        inv[j] = ip
        L[j + 1:, j] = a[j + 1:, j] * ip
        hi = d - 1 if defect == "chol_skip_last" else d
        for c in range(j + 1, hi):
            a[j + 1:, c] = a[j + 1:, c] - L[j + 1:, j] * L[c, j]
    return L, inv, bad


def standin_solve_sq(L, inv, Y):
    """forward substitution of k_boot_solvemax, column by column: y_k = acc_k * (1 / L_kk), ss += y_k^2, acc_r -= L_rk y_k"""
    acc = np.array(Y, dtype=np.float64)
    d = L.shape[0]
    ss = np.zeros(len(acc))
    for k in range(d):
        yk = acc[:, k] * inv[k]
        ss = ss + yk * yk
        for r in range(k + 1, d):
            acc[:, r] = acc[:, r] - L[r, k] * yk
    return ss


def standin_factor_given(u, sel, mean, cov, scale, defect=None):
    """k_boot_chol + k_boot_solvemax on given moments: NaN for a failed factorisation or a NaN among the left-out rows"""
    u = np.asarray(u, dtype=np.float64)
    sel = np.asarray(sel, dtype=bool)
    with np.errstate(all="ignore"):
        L, inv, bad = standin_chol(np.asarray(cov, dtype=np.float64) * float(scale), defect=defect)
        ss = standin_solve_sq(L, inv, u - np.asarray(mean, dtype=np.float64))
    use = sel if defect == "max_over_selected" else ~sel
    if bad or not use.any() or np.isnan(ss[use]).any():
        return np.nan
    return float(np.maximum(ss[use], 0.0).max())


def standin_factor(u, sel, scale, defect=None):
    """the whole chain of mlf_bootstrap_factor in binary64"""
    mean = standin_mean(u, sel)
    with np.errstate(all="ignore"):
        cov = standin_cov(u, sel, mean)
    return standin_factor_given(u, sel, mean, cov, scale, defect=defect)


def standin_quadform(u_rows, ctr, P, dp=None):
    """k_boot_quadmax / k_prep: dl = u - ctr, one accumulator, j outer, k inner, (dl_j P_jk) dl_k, no fma"""
    dl = np.atleast_2d(np.asarray(u_rows, dtype=np.float64)) - np.asarray(ctr, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    d = dl.shape[1]
    acc = np.zeros(len(dl))
    for j in range(d):
        for k in range(d):
            acc = acc + (dl[:, j] * P[j, k]) * dl[:, k]
    return acc
