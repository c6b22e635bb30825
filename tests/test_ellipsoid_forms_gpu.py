"""The wrapping-ellipsoid arithmetic of the region rebuild against long double / mpmath references, within error bounds
derived from the kernels' documented summation orders (references, derivations and binary64 stand-ins:
ellipsoid_reference.py; test_ellipsoid_reference.py shows on the CPU that the bounds admit a correct binary64
implementation and reject seeded defects).  Run with `-m gpu`.

  Stage A  K.bootstrap_moments: k_boot_index, k_boot_mean<1|2>, k_boot_mean_wide, k_boot_cov16<1..4>, k_boot_cov<2>,
           k_boot_cov_wide -- mean within bound_mean, covariance within bound_cov of ref_cov evaluated with the DEVICE's
           mean, exact symmetry up to 64 dimensions, rounds independent of each other bit for bit
  Stage B  K.bootstrap_factor given the device's moments: k_boot_chol<32|64>, k_boot_solvemax<8 ... 64>
  Stage C  K.bootstrap_factor end to end against the exact factor, within the composite bound; next to it the reference's
           own formulation in binary64 (numpy mean, cov, inv, einsum) on the same inputs (printed, not asserted)
  Stage D  K.bootstrap_quadform_max (k_boot_quadmax<DP>, k_quadmax_wide) and K.inside_ellipsoid (k_prep<DP>, k_prep_wide)
  Stage E  failure paths: degenerate, one-row and empty selections

Input families (ellipsoid_reference.family): W well spread, C concentrated (0.3 +- 1e-6, correlated), I ill conditioned
(kappa_2 about 1e6).  Masks are constructed (mask_with): exactly cnt ones, rows 0 and n - 1 among them, the left-out rows
scattered, so the list-length seams of the kernels (16 / 32 entries per step, 512 and 1024 per trip, 256 rows per
k_boot_solvemax workgroup) are hit on purpose.

Largest error / bound measured on the MI355X, with the case it occurred in (each test prints its figures; a ratio above 1
is a failed assertion):

  A mean        0.32    W, d = 129, cnt = 2 (k_boot_mean_wide)
  A covariance  0.37    W, d = 129, cnt = 2 (k_boot_cov_wide)
  B             0.15    I, d = 1 (bound 1.2e-15).  The bound grows like d^2 kappa_2 and the measured error does not: at its
                        largest, 7.9e-7 (I, d = 64), the ratio is 3.8e-7 -- the worst case of the backward error analysis
                        is far from attained at large d; the constant is the derivation's and is left alone
  C             0.0080  C, d = 8 (bound 2.5e-8, error 1.95e-10)
  D maximum     0.32    W, d = 1, n = 257;   D inside_ellipsoid  0.39  W, d = 2, p = 257, no row undecided in any case
                        (at d = 300 the ratios are near 1e-4: a chain of d * dp roundings does not line up)

Stage C, relative error against the exact factor: device / the reference's formulation in binary64 (numpy mean, cov, inv,
einsum); bound in brackets:

  d     W (well spread)                   C (0.3 +- 1e-6, correlated)
  2     2.3e-17 / 1.7e-16  [1.5e-14]      2.6e-11 / 2.6e-11  [1.6e-8]
  8     3.7e-16 / 7.4e-19  [2.2e-13]      1.95e-10 / 4.3e-10 [2.5e-8]
  50    3.5e-16 / 5.8e-16  [1.7e-11]      5.2e-12 / 5.1e-10  [9.3e-8]
  64    2.4e-16 / 4.1e-16  [3.2e-11]      9.3e-11 / 4.75e-10 [1.1e-7]

On well-spread data both are exact to a few units of the last place.  On the concentrated family the PROBLEM is ill
conditioned -- a rounding of the mean, 1e-16 of 0.3, is 1e-10 of the spread -- and neither formulation holds a 1e-10
class there: the device is as far from the exact value as the reference's own formulation at d = 2, and two (d = 8), a
hundred (d = 50) and five (d = 64) times closer.
"""
import numpy as np
import pytest

import ellipsoid_reference as R

pytestmark = pytest.mark.gpu

LD = R.LD


@pytest.fixture(scope="module")
def K():
    from ultranest_amd import _lib, kernels
    assert _lib.device_count() >= 1, "no MI355X visible"
    return kernels


def _seed(*parts):
    s = 12345
    for p in parts:
        s = (s * 1000003 + (sum(map(ord, p)) if isinstance(p, str) else int(p))) % (2 ** 31 - 1)
    return s


# ================================================================================================ Stage A: moments
CNT_FULL = (2, 3, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025)
CNT_DEFAULT = 77   # three steps of a k_boot_cov16 group, five of a k_boot_mean wave, not a multiple of anything

A_CASES = []
for _d in (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 100, 128, 129, 257):
    A_CASES += [(k, _d, CNT_DEFAULT) for k in ("W", "C")]
for _d in (16, 64):
    A_CASES.append(("I", _d, CNT_DEFAULT))
    A_CASES += [(k, _d, c) for k in ("W", "C", "I") for c in CNT_FULL]
A_CASES += [(k, 100, c) for k in ("W", "C") for c in (511, 512, 513)]
A_CASES += [(k, 129, c) for k in ("W", "C") for c in (2, 33, 513)]


def _check_moments(tag, u, masks, mean, cov):
    d = u.shape[1]
    for b, sel in enumerate(masks):
        r_mean, r_cov = R.moments_ratios(u, sel, mean[b], cov[b])
        print("STAGE-A %s round %d cnt %d: mean err/bound %.3g  cov err/bound %.3g" % (tag, b, int(sel.sum()), r_mean, r_cov))
        assert r_mean <= 1, (tag, b, r_mean)
        assert r_cov <= 1, (tag, b, r_cov)
        if d <= 64:   # k_boot_cov16 writes the mirror image of every off-diagonal chunk itself
            assert np.array_equal(cov[b], cov[b].T), (tag, b)


@pytest.mark.parametrize("kind,d,cnt", A_CASES)
def test_moments_within_bounds(kind, d, cnt, K):
    """Three rounds of different list lengths in one call; every round within the bounds, and round 0 run alone gives the
    same bits (the rounds share the index scratch, the partial-sum arrays and the grid)."""
    n = cnt + 40
    u = R.family(kind, _seed("A", kind, d, cnt), n, d)
    masks = np.array([R.mask_with(n, cnt), R.mask_with(n, max(2, cnt // 2 + 1)), R.mask_with(n, cnt + 20)])
    mean, cov = K.bootstrap_moments(u, masks)
    _check_moments("%s d=%d cnt=%d" % (kind, d, cnt), u, masks, mean, cov)
    mean0, cov0 = K.bootstrap_moments(u, masks[:1])
    assert np.array_equal(mean0[0], mean[0]) and np.array_equal(cov0[0], cov[0])


@pytest.mark.parametrize("kind", ["W", "C"])
def test_moments_every_row_selected(kind, K):
    """the call of the device-resident rebuild: an all-ones selection (next to it a round that leaves rows out)"""
    n, d = 1100, 50
    u = R.family(kind, _seed("A-all", kind), n, d)
    masks = np.array([np.ones(n, dtype=bool), R.mask_with(n, n - 40)])
    mean, cov = K.bootstrap_moments(u, masks)
    _check_moments("%s d=%d all rows" % (kind, d), u, masks, mean, cov)
    mean0, cov0 = K.bootstrap_moments(u, masks[:1])
    assert np.array_equal(mean0[0], mean[0]) and np.array_equal(cov0[0], cov[0])


# ================================================================================================ Stage B: factor, moments given
def _check_factor_given(tag, K, u, masks):
    """mlf_bootstrap_factor (mlf_stateless.hip:442-477) calls launch_boot_moments (:457) with the arguments and on the
    buffers of mlf_bootstrap_moments (:420-440, launch at :433): rows in c.src, masks in c.selbytes, mean in c.small0,
    counts in c.small1, covariance in c.out, index lists in c.small2.  The same kernels on the same inputs are
    deterministic (fixed orders, no atomics in the moments), so the mean and covariance K.bootstrap_moments returns are the
    ones k_boot_chol and k_boot_solvemax read inside K.bootstrap_factor, and f is held to the bound of that chain alone."""
    d = u.shape[1]
    mean, cov = K.bootstrap_moments(u, masks)
    f = K.bootstrap_factor(u, masks, d + 2)
    for b, sel in enumerate(masks):
        r, bound = R.factor_ratio(f[b], u, sel, mean[b], cov[b], d + 2)
        print("STAGE-B %s round %d: bound %.3g  err/bound %.3g" % (tag, b, bound, r))
        assert bound <= 1e-6, (tag, b, bound)   # no case passes on a vacuous bound
        assert r <= 1, (tag, b, r)


B_DIMS = (1, 7, 8, 9, 16, 17, 24, 25, 31, 32, 33, 40, 41, 48, 49, 56, 57, 63, 64)


@pytest.mark.parametrize("kind", ["W", "C", "I"])
@pytest.mark.parametrize("d", B_DIMS)
def test_factor_given_moments_every_size_class(kind, d, K):
    n = 3 * d + 60
    u = R.family(kind, _seed("B", kind, d), n, d)
    masks = np.array([R.mask_with(n, n - 40), R.mask_with(n, n - 27)])
    _check_factor_given("%s d=%d" % (kind, d), K, u, masks)


@pytest.mark.parametrize("kind", ["W", "C", "I"])
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_factor_workgroup_seams(kind, n, K):
    """one or two left-out rows: the last row of a k_boot_solvemax workgroup (256 rows) and the first of the next"""
    d = 24
    u = R.family(kind, _seed("B-seam", kind, n), n, d)
    rounds = []
    for first in (256, 512):
        out = [r for r in (first - 1, first) if r < n]
        if not out:
            out = [n - 1]
        if out in rounds:
            continue
        rounds.append(out)
    masks = np.ones((len(rounds), n), dtype=bool)
    for b, out in enumerate(rounds):
        masks[b, out] = False
    _check_factor_given("%s seam n=%d left out %s" % (kind, n, rounds), K, u, masks)


# ================================================================================================ Stage C: end to end
@pytest.mark.parametrize("kind", ["W", "C"])
@pytest.mark.parametrize("d", [2, 8, 50, 64])
def test_factor_end_to_end(kind, d, K):
    mp = R._mp()
    n = 3 * d + 60
    u = R.family(kind, _seed("C", kind, d), n, d)
    sel = R.mask_with(n, n - 40)
    f = float(K.bootstrap_factor(u, sel[None, :], d + 2)[0])
    exact = R.ref_factor_exact(u, sel, d + 2)
    bound = R.bound_factor_composite(u, sel, d + 2, f=exact)
    err = float(abs(mp.mpf(f) - exact) / exact)
    # the reference's formulation in binary64 (mlfriends.pyx:1056-1066): numpy mean, cov, inv, einsum
    s = u[sel]
    delta = u[~sel] - s.mean(axis=0)
    f_np = float(np.einsum("ij,jk,ik->i", delta, np.linalg.inv(np.atleast_2d(np.cov(s, rowvar=0)) * (d + 2)), delta).max())
    err_np = float(abs(mp.mpf(f_np) - exact) / exact)
    print("STAGE-C %s d=%d: bound %.3g  device err %.3g (err/bound %.3g)  numpy formulation err %.3g"
          % (kind, d, bound, err, err / bound, err_np))
    assert err <= bound, (kind, d, err, bound)


# ================================================================================================ Stage D: quadratic forms
D_DIMS = (1, 2, 3, 50, 64, 65, 128, 129, 300)


def _quad_inputs(kind, d, n, B, tag):
    rs = np.random.RandomState(_seed(tag, kind, d, n))
    u = R.family(kind, _seed(tag, "u", kind, d, n), n, d)
    spread = {"W": 1.0, "C": 1e-6}[kind]
    ctrs = u.mean(axis=0) + 0.1 * spread * rs.normal(size=(B, d))
    Ps = np.array([R.symmetric_matrix(rs, d, 1e6) / spread ** 2 for _ in range(B)])
    return rs, u, ctrs, Ps


@pytest.mark.parametrize("kind", ["W", "C"])
@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("d", D_DIMS)
def test_quadform_max(kind, d, n, K):
    """f_b must lie between max_i (q_i - bound_i) and max_i (q_i + bound_i) over the left-out rows of round b; a NaN in a
    left-out row of one round makes that round NaN and leaves the others as they were, bit for bit"""
    B = 3
    rs, u, ctrs, Ps = _quad_inputs(kind, d, n, B, "D-max")
    masks = np.array([R.mask_with(n, n - 40), R.mask_with(n, n - 33), R.mask_with(n, n - 2)])
    f = K.bootstrap_quadform_max(u, masks, ctrs, Ps)
    for b in range(B):
        y = u[~masks[b]].astype(LD) - ctrs[b].astype(LD)
        q, bd = R.ref_quadform(y, Ps[b]), R.bound_quadform(y, Ps[b]).astype(LD)
        lo, hi = (q - bd).max(), (q + bd).max()
        r = float(abs(LD(f[b]) - q.max()) / bd.max())
        print("STAGE-D max %s d=%d n=%d round %d: rel bound %.3g  err/bound %.3g" % (kind, d, n, b, float(bd.max() / q.max()), r))
        assert lo <= LD(f[b]) <= hi, (kind, d, n, b, r)
    row = int(np.nonzero(~masks[1] & masks[0] & masks[2])[0][0])   # left out in round 1 only
    bad = u.copy()
    bad[row, d // 2] = np.nan
    g = K.bootstrap_quadform_max(bad, masks, ctrs, Ps)
    assert np.isnan(g[1]) and g[0] == f[0] and g[2] == f[2], (g, f)


@pytest.mark.parametrize("kind", ["W", "C"])
@pytest.mark.parametrize("p", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("d", D_DIMS)
def test_inside_ellipsoid_q_and_mask(kind, d, p, K):
    """q within bound_quadform; the mask equal to ref_q <= r2 wherever the reference decides (|ref_q - r2| > bound), with r2
    halfway between the two middle values of ref_q (half of ref_q itself for a single row, whose own value would be
    undecided by construction) and at most 1 % undecided; with r2 one of the returned q the mask is q <= r2 on the kernel's
    own q for every row"""
    rs, pts, ctrs, Ps = _quad_inputs(kind, d, p, 1, "D-in")
    c, P = ctrs[0], Ps[0]
    y = pts.astype(LD) - c.astype(LD)
    q_ref, bd = R.ref_quadform(y, P), R.bound_quadform(y, P).astype(LD)
    srt = np.sort(q_ref)
    r2 = float((srt[p // 2 - 1] + srt[p // 2]) / 2) if p > 1 else float(srt[0] / 2)
    mask, q = K.inside_ellipsoid(pts, c, P, r2, return_q=True)
    r = R.ratio(q.astype(LD) - q_ref, bd)
    decided = np.abs(q_ref - LD(r2)) > bd
    print("STAGE-D inside %s d=%d p=%d: rel bound %.3g  err/bound %.3g  undecided %d"
          % (kind, d, p, float((bd / q_ref).max()), r, int((~decided).sum())))
    assert r <= 1, (kind, d, p, r)
    assert (~decided).sum() <= 0.01 * p
    assert np.array_equal(mask[decided], (q_ref <= LD(r2))[decided])
    if p == 1:
        mask_in = K.inside_ellipsoid(pts, c, P, float(2 * srt[0]))
        assert mask_in.all() and not mask.any()
    for pick in sorted({0, p // 2, p - 1}):    # the boundary itself
        m2, q2 = K.inside_ellipsoid(pts, c, P, float(q[pick]), return_q=True)
        assert np.array_equal(q2, q)
        assert np.array_equal(m2, q <= q[pick]) and m2[pick], (kind, d, p, pick)


# ================================================================================================ Stage E: failure paths
@pytest.mark.parametrize("d", [3, 40])
def test_factor_failure_paths_touch_their_round_only(d, K):
    """a selection that spans no volume, a single selected row, an empty selection: NaN for that round, the other rounds
    finite and equal, bit for bit, to what they are in a call of their own"""
    n = 3 * d + 60
    u = R.family("W", _seed("E", d), n, d)
    u[: n // 2, 0] = 0.25                                  # the first half of the rows lies in a plane
    good0, good1 = R.mask_with(n, n - 40), R.mask_with(n, n - 27)
    flat = np.zeros(n, dtype=bool)
    flat[: n // 2: 2] = True                               # spans no volume: variance of coordinate 0 exactly 0
    one = np.zeros(n, dtype=bool)
    one[n // 3] = True
    none = np.zeros(n, dtype=bool)
    masks = np.array([good0, flat, one, good1, none])
    f = K.bootstrap_factor(u, masks, d + 2)
    assert np.isnan(f[[1, 2, 4]]).all(), f
    assert np.isfinite(f[[0, 3]]).all() and (f[[0, 3]] > 0).all(), f
    assert np.array_equal(f[[0, 3]], K.bootstrap_factor(u, masks[[0, 3]], d + 2))


@pytest.mark.parametrize("d", [3, 40, 64, 100, 129, 257])
def test_moments_of_fewer_than_two_rows(d, K):
    """cnt = 1: the mean is the row, the covariance non-finite in every element in the narrow forms and in the wide one alike;
    cnt = 0: mean and covariance NaN in both; the round next to them is untouched"""
    n = 90
    u = R.family("W", _seed("E-one", d), n, d)
    one = np.zeros(n, dtype=bool)
    one[n - 7] = True
    good = R.mask_with(n, n - 40)
    masks = np.array([one, good, np.zeros(n, dtype=bool)])
    mean, cov = K.bootstrap_moments(u, masks)
    assert np.array_equal(mean[0], u[n - 7])
    assert not np.isfinite(cov[0]).any(), cov[0]
    assert np.isnan(mean[2]).all() and np.isnan(cov[2]).all()
    mean1, cov1 = K.bootstrap_moments(u, masks[1:2])
    assert np.array_equal(mean[1], mean1[0]) and np.array_equal(cov[1], cov1[0])
    r_mean, r_cov = R.moments_ratios(u, good, mean[1], cov[1])
    assert r_mean <= 1 and r_cov <= 1
