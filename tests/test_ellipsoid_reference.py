"""CPU checks of tests/ellipsoid_reference.py, the yardstick of test_ellipsoid_forms_gpu.py:

  * the long double references against mpmath on small cases, within 1e-17 * scale;
  * the binary64 stand-ins (the kernels' orders restated in numpy) stay within every derived bound on the input families
    W, C and I -- the condition under which a bound may be asserted of the device;
  * each seeded defect in a stand-in fails at least one assertion of the kind the GPU test makes.
"""
import numpy as np
import pytest

import ellipsoid_reference as R

LD = R.LD


def _mpf(x):
    return R._mpf_of_ld(LD(x))


# ------------------------------------------------------------------------------------------------ reference against itself
@pytest.mark.parametrize("kind", ["W", "C", "I"])
@pytest.mark.parametrize("n,d,cnt", [(12, 1, 5), (40, 3, 25), (60, 8, 40)])
def test_longdouble_references_against_mpmath(kind, n, d, cnt):
    mp = R._mp()
    u = R.family(kind, 10 * n + d, n, d)
    sel = R.mask_with(n, cnt)
    m_ld = R.ref_mean(u, sel)
    m_mp = R.mp_mean(u, sel)
    scale_m = np.abs(u[sel]).sum(axis=0) / cnt
    for k in range(d):
        assert abs(_mpf(m_ld[k]) - m_mp[k]) <= 1e-17 * scale_m[k]
    m64 = m_ld.astype(np.float64)
    c_ld = R.ref_cov(u, sel, m64)
    c_mp = R.mp_cov(u, sel, m64)
    x = np.abs(u[sel].astype(LD) - m64.astype(LD))
    scale_c = (x.T @ x) / (cnt - 1)
    for k in range(d):
        for l in range(d):
            assert abs(_mpf(c_ld[k, l]) - c_mp[k][l]) <= 1e-17 * float(scale_c[k, l]), (k, l)
    # quadratic form with a symmetric, indefinite-looking P
    rs = np.random.RandomState(n + d)
    P = rs.normal(size=(d, d))
    P = P + P.T
    ctr = m64
    y_ld = u.astype(LD) - ctr.astype(LD)
    q_ld = R.ref_quadform(y_ld, P)
    y_mp = [[mp.mpf(float(v)) - mp.mpf(float(c)) for v, c in zip(row, ctr)] for row in u]
    q_mp = R.mp_quadform(y_mp, P)
    scale_q = ((np.abs(y_ld) @ np.abs(P).astype(LD)) * np.abs(y_ld)).sum(axis=1)
    for i in range(n):
        assert abs(_mpf(q_ld[i]) - q_mp[i]) <= 1e-17 * float(scale_q[i]), i


@pytest.mark.parametrize("kind", ["W", "C", "I"])
@pytest.mark.parametrize("n,d,cnt", [(12, 1, 5), (40, 3, 25), (60, 8, 40)])
def test_factor_reference_against_explicit_inverse(kind, n, d, cnt):
    """ref_factor (Cholesky factor and substitution in mpmath, rows ranked in long double) against the definition: mpmath's
    explicit inverse and the quadratic form of EVERY left-out row; ref_factor_exact the same with mpmath moments"""
    mp = R._mp()
    u = R.family(kind, 20 * n + d, n, d)
    sel = R.mask_with(n, cnt)
    scale = d + 2
    mean = R.ref_mean(u, sel).astype(np.float64)
    cov = R.ref_cov(u, sel, mean).astype(np.float64)

    def by_definition(m, C):
        Ai = mp.inverse(mp.matrix([[C[i][j] * scale for j in range(d)] for i in range(d)]))
        best = None
        for row in u[~sel]:
            y = mp.matrix([mp.mpf(float(v)) - m[k] for k, v in enumerate(row)])
            q = (y.T * Ai * y)[0]
            best = q if best is None or q > best else best
        return best

    want = by_definition([mp.mpf(float(v)) for v in mean], [[mp.mpf(float(v)) for v in r] for r in cov])
    got = R.ref_factor(u, sel, mean, cov, scale)
    assert abs(got - want) <= mp.mpf(10) ** -40 * want
    m_mp = R.mp_mean(u, sel)
    want = by_definition(m_mp, R.mp_cov(u, sel, m_mp))
    got = R.ref_factor_exact(u, sel, scale)
    assert abs(got - want) <= mp.mpf(10) ** -40 * want


def test_masks_are_constructed():
    for n, cnt in [(42, 2), (43, 3), (552, 512), (1065, 1025), (255, 254), (100, 100)]:
        sel = R.mask_with(n, cnt)
        assert sel.sum() == cnt and sel[0] and sel[-1]
    sel = R.mask_with(1065, 1025)
    out = np.nonzero(~sel)[0]
    assert len(out) == 40 and out.min() > 0 and out.max() < 1064 and np.diff(out).min() > 20   # scattered


def test_chain_lengths():
    assert R.mean_chain(1024, "h16") == 64 + 16 and R.mean_chain(1025, "h16") == 65 + 16 and R.mean_chain(513, "wide") == 514
    assert R.cov_chain(512, "cov16") == 16 + 13 and R.cov_chain(513, "cov16") == 17 + 13
    assert R.cov_chain(513, "cov8") == 65 + 11 and R.cov_chain(33, "wide") == 36
    assert [R.pick_dp(d) for d in (1, 3, 49, 50, 65, 128, 129, 300)] == [2, 4, 50, 50, 80, 128, 144, 304]


# ------------------------------------------------------------------------------------------------ stand-ins pass
MOMENT_CASES = ([(d, cnt) for d in (1, 16, 17, 33, 64) for cnt in (2, 3, 33, 513, 1025)]
                + [(d, cnt) for d in (65, 128) for cnt in (2, 511, 513)] + [(129, 2), (129, 33), (257, 513)])


@pytest.mark.parametrize("kind", ["W", "C", "I"])
@pytest.mark.parametrize("d,cnt", MOMENT_CASES)
def test_standin_moments_within_bounds(kind, d, cnt):
    n = cnt + 40
    u = R.family(kind, 1000 * d + cnt, n, d)
    sel = R.mask_with(n, cnt)
    mean = R.standin_mean(u, sel)
    cov = R.standin_cov(u, sel, mean)
    r_mean, r_cov = R.moments_ratios(u, sel, mean, cov)
    assert r_mean <= 1 and r_cov <= 1, (r_mean, r_cov)
    assert np.array_equal(cov, cov.T)


@pytest.mark.parametrize("kind", ["W", "C", "I"])
@pytest.mark.parametrize("d", [1, 2, 8, 9, 17, 33, 50, 64])
def test_standin_factor_within_bounds(kind, d):
    """Stage B (given moments) and Stage C (end to end) of the GPU test, with the stand-ins in the device's place"""
    n = 3 * d + 60
    u = R.family(kind, 31 * d, n, d)
    sel = R.mask_with(n, n - 40)
    mean = R.standin_mean(u, sel)
    cov = R.standin_cov(u, sel, mean)
    f = R.standin_factor_given(u, sel, mean, cov, d + 2)
    r, b = R.factor_ratio(f, u, sel, mean, cov, d + 2)
    assert b <= 1e-6, b
    assert r <= 1, (r, b)
    exact = R.ref_factor_exact(u, sel, d + 2)
    bc = R.bound_factor_composite(u, sel, d + 2, f=exact)
    assert abs(R._mp().mpf(f) - exact) <= bc * exact, (float(abs(f - exact) / exact), bc)
    assert R.standin_factor(u, sel, d + 2) == f


@pytest.mark.parametrize("d,n", [(1, 40), (2, 255), (3, 60), (50, 257), (64, 60), (65, 40), (129, 33)])
def test_standin_quadform_within_bound(d, n):
    rs = np.random.RandomState(d + n)
    u = R.family("C", d, n, d)
    ctr = u.mean(axis=0)
    P = R.symmetric_matrix(rs, d, 1e6) / 1e-12
    q = R.standin_quadform(u, ctr, P)
    y = u.astype(LD) - ctr.astype(LD)
    assert R.ratio(q.astype(LD) - R.ref_quadform(y, P), R.bound_quadform(y, P)) <= 1


# ------------------------------------------------------------------------------------------------ seeded defects fail
def _moments(kind, d, cnt, mean_defect=None, cov_defect=None):
    n = cnt + 40
    u = R.family(kind, 77 * d + cnt, n, d)
    sel = R.mask_with(n, cnt)
    mean = R.standin_mean(u, sel, defect=mean_defect)
    cov = R.standin_cov(u, sel, mean, defect=cov_defect)
    return u, sel, mean, cov


@pytest.mark.parametrize("kind", ["W", "C"])
@pytest.mark.parametrize("d,cnt", [(16, 33), (64, 1025), (100, 513), (129, 33)])
def test_defect_last_entry_dropped(kind, d, cnt):
    u, sel, mean, cov = _moments(kind, d, cnt, mean_defect="drop_last")
    assert R.moments_ratios(u, sel, mean, cov)[0] > 1
    u, sel, mean, cov = _moments(kind, d, cnt, cov_defect="drop_last")
    assert R.moments_ratios(u, sel, mean, cov)[1] > 1


@pytest.mark.parametrize("kind", ["W", "C"])
@pytest.mark.parametrize("d,cnt", [(16, 33), (64, 1025), (100, 513), (129, 33)])
def test_defect_divisor_cnt(kind, d, cnt):
    u, sel, mean, cov = _moments(kind, d, cnt, cov_defect="divisor_cnt")
    assert R.moments_ratios(u, sel, mean, cov)[1] > 1


@pytest.mark.parametrize("kind", ["W", "C"])
@pytest.mark.parametrize("d,cnt", [(16, 33), (64, 1025), (100, 513)])
def test_defect_mean_in_binary32(kind, d, cnt):
    u, sel, mean, cov = _moments(kind, d, cnt, mean_defect="mean_f32")
    assert R.moments_ratios(u, sel, mean, cov)[0] > 1


@pytest.mark.parametrize("d,cnt", [(16, 33), (64, 1025), (100, 513), (129, 33)])
def test_defect_one_pass_covariance_on_concentrated_data(d, cnt):
    u, sel, mean, cov = _moments("C", d, cnt, cov_defect="one_pass")
    assert R.moments_ratios(u, sel, mean, cov)[1] > 1


@pytest.mark.parametrize("d", [17, 33, 64])
def test_defect_mirror_image_unwritten(d):
    u, sel, mean, cov = _moments("W", d, 100, cov_defect="mirror_missing")
    assert not np.array_equal(cov, cov.T)
    assert R.moments_ratios(u, sel, mean, cov)[1] > 1


@pytest.mark.parametrize("kind", ["W", "C", "I"])
@pytest.mark.parametrize("d", [2, 9, 33, 64])
@pytest.mark.parametrize("defect", ["chol_skip_last", "max_over_selected"])
def test_defect_in_factor(kind, d, defect):
    n = 3 * d + 60
    u = R.family(kind, 31 * d, n, d)
    sel = R.mask_with(n, n - 40)
    mean = R.standin_mean(u, sel)
    cov = R.standin_cov(u, sel, mean)
    f = R.standin_factor_given(u, sel, mean, cov, d + 2, defect=defect)
    r, _ = R.factor_ratio(f, u, sel, mean, cov, d + 2)
    assert r > 1, r
