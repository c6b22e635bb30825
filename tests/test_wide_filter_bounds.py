"""Soundness of the thresholds of the pre-filter for 129 ... 1024 dimensions (csrc/mlf_wide_filter.hip: wide_thresholds), on the
CPU with the numpy emulation of test_filter_bounds.py: binary16 operands, exact products, binary32 accumulation in the orders
"reversed" (one rounding per product, the pessimistic model the accumulation coefficient is derived for), "groups" and "tree"
(how v_mfma_f32_32x32x16_f16 was found to accumulate).  The sweep keeps one accumulator chain per pair over all K columns:
there is no split-K join to model.

Property (for every pair): Dt <= T_lo  =>  s <= r2 ;  Dt > T_hi  =>  s > r2, s = the reference's sequential binary64 distance.
"""
import functools

import numpy as np
import pytest

import test_filter_bounds as narrow


def acc_coef(K):
    """the power of two >= K 2^-24, not below the 2^-15 of the kernels for up to 128 dimensions"""
    c = 2.0**-15
    while c < K * 2.0**-24:
        c *= 2.0
    return c


def thresholds(sigma, namax, nbn2, r2, K):
    """float64 restatement of wide_thresholds() incl. the directed float32 rounding"""
    nbn = np.sqrt(nbn2)
    delta = 2.0**-11 * (1 + 2.0**-9) * (namax + nbn) + 2 * np.sqrt(K) * 2.0**-24 + 2.0**-40 * (namax + nbn)
    w = namax + nbn + 2.0**-8
    eacc = (acc_coef(K) + 2.0**-32) * w * w + 2.0**-20
    sr = sigma * np.sqrt(r2)
    lo = sr * (1 - 2.0**-30) - delta
    hi = sr * (1 + 2.0**-30) + delta
    t_lo = lo * lo - eacc if (lo > 0 and lo * lo - eacc >= 0) else -np.inf
    t_hi = hi * hi + eacc
    lo_f = np.float32(t_lo)
    if float(lo_f) > t_lo:
        lo_f = np.nextafter(lo_f, np.float32(-np.inf))
    hi_f = np.float32(t_hi)
    if float(hi_f) < t_hi:
        hi_f = np.nextafter(hi_f, np.float32(np.inf))
    return float(lo_f), float(hi_f), t_hi < 30000.0


def test_accumulation_coefficient_is_the_stated_function_of_k():
    assert acc_coef(160) == acc_coef(512) == 2.0**-15
    assert acc_coef(528) == acc_coef(1024) == 2.0**-14
    assert acc_coef(1040) == 2.0**-13
    for K in range(160, 1041, 16):
        assert acc_coef(K) >= K * 2.0**-24 and acc_coef(K) >= 2.0**-15
    # up to 512 columns the accumulation term is filter_thresholds' own: the interval can only differ by the absolute term
    lo_n, hi_n, _ = narrow.thresholds(0.25, 9.0, 30.0, 40.0, 272)
    lo_w, hi_w, _ = thresholds(0.25, 9.0, 30.0, 40.0, 272)
    assert lo_w <= lo_n and hi_w >= hi_n and hi_w - hi_n < 1e-5 and lo_n - lo_w < 1e-5


N_LIVE, N_PROP = 400, 100


@functools.lru_cache(maxsize=None)
def operands(d, scale, offset):
    """live points, proposals, both binary16 operands and the reference distances of one case: computed once, shared by the
    three accumulation models, never modified"""
    rs = np.random.RandomState(7000 + d)
    a = offset + scale * rs.normal(size=(N_LIVE, d))
    b = a[rs.randint(N_LIVE, size=N_PROP)] + scale * rs.normal(size=(N_PROP, d)) * rs.uniform(0.2, 1.2, size=(N_PROP, 1))
    dp = (d + 15) // 16 * 16                  # the filter runs on the padded dimensionality: zero columns
    K = (dp + 6 + 15) // 16 * 16
    c = a.mean(axis=0)
    amax = np.abs(a - c).max()
    sigma = 2.0 ** -np.frexp(amax)[1]
    xa = sigma * (a - c)
    assert np.abs(xa).max() <= 1.0
    namax = np.sqrt((xa**2).sum(axis=1)).max() * (1 + 1e-12)
    ah = xa.astype(np.float32).astype(np.float16)
    A = np.zeros((N_LIVE, K), dtype=np.float16)
    A[:, :d] = ah
    na = (ah.astype(np.float64) ** 2).sum(axis=1)
    for i in range(N_LIVE):
        A[i, dp:dp + 3] = narrow.split3(na[i])
    A[:, dp + 3:dp + 6] = 1.0
    B = np.zeros((N_PROP, K), dtype=np.float16)
    nbn2 = np.zeros(N_PROP)
    for j in range(N_PROP):
        xb = sigma * (b[j] - c)
        nbn2[j] = float((xb**2).sum())
        bh = xb.astype(np.float32).astype(np.float16)
        B[j, :d] = (-2.0 * bh.astype(np.float32)).astype(np.float16)
        assert np.array_equal(B[j, :d].astype(np.float64), -2.0 * bh.astype(np.float64))   # exact
        B[j, dp:dp + 3] = 1.0
        B[j, dp + 3:dp + 6] = narrow.split3((bh.astype(np.float64) ** 2).sum())
    s = np.stack([narrow.seq_dist2(a, b[j]) for j in range(N_PROP)])
    la = a[:150]
    dd = np.stack([narrow.seq_dist2(la, la[i]) for i in range(150)])
    np.fill_diagonal(dd, np.inf)
    r2_nn = float(np.quantile(dd.min(axis=1), 0.8))
    for arr in (A, B, s, nbn2):
        arr.setflags(write=False)
    return dict(K=K, sigma=sigma, namax=namax, A=A, B=B, s=s, nbn2=nbn2, r2_nn=r2_nn)


CASES = [(129, 1.0, 0.0), (256, 1.0, 0.0), (515, 1.0, 0.0), (1018, 1.0, 0.0), (1024, 1.0, 0.0),
         (256, 1e-5, 0.5), (1024, 3e3, -7e4)]


@pytest.mark.parametrize("model", ["reversed", "groups", "tree"])
@pytest.mark.parametrize("d,scale,offset", CASES)
def test_wide_thresholds_are_sound(d, scale, offset, model):
    o = operands(d, scale, offset)
    K, A, B, s_all = o["K"], o["A"], o["B"], o["s"]
    if d == 1024:
        assert K == 1040
    A64 = A.astype(np.float64)
    checked = band = min_band = 0
    for j in range(N_PROP):
        prod = A64 * B[j].astype(np.float64)       # exact: 11-bit x 11-bit significands
        dt = narrow.mfma_accumulate(prod, model)
        s = s_all[j]
        for r2 in (o["r2_nn"], np.sort(s)[0] * (1 + 1e-9), np.median(s)):
            lo, hi, ok = thresholds(o["sigma"], o["namax"], float(o["nbn2"][j]), r2, K)
            if not ok:
                continue
            assert not (dt[(s > r2)] <= lo).any(), "certain-hit threshold admitted a miss"
            assert not (dt[(s <= r2)] > hi).any(), "certain-miss threshold rejected a hit"
            checked += N_LIVE
            band += int(((dt > lo) & (dt <= hi)).sum())
            if r2 == o["r2_nn"]:
                min_band += int(lo < dt.min() <= hi)
    assert checked == 3 * N_LIVE * N_PROP          # no case is skipped: every T_hi stays below the 3e4 guard
    # the band must stay a small minority (test_filter_bounds.py's cap), and at the neighbour radius hardly any proposal's
    # MINIMUM may end in it: those are the proposals the sweep hands to the exact scan
    assert band / checked < 0.2, band / checked
    assert min_band <= N_PROP // 10, min_band


def certain_miss_by_norms(sigma, namax, nbn2, r2):
    """restatement of the quantising kernel's norm test (route 3): farther from the centre than any live point plus the radius"""
    return nbn2 <= 1e300 and np.sqrt(nbn2) * (1 - 2.0**-30) - namax > sigma * np.sqrt(r2) * (1 + 2.0**-30)


@pytest.mark.parametrize("d", [129, 1024])
def test_the_norm_test_never_rejects_a_hit(d):
    """proposals at graded distances from the live set, radii from far below to far above those distances: wherever the
    test fires, the reference's sequential distance to EVERY live point is above r2; and it does fire for the far ones"""
    rs = np.random.RandomState(7100 + d)
    a = 0.5 + 0.05 * rs.normal(size=(N_LIVE, d))
    c = a.mean(axis=0)
    sigma = 2.0 ** -np.frexp(np.abs(a - c).max())[1]
    namax = sigma * np.sqrt(((a - c) ** 2).sum(axis=1)).max() * (1 + 1e-12)
    fired = 0
    for j, far in enumerate(np.geomspace(0.5, 300.0, 60)):
        z = rs.normal(size=d)
        b = a[j % N_LIVE] + far * 0.05 * z
        s = narrow.seq_dist2(a, b)
        xb = sigma * (b - c)
        nbn2 = float((xb**2).sum())
        for r2 in (s.min() * (1 - 1e-12), s.min() * (1 + 1e-12), s.min() * 0.25, s.min() * 1e-3, s.min() * 4.0):
            if certain_miss_by_norms(sigma, namax, nbn2, r2):
                assert s.min() > r2
                fired += 1
    assert fired > 20
    assert not certain_miss_by_norms(1.0, 1.0, float("nan"), 1.0) and not certain_miss_by_norms(1.0, 1.0, float("inf"), 1.0)
