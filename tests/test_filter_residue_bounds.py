"""Soundness and tightness of the thresholds with MEASURED binary16 residues (csrc/mlf_filter_dev.hpp:
filter_thresholds4r; used by k_prep_sweep and k_prep4), on the CPU: a numpy restatement of the device arithmetic
-- the live side's residue maximum as k_quant_refs computes it (binary64), the query side's as the packing loop does
(binary32) -- with the three accumulation models of test_filter_bounds.py, checked against the reference's sequential
binary64 distance.

Properties (for every pair):
  soundness   Dt <= T_lo  =>  s <= r2 ;  Dt > T_hi  =>  s > r2, with r2 placed a few ulps on either side of pair
              distances and on both edges of the band, for operands with full-size coordinates, coordinates in the
              binary16 subnormal range and coordinates that ARE binary16 values (residue 0)
  tightness   [T_lo, T_hi] of filter_thresholds4r lies inside [T_lo, T_hi] of filter_thresholds4 on the same inputs
"""
import numpy as np
import pytest

from test_filter_bounds import mfma_accumulate, seq_dist2
from test_prep4_bounds import DN, UP, _split3_f64, dn32, f32, split3, thresholds4, up32


def c_of_k(K):
    """the power of two >= K 2^-24, not below 2^-18, as a binary32 value times (1 + 2^-9)"""
    c = 2.0**-18 if K <= 64 else 2.0**-17 if K <= 128 else 2.0**-16 if K <= 256 else 2.0**-15
    assert K <= 512 and c >= K * 2.0**-24
    return f32(c) * (f32(1) + f32(2.0**-9))


def thresholds4r(ea_max, eb, namax, nb, zeta, sqrt_k, sr_lo, sr_hi, K):
    """float32 restatement of filter_thresholds4r (csrc/mlf_filter_dev.hpp)"""
    ea_max, eb, namax, nb, zeta, sqrt_k, sr_lo, sr_hi = (f32(v) for v in (ea_max, eb, namax, nb, zeta, sqrt_k, sr_lo, sr_hi))
    nbh = np.sqrt(nb) * UP
    nbn = ((nbh + sqrt_k * f32(2.0**-25)) * (f32(1) + f32(2.0**-10)) + zeta) * UP
    w0 = namax + nbn
    delta = (ea_max + eb + f32(2.0**-40) * w0 + (f32(1) + f32(2.0**-10)) * zeta) * UP
    w = w0 + ea_max + f32(2.0**-8)
    eacc = (c_of_k(K) * w * w + f32(2.0**-22) + f32(2.0**-18) * nb) * UP
    lo = (sr_lo * DN - delta) * DN
    hi = (sr_hi * UP + delta) * UP
    t_lo = (lo * lo) * DN - eacc * UP if lo > 0 else f32(-np.inf)
    if t_lo < 0:
        t_lo = f32(-np.inf)
    t_hi = ((hi * hi) * UP + eacc) * UP
    return float(t_lo), float(t_hi), bool(t_hi < 30000)


def live_side(a):
    """centre, scale, binary64 scaled rows, binary16 operand, namax and ea_max as k_ref_finish / k_quant_refs publish them"""
    c = a.mean(axis=0)
    amax = np.abs(a - c).max()
    sigma = 2.0 ** -np.frexp(amax)[1]
    xa = sigma * (a - c)
    ah = xa.astype(np.float32).astype(np.float16)
    res = ah.astype(np.float64) - xa
    ea2 = np.zeros(len(a))
    for k in range(a.shape[1]):                       # some order of a binary64 sum (the kernel's differs: inside 2^-40)
        ea2 = ea2 + res[:, k] * res[:, k]
    ea = np.sqrt(ea2 * (1 + 2.0**-40)) * (1 + 2.0**-40) + 2.0**-500
    namax = np.sqrt((xa**2).sum(axis=1)).max() * (1 + 1e-12)
    return c, sigma, xa, ah, namax, float(ea.max())


def live_operand(ah, d, dp, K):
    A = np.zeros((len(ah), K), dtype=np.float16)
    A[:, :d] = ah
    na = (ah.astype(np.float64) ** 2).sum(axis=1)
    for i in range(len(ah)):
        A[i, dp:dp + 3] = [np.float16(np.float32(p)) for p in _split3_f64(na[i])]
    A[:, dp + 3:dp + 6] = 1.0
    return A


def query_operand(bq, d, dp, K):
    """the packing loop: v = -2 bq in binary32, operand fl16(v), |bh|^2 and the residue sum in binary32 (one fused
    multiply-add per value)"""
    v = (f32(-2) * bq.astype(np.float32)).astype(np.float32)
    m2 = v.astype(np.float16)
    back = m2.astype(np.float32)
    res = v - back
    assert np.array_equal(res.astype(np.float64), v.astype(np.float64) - back.astype(np.float64))   # exact in binary32
    nb = f32(0)
    e2 = f32(0)
    for x, r in zip(back, res):
        nb = f32(np.float64(x) * np.float64(x) + np.float64(nb))
        e2 = f32(np.float64(r) * np.float64(r) + np.float64(e2))
    nb = f32(0.25) * nb
    eb = f32(0.5) * np.sqrt(e2) * UP + f32(2.0**-60)
    B = np.zeros(K, dtype=np.float16)
    B[:d] = m2
    B[dp:dp + 3] = 1.0
    B[dp + 3:dp + 6] = split3(nb)
    return B, nb, eb


def make_points(kind, d, rs, n, nq):
    """live points and queries of one operand class"""
    if kind == "plain":
        a = rs.normal(size=(n, d))
        b = rs.normal(size=(nq, d))
        b[::2] = a[rs.randint(n, size=len(b[::2]))] + 0.3 * rs.normal(size=(len(b[::2]), d))
    elif kind == "offset":                       # far from the origin, small extent: the centring rounds
        a = -7e4 + 3e3 * rs.normal(size=(n, d))
        b = -7e4 + 3e3 * rs.normal(size=(nq, d))
        b[::2] = a[rs.randint(n, size=len(b[::2]))] + 9e2 * rs.normal(size=(len(b[::2]), d))
    elif kind == "subnormal":                    # every second coordinate lands in the binary16 subnormal range or below it
        width = np.where(np.arange(d) % 2 == 0, 1.0, 10.0 ** rs.uniform(-9, -5, size=d))
        a = rs.normal(size=(n, d)) * width
        b = rs.normal(size=(nq, d)) * width
        b[::2] = a[rs.randint(n, size=len(b[::2]))] + 0.3 * rs.normal(size=(len(b[::2]), d)) * width
    else:                                        # "exact": +- pairs of multiples of 2^-10 below 1: centre 0, sigma 1, residue 0
        assert kind == "exact"
        half_n = rs.randint(-1023, 1024, size=(n // 2, d)) * 2.0**-10
        half_n[0, 0] = 1023 * 2.0**-10           # amax in [0.5, 1): sigma = 1
        a = np.concatenate((half_n, -half_n))
        b = rs.randint(-1023, 1024, size=(nq, d)) * 2.0**-10
        b[::2] = a[rs.randint(n, size=len(b[::2]))] + rs.randint(-200, 201, size=(len(b[::2]), d)) * 2.0**-10
    return a, b


@pytest.mark.parametrize("model", ["reversed", "groups", "tree"])
@pytest.mark.parametrize("kind", ["plain", "offset", "subnormal", "exact"])
@pytest.mark.parametrize("d", [2, 20, 49, 50])
def test_residue_thresholds_are_sound_and_never_wider(d, kind, model):
    rs = np.random.RandomState(1000 * d + len(kind))
    n, nq = 160, 14
    a, b = make_points(kind, d, rs, n, nq)
    c, sigma, xa, ah, namax, ea_max = live_side(a)
    if kind == "exact":
        assert sigma == 1.0 and not c.any() and ea_max <= 2.0**-499
    dp = d + (d & 1)
    K = (dp + 6 + 15) // 16 * 16
    sqrt_k = np.sqrt(f32(K))
    A = live_operand(ah, d, dp, K)
    checked = band = band_old = decided_near = 0
    for j in range(nq):
        if kind in ("plain", "offset") and j & 1:
            # the bound is a triangle inequality: it is attained when the residue points along a' - b'.  Of 80 candidates
            # around a live point keep the one whose query residue is best aligned with that direction
            i0 = rs.randint(n)
            cand = a[i0] + 0.1 * np.abs(a - c).max() * rs.normal(size=(80, d))
            xc = sigma * (cand - c)
            rc = xc.astype(np.float32).astype(np.float16).astype(np.float64) - xc
            vc = xa[i0] - xc
            align = np.abs((rc * vc).sum(axis=1)) / (np.linalg.norm(rc, axis=1) * np.linalg.norm(vc, axis=1))
            b[j] = cand[np.argmax(align)]
        xb = sigma * (b[j] - c)                                   # exact scaled whitened point
        if kind == "exact" or (kind in ("plain", "offset") and j & 1):
            # the binary32 rounding of the exact point itself: no slack from zeta beyond that rounding
            zeta = 2.0**-24 * np.linalg.norm(xb) * (1 + 1e-9)
            bq = xb.astype(np.float32)
        else:
            # the kernel's approximate point: anywhere within zeta (towards a live point, or random)
            zeta = 3e-5 * (np.linalg.norm(xb) + namax)
            direction = xa[rs.randint(n)] - xb if j & 2 else rs.normal(size=d)
            bq = (xb + 0.99 * zeta * direction / max(np.linalg.norm(direction), 1e-300)).astype(np.float32)
        if kind == "exact":
            assert np.array_equal(bq.astype(np.float64), xb)
        assert np.linalg.norm(bq.astype(np.float64) - xb) <= zeta
        B, nb, eb = query_operand(bq, d, dp, K)
        if kind == "exact":
            assert eb == f32(2.0**-60)
        prod = A.astype(np.float64) * B.astype(np.float64)
        dt = mfma_accumulate(prod, model)
        s = seq_dist2(a, b[j])
        order = np.argsort(s)
        # r2 a few ulps on either side of pair distances (the pair itself must not be decided wrongly), and around both
        # edges of the band of those pairs: relative offsets of the size of the band's half-width 2 Delta / (sigma r)
        r2s = []
        for i in (order[0], order[1], order[n // 4], rs.randint(n)):
            for ulps in (-3, -1, 0, 1, 3):
                v = s[i]
                for _ in range(abs(ulps)):
                    v = np.nextafter(v, np.inf if ulps > 0 else -np.inf)
                r2s.append((v, None))
            rel = 2.0 * (ea_max + float(eb) + 1.001 * zeta) / max(sigma * np.sqrt(s[i]), 1e-300)
            r2s += [(s[i] * (1 + t * rel), i if abs(t) > 1 else None) for t in (-1.3, -1.05, -0.95, -0.7, 0.7, 0.95, 1.05, 1.3)
                    if 1 + t * rel > 0]
        for r2, edge_pair in r2s:
            if not r2 > 0:
                continue
            sr = sigma * np.sqrt(r2)
            args = (up32(namax) * UP, nb, up32(zeta), sqrt_k, dn32(sr * (1 - 2.0**-30)) * DN, up32(sr * (1 + 2.0**-30)) * UP)
            lo, hi, ok = thresholds4r(up32(ea_max) * UP + f32(2.0**-100), eb, *args, K)
            lo_old, hi_old, ok_old = thresholds4(*args)
            # tightness: never wider than the worst-case form on the same inputs
            assert lo >= lo_old and hi <= hi_old, (lo, lo_old, hi, hi_old)
            assert ok or not ok_old
            if not ok:
                continue
            assert not (dt[s > r2] <= lo).any(), "certain-hit threshold admitted a miss"
            assert not (dt[s <= r2] > hi).any(), "certain-miss threshold rejected a hit"
            checked += n
            inband = (dt > lo) & (dt <= hi)
            band += int(inband.sum())
            band_old += int(((dt > lo_old) & (dt <= hi_old)).sum())
            if edge_pair is not None:
                decided_near += int(not inband[edge_pair])
    assert checked > 0
    assert band <= band_old
    if kind in ("plain", "offset"):
        # the checks above bite: pairs placed just outside the band's edges were decided, not parked in the band
        assert decided_near > 0
        assert band < 0.75 * band_old, (band, band_old)


def test_c_of_k_is_the_pessimistic_bound():
    """one rounding per product, every partial sum at most S: K 2^-24 S (1 + K 2^-24) (1 + 2^-11) <= c(K) (1 + 2^-9) S"""
    for K in (16, 32, 48, 64, 80, 128, 144, 256, 512):
        need = K * 2.0**-24 * (1 + K * 2.0**-24) * (1 + 2.0**-11)
        assert need <= float(c_of_k(K))
    assert float(c_of_k(64)) < 2.0**-15 / 7
