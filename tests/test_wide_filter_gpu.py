"""The f16 matrix-core pre-filter of MLFriends.inside for 129 ... 1024 dimensions (csrc/mlf_wide_filter.hip) on the GPU: masks
bit-identical to the oracle's and to the exact scan's ("filter" = 0), the filter actually on, deciding rather than handing
the batch to the exact tail, band cases and guard cases reaching the exact scan, row replacement, device-side sampling.

Shapes: n = 333 live points (not a multiple of 32: the sentinel rows of the last tile are swept) at 0.5 + 0.05 N(0, 1), layer
and ellipsoid from cov (d + 2), r2 = the 0.8-quantile of the nearest-neighbour distances among the first 150 whitened live
points.  Above 332 dimensions the covariance is rank deficient (the 1e-6 jitter carries the null directions), so proposals
are built in the whitened space and taken back to the cube through the layer."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_LIVE = 333


@pytest.fixture(scope="module")
def K():
    from ultranest_amd import _lib, kernels
    assert _lib.device_count() >= 1, "no MI355X visible"
    return kernels


def kdim(d):
    dp = (d + 15) // 16 * 16
    return 16 * ((dp + 6 + 15) // 16)


@functools.lru_cache(maxsize=None)
def setup(d, n=N_LIVE):
    """live points, layer, ellipsoid, radius of one dimensionality; shared by the tests, never modified"""
    from ultranest_amd import kernels
    rs = np.random.RandomState(9200 + d + 7 * n)
    u = 0.5 + 0.05 * rs.normal(size=(n, d))
    ctr = u.mean(axis=0)
    cov = np.cov(u, rowvar=0) * (d + 2) + 1e-6 * np.eye(d)
    ev, evec = np.linalg.eigh(cov)
    T = evec * ev ** -0.5
    invT = (evec * ev ** 0.5).T
    inv = np.linalg.inv(cov)
    tl = kernels.affine_transform(u, ctr, T)       # the device whitens the live points with this chain
    m = min(n, 150)
    dd = ((tl[:m, None, :] - tl[None, :m, :]) ** 2).sum(axis=2)
    np.fill_diagonal(dd, np.inf)
    r2 = float(np.quantile(dd.min(axis=1), 0.8))
    out = dict(d=d, n=n, u=u, ctr=ctr, T=T, invT=invT, inv=inv, tl=tl, r2=r2, enlarge=2.0 * d, tstd=float(tl.std()))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def region(K, s, r2=None):
    reg = K.DeviceRegion()
    reg.set(s["u"], 0, s["ctr"], s["T"], None, s["ctr"], s["inv"], s["enlarge"], s["r2"] if r2 is None else r2, live_space=1)
    return reg


def to_cube(s, t):
    return np.ascontiguousarray(t @ s["invT"] + s["ctr"])


def mixed_proposals(s, p, seed):
    """whitened space: jittered live points (near: neighbours; far: none), a Gaussian of the live set's width, and a shell that
    straddles the ellipsoid's enlargement (|t|^2 = q up to the covariance jitter); back to the cube through the layer"""
    rs = np.random.RandomState(seed)
    d, n, tl, sd = s["d"], s["n"], s["tl"], s["tstd"]
    a = tl[rs.randint(n, size=p)] + sd * rs.normal(size=(p, d)) * rs.uniform(0.05, 1.2, size=(p, 1))
    b = sd * 1.3 * rs.normal(size=(p, d))
    z = rs.normal(size=(p, d))
    z /= np.sqrt((z ** 2).sum(axis=1, keepdims=True))
    c = z * np.sqrt(s["enlarge"] * rs.uniform(0.9, 1.1, size=(p, 1)))
    which = (np.arange(p) % 4)[:, None]
    return to_cube(s, np.where(which <= 1, a, np.where(which == 2, b, c)))


@functools.lru_cache(maxsize=None)
def mask_case(d, n=N_LIVE):
    """2049 proposals and the oracle's mask, computed once per dimensionality; the smaller batches are its leading rows"""
    from oracle import oracle
    s = setup(d, n)
    pts = mixed_proposals(s, 2049, 9300 + d)
    want = oracle.region_inside(pts, s["tl"], s["ctr"], s["T"], s["ctr"], s["inv"], s["enlarge"], s["r2"])
    pts.setflags(write=False)
    want.setflags(write=False)
    return pts, want


def inside_both(reg, pts):
    """the mask by the default route and by the exact scan alone"""
    got = reg.inside(pts)
    reg.set_option("filter", 0)
    try:
        exact = reg.inside(pts)
    finally:
        reg.set_option("filter", None)
    return got, exact


@pytest.mark.parametrize("p", [257, 700, 2049])
@pytest.mark.parametrize("d", [129, 144, 200, 256, 515, 1024])
def test_masks_equal_the_oracle_and_the_exact_scan(d, p, K):
    s = setup(d)
    pts, want = mask_case(d)
    pts, want = pts[:p], want[:p]
    reg = region(K, s)
    try:
        assert reg.filter_info(p)[0]
        got, exact = inside_both(reg, pts)
        assert np.array_equal(got, want)
        assert np.array_equal(exact, want)
        assert 0 < want.sum() < p
    finally:
        reg.close()


def test_masks_with_33_live_points(K):
    """two live tiles, the second with one live point and 31 sentinel rows"""
    d, p = 200, 2049
    s = setup(d, 33)
    pts, want = mask_case(d, 33)
    reg = region(K, s)
    try:
        assert reg.filter_info(p) == (True, kdim(d), 2)
        got, exact = inside_both(reg, pts)
        assert np.array_equal(got, want)
        assert np.array_equal(exact, want)
        assert 0 < want.sum() < p
    finally:
        reg.close()


@pytest.mark.parametrize("d", [129, 144, 200, 256, 515, 1024])
def test_the_filter_is_on_above_128_dimensions(d, K):
    reg = region(K, setup(d))
    try:
        for p in (257, 700, 2049):
            assert reg.filter_info(p) == (True, kdim(d), math.ceil(N_LIVE / 32))
        reg.set_option("filter", 0)
        assert reg.filter_info(2049)[0] is False
        reg.set_option("filter", None)
        reg.set_option("filter_min_queries", 5000)
        assert reg.filter_info(2049)[0] is False and reg.filter_info(5000)[0] is True
        reg.set_option("filter_min_queries", None)
    finally:
        reg.close()


@pytest.mark.parametrize("unit", ["live set's spread", "one"])
@pytest.mark.parametrize("d", [200, 1024])
def test_the_filter_decides(d, unit, K):
    """proposals = a live point + N(0, 1) U(0.2, 1.2) in the whitened space -- in units of the live points' own coordinate
    spread (the geometry of tests/test_wide_filter_bounds.py, whose live points have unit spread: there 0 of the proposals'
    minima end in the band) and in units of one (every proposal far from every live point) -- back to the cube through the
    layer.  At most 10 % of the proposals inside the ellipsoid may be left to the exact scan, whether by the sweep (minimum
    in the band) or by the quantising kernel's guards."""
    from oracle import oracle
    s = setup(d)
    rs = np.random.RandomState(9500 + d)
    p = 2000 if d <= 256 else 600            # the oracle's whitening and ellipsoid test cost p d^2
    scale = s["tstd"] if unit != "one" else 1.0
    t = s["tl"][rs.randint(N_LIVE, size=p)] + scale * rs.normal(size=(p, d)) * rs.uniform(0.2, 1.2, size=(p, 1))
    pts = to_cube(s, t)
    delta = pts - s["ctr"]
    in_ell = ((delta @ s["inv"]) * delta).sum(axis=1) <= s["enlarge"]      # a count only: none of them is near the surface
    reg = region(K, s)
    try:
        assert reg.filter_info(p)[0]
        got = reg.inside(pts)
        stats = reg.debug_stats()
        uncertain, to_scan = stats["uncertain_queries"], stats["exact_scan_queries"]
        print("d", d, "unit", unit, "inside the ellipsoid", int(in_ell.sum()), "neighbour found", int(got.sum()), "uncertain", uncertain,
              "left to the exact scan", to_scan)
        assert in_ell.sum() > p // 2
        assert uncertain <= 0.1 * in_ell.sum()
        assert uncertain <= to_scan <= 0.1 * in_ell.sum()      # band queries AND what the quantiser's guards route there
        assert np.array_equal(got, oracle.region_inside(pts, s["tl"], s["ctr"], s["T"], s["ctr"], s["inv"], s["enlarge"], s["r2"]))
    finally:
        reg.close()


def identity_region(K, d, rs):
    """identity layer with centre 0 (the whitening chain fma(x_k - 0, 1, acc) is exact: whitened row = cube row), a loose
    ellipsoid, and live point 0 -- the origin -- far away from all others"""
    u = 0.5 + 0.05 * rs.normal(size=(N_LIVE, d))
    u[0] = 0.0
    dd = ((u[1:151, None, :] - u[None, 1:151, :]) ** 2).sum(axis=2)
    np.fill_diagonal(dd, np.inf)
    r2 = float(np.quantile(dd.min(axis=1), 0.8))
    ctr0, T = np.zeros(d), np.eye(d)
    ell = dict(ctr=u.mean(axis=0), inv=np.eye(d) * 1e-20, enlarge=1.0)
    reg = K.DeviceRegion()
    reg.set(u, 0, ctr0, T, None, ell["ctr"], ell["inv"], ell["enlarge"], r2, live_space=1)
    return reg, u, r2, ctr0, T, ell


def oracle_mask(pts, u, r2, ctr0, T, ell):
    from oracle import oracle
    return oracle.region_inside(pts, u, ctr0, T, ell["ctr"], ell["inv"], ell["enlarge"], r2)


def filler(u, p, rs):
    return u[rs.randint(1, len(u), size=p)] + 0.05 * rs.normal(size=(p, u.shape[1])) * rs.uniform(0.05, 1.2, size=(p, 1))


@pytest.mark.parametrize("d", [200, 1024])
def test_band_cases_reach_the_exact_scan(d, K):
    """proposals at a whitened distance sqrt(r2) (1 +- k 2^-52), k = 0 ... 8, and sqrt(r2) (1 +- 2^-20) from the isolated live
    point: one coordinate differs, so the reference's distance is the rounded square of that coordinate"""
    rs = np.random.RandomState(9600 + d)
    reg, u, r2, ctr0, T, ell = identity_region(K, d, rs)
    try:
        factors = [1.0 + k * 2.0 ** -52 for k in range(9)] + [1.0 - k * 2.0 ** -52 for k in range(1, 9)] + [1 + 2.0 ** -20, 1 - 2.0 ** -20]
        band = np.zeros((len(factors), d))
        band[:, 3] = np.sqrt(r2) * np.array(factors)
        pts = np.concatenate([band, filler(u, 400, rs), -band])
        want = oracle_mask(pts, u, r2, ctr0, T, ell)
        assert want[:len(band)].any() and not want[:len(band)].all()        # both sides of r2 are present
        assert reg.filter_info(len(pts))[0]
        got, exact = inside_both(reg, pts)
        reg.inside(pts)                                                     # debug_stats speaks of the last FILTERED batch
        assert np.array_equal(got, want) and np.array_equal(exact, want)
        assert reg.debug_stats()["uncertain_queries"] >= 2 * len(band) - 4  # all but the +- 2^-20 rows are in the band for certain
    finally:
        reg.close()


def test_guards(K):
    """a coordinate of 1e6 (beyond the binary16 operand, but finite: the quantising kernel's norm test calls it a certain miss
    before its binary16 guard is asked -- only NaN / inf rows still reach that guard and, through it, the exact scan), a NaN row, live points as proposals at a radius far
    below the band's width, r2 = 0 and r2 = 1e300: the exact scan's answer every time"""
    d = 200
    rs = np.random.RandomState(9700)
    reg, u, r2, ctr0, T, ell = identity_region(K, d, rs)
    try:
        pts = np.concatenate([filler(u, 300, rs), u[:40]])
        pts[5, 17] = 1e6
        pts[6, :] = 0.0
        pts[6, 0] = 1e6                      # next to nothing
        pts[9, 3] = np.nan
        pts[11, :] = np.nan
        for radius in (r2, 1e-20, 0.0, 1e300):
            reg.set_thresholds(ell["enlarge"], radius)
            got, exact = inside_both(reg, pts)
            assert np.array_equal(got, exact), radius
            finite = np.isfinite(pts).all(axis=1)
            assert np.array_equal(got[finite], oracle_mask(pts[finite], u, radius, ctr0, T, ell)), radius
            assert not got[~finite].any()
            assert got[300:].all()           # a live point is at distance 0 from itself
        reg.set_thresholds(ell["enlarge"], r2)
        assert reg.filter_info(len(pts))[0]
        reg.set_thresholds(ell["enlarge"], 0.0)
        assert not reg.filter_info(len(pts))[0]
    finally:
        reg.close()


@pytest.mark.parametrize("d", [129, 200])
def test_large_batch_takes_four_query_groups_per_workgroup(d, K):
    """from 65 536 proposals on (2048 groups of 32) and up to 592 columns the sweep stages FOUR query groups per workgroup (148 KB
    of LDS at d = 576; k_wide_sweep<4>): 66 000 proposals, the last group partly filled, against the exact scan alone"""
    s = setup(d)
    p = 66000
    pts = mixed_proposals(s, p, 9900 + d)
    reg = region(K, s)
    try:
        assert reg.filter_info(p) == (True, kdim(d), math.ceil(N_LIVE / 32))
        got, exact = inside_both(reg, pts)
        assert np.array_equal(got, exact)
        assert 0.2 * p < got.sum() < 0.8 * p
        assert reg.debug_stats()["exact_scan_queries"] >= 0
    finally:
        reg.close()


@pytest.mark.parametrize("d", [129, 515])
def test_update_point_then_inside(d, K):
    from oracle import oracle
    s = setup(d)
    pts, _ = mask_case(d)
    pts = pts[:700]
    t = K.affine_transform(pts, s["ctr"], s["T"])
    reg = region(K, s)
    try:
        assert reg.inside(pts[:300]).shape == (300,)         # the operands are built and used before the row changes
        tl2 = s["tl"].copy()
        tl2[7] = t[1]
        reg.update_point(7, pts[1])
        assert reg.filter_info(700)[0]
        want = oracle.region_inside(pts, tl2, s["ctr"], s["T"], s["ctr"], s["inv"], s["enlarge"], s["r2"])
        got, exact = inside_both(reg, pts)
        assert np.array_equal(got, want) and np.array_equal(exact, want)
        assert want[1]
    finally:
        reg.close()


@pytest.mark.parametrize("method", ["sample_from_points", "sample_from_transformed_boundingbox", "sample_from_boundingbox"])
def test_device_side_sampling_is_the_same_with_the_filter_on_and_off(method):
    """the t-space neighbour test of device-side sampling (and the cube-space one) at d = 200"""
    import ultranest_amd.mlfriends as m
    from ultranest_amd import _lib
    from ultranest_amd.regions import DeviceRNG
    d, n = 200, 400
    rs = np.random.RandomState(9800)
    u = np.clip(0.5 + 0.05 * rs.normal(size=(n, d)), 0.01, 0.99)
    layer = m.AffineLayer()
    layer.optimize(u, u)
    reg = m.MLFriends(u, layer)
    un = reg.unormed
    dd = ((un[:150, None, :] - un[None, :150, :]) ** 2).sum(axis=2)
    np.fill_diagonal(dd, np.inf)
    reg.maxradiussq, reg.enlarge = float(np.quantile(dd.min(axis=1), 0.8)), 2.0 * d
    reg.create_ellipsoid()
    rows = {}
    for flt in (1, 0):
        _lib.set_option("filter", flt)
        try:
            reg.device_rng = DeviceRNG(seed=17)
            rows[flt] = np.array(getattr(reg, method)(nsamples=4096))
            if flt:
                assert reg._dev.handle.filter_info(4096)[0]
        finally:
            _lib.set_option("filter", 1)
    print(method, "accepted", len(rows[1]), "of 4096")
    assert np.array_equal(rows[1], rows[0])
    if method == "sample_from_points":
        assert len(rows[1]) > 0
