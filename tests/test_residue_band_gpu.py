"""The pre-filter band from MEASURED binary16 residues (filter_thresholds4r in k_prep_sweep / k_prep4: stats[4] = ea_max from
k_quant_refs, eb per proposal) and k_uncertain's sets sized to the uncertain count, on proposals placed AT the radius.

A third of every batch lies within 2^-9 (relative) of the radius around some live point, in whitened space: that is where a
band that is too narrow decides a pair wrongly.  Masks and first-hit indices are held to the exact scan (filter = 0) and to the
CPU oracle.  The phased routing is forced for small batches (from 16 live-point tiles on the first launch is k_prep_sweep and
the band goes to k_uncertain; with fewer tiles the same options lead to k_prep4 and the single sweep, which uses the same
thresholds).

k_uncertain takes QW = clamp(ceil(groups / 256), 2, 4) groups of 32 per set: up to 16 384 uncertain proposals sets of 64, above
24 576 sets of 128.  Both ends are produced with offsets of 2^-14 of the radius (every such proposal whose other neighbours
are out of reach is uncertain) and read back through debug_stats()["uncertain_queries"]."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTIONS = {"filter": 1, "filter_min_queries": 32, "filter_phases": 1, "filter_phase_min_queries": 32, "mid_max_queries": 0}
DEFAULTS = {"filter": 1, "filter_min_queries": 257, "filter_phases": 1, "filter_phase_min_queries": 32768, "mid_max_queries": 2048}
NPROP = 65536


@pytest.fixture(scope="module")
def forced():
    from ultranest_amd import _lib
    assert _lib.device_count() >= 1
    for k, v in OPTIONS.items():
        _lib.set_option(k, v)
    yield _lib
    for k, v in DEFAULTS.items():
        _lib.set_option(k, v)


def _region(d, n, seed=0):
    import ultranest_amd.mlfriends as m
    rs = np.random.RandomState(977 * d + n + seed)
    u = 0.5 + 0.05 * rs.normal(size=(n, d)) * np.linspace(0.5, 1.5, d)
    layer = m.AffineLayer()
    layer.optimize(u, u)
    region = m.MLFriends(u, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    return u, region


def _live(region):
    """the whitened live points as the device holds them: it whitens region.u itself, with the chain of the proposals (k ascending,
    one fused multiply-add per term), so that pairs within a few ulps of the radius are the same pairs on both sides"""
    from oracle import oracle as orc
    layer = region.transformLayer
    return np.ascontiguousarray(orc.affine_transform(np.ascontiguousarray(region.u, dtype=float), layer.ctr, layer.T))


def _proposals(region, p, seed, near_share=3, rel=2.0**-9, around=None, inward=False):
    """every near_share-th proposal at (1 + delta) x radius from a live point (|delta| <= rel, random direction, whitened space),
    the rest spread through the wrapping ellipsoid; inward: the direction leans towards the centre, which keeps the proposal
    inside the wrapping ellipsoid (in 50 dimensions a random direction leaves it nearly always)"""
    rs = np.random.RandomState(seed)
    layer = region.transformLayer
    t_live = _live(region)
    n, d = t_live.shape
    z = rs.normal(size=(p, d))
    zz = z / np.linalg.norm(z, axis=1, keepdims=True)
    pts = region.ellipsoid_center + (zz * (region.enlarge ** 0.5 * rs.uniform(size=p) ** (1.0 / d))[:, None]) @ region.ellipsoid_axes_T
    near = np.arange(p) % near_share == 0
    k = int(near.sum())
    which = rs.randint(n, size=k) if around is None else np.full(k, around)
    w = rs.normal(size=(k, d))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    if inward:
        w -= t_live[which] / np.linalg.norm(t_live[which], axis=1, keepdims=True)
        w /= np.linalg.norm(w, axis=1, keepdims=True)
    delta = rel * rs.uniform(-1, 1, size=k)
    delta[::7] = 0.0                                   # and some as close to the radius as binary64 puts them
    t = t_live[which] + w * (region.maxradiussq ** 0.5 * (1.0 + delta))[:, None]
    pts[near] = layer.untransform(t)
    return np.ascontiguousarray(pts)


def _resident(region, pts, want_index=False):
    import torch
    handle = region._dev.sync(region, True)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    d_pts = torch.as_tensor(pts, device=dev)
    d_mask = torch.zeros(len(pts), dtype=torch.uint8, device=dev)
    handle.inside_dev(d_pts.data_ptr(), len(pts), d_mask.data_ptr(), stream)
    torch.cuda.synchronize()
    stats = handle.debug_stats()
    idx = None
    if want_index:
        d_idx = torch.zeros(len(pts), dtype=torch.int64, device=dev)
        handle.first_index_dev(d_pts.data_ptr(), len(pts), d_idx.data_ptr(), stream)
        torch.cuda.synchronize()
        idx = d_idx.cpu().numpy()
    return d_mask.cpu().numpy().astype(bool), stats, idx


def _oracle(region, pts):
    from oracle import oracle as orc
    layer = region.transformLayer
    gate = orc.inside_ellipsoid(pts, region.ellipsoid_center, region.ellipsoid_invcov, region.enlarge).astype(bool)
    # the membership mask is the ellipsoid gate and "has a neighbour" (mlfriends.pyx:1186-1211); the scan is the costly part
    # (8 s at 65 536 x 4000 x 50 on one core): eight slices side by side, the C oracle releases the interpreter lock
    from concurrent.futures import ThreadPoolExecutor
    live = _live(region)
    t = np.ascontiguousarray(orc.affine_transform(pts, layer.ctr, layer.T))
    parts = np.array_split(np.arange(len(pts)), 8)
    with ThreadPoolExecutor(8) as ex:
        near = np.concatenate(list(ex.map(lambda rows: orc.find_nearby(live, np.ascontiguousarray(t[rows]), region.maxradiussq), parts)))
    return gate & (near >= 0), np.where(gate, near, -2)


def _check(region, pts, forced, want_index=True):
    got, stats, idx = _resident(region, pts, want_index)
    forced.set_option("filter", 0)
    try:
        exact, _, exact_idx = _resident(region, pts, want_index)
    finally:
        forced.set_option("filter", 1)
    want, want_idx = _oracle(region, pts)
    print("uncertain_queries", stats["uncertain_queries"], "inside", int(want.sum()), "of", len(pts))
    assert 0 < want.sum() < len(pts)
    assert np.array_equal(got, exact), np.flatnonzero(got != exact)[:5]
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]
    if want_index:
        assert np.array_equal(idx, exact_idx), np.flatnonzero(idx != exact_idx)[:5]
        assert np.array_equal(idx, want_idx), np.flatnonzero(idx != want_idx)[:5]
    return stats


@pytest.mark.parametrize("n", [128, 4000])
@pytest.mark.parametrize("d", [2, 20, 49, 50])
def test_masks_and_first_indices_at_the_radius(d, n, forced):
    u, region = _region(d, n)
    pts = _proposals(region, NPROP, 31 * d + n)
    stats = _check(region, pts, forced)
    if n >= 512:      # 16 tiles or more: the first launch of the batch is k_prep_sweep, the band goes to k_uncertain
        assert stats["range_cuts"][0] > 0, stats
        assert stats["uncertain_queries"] > 0, stats


def _small_radius_region():
    """d = 50, 1000 live points, a fifth of the bootstrapped radius: no proposal at the radius of one live point is within reach of
    another, so every one of them that passes the ellipsoid has its nearest pair in the band"""
    u, region = _region(50, 1000)
    region.maxradiussq *= 0.04
    return u, region


def test_sets_of_four_groups_above_16384_uncertain_proposals(forced):
    u, region = _small_radius_region()
    pts = _proposals(region, NPROP, 5, near_share=2, rel=2.0**-14, inward=True)
    stats = _check(region, pts, forced, want_index=False)
    assert stats["range_cuts"][0] > 0, stats
    assert stats["uncertain_queries"] > 24576, stats          # more than 3 x 256 groups: QW = 4


def test_sets_of_two_groups_below_8192_uncertain_proposals(forced):
    u, region = _small_radius_region()
    pts = _proposals(region, NPROP, 6, near_share=16, rel=2.0**-14, inward=True)
    stats = _check(region, pts, forced, want_index=False)
    assert stats["range_cuts"][0] > 0, stats
    assert 1000 < stats["uncertain_queries"] < 8192, stats    # at most 256 groups: QW = 2


def test_row_with_the_largest_residue_replaced(forced):
    """mlf_region_update_points: ea_max is taken again over the rows as they are then.  The row that held the largest binary16
    residue is replaced by a point further out (a larger residue), and the proposals sit at the radius around the NEW row."""
    d, n = 20, 1000
    u, region = _region(d, n)
    pts = _proposals(region, 8192, 3)
    _check(region, pts, forced, want_index=False)                  # the operands of the first set are on the device
    t = _live(region)
    c = t.mean(axis=0)
    sigma = 2.0 ** -np.frexp(np.abs(t - c).max())[1]
    xa = sigma * (t - c)
    res = np.linalg.norm(xa.astype(np.float32).astype(np.float16).astype(np.float64) - xa, axis=1)
    row = int(np.argmax(res))
    centre = region.u.mean(axis=0)
    region.u[row] = centre + 1.2 * (region.u[int(np.argmax(np.linalg.norm(region.u - centre, axis=1)))] - centre)
    assert 0 < region.u[row].min() and region.u[row].max() < 1
    pts = _proposals(region, NPROP, 4, near_share=3, rel=2.0**-11, around=row)
    from ultranest_amd import kernels
    sent = []
    real_rows = kernels.DeviceRegion.update_points

    def counted_rows(self, rows, live_rows):
        sent.append(len(rows))
        return real_rows(self, rows, live_rows)
    kernels.DeviceRegion.update_points = counted_rows
    try:
        stats = _check(region, pts, forced)
    finally:
        kernels.DeviceRegion.update_points = real_rows
    assert sent == [1], sent                                       # the row went through mlf_region_update_points, once
    assert stats["uncertain_queries"] > 0, stats


def test_uncertain_count_of_the_benchmark_batch_is_below_the_parent():
    """the benchmark's region and its batch of seed 1000 (default routing): 23 100 uncertain proposals with the worst-case
    band, 10 804 with the measured residues (MI355X; the count is a function of the inputs, not of the run)"""
    import torch
    import bench
    u, region = bench.build_region(None)
    dev = torch.device("cuda", 0)
    pts = bench.proposals_in_ellipsoid(region, bench.NPROPOSALS, 1000, dev)
    handle = region._dev.sync(region, True)
    mask = torch.zeros(len(pts), dtype=torch.uint8, device=dev)
    handle.inside_dev(pts.data_ptr(), len(pts), mask.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    stats = handle.debug_stats()
    print("uncertain_queries on the benchmark batch:", stats["uncertain_queries"])
    assert 0 < stats["uncertain_queries"] < 23100, stats
