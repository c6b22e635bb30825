"""k_prep_sweep (csrc/mlf_fused.hip) at small sizes, every path of its per-proposal stage: the phased min-only routing is forced
for batches of a few hundred proposals, and the masks are held to the exact scan (filter = 0) and to the CPU oracle.

What the shapes are for (DP = the padded dimension of the instantiation, NS = its 16-column steps):
  d = 50  DP = 50, NS = 4, the last step holds 2 real columns; d == DP
  d = 49  the same instantiation with d < DP: the padding selects on k < d, a row pitch that is no multiple of 16 bytes
  d = 48  DP = 48, no ragged step
  d = 34  DP = 36 (there is no instantiation for 34): NS = 3, two padded columns
  d = 18  DP = 18, NS = 2, the last step holds 2 real columns
  d = 2   the smallest DP
  517 proposals = four full sets of 4 x 32 and a partial group: one workgroup has empty waves, one group ends behind the batch;
  33 = one full group and one proposal.
The router takes the phased route only from 16 live-point tiles on (mlf_route.hip: every range at least 4 tiles), so with 96 and
200 live points (3 and 7 tiles) the same options lead to the single sweep: those sizes are compared all the same, and N = 520
(17 tiles, the last one with 8 rows) is where the first launch is k_prep_sweep -- asserted through the batch counters.  Its
own tile range there is 5 tiles by default; "filter_first_range_pct" makes it 7 and 13 (no range is shorter than 4 tiles, so
3 cannot be had, and the partial last tile always belongs to a later launch).
The first-index entry never takes the min-only route (it needs the index, not the minimum); its answers are compared with the
oracle's on the same batches, so that both entries are pinned on these shapes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTIONS = {"filter": 1, "filter_min_queries": 32, "filter_phases": 1, "filter_phase_min_queries": 32, "mid_max_queries": 0}
DEFAULTS = {"filter": 1, "filter_min_queries": 257, "filter_phases": 1, "filter_phase_min_queries": 32768, "mid_max_queries": 2048}


@pytest.fixture(scope="module")
def forced():
    from ultranest_amd import _lib
    assert _lib.device_count() >= 1
    for k, v in OPTIONS.items():
        _lib.set_option(k, v)
    yield _lib
    for k, v in DEFAULTS.items():
        _lib.set_option(k, v)
    _lib.set_option("fused_variant", 3)


def _region(d, n, shifted, seed=0):
    """AffineLayer fitted to ONE cluster: the wrapping ellipsoid has the layer's quadratic form (k_prep_sweep<.., SQ>);
    shifted: the ellipsoid's centre moved by one ulp, which must switch that form off."""
    import ultranest_amd.mlfriends as m
    rs = np.random.RandomState(1000 * d + n + seed)
    u = 0.5 + 0.05 * rs.normal(size=(n, d)) * np.linspace(0.5, 1.5, d)
    layer = m.AffineLayer()
    layer.optimize(u, u)
    region = m.MLFriends(u, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    if shifted:
        region.ellipsoid_center = region.ellipsoid_center.copy()
        k = min(7, d - 1)
        region.ellipsoid_center[k] = np.nextafter(region.ellipsoid_center[k], 1.0)
    return u, region


def _proposals(region, u, p, seed):
    """a quarter each: just inside and just outside the wrapping ellipsoid (relative offsets 2^-20 ... 2^-40 of the radius, along
    random directions: the band list and both certain sides), next to live points (hits), spread through the ellipsoid"""
    rs = np.random.RandomState(seed)
    n, d = u.shape
    z = rs.normal(size=(p, d))
    zz = z / np.linalg.norm(z, axis=1, keepdims=True)
    off = 2.0 ** -(20 + (np.arange(p) // 4) % 21)
    kind = np.arange(p) % 4
    radius = np.where(kind == 0, 1.0 - off, np.where(kind == 1, 1.0 + off, rs.uniform(size=p) ** (1.0 / d)))
    pts = region.ellipsoid_center + (zz * (region.enlarge ** 0.5 * radius)[:, None]) @ region.ellipsoid_axes_T
    near = kind == 2
    pts[near] = u[rs.randint(n, size=near.sum())] + 1e-3 * region.maxradiussq ** 0.5 * 0.05 * rs.normal(size=(near.sum(), d))
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
    return d_mask.cpu().numpy().astype(bool), stats, idx, handle


@pytest.mark.parametrize("n", [96, 200, 520])
@pytest.mark.parametrize("d", [50, 49, 48, 34, 18, 2])
def test_masks_and_first_indices_on_every_path(d, n, forced):
    from oracle import oracle as orc
    for shifted in (False, True):
        u, region = _region(d, n, shifted)
        layer = region.transformLayer
        for p in (517, 33):
            pts = _proposals(region, u, p, 17 * d + p)
            got, stats, idx, _ = _resident(region, pts, want_index=True)
            if n >= 512:      # 16 tiles or more: the first launch of the batch is k_prep_sweep
                assert stats["range_cuts"][0] > 0, (d, n, p, stats)
                assert stats["same_quadratic_form"] == (0 if shifted else 1), (d, n, p, shifted, stats)
            forced.set_option("filter", 0)
            try:
                exact = region.inside(pts)
            finally:
                forced.set_option("filter", 1)
            gate = orc.inside_ellipsoid(pts, region.ellipsoid_center, region.ellipsoid_invcov, region.enlarge).astype(bool)
            want = orc.region_inside(pts, region.unormed, layer.ctr, layer.T, region.ellipsoid_center, region.ellipsoid_invcov,
                                     region.enlarge, region.maxradiussq).astype(bool)
            assert 0 < gate.sum() < p and 0 < want.sum() < p, (d, n, p, gate.mean(), want.mean())    # every side is populated
            assert np.array_equal(got, exact), (d, n, p, shifted, np.flatnonzero(got != exact)[:5])
            assert np.array_equal(got, want), (d, n, p, shifted, np.flatnonzero(got != want)[:5])
            if n >= 512 and p == 517:      # the launch's own tile range at other lengths: 7 tiles, and all but the last four
                try:
                    for pct, cut in ((42, 7), (90, 13)):
                        forced.set_option("filter_first_range_pct", pct)
                        other, stats, _, _ = _resident(region, pts)
                        assert stats["range_cuts"][0] == cut, (pct, stats)
                        assert np.array_equal(other, want), (d, n, pct, shifted, np.flatnonzero(other != want)[:5])
                finally:
                    forced.set_option("filter_first_range_pct", 30)
            near = orc.find_nearby(region.unormed, orc.affine_transform(pts, layer.ctr, layer.T), region.maxradiussq)
            want_idx = np.where(gate, near, -2)
            assert np.array_equal(idx, want_idx), (d, n, p, shifted, np.flatnonzero(idx != want_idx)[:5])


def test_stamped_launch_returns_monotone_stamps_and_the_same_mask(forced):
    """mlf_region_debug_fused_stamps: the launch that writes stage stamps decides like the one that does not"""
    u, region = _region(50, 520, False)
    pts = _proposals(region, u, 517, 5)
    plain, stats, _, handle = _resident(region, pts)
    assert stats["range_cuts"][0] > 0, stats
    try:
        handle.fused_stamps(0)
        stamped, stats, _, _ = _resident(region, pts)
        st = handle.fused_stamps(None)
    finally:
        handle.fused_stamps(None)
    assert stats["range_cuts"][0] > 0, stats
    assert np.array_equal(stamped, plain)
    assert st is not None and st[0] == 0, st
    seen = [x for x in st if x is not None]
    assert len(seen) >= 8 and all(b > a for a, b in zip(seen, seen[1:])), st
    again, _, _, _ = _resident(region, pts)
    assert np.array_equal(again, plain)


def test_load_store_loop_for_the_tables_gives_the_same_mask(forced):
    """"fused_variant" bit 0 clear: the matrix fragments reach LDS through registers (the A/B form of the table load)"""
    u, region = _region(18, 520, False)
    pts = _proposals(region, u, 517, 6)
    try:
        forced.set_option("fused_variant", 2)
        loop, stats, _, _ = _resident(region, pts)
        assert stats["range_cuts"][0] > 0 and stats["same_quadratic_form"] == 1, stats
    finally:
        forced.set_option("fused_variant", 3)
    dma, _, _, _ = _resident(region, pts)
    assert np.array_equal(loop, dma) and 0 < dma.sum() < len(pts)


def test_pre_gated_first_launch_through_device_sampling(forced):
    """"fused_variant" bit 2: device-side sampling from the wrapping ellipsoid hands k_prep_sweep the cube test in the gate array.
    The live points sit at a corner of the cube, so that about half of the draws fail it; the accepted points equal those of
    the routing with a separate per-proposal stage."""
    import ultranest_amd.mlfriends as m
    from ultranest_amd.regions import DeviceRNG
    from oracle import philox
    d, nsamples = 18, 4000
    rng = np.random.RandomState(418)
    u = 0.965 + 0.012 * rng.normal(size=(2000, d))
    u = u[np.logical_and(u > 0, u < 1).all(axis=1)]
    assert len(u) >= 512          # 16 tiles: the phased route is open
    layer = m.AffineLayer()
    layer.optimize(u, u)
    region = m.MLFriends(u, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=rng)
    region.create_ellipsoid()
    got = {}
    try:
        for phase_min in (32768, 32):
            forced.set_option("filter_phase_min_queries", phase_min)
            region.device_rng = DeviceRNG(77)
            got[phase_min] = region.sample_from_wrapping_ellipsoid(nsamples)
            if phase_min == 32:
                assert region._dev.handle.debug_stats()["range_cuts"][0] > 0
    finally:
        forced.set_option("filter_phase_min_queries", OPTIONS["filter_phase_min_queries"])
    z, _ = philox.ball_points(77, 0, nsamples, d, region.enlarge)
    w = region.ellipsoid_center + np.dot(z, region.ellipsoid_axes_T)
    in_cube = np.logical_and(w > 0, w < 1).all(axis=1)
    assert 0.2 < in_cube.mean() < 0.8, in_cube.mean()
    assert len(got[32]) > 5 and np.array_equal(got[32], got[32768])
    # ... and the oracle's: the restated draws that pass the cube test and the region's membership test, row by row
    from oracle import oracle as orc
    import sampling_reference as S
    ok = in_cube.copy()
    ok[ok] = orc.region_inside(np.ascontiguousarray(w[ok]), region.unormed, layer.ctr, layer.T, region.ellipsoid_center,
                               region.ellipsoid_invcov, region.enlarge, region.maxradiussq).astype(bool)
    assert abs(len(got[32]) - int(ok.sum())) <= 3       # np.dot against the device's FMA chain: a border point may flip
    S.Reference(S.Geometry.of_region(region), 1, nsamples, 77, 0).match(got[32])
    assert np.logical_and(got[32] > 0, got[32] < 1).all()
