"""The device proposal generator (csrc/mlf_sample.hip, csrc/mlf_region_sample.hip) draw by draw against the high-precision
restatement of sampling_reference.py: every accepted row the device returns is matched, in draw order, with the reference's
row of the same draw within 1e-12 * scale; a draw may be absent or present against the reference's verdict only where a
margin of its tests lies within 1e-9 of that test's scale (see that module).

What runs: every instantiation of k_generate_ellipsoid<CH> and k_rows_affine<CH> (CH = 1, 2, 4, 8, 13, 16, 32 <=> d <= 4, 8,
16, 32, 52, 64, 128) on both sides of every class boundary, the d = 1 branch of the magic-number divisions, the chains above
128 dimensions (k_generate_ball -> k_prep -> k_center_and_cube; k_untransform_rows), the fmod branch of rows_times_matrix
in two CH classes, counters across a multiple of 2^32 with a key whose high word is set, and the second trip of
k_scan_counts (more than 262 144 rows) bit for bit.  Each case prints the rows it compared and its undecided draws.

Above 130 dimensions (the last section): method 3 at d = 131, 200, 317, 318, 512 and 1024 -- 317 | 318 is where the 64 staged
rows of k_generate_around_points outgrow the LDS of an MI355X workgroup and k_generate_around_points_wide takes over --, the
two kernels against each other bit for bit below that seam, method 1 at d = 200 and 512, the batches of methods 1 and 2 that
leave no row at these dimensions, and a refill at d = 318.
"""
import functools

import numpy as np
import pytest

from oracle import philox

import loglike_reference as LR
import sampling_reference as S

gpu = pytest.mark.gpu

N = 4133                                    # 64 workgroups of 64 rows and a ragged one of 37
BIG_SEED = 2**63 + 12345
D_ELLIPSOID = (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 52, 53, 64, 65, 127, 128, 129, 130)
D_POINTS = (1, 2, 4, 5, 9, 16, 17, 33, 52, 53, 64, 65, 128, 129)
METHOD_NAME = ("sample_from_boundingbox", "sample_from_wrapping_ellipsoid", "sample_from_transformed_boundingbox",
               "sample_from_points")


# ------------------------------------------------------------------------------------------------ regions
def live_points(d, seed, nlive=None, spread=0.08, centre=0.5, wrapped=False):
    """test_philox._region's live points (about 300 for d <= 65, about 600 above); `wrapped`: axis 0 straddles the 0 / 1 border
    as in test_philox.test_tspace_sampling_with_a_circular_axis"""
    rng = np.random.RandomState(seed)
    n = nlive or (300 if d <= 65 else 600)
    u = centre + spread * rng.normal(size=(n, d)) * np.linspace(0.5, 1.5, d)
    if wrapped:
        u[:, 0] = (0.98 + 0.05 * rng.normal(size=n)) % 1.0
    return u[np.logical_and(u > 0, u < 1).all(axis=1)], rng


def build_region(kind, u, rng, wrapped=False):
    """test_philox._region_of, with the layer of sampling_reference.affine_layer (the same call; d = 1 written out)"""
    import ultranest_amd.mlfriends as m
    region = getattr(m, kind)(u, S.affine_layer(u, [0] if wrapped else []))
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=rng)
    region.create_ellipsoid()
    return region


def device_draw(region, method, n, seed, offset):
    """(accepted rows, next offset) of the public sampling method"""
    from ultranest_amd.regions import DeviceRNG
    region.device_rng = DeviceRNG(seed)
    region.device_rng.offset = offset
    try:
        return getattr(region, METHOD_NAME[method])(n), region.device_rng.offset
    finally:
        region.device_rng = None


def check_draws(region, method, n, seed=1234, offset=0, label=""):
    """reference and caps first, then the device: next offset, every returned row against its draw"""
    ref = S.Reference(S.Geometry.of_region(region), method, n, seed, offset)
    ref.assert_caps()
    got, nxt = device_draw(region, method, n, seed, offset)
    assert nxt == ref.next_offset
    undecided, compared = ref.match(got)
    assert compared == len(got) and ref.decided_in <= compared <= ref.decided_in + undecided
    print("%s method %d d=%d n=%d: %d rows compared, %d undecided draws" % (label, method, region.u.shape[1], n, compared, undecided))
    return ref, got


# ------------------------------------------------------------------------------------------------ method 1
@gpu
@pytest.mark.parametrize("d", D_ELLIPSOID)
def test_wrapping_ellipsoid_draws_of_an_ellipsoid_region(d):
    """nearly every draw is returned, so nearly every draw is checked; d = 129, 130: the three-kernel chain"""
    u, rng = live_points(d, 100 + d)
    ref, got = check_draws(build_region("RobustEllipsoidRegion", u, rng), 1, N, seed=17 + d, label="ellipsoid region")
    assert (got > 0).all() and (got < 1).all()


@gpu
@pytest.mark.parametrize("d", [2, 8, 17])
def test_wrapping_ellipsoid_draws_of_a_friends_region(d):
    u, rng = live_points(d, 500 + d)
    check_draws(build_region("MLFriends", u, rng), 1, N if d < 17 else 5 * N, seed=3 * d, label="friends region")


@gpu
@pytest.mark.parametrize("d", [4, 50])
def test_wrapping_ellipsoid_draws_in_a_corner(d):
    """live points around 0.93 (test_philox's fused-launch region): the cube margin decides a large share of the draws"""
    rng = np.random.RandomState(400 + d)
    u = 0.93 + (0.03 if d == 4 else 0.025) * rng.normal(size=(600, d))      # (d = 50 at 0.03: 184 of 4133 draws in the cube)
    u = u[np.logical_and(u > 0, u < 1).all(axis=1)]
    region = build_region("MLFriends" if d == 4 else "RobustEllipsoidRegion", u, rng)
    ref, got = check_draws(region, 1, N, seed=77, label="corner")
    g = S.Geometry.of_region(region)
    w, ws, _ = S.ellipsoid_draws(g, 77, 0, N)
    in_cube = S.cube_verdict(S.REFERENCE, w, ws) == S.IN
    assert 0.02 < in_cube.mean() < 0.98, in_cube.mean()


# ------------------------------------------------------------------------------------------------ method 3
def points_region(d, wrapped=False):
    """Method 3 keeps a draw with probability 1 / multiplicity: in few dimensions the balls of test_philox._region's Gaussian
    cloud of 300 overlap dozens of times and 4133 draws leave fewer than 200 rows (128 at d = 4, 155 at d = 5).  So up to 9
    dimensions there are 80 live points, and below 4 they are spread evenly, which keeps the bootstrapped radius near the
    spacing."""
    if d >= 4:
        u, rng = live_points(d, 300 + d, nlive=80 if d <= 9 else None, wrapped=wrapped)
    else:
        rng = np.random.RandomState(300 + d)
        u = rng.uniform(0.2, 0.8, size=(60 if d == 1 else 150, d))
    return build_region("MLFriends", u, rng, wrapped=wrapped)


def one_ball_region(d, seed):
    """Method 2 draws in the bounding box of the live points padded by the radius and keeps what lies in some ball: never
    more than V_d / 2^d of the batch (16 % at d = 5, 0.64 % at d = 9), and far less for the cloud of test_philox._region
    (30 of 40 000 at d = 9).  The bound is approached where the radius dwarfs the cloud, so that the union of the balls is
    nearly one ball: 60 live points within 0.01 of the centre, radius and enlargement set by hand as the driver sets them."""
    u, rng = live_points(d, seed, nlive=60, spread=0.005)
    region = build_region("MLFriends", u, rng)
    region.maxradiussq, region.enlarge = 200.0, 400.0
    return region


@gpu
@pytest.mark.parametrize("d", D_POINTS)
def test_draws_around_the_live_points(d):
    """k_generate_around_points and k_rows_affine<CH>; d = 129: k_untransform_rows"""
    ref, got = check_draws(points_region(d), 3, N, seed=31 + d, label="around points")
    assert len(np.unique(ref.which)) > 50


@gpu
@pytest.mark.parametrize("d", [5, 17])
def test_draws_around_the_live_points_with_a_circular_axis(d):
    """the fmod branch of rows_times_matrix in two CH classes"""
    region = points_region(d, wrapped=True)
    assert (region.u[:, 0] < 0.2).any() and (region.u[:, 0] > 0.8).any()
    ref, got = check_draws(region, 3, N, seed=9, label="circular axis")
    assert (got[:, 0] < 0.2).any() and (got[:, 0] > 0.8).any()       # both sides of the cut are populated


# ------------------------------------------------------------------------------------------------ method 2
@gpu
@pytest.mark.parametrize("d", [1, 2, 5, 9])
def test_draws_in_the_transformed_bounding_box(d):
    region = points_region(d) if d < 9 else one_ball_region(d, 209)
    g = S.Geometry.of_region(region)
    n = N if S.Reference(g, 2, N, 23, 77).decided_in >= 200 else 40000
    check_draws(region, 2, n, seed=23, offset=77, label="t-space box")


# ------------------------------------------------------------------------------------------------ counters and keys
@functools.lru_cache(maxsize=None)
def counter_region(method):
    """2069 draws have to leave 200 rows: of the unit cube (method 0) in a wide cloud only, of the padded box (method 2) in
    a region of one ball only"""
    if method == 2:
        return one_ball_region(5, 906)
    u, rng = live_points(5, 905, nlive=80, spread=0.2 if method == 0 else 0.08)
    return build_region("MLFriends", u, rng)


@gpu
@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_counter_and_key_words_beyond_32_bits(method):
    """seed with its high word set; draw 1000 of 2069 starts at counter 2^32 (methods 0 and 2: two elements per block, so the
    batch's block 2500 does)"""
    d, n = 5, 2069
    region = counter_region(method if method in (0, 2) else 1)
    per = {1: (d + 1) // 2 + 1, 3: (d + 1) // 2 + 2}.get(method)
    offset = 2**32 - (per * 1000 if per else d * 1000 // 2)
    if method:
        ref, got = check_draws(region, method, n, seed=BIG_SEED, offset=offset, label="counters")
        assert ref.next_offset > 2**32
        return
    pts, nxt = philox.cube_points(BIG_SEED, offset, n, d)
    want = pts[region.inside(pts)]
    got, got_nxt = device_draw(region, 0, n, BIG_SEED, offset)
    assert got_nxt == nxt and nxt > 2**32 and len(want) >= 200
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ compaction
NSCAN = 262144 + 256 + 1        # nblk = 1026 blocks of 256 rows: two per thread of k_scan_counts, the last threads own none


@functools.lru_cache(maxsize=None)
def scan_case(d, thin):
    """(region, the Philox batch, its accepted rows by region.inside, next offset)"""
    rng = np.random.RandomState(700 + d + 10 * thin)
    u = 0.5 + (0.012 if thin else 0.2) * rng.normal(size=(200, d))
    region = build_region("MLFriends", u[np.logical_and(u > 0, u < 1).all(axis=1)], rng)
    pts, nxt = philox.cube_points(41, 5, NSCAN, d)
    want = pts[region.inside(pts)]
    want.setflags(write=False)
    return region, want, nxt


@gpu
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("thin", [False, True])
def test_compaction_past_one_scan_trip_is_exact(d, thin):
    """method 0 has a bit-exact reference; a lost, repeated or misplaced 256-row block shows in array_equal"""
    region, want, nxt = scan_case(d, thin)
    assert len(want) > 1000
    got, got_nxt = device_draw(region, 0, NSCAN, 41, 5)
    assert got_nxt == nxt
    assert got.shape == want.shape and np.array_equal(got, want)
    # truncation inside a block: the exact prefix
    cap = len(want) - 300
    part, part_nxt = region._dev.sync(region, True).sample(0, NSCAN, 41, 5, capacity=cap)
    assert part_nxt == nxt and part.shape == (cap, d) and np.array_equal(part, want[:cap])
    print("compaction d=%d thin=%d n=%d: %d rows compared bit for bit, 0 undecided draws" % (d, thin, NSCAN, len(got) + len(part)))


@gpu
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("thin", [False, True])
def test_refill_past_one_scan_trip_is_the_host_pipeline(d, thin):
    """region.refill with the built-in identity transform and Gaussian likelihood: more than a quarter of the batch accepted
    -> evaluated where it was drawn; less -> compacted first.  u and p are the host pipeline's rows exactly, L within
    1e-12 * scale of the long double Gaussian."""
    from ultranest_amd import likelihoods
    from ultranest_amd.regions import DeviceRNG
    region, want, nxt = scan_case(d, thin)
    assert (4 * len(want) < NSCAN) == thin and len(want) > 1000          # the route this case takes
    sigma = 0.1
    loglike = likelihoods.GaussLikelihood(0.5, sigma, d)
    L = LR.Reference("gauss", want, loglike.centers, sigma, with_mpmath=False)
    order = np.sort(L.ref)
    Lmin = float((order[len(order) // 2] + order[len(order) // 2 + 1]) / 2)
    clear = np.abs(L.ref - Lmin) > S.BAND * L.scale
    assert clear.all(), "a likelihood within 1e-9 * scale of the threshold: choose another Lmin"
    keep = L.ref > Lmin
    region.device_rng = DeviceRNG(41)
    region.device_rng.offset = 5
    region.current_sampling_method = region.sample_from_boundingbox
    try:
        u, p, Lgot, nc = region.refill(NSCAN, Lmin, likelihoods.identity_transform, loglike)
        assert region.device_rng.offset == nxt and nc == len(want)
    finally:
        region.device_rng = None
    assert u.shape == (int(keep.sum()), d) and np.array_equal(u, want[keep]) and np.array_equal(p, want[keep])
    err = np.abs(Lgot.astype(L.ref.dtype) - L.ref[keep]).astype(np.float64)
    assert (err <= LR.RTOL * L.scale[keep]).all(), float((err / L.scale[keep]).max())
    print("refill d=%d thin=%d n=%d: %d rows compared, 0 undecided draws" % (d, thin, NSCAN, len(u)))


# ------------------------------------------------------------------------------------------------ 131 ... 1024 dimensions
NW = 449                                    # seven workgroups of 64 rows and a ragged one of 1
D_POINTS_WIDE = (131, 200, 317, 318, 512)   # 317 | 318: the last row width k_generate_around_points stages in the 160 KiB of LDS
                                            # of an MI355X workgroup, and the first of k_generate_around_points_wide


@functools.lru_cache(maxsize=None)
def wide_region(kind, d, nlive=None):
    """Above 130 dimensions the cloud of live_points (spread 0.08) and the bootstrap of build_region decide nothing in: the
    bootstrapped enlargement of 700 live points cuts off 446 of 449 method 3 draws at d = 131 and 324 at d = 200 (the
    reference alone, on the CPU).  So: spread 0.02, 700 live points up to d = 318 and 1100 above, and radius and enlargement set
    by hand, as the driver sets them -- radius^2 = 1.05 x the largest nearest-neighbour distance^2, enlargement = 6 x the
    largest Mahalanobis value of a live point.  With these the reference decides 449 of 449 method 3 draws in and leaves
    none undecided at every dimension used here (assert_caps, below, on the region itself), every method 1 draw of the
    ellipsoid alone in, and no method 1 or method 2 draw of the MLFriends region in."""
    import ultranest_amd.mlfriends as m
    u, rng = live_points(d, 600 + d, nlive=nlive or (700 if d <= 318 else 1100), spread=0.02)
    region = getattr(m, kind)(u, S.affine_layer(u))
    t = region.unormed
    norm2 = (t * t).sum(axis=1)
    dist2 = norm2[:, None] + norm2[None, :] - 2 * np.dot(t, t.T)
    np.fill_diagonal(dist2, np.inf)
    region.maxradiussq = 1.05 * float(dist2.min(axis=1).max()) if region._uses_scan() else 1e300
    region.enlarge = 1.0                    # (create_ellipsoid does not read it; it only wants it set)
    region.create_ellipsoid()
    dl = u - region.ellipsoid_center
    region.enlarge = 6 * float((np.dot(dl, region.ellipsoid_invcov) * dl).sum(axis=1).max())
    return region


@gpu
@pytest.mark.parametrize("d", D_POINTS_WIDE)
def test_draws_around_the_live_points_above_130_dimensions(d):
    """k_generate_around_points up to d = 317 and k_generate_around_points_wide from 318 on; k_untransform_rows"""
    ref, got = check_draws(wide_region("MLFriends", d), 3, NW, seed=31 + d, label="around points, wide")
    assert len(np.unique(ref.which)) > 50 and ref.decided_in == NW


@gpu
@pytest.mark.parametrize("d", [200, 512])
def test_wrapping_ellipsoid_draws_above_130_dimensions(d):
    """k_generate_ball -> k_prep wide -> k_center_and_cube"""
    ref, got = check_draws(wide_region("RobustEllipsoidRegion", d), 1, NW, seed=17 + d, label="ellipsoid region, wide")
    assert (got > 0).all() and (got < 1).all()


@gpu
@pytest.mark.parametrize("d", [1, 2, 3, 5, 64, 129, 256, 257, 317])
def test_the_two_forms_of_the_draws_around_the_live_points_are_one_function(d):
    """k_generate_around_points_wide below the LDS limit, where the staged kernel runs (the library's test hook sends the
    batch through it): the same rows and the same offset, bit for bit.  d = 1 ... 3: fewer columns than the four lanes that
    add up |z|^2; 256 | 257: one piece of the row, and one more column; an odd d: the unused sine of the last pair."""
    from ultranest_amd import _lib
    region = points_region(d) if d <= 129 else wide_region("MLFriends", d)
    n = N if d <= 129 else NW
    staged, nxt = device_draw(region, 3, n, 31 + d, 3)
    _lib.around_points_wide(True)
    try:
        wide, wide_nxt = device_draw(region, 3, n, 31 + d, 3)
    finally:
        _lib.around_points_wide(False)
    assert len(staged) > 50 and wide_nxt == nxt
    assert wide.shape == staged.shape and np.array_equal(wide, staged)
    print("two forms method 3 d=%d n=%d: %d rows compared bit for bit" % (d, n, len(staged)))


def check_no_draws(region, method, n, seed, offset, label):
    """a batch of which the reference decides every draw out: no row, and the reference's next offset"""
    ref = S.Reference(S.Geometry.of_region(region), method, n, seed, offset)
    assert ref.decided_in == 0 and ref.undecided == 0, (ref.decided_in, ref.undecided)
    got, nxt = device_draw(region, method, n, seed, offset)
    assert nxt == ref.next_offset and got.shape == (0, region.u.shape[1]), got.shape
    print("%s method %d d=%d n=%d: 0 rows compared (0 decided in), 0 undecided draws" % (label, method, region.u.shape[1], n))


@gpu
def test_wrapping_ellipsoid_draws_of_a_friends_region_at_200_dimensions():
    """a uniform draw of the ellipsoid lies in no ball at this dimension"""
    check_no_draws(wide_region("MLFriends", 200), 1, NW, 17, 0, "friends region, wide")


@gpu
@pytest.mark.parametrize("d", [129, 318])
def test_draws_in_the_transformed_bounding_box_above_128_dimensions(d):
    """the padded box leaves the cube and no draw lies in a ball: the generator, the neighbour scan and the empty compaction"""
    check_no_draws(wide_region("MLFriends", d), 2, NW, 23, 77, "t-space box, wide")


@gpu
def test_draws_around_the_live_points_at_the_largest_dimension():
    """d = 1024 = MLF_MAX_DIM, 129 draws.  Whitening all 1300 live points in long double takes half a minute, so the verdicts
    are taken in binary64 on the host, of inputs for which none of them is close: every draw has multiplicity 1 and margins
    of at least 1e-6 of their scales (a thousand bands) to the cube, the ellipsoid and the nearest ball it is not in.  Its OWN
    ball it cannot leave by that much: the draw lies at r U^(1/d) from the live point, a shell of 2 (-ln U) / d of r^2 under the
    surface, and the scale of the test is 2 r (|s_t| + |s_l|) = 17 000 here (the whitened coordinates are sums of 1024 terms
    taken positive), so 1e-6 of it would ask for U < 0.013 in all 129 draws.  The seed is the one of 1000 ... 1199 whose
    largest radial uniform is smallest (0.953): ten bands (1e-8 of the scale) there.  Every draw is then a row of the
    device, compared with the reference restricted to the drawn live points."""
    from ultranest_amd import kernels
    d, n, seed = 1024, 129, 1111
    region = wide_region("MLFriends", d, 1300)
    g = S.Geometry.of_region(region)
    layer, r2 = region.transformLayer, region.maxradiussq
    t64, thin, which, nxt = philox.around_points(seed, 0, n, d, region.unormed, r2)
    mult = np.empty(n, dtype=np.int64)
    kernels.count_nearby(region.unormed, t64, r2, mult)
    assert (mult == 1).all() and (thin < 1).all()
    w64 = layer.untransform(t64)
    assert np.logical_and(w64 > 0, w64 < 1).all() and region.inside_ellipsoid(w64).all()
    t, ts, thin_ref, which_ref, nxt_ref = S.around_draws(g, seed, 0, n)
    assert nxt_ref == nxt and np.array_equal(which_ref, which) and np.array_equal(thin_ref, thin)
    w, ws = S.untransform(S.REFERENCE, g, t, ts)
    # the margins, in the scales of sampling_reference's verdicts
    assert (np.minimum(w64, 1 - w64) >= 1e-6 * ws).all()
    dl = w64 - g.center
    Pd = np.dot(dl, g.invcov)
    ell_scale = 2 * ((ws + np.abs(g.center)) * np.abs(Pd)).sum(axis=1) + (np.dot(np.abs(dl), np.abs(g.invcov)) * np.abs(dl)).sum(axis=1)
    assert (g.enlarge - (Pd * dl).sum(axis=1) >= 1e-6 * ell_scale).all()
    live_scale = np.sqrt((np.dot(np.abs(g.u) + np.abs(g.ctr), np.abs(g.T)) ** 2).sum(axis=1))
    t_scale = np.sqrt((ts ** 2).sum(axis=1))
    for i in range(n):
        dist2 = ((region.unormed - t64[i]) ** 2).sum(axis=1)
        own = np.arange(len(dist2)) == which[i]
        margin = np.where(own, r2 - dist2, dist2 - r2)
        assert (margin >= np.where(own, 1e-8, 1e-6) * (2 * np.sqrt(dist2) * (t_scale[i] + live_scale) + dist2)).all(), i
    got, got_nxt = device_draw(region, 3, n, seed, 0)
    assert got_nxt == nxt and got.shape == (n, d)
    worst = S.excess(got, w, ws)
    print("around points, widest method 3 d=%d n=%d: %d rows compared, 0 undecided draws (largest error %.3g of the tolerance)"
          % (d, n, len(got), worst))
    assert worst <= 1.0


@gpu
@pytest.mark.parametrize("user", [False, True])
def test_refill_around_the_live_points_at_318_dimensions_is_the_host_pipeline(user):
    """region.refill with method 3 on k_generate_around_points_wide, identity transform and a Gaussian likelihood, built in
    and as a user model: u and p are the rows of sample() that the callbacks keep, bit for bit; L within 1e-12 * scale of the
    long double Gaussian, the threshold clear of every value by the band"""
    from ultranest_amd import likelihoods, usermodels
    from ultranest_amd.regions import DeviceRNG
    d, sigma, seed = 318, 0.1, 41
    region = wide_region("MLFriends", d)
    rows, nxt = device_draw(region, 3, NW, seed, 5)
    assert len(rows) > 400
    if user:
        model = usermodels.gauss(d, sigma)
        loglike, centers = model.loglike, usermodels.gauss_centers(d, sigma)
    else:
        loglike = likelihoods.GaussLikelihood(0.5, sigma, d)
        centers = loglike.centers
    L = LR.Reference("gauss", rows, centers, sigma, with_mpmath=False)
    order = np.sort(L.ref)
    Lmin = float((order[len(order) // 2] + order[len(order) // 2 + 1]) / 2)
    assert (np.abs(L.ref - Lmin) > S.BAND * L.scale).all(), "a likelihood within 1e-9 * scale of the threshold: choose another Lmin"
    keep = L.ref > Lmin
    p_host = likelihoods.identity_transform(rows)
    L_host = loglike(p_host)
    assert np.array_equal(L_host > Lmin, keep)
    region.device_rng = DeviceRNG(seed)
    region.device_rng.offset = 5
    region.current_sampling_method = region.sample_from_points
    try:
        u, p, Lgot, nc = region.refill(NW, Lmin, likelihoods.identity_transform, loglike)
        assert region.device_rng.offset == nxt and nc == len(rows)
    finally:
        region.device_rng = None
        if user:
            model.close()
    assert u.shape == (int(keep.sum()), d) and np.array_equal(u, rows[keep]) and np.array_equal(p, p_host[keep])
    err = np.abs(Lgot.astype(L.ref.dtype) - L.ref[keep]).astype(np.float64)
    assert (err <= LR.RTOL * L.scale[keep]).all(), float((err / L.scale[keep]).max())
    print("refill method 3 d=%d user=%d n=%d: %d rows compared, 0 undecided draws" % (d, user, NW, len(u)))
