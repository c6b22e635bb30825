"""The driver's parameter-space wrapping ellipsoid (tregion) inside the device refill, on the GPU: the gated refill against the
host sequence of harness.refill_samples (sample -> transform -> tregion.inside -> likelihood -> cut) on the same Philox draws,
for the built-in transforms (k_transform_gate) and for user models (the gated mlf_user_rows), fixed dimensions, the device
copy of the tregion following the host object, and an end-to-end run.

Common recipe (`_check`): with DeviceRNG(41) the host sequence; the tregion's enlargement is then set to the median of its
quadratic form over the transformed batch, so that the gate decides about half of the rows; Lmin sits in the widest gap of
the middle tenth of the sorted likelihoods, so that the row count does not hinge on the last bits of L.  With a fresh
DeviceRNG(41) the gated refill must return the host sequence's rows bit for bit (L within 1e-12, as test_philox compares it)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from ultranest_amd import likelihoods as lk  # noqa: E402
from ultranest_amd import usermodels  # noqa: E402

N = 30000      # not a multiple of 64 or 256


def _region_of(kind, u, seed=2):
    import ultranest_amd.mlfriends as m
    layer = m.AffineLayer() if u.shape[1] > 1 else m.ScalingLayer()      # (the affine layer inverts a covariance MATRIX)
    layer.optimize(u, u)
    region = getattr(m, kind)(u, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(seed))
    region.create_ellipsoid()
    return region


def _blob(n, d, seed, width=0.08):
    rng = np.random.RandomState(seed)
    u = 0.5 + width * rng.normal(size=(n, d)) * np.linspace(0.5, 1.5, d)
    return u[np.logical_and(u > 0, u < 1).all(axis=1)]


def _curve():
    """the thin closed-curve live set of test_philox: the wrapping ellipsoid is mostly empty"""
    rng = np.random.RandomState(78)
    t = rng.uniform(0, 2 * np.pi, 400)
    return 0.5 + 0.2 * np.stack([np.cos(t), np.sin(t), np.cos(2 * t), np.sin(2 * t)], axis=1) + 0.02 * rng.normal(size=(400, 4))


def _tregion(p_live, seed=5):
    from ultranest_amd.mlfriends import WrappingEllipsoid
    t = WrappingEllipsoid(np.array(p_live))
    t.enlarge = t.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(seed))
    t.create_ellipsoid()
    return t


def _quadratic_form(tregion, p):
    d = p[:, tregion.variable_dims] - tregion.ellipsoid_center
    return np.einsum('ij,jk,ik->i', d, tregion.ellipsoid_invcov, d)


def _gap_threshold(L):
    """midpoint of the widest gap between adjacent values in the middle tenth of sorted L"""
    s = np.sort(L)
    assert len(s) >= 4, len(s)
    mid = s[int(0.45 * len(s)):int(0.55 * len(s)) + 2]      # at least two values
    i = int(np.argmax(np.diff(mid)))
    assert mid[i + 1] > mid[i]
    return 0.5 * (mid[i] + mid[i + 1])


def _host_sequence(region, method_name, n, transform, loglike, tregion, halve=True):
    """what harness.refill_samples computes on the host; with `halve` the tregion's enlargement is first set to the median of
    its quadratic form over the batch"""
    from ultranest_amd.regions import DeviceRNG
    region.current_sampling_method = getattr(region, method_name)
    region.device_rng = DeviceRNG(41)
    pts = region.sample(n)
    nxt = region.device_rng.offset
    p_host = np.asarray(transform(pts))
    if halve:
        tregion.enlarge = float(np.median(_quadratic_form(tregion, p_host)))
    acc = tregion.inside(p_host)
    if halve:       # a condition on the reference computation: the gate decides something
        assert 0.2 <= 1.0 - acc.mean() <= 0.8, acc.mean()
    L_host = np.asarray(loglike(p_host[acc]))
    return pts, p_host, acc, L_host, nxt


def _gated(region, method_name, n, Lmin, transform, loglike, tregion):
    from ultranest_amd.regions import DeviceRNG
    region.current_sampling_method = getattr(region, method_name)
    region.device_rng = DeviceRNG(41)
    got = region.refill(n, Lmin, transform, loglike, tregion=tregion) if tregion is not None else \
        region.refill(n, Lmin, transform, loglike)
    assert got is not None
    return got + (region.device_rng.offset,)


def _compare(got, host, Lmin, tregion):
    u, p, L, nc, offset = got
    pts, p_host, acc, L_host, nxt = host
    print("accepted by the region %d, by the tregion %d, above Lmin %d; returned %d" % (len(pts), acc.sum(), (L_host > Lmin).sum(), len(u)))
    assert nc == acc.sum()
    assert offset == nxt
    keep = L_host > Lmin
    assert np.array_equal(u, pts[acc][keep]) and np.array_equal(p, p_host[acc][keep])
    assert np.allclose(L, L_host[keep], rtol=1e-12, atol=1e-12)
    assert tregion.inside(p).all()


def _check(region, method_name, transform, loglike, p_live=None, n=N):
    tregion = _tregion(transform(np.asarray(region.u)) if p_live is None else p_live)
    host = _host_sequence(region, method_name, n, transform, loglike, tregion)
    Lmin = _gap_threshold(host[3])
    got = _gated(region, method_name, n, Lmin, transform, loglike, tregion)
    _compare(got, host, Lmin, tregion)
    return got, host, tregion, Lmin


# ---- 1. built-in route -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method_name", ["sample_from_boundingbox", "sample_from_wrapping_ellipsoid",
                                         "sample_from_transformed_boundingbox", "sample_from_points"])
def test_builtin_gated_refill_equals_the_host_sequence(method_name):
    region = _region_of("MLFriends", _blob(400, 4, 77))
    _check(region, method_name, lk.rosenbrock_transform, lk.rosenbrock_loglike)


def test_builtin_gated_refill_of_a_single_ellipsoid_region():
    region = _region_of("RobustEllipsoidRegion", _blob(400, 4, 77))
    _check(region, "sample_from_wrapping_ellipsoid", lk.rosenbrock_transform, lk.rosenbrock_loglike)


def test_builtin_gated_refill_compacts_a_thin_batch_and_evaluates_a_dense_one_in_place():
    thin = _region_of("MLFriends", _curve())
    got, host, _, _ = _check(thin, "sample_from_wrapping_ellipsoid", lk.rosenbrock_transform, lk.rosenbrock_loglike)
    assert 0 < 4 * len(host[0]) < N            # under a quarter accepted by the region: compacted before the evaluation
    dense = _region_of("MLFriends", _blob(400, 4, 77))
    got, host, _, _ = _check(dense, "sample_from_wrapping_ellipsoid", lk.rosenbrock_transform, lk.rosenbrock_loglike)
    assert 4 * len(host[0]) >= N               # evaluated where it was drawn, under the narrowed mask


def test_builtin_gated_refill_of_65_draws():
    region = _region_of("MLFriends", _blob(400, 4, 77))
    got, host, _, _ = _check(region, "sample_from_wrapping_ellipsoid", lk.rosenbrock_transform, lk.rosenbrock_loglike, n=65)
    assert len(got[0]) >= 1


def test_builtin_gated_refill_with_the_identity_transform():
    """tkind 0: the rows are the parameters, no p buffer is written"""
    region = _region_of("MLFriends", _blob(400, 4, 77))
    _check(region, "sample_from_wrapping_ellipsoid", lk.identity_transform, lk.GaussLikelihood(0.5, 0.08, 4))


@pytest.mark.parametrize("kind,d", [("MLFriends", 50), ("RobustEllipsoidRegion", 100), ("RobustEllipsoidRegion", 130)])
def test_builtin_gated_refill_in_more_dimensions(kind, d):
    """d = 50: the headline instance; 100: a matrix above 48 KiB of LDS (its own grant); 130: the thread-per-row form of the
    gate kernel above 128 dimensions.  Around 400 live points in 100 dimensions and more, a draw from the wrapping ellipsoid lies
    further from every live point than they lie from each other, so MLFriends accepts none of 30000; the single-ellipsoid
    region accepts every draw inside the cube and hands the gate kernel a full batch."""
    u = 0.5 + 0.03 * np.random.RandomState(6).normal(size=(400, d))
    region = _region_of(kind, u)
    got, host, _, _ = _check(region, "sample_from_wrapping_ellipsoid", lk.rosenbrock_transform, lk.rosenbrock_loglike)
    assert len(host[0]) >= (40 if kind == "MLFriends" else N // 2) and len(got[0]) >= 5


# ---- 2. user route ---------------------------------------------------------------------------------------------------

def _user_case(which):
    """(model, transform callback, live points, region kind).  400 live points in 70 dimensions: MLFriends accepts about ten of
    30000 draws from its wrapping ellipsoid (none from 100 dimensions on), too few for the recipe's median and gap; from 63
    dimensions on the single-ellipsoid region hands the kernel a full batch"""
    if which == "rosenbrock7":            # staged form with the p buffer
        M = usermodels.rosenbrock(7)
        return M, M.transform, np.clip(0.5 + 0.12 * np.random.RandomState(4).normal(size=(400, 7)), 0.01, 0.99), "MLFriends"
    if which == "funnel51":               # staged, near the LDS budget
        M = usermodels.funnel(51)
        return M, M.transform, 0.5 + 0.03 * np.random.RandomState(5).normal(size=(400, 51)), "MLFriends"
    if which == "rosenbrock70":           # direct form
        M = usermodels.rosenbrock(70)
        return M, M.transform, 0.5 + 0.03 * np.random.RandomState(7).normal(size=(400, 70)), "RobustEllipsoidRegion"
    if which in ("funnel63", "funnel64"):  # the last staged and the first direct d with a p buffer
        d = int(which[6:])
        M = usermodels.funnel(d)
        return M, M.transform, 0.5 + 0.03 * np.random.RandomState(5).normal(size=(400, d)), "RobustEllipsoidRegion"
    if which == "rosenbrock4_65draws":    # a second, partial wave (the live set of test_builtin_gated_refill_of_65_draws)
        M = usermodels.rosenbrock(4)
        return M, M.transform, _blob(400, 4, 77), "MLFriends"
    if which == "gauss1":                 # d = 1: the staging steps by 64 rows and 0 columns
        M = usermodels.gauss(1, affine=True)
        return M, M.transform, _blob(400, 1, 77), "MLFriends"
    M = usermodels.gauss(7)               # no transform: no p buffer
    return M, lk.identity_transform, np.clip(0.5 + 0.12 * np.random.RandomState(4).normal(size=(400, 7)), 0.01, 0.99), "MLFriends"


@pytest.mark.parametrize("which", ["rosenbrock7", "funnel51", "rosenbrock70", "gauss7_identity", "funnel63", "funnel64",
                                   "rosenbrock4_65draws", "gauss1"])
def test_user_gated_refill_equals_the_host_sequence(which):
    from ultranest_amd import kernels
    M, transform, u, kind = _user_case(which)
    region = _region_of(kind, u)
    calls = []
    orig = kernels.DeviceRegion.refill_user

    def counting(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    kernels.DeviceRegion.refill_user = counting
    try:
        _check(region, "sample_from_wrapping_ellipsoid", transform, M.loglike, n=65 if which.endswith("65draws") else N)
    finally:
        kernels.DeviceRegion.refill_user = orig
    assert len(calls) == 1


def test_user_and_builtin_gated_rosenbrock_agree_bit_for_bit():
    M, _, u, _ = _user_case("rosenbrock7")
    out = []
    for transform, loglike in [(lk.rosenbrock_transform, lk.rosenbrock_loglike), (M.transform, M.loglike)]:
        region = _region_of("MLFriends", u)
        got, host, _, _ = _check(region, "sample_from_wrapping_ellipsoid", transform, loglike)
        out.append(got)
    (ua, pa, La, nca, oa), (ub, pb, Lb, ncb, ob) = out
    assert nca == ncb and oa == ob and len(ua) > 10
    assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and np.array_equal(La, Lb)


# ---- 3. fixed dimensions ---------------------------------------------------------------------------------------------

FIXED_TRANSFORM = r"""
__device__ void mlf_user_transform(const double *u, double *p, int d, const double *aux, long long naux) {
  for (int k = 0; k + 1 < d; ++k) {
    const double m = u[k] * 20.0;
    p[k] = m + -10.0;
  }
  p[d - 1] = 0.25;
}
"""


def test_fixed_dimension_is_checked_for_equality():
    from ultranest_amd.devicemodel import DeviceModel
    d = 5
    M = DeviceModel(d, usermodels.ROSENBROCK_LOGLIKE, FIXED_TRANSFORM, name="fixed_last")
    region = _region_of("MLFriends", np.clip(0.5 + 0.12 * np.random.RandomState(4).normal(size=(400, d)), 0.01, 0.99))
    p_live = M.transform(np.asarray(region.u))
    assert (p_live[:, -1] == 0.25).all()
    got, host, tregion, Lmin = _check(region, "sample_from_wrapping_ellipsoid", M.transform, M.loglike, p_live=p_live)
    assert tregion.variable_dims is not Ellipsis and not tregion.variable_dims[-1] and tregion.variable_dims[:-1].all()
    assert len(got[0]) > 10
    # live rows that hold ANOTHER constant: nothing passes, nothing comes back, the sampling method is drawn again
    other = p_live.copy()
    other[:, -1] = 0.75
    t2 = _tregion(other)
    t2.enlarge = 1e300
    assert t2.variable_dims is not Ellipsis
    region.sampling_methods = [region.sample_from_points]
    u, p, L, nc, offset = _gated(region, "sample_from_wrapping_ellipsoid", N, Lmin, M.transform, M.loglike, t2)
    assert nc == 0 and len(u) == 0 and len(p) == 0 and len(L) == 0 and offset == host[4]
    assert region.current_sampling_method.__name__ == "sample_from_points"


# ---- 4. neutral gate / 5. the device copy follows the host object ---------------------------------------------------------

@pytest.mark.parametrize("route", ["builtin", "user"])
def test_neutral_gate_changes_nothing(route):
    M, _, u, _ = _user_case("rosenbrock7")
    transform, loglike = (M.transform, M.loglike) if route == "user" else (lk.rosenbrock_transform, lk.rosenbrock_loglike)
    region = _region_of("MLFriends", u)
    Lmin = np.sort(lk.rosenbrock_loglike(lk.rosenbrock_transform(u)))[40]
    plain = _gated(region, "sample_from_wrapping_ellipsoid", N, Lmin, transform, loglike, None)
    tregion = _tregion(transform(np.asarray(region.u)))
    tregion.enlarge = 1e300
    gated = _gated(region, "sample_from_wrapping_ellipsoid", N, Lmin, transform, loglike, tregion)
    assert plain[3] == gated[3] > 0 and plain[4] == gated[4] and len(plain[0]) > 10
    assert all(np.array_equal(a, b) for a, b in zip(plain[:3], gated[:3]))


@pytest.mark.parametrize("route", ["builtin", "user"])
def test_device_copy_follows_update_center_and_is_cleared(route):
    M, _, u, _ = _user_case("rosenbrock7")
    transform, loglike = (M.transform, M.loglike) if route == "user" else (lk.rosenbrock_transform, lk.rosenbrock_loglike)
    region = _region_of("MLFriends", u)
    got, host, tregion, Lmin = _check(region, "sample_from_wrapping_ellipsoid", transform, loglike)
    # re-centred as the driver does after a replacement: the next gated refill is the host sequence with the shifted centre
    tregion.update_center(np.asarray(tregion.ellipsoid_center) + 0.3 * np.sqrt(np.diag(tregion.ellipsoid_cov)))
    host2 = _host_sequence(region, "sample_from_wrapping_ellipsoid", N, transform, loglike, tregion, halve=False)
    assert not np.array_equal(host2[2], host[2]) and host2[2].sum() >= 40
    Lmin2 = _gap_threshold(host2[3])
    _compare(_gated(region, "sample_from_wrapping_ellipsoid", N, Lmin2, transform, loglike, tregion), host2, Lmin2, tregion)
    # without a tregion the same region refills ungated again
    fresh = _region_of("MLFriends", u)
    want = _gated(fresh, "sample_from_wrapping_ellipsoid", N, Lmin2, transform, loglike, None)
    again = _gated(region, "sample_from_wrapping_ellipsoid", N, Lmin2, transform, loglike, None)
    assert want[3] == again[3] and want[4] == again[4] and again[3] > host2[2].sum()
    assert all(np.array_equal(a, b) for a, b in zip(want[:3], again[:3]))


def test_a_user_model_of_the_other_variant_is_refused():
    """The two variants of the wrapper kernel differ in their parameter lists.  A refill with a t-region on the handle and a
    model loaded ungated, or the reverse, is an error with a message, and so is a code object loaded as the variant it was not
    compiled as: none of them launches."""
    from ultranest_amd import devicemodel as dm
    M, _, u, _ = _user_case("rosenbrock7")
    region = _region_of("MLFriends", u)
    tregion = _tregion(M.transform(np.asarray(region.u)))
    got = _gated(region, "sample_from_wrapping_ellipsoid", N, -1e300, M.transform, M.loglike, tregion)
    assert got[3] > 0
    handle = region._dev.handle       # the t-region is set on it
    with pytest.raises(ValueError, match="the region has a t-region"):
        handle.refill_user(1, N, 41, 0, -1e300, M.handle(True))
    handle.clear_tregion()
    with pytest.raises(ValueError, match="the region has no t-region"):
        handle.refill_user(1, N, 41, 0, -1e300, M.handle(True, gated=True))
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(M.code, 7, True, M.aux, gated=True)
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(dm.compile_model(M.source, True, gated=True), 7, True, M.aux)
    assert len(handle.refill_user(1, N, 41, 0, -1e300, M.handle(True))[0]) >= got[3]       # the handle still works, ungated


# ---- 6. end to end ---------------------------------------------------------------------------------------------------

def test_nested_sampling_with_the_tregion_on_the_device(monkeypatch):
    """d = 4 Gaussian (sigma 0.1, normalised) under the prior u * 20 - 10: analytic ln Z = -4 ln 20; every refill is a gated
    user refill, none falls to the host sequence"""
    from ultranest_amd import harness, kernels, regions
    from ultranest_amd.harness import StaticNestedSampler
    from ultranest_amd.regions import DeviceRNG
    G = usermodels.gauss(4, affine=True)
    gated, host_route = [], []
    orig = kernels.DeviceRegion.refill_user
    orig_sync = regions._DeviceState.sync_tregion

    def counting(self, *a, **k):
        gated.append(self._tregion_set)
        return orig(self, *a, **k)

    def sync(self, handle, tregion, ndim):
        orig_sync(self, handle, tregion, ndim)
        handle._tregion_set = self.tregion is not None

    def no_host_sample(self, *a, **k):
        host_route.append(1)
        raise AssertionError("the host sequence ran")

    monkeypatch.setattr(kernels.DeviceRegion, "refill_user", counting)
    monkeypatch.setattr(regions._DeviceState, "sync_tregion", sync)
    monkeypatch.setattr(regions.MLFriends, "sample", no_host_sample)
    s = StaticNestedSampler(4, G.loglike, transform=G.transform, build_tregion=True, num_live_points=400, ndraw=4096,
                            device_rng=DeviceRNG(21))
    res = s.run(dlogz=0.5)
    want = -4 * np.log(20.0)
    print(res, want, len(gated))
    assert abs(res["logz"] - want) < 4 * res["logzerr"] + 0.15, (res, want)
    assert sum(gated) >= 10 and all(gated) and not host_route
    assert s.updater.tregion is not None and s.phases["refills"] == len(gated)
