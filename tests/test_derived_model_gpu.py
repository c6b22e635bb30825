"""Derived parameters of a user model on the GPU (DeviceModel(..., nderived=Q): mlf_user_derive_rows and the routes that hand
out its rows).  The derive kernel against numpy bit for bit in both of its forms; the callbacks; and every device route with
usermodels.gauss_derived against usermodels.gauss under equal seeds: u, L, the counts and the first ndim columns of p are
identical (no route changes its row width), the columns behind them are numpy's on those bits."""
import functools
import os
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from ultranest_amd import devicemodel as dm  # noqa: E402
from ultranest_amd import likelihoods as lk  # noqa: E402
from ultranest_amd import usermodels  # noqa: E402

Q = 3
columns = usermodels.gauss_derived_columns

ONE_DERIVED = r"""
__device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux) {
  q[0] = p[0] * p[d - 1] + aux[0];
}
"""

PRODUCT_DERIVED = r"""
__device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux) {
  q[0] = p[0] * p[1];
}
"""


def _wide(p):
    return np.hstack([p, columns(p)])


@functools.lru_cache(maxsize=None)
def _model(d, nq):
    if nq == 3:
        return usermodels.gauss_derived(d)
    return dm.DeviceModel(d, usermodels.GAUSS_LOGLIKE % 0.1, aux=usermodels.gauss_centers(d), nderived=1, derived_source=ONE_DERIVED)


def _want(m, p):
    if m.nderived == 3:
        return _wide(p)
    return np.hstack([p, (p[:, 0] * p[:, -1] + m.aux[0])[:, None]])


def _rows(n, d, seed=1):
    rs = np.random.RandomState(seed)
    return rs.normal(size=(n, d)) * 10.0 ** rs.uniform(-3, 3, size=(n, d))


# ---- the kernel against numpy ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,nq", [(2, 1), (5, 3), (50, 3), (123, 3), (124, 3)])
def test_derive_equals_numpy_bit_for_bit(d, nq):
    """(124, 3) is the direct form (one thread per row), the others are staged through LDS; d = 5 and 50 do not divide 64;
    (123, 3) is the largest staged shape: 64 * (124 + 4) * 8 = 65536 bytes, exactly the budget"""
    m = _model(d, nq)
    assert (dm._lib.lib().mlf_usermodel_derive_lds_bytes(d, nq) == 0) == (d == 124)
    for n in (0, 1, 63, 64, 65, 130):
        p = _rows(n, d, seed=n + 1)
        before = p.copy()
        out = m.derive(p)
        assert out.shape == (n, d + nq) and out.dtype == np.float64
        assert np.array_equal(out, _want(m, p)), (d, nq, n)
        assert np.array_equal(p, before)


@pytest.mark.parametrize("d", [5, 124])
def test_a_row_gives_the_same_bits_wherever_it_stands(d):
    m = _model(d, 3)
    n = 130
    p = _rows(n, d, seed=3)
    row = _rows(1, d, seed=4)[0]
    places = (0, 63, 64, n - 1)
    p[list(places)] = row
    out = m.derive(p)
    assert np.array_equal(out, _wide(p))
    for k in places:
        assert np.array_equal(out[k], out[0]) and np.array_equal(out[k, :d], row)


@pytest.mark.parametrize("d,n", [(5, 130), (50, 65), (124, 70)])
def test_derive_dev_writes_its_rows_and_nothing_else(d, n):
    import torch
    from ultranest_amd import _lib
    m = _model(d, 3)
    p = _rows(n, d, seed=5)
    dev = torch.device("cuda")
    tp = torch.from_numpy(p).to(dev)
    pad = 4096
    tout = torch.full((n * (d + Q) + pad,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    m.derive_dev(tp.data_ptr(), n, tout.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().mlf_synchronize())
    out = tout.cpu().numpy()
    assert np.array_equal(out[:n * (d + Q)].reshape(n, d + Q), _wide(p))
    assert np.isnan(out[n * (d + Q):]).all()                               # the sentinels behind the last row
    assert np.array_equal(tp.cpu().numpy(), p)                             # the input as it was


def test_handles_of_the_wrong_kind_are_refused():
    from ultranest_amd import _lib
    m = _model(5, 3)
    L = _lib.lib()
    p = _rows(4, 5)
    out = np.empty((4, 8))
    assert L.mlf_usermodel_derive(m.handle(), _lib.ptr(p), 4, _lib.ptr(out)) == 4                 # MLF_E_STATE: no derive handle
    assert L.mlf_usermodel_derive_dev(m.handle(), None, 4, None, None) == 4
    like = np.empty(4)
    assert L.mlf_usermodel_eval(m.derive_handle(), _lib.ptr(p), 4, None, _lib.ptr(like)) == 4     # a derive handle evaluates nothing
    assert np.array_equal(m.derive(p), _wide(p))                                                  # and both still work
    assert np.array_equal(m.loglike(p), usermodels.gauss(5).loglike(p))


# ---- callbacks ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [5, 50])
def test_callbacks(d):
    m, g = usermodels.gauss_derived(d, affine=True), usermodels.gauss(d, affine=True)
    u = np.random.RandomState(6).uniform(size=(130, d))
    p = m.transform(u)
    narrow = g.transform(u)
    assert p.shape == (130, d + Q) and np.array_equal(p[:, :d], narrow)
    assert np.array_equal(p[:, d:], columns(narrow))
    La, Lb, Lc = m.loglike(p), m.loglike(narrow), g.loglike(narrow)
    assert np.array_equal(La, Lb) and np.array_equal(La, Lc) and np.isfinite(La).all()
    assert m.transform(u[:0]).shape == (0, d + Q)


# ---- region refill -----------------------------------------------------------------------------------------------------------

D, N = 5, 200
METHODS = {"MLFriends": ("sample_from_boundingbox", "sample_from_wrapping_ellipsoid", "sample_from_transformed_boundingbox",
                         "sample_from_points"),
           "RobustEllipsoidRegion": ("sample_from_boundingbox", "sample_from_wrapping_ellipsoid"),
           "SimpleRegion": ("sample_from_boundingbox", "sample_from_wrapping_ellipsoid")}


@functools.lru_cache(maxsize=None)
def _pair(d=D):
    return usermodels.gauss_derived(d, affine=True), usermodels.gauss(d, affine=True)


@functools.lru_cache(maxsize=None)
def _live(n=N, d=D):
    u = np.clip(0.5 + 0.1 * np.random.RandomState(21).normal(size=(n, d)), 0.01, 0.99)
    g = _pair(d)[1]
    return u, g.loglike(g.transform(u))


@functools.lru_cache(maxsize=None)
def _region(kind):
    import ultranest_amd.mlfriends as mf
    u = _live()[0]
    layer = mf.AffineLayer()
    layer.optimize(u, u)
    region = getattr(mf, kind)(u, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    return region


def _refill(region, method, nsamples, Lmin, transform, loglike):
    from ultranest_amd.regions import DeviceRNG
    region.device_rng = DeviceRNG(seed=11)
    region.current_sampling_method = getattr(region, method)
    np.random.seed(3)
    return region.refill(nsamples, Lmin, transform, loglike) + (region.device_rng.offset,)


@pytest.mark.parametrize("kind,method,nsamples", [(k, m, 4096) for k in sorted(METHODS) for m in METHODS[k]]
                         + [("MLFriends", "sample_from_wrapping_ellipsoid", 4001)])
def test_region_refill_equals_the_narrow_model(kind, method, nsamples):
    from ultranest_amd import kernels
    m, g = _pair()
    Ls = _live()[1]
    Lmin = np.sort(Ls)[20]
    region = _region(kind)
    calls = []
    orig = kernels.DeviceRegion.refill_user_derived

    def counting(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    kernels.DeviceRegion.refill_user_derived = counting
    try:
        ua, pa, La, nca, oa = _refill(region, method, nsamples, Lmin, m.transform, m.loglike)
        ub, pb, Lb, ncb, ob = _refill(region, method, nsamples, Lmin, g.transform, g.loglike)
        # above every likelihood: no row is kept, and p is still ndim + Q wide
        ue, pe, Le, nce, oe = _refill(region, method, nsamples, 1e300, m.transform, m.loglike)
    finally:
        kernels.DeviceRegion.refill_user_derived = orig
    assert len(calls) == 2
    assert nca == ncb == nce and oa == ob == oe and oa > 0
    assert np.array_equal(ua, ub) and np.array_equal(La, Lb) and (La > Lmin).all()
    assert pa.shape == (len(ua), D + Q) and pb.shape == (len(ua), D)
    assert np.array_equal(pa[:, :D], pb) and np.array_equal(pa[:, D:], columns(pb))
    if method != "sample_from_boundingbox":            # (the cube accepts a handful of 4096 draws at best)
        assert nca > 100 and len(ua) >= 5              # not vacuous: kept rows whose derived columns were compared
    assert pe.shape == (0, D + Q) and ue.shape == (0, D) and Le.shape == (0,)


def test_identity_transform_pairing_yields_no_derived_columns():
    m, g = _pair()
    Ls = g.loglike(_live()[0])
    Lmin = np.sort(Ls)[20]
    region = _region("MLFriends")
    ua, pa, La, nca, oa = _refill(region, "sample_from_wrapping_ellipsoid", 4096, Lmin, lk.identity_transform, m.loglike)
    ub, pb, Lb, ncb, ob = _refill(region, "sample_from_wrapping_ellipsoid", 4096, Lmin, lk.identity_transform, g.loglike)
    assert pa.shape == (len(ua), D) and len(ua) > 50 and np.array_equal(pa, ua)
    assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and np.array_equal(La, Lb) and nca == ncb and oa == ob


def test_a_tregion_on_the_handle_refuses_the_derive_program():
    """the library's own guard (MLFriends.refill never gets there: it returns None for a tregion with such a model)"""
    import test_tregion_routing as TR
    m, g = _pair()
    u = _live()[0]
    region = _region("MLFriends")
    t = TR._tregion(d=D)
    assert _refill(region, "sample_from_wrapping_ellipsoid", 4096, -1e300, g.transform, g.loglike)[3] > 0
    region._dev.sync_tregion(region._dev.handle, t, D)
    with pytest.raises(ValueError, match="t-region"):
        region._dev.handle.refill_user_derived(1, 4096, 11, 0, -1e300, m.handle(True), m.derive_handle(), Q)
    region.current_sampling_method = region.sample_from_wrapping_ellipsoid
    assert region.refill(4096, -1e300, m.transform, m.loglike, tregion=t) is None
    got = _refill(region, "sample_from_wrapping_ellipsoid", 4096, -1e300, m.transform, m.loglike)       # cleared again
    assert got[1].shape[1] == D + Q and len(got[0]) > 50 and u.shape[1] == D


# ---- samplers ----------------------------------------------------------------------------------------------------------------

DS, NS, POP, NSTEPS = 4, 100, 64, 4


def _host_region(u):
    import ultranest_amd.mlfriends as mf
    tl = mf.AffineLayer()
    tl.optimize(u, u)
    return types.SimpleNamespace(u=u, transformLayer=tl, maxradiussq=float(u.shape[1]))


def _sampler(which):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    direction = pop.generate_mixture_random_direction
    if which == "randomwalk":
        return pop.PopulationRandomWalkSampler(POP, NSTEPS, direction, 0.05, device_rng=DeviceRNG(6))
    if which == "simpleslice":
        return pop.PopulationSimpleSliceSampler(POP, NSTEPS, direction, scale_adapt_factor=0.8, max_it=20, device_rng=DeviceRNG(7))
    return pop.PopulationSliceSampler(popsize=POP, nsteps=NSTEPS, generate_direction=direction, scale=0.2,
                                      device_rng=DeviceRNG(5) if which == "slice_philox" else None)


@pytest.mark.parametrize("which", ["randomwalk", "simpleslice", "slice_host_rng", "slice_philox"])
def test_samplers_equal_the_narrow_model(which):
    m, g = _pair(DS)
    u, Ls = _live(NS, DS)
    Lmin = Ls.min() - 1.0
    batched = which in ("randomwalk", "simpleslice")
    region = _host_region(u) if batched else _slice_region()
    runs = []
    for model in (m, g):
        np.random.seed(8)
        s = _sampler(which)
        runs.append([s.__next__(region, Lmin, u, Ls, model.transform, model.loglike) for _ in range(2 * POP)])
    wide, narrow = runs
    npoints = 0
    for (ua, pa, La, nca), (ub, pb, Lb, ncb) in zip(wide, narrow):
        assert nca == ncb and (ua is None) == (ub is None)
        if ua is None:
            continue
        npoints += 1
        assert np.array_equal(ua, ub) and La == Lb
        assert pa.shape == (DS + Q,) and pb.shape == (DS,)
        assert np.array_equal(pa[:DS], pb) and np.array_equal(pa[DS:], columns(pb[None, :])[0])
    assert sum(x[3] for x in wide) > 0
    if batched:
        assert npoints == 2 * POP and wide[0][3] > 0 and wide[POP][3] > 0 and wide[1][3] == 0      # two refills
    else:
        assert npoints >= 1


@functools.lru_cache(maxsize=None)
def _slice_region():
    import ultranest_amd.mlfriends as mf
    u = _live(NS, DS)[0]
    layer = mf.AffineLayer()
    layer.optimize(u, u)
    region = mf.MLFriends(u, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    return region


# ---- harness -----------------------------------------------------------------------------------------------------------------

def _nested(model, **kw):
    from ultranest_amd.harness import StaticNestedSampler
    from ultranest_amd.regions import DeviceRNG
    s = StaticNestedSampler(2, model.loglike, transform=model.transform, num_live_points=100, ndraw=4096, seed=2,
                            device_rng=DeviceRNG(21), **kw)
    return s, s.run(dlogz=0.5)


@functools.lru_cache(maxsize=None)
def _narrow_run():
    return _nested(usermodels.gauss(2))[1]


def test_static_nested_sampler_equals_the_narrow_model(tmp_path):
    from ultranest_amd import kernels
    calls = []
    orig = kernels.DeviceRegion.refill_user_derived

    def counting(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    kernels.DeviceRegion.refill_user_derived = counting
    try:
        s, wide = _nested(usermodels.gauss_derived(2), log_dir=str(tmp_path))
    finally:
        kernels.DeviceRegion.refill_user_derived = orig
    narrow = _narrow_run()
    assert len(calls) >= 1
    assert wide["logz"] == narrow["logz"] and wide["niter"] == narrow["niter"] and wide["ncall"] == narrow["ncall"]
    assert abs(wide["logz"]) < 4 * wide["logzerr"] + 0.15, wide                     # (analytic ln Z = 0)
    # live points, tree and result files carry ndim + Q columns
    assert s.pointpile.pdim == 2 + Q and s.pointpile.udim == 2
    assert np.shape(s.results["samples"])[1] == 2 + Q and len(s.results["paramnames"]) == 2 + Q
    p = np.asarray(s.results["samples"])
    assert np.array_equal(p[:, 2:], columns(p[:, :2]))
    with open(os.path.join(wide["run_dir"], "chains", "equal_weighted_post.txt")) as fh:
        assert len(fh.readline().split()) == 2 + Q
        assert len(fh.readline().split()) == 2 + Q


def test_static_nested_sampler_with_build_tregion_completes():
    """gauss_derived at d = 2: the derived columns p0 + p1 and sum_k p_k coincide, so the driver's wrapping ellipsoid over all
    five columns is singular and (as in the reference) is dropped at every rebuild: no tregion is ever handed on, the batches
    take the derived entry, and the run is the narrow run.  The host sequence with a tregion built is the next test's."""
    from ultranest_amd import harness, kernels
    calls, built = [], []
    orig = kernels.DeviceRegion.refill_user_derived
    orig_update = harness.RegionUpdater.update

    def counting(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    def update(self, *a, **k):
        out = orig_update(self, *a, **k)
        built.append(self.tregion)
        return out

    kernels.DeviceRegion.refill_user_derived = counting
    harness.RegionUpdater.update = update
    try:
        s, wide = _nested(usermodels.gauss_derived(2), build_tregion=True)
    finally:
        kernels.DeviceRegion.refill_user_derived = orig
        harness.RegionUpdater.update = orig_update
    narrow = _narrow_run()
    print("ln Z wide %.6f +- %.3f, narrow %.6f +- %.3f, rebuilds %d" % (wide["logz"], wide["logzerr"], narrow["logz"],
                                                                       narrow["logzerr"], len(built)))
    assert len(built) >= 2 and all(t is None for t in built) and s.updater.tregion is None
    assert len(calls) >= 1
    assert abs(wide["logz"] - narrow["logz"]) <= wide["logzerr"]


def test_static_nested_sampler_with_a_tregion_takes_the_host_sequence():
    """one derived column p0 * p1: the wrapping ellipsoid over (p0, p1, p0 * p1) exists, so every batch takes the host sequence
    through the model's callbacks (transform with the derived column, tregion.inside, likelihood).  The two runs then draw
    from different streams: two independent estimates of ln Z, whose difference has the standard deviation
    sqrt(err_wide^2 + err_narrow^2); three of those is the bound."""
    from ultranest_amd import kernels
    model = dm.DeviceModel(2, usermodels.GAUSS_LOGLIKE % 0.1, aux=usermodels.gauss_centers(2), nderived=1,
                           derived_source=PRODUCT_DERIVED)
    calls = []
    orig = kernels.DeviceRegion.refill_user_derived

    def counting(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    kernels.DeviceRegion.refill_user_derived = counting
    try:
        s, wide = _nested(model, build_tregion=True)
    finally:
        kernels.DeviceRegion.refill_user_derived = orig
    narrow = _narrow_run()
    print("ln Z wide %.6f +- %.3f, narrow %.6f +- %.3f" % (wide["logz"], wide["logzerr"], narrow["logz"], narrow["logzerr"]))
    assert s.updater.tregion is not None and s.updater.tregion.u.shape[1] == 3 and not calls
    assert abs(wide["logz"] - narrow["logz"]) <= 3.0 * np.hypot(wide["logzerr"], narrow["logzerr"])
