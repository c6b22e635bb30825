"""The t-region gate over a user model's derived parameters on the GPU (DeviceModel(..., nderived=Q, gate_derived=True):
mlf_region_refill_user_derived_gated and the three gate-derived programs) against the host sequence of harness.refill_samples
on the same Philox draws, by the recipe of test_tregion_refill_gpu (`_check`: the t-region is built over all d + Q columns of
the transformed live points, its enlargement set to the median of its quadratic form so that the gate rejects about half of the
rows; u and the (d + Q)-wide p bit for bit, the count and the counter offset equal, L within 1e-12).  The models carry NONLINEAR
derived columns (p0 p1, p_{d-1}^2, exp(p0 / 8)), so that the covariance over the d + Q columns is not singular."""
import contextlib
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_derived_model_gpu as DG  # noqa: E402  (its one-column model and its nested-sampling run)
import test_gate_derived_compile as GC  # noqa: E402  (the models, and the staged / direct boundary pair)
import test_tregion_refill_gpu as TR  # noqa: E402  (the recipe)
import test_tregion_routing as R  # noqa: E402  (a host-built t-region of any width)
from ultranest_amd import devicemodel as dm  # noqa: E402
from ultranest_amd import usermodels  # noqa: E402

N = TR.N
ELL = "sample_from_wrapping_ellipsoid"


@functools.lru_cache(maxsize=None)
def _model(d, nq):
    return GC._default(d, nq)


@contextlib.contextmanager
def _counted():
    """counts the calls of the new entry; the derived entry without a gate must not be called by the new route"""
    from ultranest_amd import kernels
    calls = []
    orig, orig_plain = kernels.DeviceRegion.refill_user_derived_gated, kernels.DeviceRegion.refill_user_derived

    def counting(self, *a, **k):
        calls.append("gated")
        return orig(self, *a, **k)

    def plain(self, *a, **k):
        calls.append("plain")
        return orig_plain(self, *a, **k)

    kernels.DeviceRegion.refill_user_derived_gated = counting
    kernels.DeviceRegion.refill_user_derived = plain
    try:
        yield calls
    finally:
        kernels.DeviceRegion.refill_user_derived_gated = orig
        kernels.DeviceRegion.refill_user_derived = orig_plain


def _check(region, method, M, n=N, **kw):
    with _counted() as calls:
        out = TR._check(region, method, M.transform, M.loglike, n=n, **kw)
    assert calls == ["gated"]
    got, host, tregion, Lmin = out
    assert got[1].shape[1] == M.nparams == np.shape(tregion.u)[1] and got[0].shape[1] == M.ndim
    return out


# ---- the default form ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,nq,method", [(2, 1, ELL), (5, 3, "sample_from_boundingbox"), (5, 3, ELL),
                                         (5, 3, "sample_from_transformed_boundingbox"), (5, 3, "sample_from_points")])
def test_default_form_equals_the_host_sequence(d, nq, method):
    region = TR._region_of("MLFriends", TR._blob(400, d, 77))
    got, host, _, _ = _check(region, method, _model(d, nq))
    assert len(got[0]) >= 5


@pytest.mark.parametrize("d", GC.BOUNDARY)
def test_the_staged_and_the_direct_form_either_side_of_the_budget(d):
    """d = 61, Q = 3: the largest staged pair (64000 bytes of LDS); d = 62: one thread per row, q in the library's scratch.  400
    live points in 60 dimensions: MLFriends accepts next to nothing of a draw from its wrapping ellipsoid; the single-ellipsoid
    region hands the kernel a full batch (as test_tregion_refill_gpu does at d = 70)."""
    assert (dm._lib.lib().mlf_usermodel_gate_derived_lds_bytes(d, 3, 1) != 0) == (d == GC.BOUNDARY[0])
    u = 0.5 + 0.03 * np.random.RandomState(7).normal(size=(400, d))
    region = TR._region_of("RobustEllipsoidRegion", u)
    got, host, _, _ = _check(region, ELL, _model(d, 3))
    assert len(host[0]) >= N // 2 and len(got[0]) >= 5


def test_a_model_without_a_transform_source_gates_its_cube_rows():
    """no p buffer: the rows are the parameters, the transform callback is the identity followed by the derived columns"""
    M = dm.DeviceModel(5, usermodels.GAUSS_LOGLIKE % 0.1, aux=usermodels.gauss_centers(5), nderived=3,
                       derived_source=GC.NONLINEAR_DERIVED, gate_derived=True)
    region = TR._region_of("MLFriends", TR._blob(400, 5, 77))
    got, host, _, _ = _check(region, ELL, M)
    assert len(got[0]) >= 5 and np.array_equal(got[1][:, :5], got[0])


def test_a_second_partial_wave():
    region = TR._region_of("MLFriends", TR._blob(400, 5, 77))
    got, host, _, _ = _check(region, ELL, _model(5, 3), n=65)
    assert len(got[0]) >= 1


def test_a_thin_region_is_compacted_before_the_evaluation():
    region = TR._region_of("MLFriends", TR._curve())
    got, host, _, _ = _check(region, ELL, _model(4, 3))
    assert 0 < 4 * len(host[0]) < N and len(got[0]) >= 5


# ---- the summed forms --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["summed", "multisum"])
def test_summed_forms_equal_the_host_sequence(which):
    """d = 4, Q = 2, K = 130 integer-valued terms (three lanes get a third term): L is exact in any order"""
    M = GC._summed() if which == "summed" else GC._multisum()
    region = TR._region_of("MLFriends", TR._blob(400, 4, 77))
    got, host, _, Lmin = _check(region, ELL, M)
    assert len(got[0]) >= 5 and np.array_equal(got[2], host[3][host[3] > Lmin])


# ---- a constant derived column: a fixed dimension of the t-region -------------------------------------------------------------

CONSTANT_DERIVED = r"""
__device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux) {
  q[0] = p[0] * p[1];
  q[1] = 0.25;
}
"""


def test_a_constant_derived_column_is_checked_for_equality():
    d = 5
    M = dm.DeviceModel(d, usermodels.GAUSS_LOGLIKE % 0.1, usermodels.AFFINE_TRANSFORM, aux=usermodels.gauss_centers(d), nderived=2,
                       derived_source=CONSTANT_DERIVED, gate_derived=True)
    region = TR._region_of("MLFriends", TR._blob(400, d, 77))
    p_live = M.transform(np.asarray(region.u))
    assert p_live.shape == (len(region.u), d + 2) and (p_live[:, -1] == 0.25).all()
    got, host, tregion, Lmin = _check(region, ELL, M, p_live=p_live)
    assert tregion.variable_dims is not Ellipsis and not tregion.variable_dims[-1] and tregion.variable_dims[:-1].all()
    assert len(got[0]) > 10 and (got[1][:, -1] == 0.25).all()
    # the t-region's fixed value one ulp away: nothing passes, nothing comes back, the draws are still the host sequence's
    other = p_live.copy()
    other[:, -1] = np.nextafter(0.25, 1.0)
    t2 = TR._tregion(other)
    t2.enlarge = 1e300
    assert t2.variable_dims is not Ellipsis
    with _counted() as calls:
        u, p, L, nc, offset = TR._gated(region, ELL, N, Lmin, M.transform, M.loglike, t2)
    assert calls == ["gated"]
    assert nc == 0 and len(u) == 0 and p.shape == (0, d + 2) and len(L) == 0 and offset == host[4]


# ---- the device copy follows the host object ---------------------------------------------------------------------------------

def test_update_center_sends_the_centre_alone(monkeypatch):
    from ultranest_amd import kernels
    M = _model(5, 3)
    region = TR._region_of("MLFriends", TR._blob(400, 5, 77))
    sent = []
    orig_set, orig_center = kernels.DeviceRegion.set_tregion, kernels.DeviceRegion.set_tregion_center

    def set_tregion(self, A, ctr, fixed, enlarge, **kw):
        sent.append(("set", np.shape(A), kw))
        return orig_set(self, A, ctr, fixed, enlarge, **kw)

    def set_center(self, ctr):
        sent.append(("center", np.shape(ctr)))
        return orig_center(self, ctr)

    monkeypatch.setattr(kernels.DeviceRegion, "set_tregion", set_tregion)
    monkeypatch.setattr(kernels.DeviceRegion, "set_tregion_center", set_center)
    got, host, tregion, Lmin = _check(region, ELL, M)
    assert sent == [("set", (8, 8), dict(width=8))]
    tregion.update_center(np.asarray(tregion.ellipsoid_center) + 0.3 * np.sqrt(np.diag(tregion.ellipsoid_cov)))
    host2 = TR._host_sequence(region, ELL, N, M.transform, M.loglike, tregion, halve=False)
    assert not np.array_equal(host2[2], host[2]) and host2[2].sum() >= 40
    Lmin2 = TR._gap_threshold(host2[3])
    with _counted() as calls:
        TR._compare(TR._gated(region, ELL, N, Lmin2, M.transform, M.loglike, tregion), host2, Lmin2, tregion)
    assert calls == ["gated"] and sent == [("set", (8, 8), dict(width=8)), ("center", (8,))]


# ---- guards ------------------------------------------------------------------------------------------------------------------

def test_mismatched_handles_and_widths_are_refused():
    d, Q = 5, 3
    M = _model(d, Q)
    region = TR._region_of("MLFriends", TR._blob(400, d, 77))
    got, host, tregion, Lmin = _check(region, ELL, M)
    handle, state = region._dev.handle, region._dev       # a t-region over d + Q columns is set on it
    gd, derive = M.handle(True, gated=True, derived=True), M.derive_handle()
    args = (1, N, 41, 0, -1e300)
    # entries whose kernels would read the (d + Q)^2 matrix as d^2
    with pytest.raises(ValueError, match=r"spans d \+ nderived columns"):
        handle.refill_user(*args, M.handle(True, gated=True))
    with pytest.raises(ValueError, match=r"spans d \+ nderived columns"):
        handle.refill(*args, (1, 20.0, -10.0), (3, None, 0.0))
    with pytest.raises(ValueError, match="t-region"):
        handle.refill_user_derived(*args, M.handle(True), derive, Q)
    # the new entry with a handle of another variant, or a derive program of another width
    with pytest.raises(ValueError, match="not of a _TREGION_DERIVED variant"):
        handle.refill_user_derived_gated(*args, M.handle(True, gated=True), derive, Q)
    with pytest.raises(ValueError, match="not of a _TREGION_DERIVED variant"):
        handle.refill_user_derived_gated(*args, M.handle(True), derive, Q)
    with pytest.raises(ValueError, match="number of derived parameters"):
        handle.refill_user_derived_gated(*args, gd, _model(d, 2).derive_handle(), 2)
    with pytest.raises(ValueError, match="not a derive handle"):
        handle.refill_user_derived_gated(*args, gd, M.handle(True), Q)
    # the new entry with a t-region over the parameters alone, and without one
    state.sync_tregion(handle, R._tregion(d=d), d)
    with pytest.raises(ValueError, match=r"width is not d \+ nderived"):
        handle.refill_user_derived_gated(*args, gd, derive, Q)
    with pytest.raises(ValueError, match="only in mlf_region_refill_user_derived_gated"):
        handle.refill_user(*args, gd)                     # the handle of the new variant in the gated user refill
    state.sync_tregion(handle, None, 0)
    with pytest.raises(ValueError, match="no t-region set"):
        handle.refill_user_derived_gated(*args, gd, derive, Q)
    with pytest.raises(ValueError):
        handle.refill_user(*args, gd)
    out = np.empty(4)
    rows = np.full((4, d), 0.5)
    assert dm._lib.lib().mlf_usermodel_eval(gd, dm.ptr(rows), 4, None, dm.ptr(out)) == 4          # MLF_E_STATE: it evaluates nowhere else
    # a code object loaded as the variant it was not compiled as
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(M._compile(True, True), d, True, M.aux, gated=True, derived="gate", nderived=Q)
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(M.compile_gate_derived(True), d, True, M.aux, gated=True)
    # a width below the region's, and everything still works afterwards
    with pytest.raises(ValueError):
        handle.set_tregion(np.eye(d - 1), np.zeros(d - 1), None, 1.0, width=d - 1)
    with _counted() as calls:
        again = TR._gated(region, ELL, N, Lmin, M.transform, M.loglike, tregion)
    assert calls == ["gated"] and all(np.array_equal(a, b) for a, b in zip(again[:3], got[:3])) and again[3:] == got[3:]


# ---- end to end --------------------------------------------------------------------------------------------------------------

def test_nested_sampling_with_the_gate_over_the_derived_column(monkeypatch):
    """The one-column model p0 p1 of test_derived_model_gpu under StaticNestedSampler(build_tregion=True), with and without the
    flag: the flagged run takes the new entry for every batch that has a t-region and never the host sequence; the unflagged run
    takes the host sequence on the same Philox draws, so iterations, calls and samples are the same."""
    from ultranest_amd import regions

    def model(flag):
        return dm.DeviceModel(2, usermodels.GAUSS_LOGLIKE % 0.1, aux=usermodels.gauss_centers(2), nderived=1,
                              derived_source=DG.PRODUCT_DERIVED, gate_derived=flag)

    np.random.seed(5)
    s0, plain = DG._nested(model(False), build_tregion=True, keep_tree=True)
    assert s0.updater.tregion is not None and s0.updater.tregion.u.shape[1] == 3

    def no_host_sample(self, *a, **k):
        raise AssertionError("the host sequence ran")

    monkeypatch.setattr(regions.MLFriends, "sample", no_host_sample)
    with _counted() as calls:
        np.random.seed(5)
        s1, flagged = DG._nested(model(True), build_tregion=True, keep_tree=True)
    print("ln Z flagged %.12f, unflagged %.12f; %d gated and %d ungated derived refills; %.2f s and %.2f s" % (
        flagged["logz"], plain["logz"], calls.count("gated"), calls.count("plain"), s1.phases["total_s"], s0.phases["total_s"]))
    assert s1.updater.tregion is not None and s1.updater.tregion.u.shape[1] == 3
    assert calls.count("gated") >= 1
    assert flagged["niter"] == plain["niter"] and flagged["ncall"] == plain["ncall"]
    assert np.array_equal(np.asarray(s1.updater.region.u), np.asarray(s0.updater.region.u))        # the final live points
    assert np.shape(s1.results["samples"])[1] == 3
    assert np.array_equal(np.asarray(s1.results["samples"]), np.asarray(s0.results["samples"]))
    assert flagged["logz"] == plain["logz"] and flagged["logz_tree"] == plain["logz_tree"]
