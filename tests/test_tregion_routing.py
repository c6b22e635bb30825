"""The driver's parameter-space wrapping ellipsoid (tregion) and the device refill, CPU side: which route a batch takes
(harness.refill_samples, MLFriends.refill; the device entry points replaced by recorders) and when the device copy of the
tregion is sent again (_DeviceState.sync_tregion; the library calls recorded by a stand-in handle)."""
import numpy as np
import pytest

from ultranest_amd import regions, usermodels
from ultranest_amd import likelihoods as lk
from ultranest_amd.regions import DeviceRNG, MLFriends, WrappingEllipsoid

D = 7


def _harness():
    # imported inside the tests, as the other test modules do: a module-level import would bind the harness's own kernel
    # imports at collection time, before a stubbed test module gets to import it under its stand-in kernels
    from ultranest_amd import harness
    return harness


def _tregion(d=D, seed=3, fixed_last=False):
    p = np.random.RandomState(seed).normal(size=(60, d))
    if fixed_last:
        p[:, -1] = 0.25
    t = WrappingEllipsoid.__new__(WrappingEllipsoid)      # no bootstrap (a device computation): the attributes it would leave
    WrappingEllipsoid.__init__(t, p)
    t.enlarge = 1.7
    v = p[:, t.variable_dims]
    t.ellipsoid_center = v.mean(axis=0)
    t.ellipsoid_cov = np.cov(v, rowvar=0) * (v.shape[1] + 2)
    t.ellipsoid_invcov = np.linalg.inv(t.ellipsoid_cov)
    return t


def _cpu_region(calls, monkeypatch, d=D):
    def refill(self, region, use_scan, method, nsamples, Lmin, tspec, lspec, **kw):
        calls.append(("refill", method, nsamples, Lmin, tspec, lspec, kw))
        return np.zeros((1, d)), np.zeros((1, d)), np.zeros(1), 1

    def refill_user(self, region, use_scan, method, nsamples, Lmin, model, with_transform, **kw):
        calls.append(("refill_user", method, nsamples, Lmin, model, with_transform, kw))
        return np.zeros((1, d)), np.zeros((1, d)), np.zeros(1), 1

    monkeypatch.setattr(regions._DeviceState, "refill", refill)
    monkeypatch.setattr(regions._DeviceState, "refill_user", refill_user)
    region = MLFriends.__new__(MLFriends)
    region.u = np.full((10, d), 0.5)
    region.device_rng = DeviceRNG(11)
    region._dev = regions._DeviceState()
    region.current_sampling_method = region.sample_from_boundingbox
    return region


def test_refill_samples_hands_the_tregion_to_the_device_route(monkeypatch):
    """fails before the gated refill existed: refill_samples took the host sequence as soon as a tregion was given"""
    calls = []
    region = _cpu_region(calls, monkeypatch)
    monkeypatch.setattr(MLFriends, "sample", lambda self, nsamples=100: pytest.fail("host sequence"))
    m = usermodels.rosenbrock(D)
    t = _tregion()
    got = _harness().refill_samples(region, t, m.transform, m.loglike, -1.0, 100)
    assert len(got) == 4 and calls[-1] == ("refill_user", 0, 100, -1.0, m, True, dict(tregion=t))
    got = _harness().refill_samples(region, t, lk.rosenbrock_transform, lk.rosenbrock_loglike, -2.0, 50)
    assert len(got) == 4 and got[3] == 1
    assert calls[-1] == ("refill", 0, 50, -2.0, lk.rosenbrock_transform.device_spec, lk.rosenbrock_loglike.device_spec, dict(tregion=t))
    t_fixed = _tregion(fixed_last=True)
    assert t_fixed.variable_dims is not Ellipsis
    _harness().refill_samples(region, t_fixed, m.transform, m.loglike, -1.0, 100)
    assert calls[-1][-1] == dict(tregion=t_fixed)


def test_without_a_tregion_the_device_calls_are_todays(monkeypatch):
    calls = []
    region = _cpu_region(calls, monkeypatch)
    m = usermodels.rosenbrock(D)

    def refill(self, region, use_scan, method, nsamples, Lmin, tspec, lspec):          # today's positional signatures
        calls.append(("refill", method, nsamples, Lmin, tspec, lspec))
        return np.zeros((1, D)), np.zeros((1, D)), np.zeros(1), 1

    def refill_user(self, region, use_scan, method, nsamples, Lmin, model, with_transform):
        calls.append(("refill_user", method, nsamples, Lmin, model, with_transform))
        return np.zeros((1, D)), np.zeros((1, D)), np.zeros(1), 1

    monkeypatch.setattr(regions._DeviceState, "refill", refill)
    monkeypatch.setattr(regions._DeviceState, "refill_user", refill_user)
    _harness().refill_samples(region, None, m.transform, m.loglike, -1.0, 100)
    assert calls[-1] == ("refill_user", 0, 100, -1.0, m, True)
    _harness().refill_samples(region, None, lk.rosenbrock_transform, lk.rosenbrock_loglike, -3.0, 100)
    assert calls[-1] == ("refill", 0, 100, -3.0, lk.rosenbrock_transform.device_spec, lk.rosenbrock_loglike.device_spec)
    region.refill(100, -3.0, m.transform, m.loglike, tregion=None)
    assert calls[-1] == ("refill_user", 0, 100, -3.0, m, True)


class _PointStore(object):
    def __init__(self):
        self.rows = []

    def add(self, row, ncall):
        self.rows.append(row)


class _Foreign(object):
    """a tregion of the caller's own: only `inside`"""

    def inside(self, p):
        return np.asarray(p)[:, 0] > 0


@pytest.mark.parametrize("case", ["other_dimension", "foreign_object", "no_ellipsoid", "own_inside", "pointstore"])
def test_what_cannot_go_to_the_device_ends_on_the_host_sequence(case, monkeypatch):
    calls = []
    region = _cpu_region(calls, monkeypatch)
    rs = np.random.RandomState(1)
    pts = rs.uniform(0.1, 0.9, size=(40, D))
    monkeypatch.setattr(MLFriends, "sample", lambda self, nsamples=100: pts)

    def inside_numpy(p, ctr, invcov, r):      # the quadratic form is a device computation: numpy stands in here
        dl = np.asarray(p) - ctr
        return np.einsum('ij,jk,ik->i', dl, invcov, dl) <= r

    monkeypatch.setattr(regions, "_inside_ellipsoid", inside_numpy)
    transform = lk.identity_transform
    host_calls = []

    def loglike(p):
        host_calls.append(len(p))
        return -((np.asarray(p) - 0.5) ** 2).sum(axis=1)

    loglike.device_spec = lk.GaussLikelihood(0.5, 0.1, D).device_spec
    store = None
    if case == "other_dimension":          # e.g. derived parameters: the tregion lives in more dimensions than the cube
        t = _tregion(d=D + 2)
        t.enlarge = 1e3
        transform = lambda u: np.hstack([u, u[:, :2]])      # noqa: E731
    elif case == "foreign_object":
        t = _Foreign()
    elif case == "no_ellipsoid":
        t = _tregion()
        del t.ellipsoid_invcov
        t.inside = lambda p: np.ones(len(p), dtype=bool)
    elif case == "own_inside":
        class Mine(WrappingEllipsoid):
            def inside(self, p):
                return np.asarray(p)[:, 0] > 0.5
        t = _tregion()
        t.__class__ = Mine
    else:
        t = _Foreign()
        store = _PointStore()
    assert not regions.tregion_on_device(t, D)
    u, v, logl, nc = _harness().refill_samples(region, t, transform, loglike, -0.5, 40, pointstore=store)
    assert not calls and len(host_calls) == 1                   # no device entry point, one host likelihood call
    acc = t.inside(transform(pts))
    assert nc == acc.sum() == host_calls[0]
    assert u.shape[1] == D and v.shape[0] == u.shape[0] == logl.shape[0] and (logl > -0.5).all()
    if store is not None:
        assert len(store.rows) == nc
    # and a tregion that could go, with a point store: the host sequence all the same (it logs the rejected evaluations)
    if case == "pointstore":
        good = _tregion()
        assert regions.tregion_on_device(good, D)
        good.inside = lambda p: np.ones(len(p), dtype=bool)
        _harness().refill_samples(region, good, transform, loglike, -0.5, 40, pointstore=_PointStore())
        assert not calls and len(host_calls) == 2


class _Handle(object):
    """stands in for kernels.DeviceRegion: records the t-region calls"""

    def __init__(self):
        self.calls = []

    def set_tregion(self, A, ctr, fixed, enlarge):
        self.calls.append(("set", np.array(A), np.array(ctr), None if fixed is None else np.array(fixed), enlarge))

    def set_tregion_center(self, ctr):
        self.calls.append(("center", np.array(ctr)))

    def clear_tregion(self):
        self.calls.append(("clear",))


def test_device_copy_of_the_tregion_is_sent_only_when_it_changed():
    state, h = regions._DeviceState(), _Handle()
    t = _tregion()
    state.sync_tregion(h, None, 0)
    assert h.calls == []                                        # nothing set, nothing to clear
    state.sync_tregion(h, t, D)
    assert [c[0] for c in h.calls] == ["set"]
    kind, A, ctr, fixed, enlarge = h.calls[-1]
    assert np.array_equal(A, t.ellipsoid_invcov) and np.array_equal(ctr, t.ellipsoid_center) and fixed is None and enlarge == 1.7
    state.sync_tregion(h, t, D)
    assert len(h.calls) == 1                                    # unchanged: no call
    t.update_center(np.asarray(t.ellipsoid_center) + 0.125)     # the driver, every iteration
    state.sync_tregion(h, t, D)
    assert [c[0] for c in h.calls] == ["set", "center"] and np.array_equal(h.calls[-1][1], t.ellipsoid_center)
    state.sync_tregion(h, t, D)
    assert len(h.calls) == 2
    t.enlarge = 2.5
    state.sync_tregion(h, t, D)
    assert [c[0] for c in h.calls] == ["set", "center", "set"] and h.calls[-1][4] == 2.5
    t.ellipsoid_invcov = t.ellipsoid_invcov * 2.0
    state.sync_tregion(h, t, D)
    assert [c[0] for c in h.calls][3:] == ["set"] and np.array_equal(h.calls[-1][1], t.ellipsoid_invcov)
    t.ellipsoid_invcov[0, 0] *= 1.5                             # written in place: seen by value
    state.sync_tregion(h, t, D)
    assert [c[0] for c in h.calls][4:] == ["set"]
    t2 = _tregion()                                             # another object with the same values: a full set
    t2.enlarge, t2.ellipsoid_invcov, t2.ellipsoid_center = t.enlarge, t.ellipsoid_invcov, t.ellipsoid_center
    state.sync_tregion(h, t2, D)
    assert [c[0] for c in h.calls][5:] == ["set"]
    state.sync_tregion(h, None, 0)
    assert [c[0] for c in h.calls][6:] == ["clear"]
    state.sync_tregion(h, None, 0)
    assert len(h.calls) == 7
    state.sync_tregion(h, t2, D)
    assert [c[0] for c in h.calls][7:] == ["set"]


def test_fixed_dimensions_travel_as_zero_rows_and_fixed_values():
    t = _tregion(fixed_last=True)
    state, h = regions._DeviceState(), _Handle()
    state.sync_tregion(h, t, D)
    kind, A, ctr, fixed, enlarge = h.calls[-1]
    assert A.shape == (D, D) and np.array_equal(A[:-1, :-1], t.ellipsoid_invcov)
    assert not A[-1].any() and not A[:, -1].any() and ctr[-1] == 0.0 and np.array_equal(ctr[:-1], t.ellipsoid_center)
    assert np.isnan(fixed[:-1]).all() and fixed[-1] == 0.25
    # the dense form is the host test: same quadratic form, same equality
    p = np.random.RandomState(8).normal(size=(200, D))
    p[::2, -1] = 0.25
    dl = p - ctr
    q = np.einsum('ij,jk,ik->i', dl, A, dl)
    ok = np.all(np.isnan(fixed) | (p == fixed), axis=1)
    dv = p[:, :-1] - t.ellipsoid_center
    qv = np.einsum('ij,jk,ik->i', dv, t.ellipsoid_invcov, dv)
    assert np.array_equal(q, qv) and np.array_equal(ok, p[:, -1] == 0.25)
    state.sync_tregion(h, t, D)
    assert len(h.calls) == 1
    t.update_center(np.append(t.ellipsoid_center + 1.0, 0.25))
    state.sync_tregion(h, t, D)
    assert h.calls[-1][0] == "center" and h.calls[-1][1][-1] == 0.0


def test_static_sampler_keeps_build_tregion_off_by_default():
    s = _harness().StaticNestedSampler(3, lambda p: -(p ** 2).sum(axis=1))
    assert s.build_tregion is False and s.updater.build_tregion is False
    s = _harness().StaticNestedSampler(3, lambda p: -(p ** 2).sum(axis=1), build_tregion=True)
    assert s.updater.build_tregion is True


def test_model_handle_keys_the_gated_variant_separately(monkeypatch):
    from ultranest_amd import devicemodel as dm
    made = []

    class H(object):
        def __init__(self, code, ndim, has_transform, aux, gated=False):
            made.append((code, has_transform, gated))
            self.handle = len(made)

    monkeypatch.setattr(dm, "_Handle", H)
    m = usermodels.rosenbrock(D)
    a, b, c = m.handle(True), m.handle(True, gated=True), m.handle(False, gated=True)
    assert len({a, b, c}) == 3 and m.handle(True, gated=True) == b and len(made) == 3
    assert made[0] == (m.code, True, False)
    assert made[1] == (dm.compile_model(m.source, True, gated=True), True, True)
    assert made[2] == (dm.compile_model(m.source, False, gated=True), False, True)
    m._handles = {}
