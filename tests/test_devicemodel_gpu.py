"""User models (ultranest_amd.devicemodel) on the GPU: the fused wrapper kernel against numpy and against the built-in
kernels, the device refill and the population sampler with a user model against the built-in Rosenbrock route, an end-to-end
evidence, and model lifetimes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import loglike_reference as LR  # noqa: E402
from ultranest_amd import likelihoods as lk  # noqa: E402
from ultranest_amd import usermodels  # noqa: E402

NS = (1, 63, 64, 65, 100000)


def _funnel_np(theta, data):
    sigma = 10 ** theta[:, 0]
    return (-0.5 * (((theta[:, 1:] - data) / sigma.reshape((-1, 1))) ** 2).sum(axis=1)
            - 0.5 * np.log(2 * np.pi * sigma ** 2) * len(data))


def _funnel_transform_np(x):
    z = x * 20 - 10
    z[:, 0] = x[:, 0] * 6 - 3
    return z


def _gauss_np(theta, centers, sigma=0.1):
    return -0.5 * (((theta - centers) / sigma) ** 2).sum(axis=1) - 0.5 * np.log(2 * np.pi * sigma ** 2) * theta.shape[1]


def _close(a, b, rtol=1e-12, scale=0.0):
    """|a - b| <= rtol (|b| + scale): `scale` = the size of the terms a likelihood near 0 is the difference of"""
    return np.all(np.abs(a - b) <= rtol * (np.abs(b) + scale))


def _gauss_scale(theta, centers, sigma=0.1):
    return 0.5 * (((theta - centers) / sigma) ** 2).sum(axis=1) + abs(0.5 * np.log(2 * np.pi * sigma ** 2) * theta.shape[1])


def _funnel_scale(theta, data):
    sigma = 10 ** theta[:, 0]
    return (0.5 * (((theta[:, 1:] - data) / sigma.reshape((-1, 1))) ** 2).sum(axis=1)
            + np.abs(0.5 * np.log(2 * np.pi * sigma ** 2) * len(data)))


def _close_to_reference(L, ref, tight_scale):
    """_close against the high-precision reference of loglike_reference (all rows with a long double, else its mpmath rows)"""
    return _close(L[ref.rows], ref.ref.astype(np.float64), scale=tight_scale[ref.rows]) and ref.excess(L)[0] <= 1


@pytest.mark.parametrize("d", [3, 10, 50, 101, 200, 63, 64, 127, 128])
def test_funnel_and_gauss_against_numpy(d):
    """(63 / 64: the staged form ends where a transform needs a second LDS buffer; 127 / 128: where it ends without one)"""
    rs = np.random.RandomState(d)
    F = usermodels.funnel(d)
    G = usermodels.gauss(d)
    data, centers = usermodels.funnel_data(d), usermodels.gauss_centers(d)
    for n in NS:
        u = rs.uniform(size=(n, d))
        keep = u.copy()
        p = F.transform(u)
        assert np.array_equal(u, keep)
        assert p.shape == (n, d) and _close(p, _funnel_transform_np(u))
        th = p.copy()
        L = F.loglike(th)
        assert np.array_equal(th, p)
        assert L.shape == (n,) and _close(L, _funnel_np(p, data), scale=_funnel_scale(p, data)), (d, n)
        assert _close_to_reference(L, LR.Reference("funnel", p, data, with_mpmath=False), _funnel_scale(p, data)), (d, n)
        g = 0.5 + 0.1 * rs.normal(size=(n, d))
        gk = g.copy()
        assert np.array_equal(G.transform(g), g)      # no transform source: identity
        Lg = G.loglike(g)
        assert _close(Lg, _gauss_np(g, centers), scale=_gauss_scale(g, centers)), (d, n)
        assert _close_to_reference(Lg, LR.Reference("gauss", g, centers, 0.1, with_mpmath=False), _gauss_scale(g, centers)), (d, n)
        assert np.array_equal(g, gk)


@pytest.mark.parametrize("d", [7, 51, 129, 200, 6, 50, 63, 64, 127, 128])
def test_rosenbrock_against_the_builtin_kernels(d):
    """odd d and d > 128: the built-in route evaluates row by row -- bit for bit; even d <= 128: pair layout, 1e-12; both
    within 1e-12 * scale of the high-precision reference (63 / 64, 127 / 128: the ends of the staged form with and without
    a transform)"""
    R = usermodels.rosenbrock(d)
    rs = np.random.RandomState(100 + d)
    for n in NS:
        u = rs.uniform(size=(n, d))
        p = R.transform(u)
        assert np.array_equal(p, lk.rosenbrock_transform(u))
        L, Lb = R.loglike(p), lk.rosenbrock_loglike(p)
        if d % 2 == 1 or d > 128:
            assert np.array_equal(L, Lb), (d, n, np.abs(L - Lb).max())
        else:
            assert _close(L, Lb), (d, n)
        ref = LR.Reference("rosenbrock", p, with_mpmath=False)
        assert ref.excess(L)[0] <= 1 and ref.excess(Lb)[0] <= 1, (d, n, ref.excess(L), ref.excess(Lb))


@pytest.mark.parametrize("d", [10, 101, 63, 64, 1])
def test_eval_dev_member_rows_only(d):
    """device pointers (torch tensors): rows outside the mask get L = -inf and keep their p row; the others are the host
    entry's values, which are numpy's (d = 1: the staging steps by 64 rows and 0 columns)"""
    import torch
    from ultranest_amd import _lib
    F = usermodels.funnel(d)
    rs = np.random.RandomState(7)
    n = 1000
    u = rs.uniform(size=(n, d))
    member = rs.uniform(size=n) < 0.4
    member[:64] = False           # a whole wave without members
    dev = torch.device("cuda")
    tu = torch.from_numpy(u).to(dev)
    tp = torch.full((n, d), 7.0, dtype=torch.float64, device=dev)
    tL = torch.zeros(n, dtype=torch.float64, device=dev)
    tm = torch.from_numpy(member.astype(np.uint8)).to(dev)
    torch.cuda.synchronize()
    F.eval_dev(tu.data_ptr(), n, tp.data_ptr(), tL.data_ptr(), tm.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().mlf_synchronize())
    p, L = tp.cpu().numpy(), tL.cpu().numpy()
    want_p = F.transform(u)
    data = usermodels.funnel_data(d)
    assert _close(want_p, _funnel_transform_np(u))
    assert _close(F.loglike(want_p), _funnel_np(want_p, data), scale=_funnel_scale(want_p, data))
    assert np.array_equal(p[member], want_p[member]) and (p[~member] == 7.0).all()
    assert np.array_equal(L[member], F.loglike(want_p[member])) and np.isneginf(L[~member]).all()


def _region(u):
    import ultranest_amd.mlfriends as m
    layer = m.AffineLayer()
    layer.optimize(u, u)
    region = m.MLFriends(u, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    return region


@pytest.mark.parametrize("method", ["sample_from_boundingbox", "sample_from_wrapping_ellipsoid", "sample_from_points"])
def test_refill_with_the_user_rosenbrock_equals_the_builtin(method):
    from ultranest_amd import kernels
    from ultranest_amd.regions import DeviceRNG
    d = 7
    rs = np.random.RandomState(4)
    u = np.clip(0.5 + 0.12 * rs.normal(size=(400, d)), 0.01, 0.99)
    R = usermodels.rosenbrock(d)
    Ls = lk.rosenbrock_loglike(lk.rosenbrock_transform(u))
    Lmin = np.sort(Ls)[40]
    out = []
    calls = []
    orig = kernels.DeviceRegion.refill_user

    def counting(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    kernels.DeviceRegion.refill_user = counting
    try:
        for transform, loglike in [(lk.rosenbrock_transform, lk.rosenbrock_loglike), (R.transform, R.loglike)]:
            region = _region(u)
            region.device_rng = DeviceRNG(seed=11)
            region.current_sampling_method = getattr(region, method)
            np.random.seed(3)
            got = region.refill(2 ** 16, Lmin, transform, loglike)
            out.append(got + (region.device_rng.offset,))
    finally:
        kernels.DeviceRegion.refill_user = orig
    assert len(calls) == 1
    (ua, pa, La, nca, oa), (ub, pb, Lb, ncb, ob) = out
    assert nca == ncb and oa == ob and nca > 0
    assert len(ua) > (0 if method == "sample_from_boundingbox" else 10)
    assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and np.array_equal(La, Lb)


def test_refill_with_the_funnel():
    from ultranest_amd.regions import DeviceRNG
    d = 51
    rs = np.random.RandomState(5)
    u = 0.5 + 0.03 * rs.normal(size=(400, d))
    F = usermodels.funnel(d)
    data = usermodels.funnel_data(d)
    Lmin = np.quantile(_funnel_np(_funnel_transform_np(u), data), 0.3)
    for method in ["sample_from_wrapping_ellipsoid", "sample_from_points"]:   # (the cube accepts nothing at d = 51)
        region = _region(u)
        region.device_rng = DeviceRNG(seed=11)
        region.current_sampling_method = getattr(region, method)
        got, p, L, nc = region.refill(2 ** 16, Lmin, F.transform, F.loglike)
        assert nc > 0 and region.device_rng.offset > 0
        assert _close(p, _funnel_transform_np(got)) and _close(L, _funnel_np(p, data), scale=_funnel_scale(p, data))
        assert (L > Lmin).all() and len(got) > 0


def _walk(transform, loglike, region, u, Ls, Lmin, device_rng=None, max_rounds=None, use_graph=None, calls=300):
    import ultranest_amd.popstepsampler as pop
    np.random.seed(8)
    s = pop.PopulationSliceSampler(popsize=32, nsteps=6, generate_direction=pop.generate_mixture_random_direction, scale=0.5,
                                   device_rng=device_rng)
    if max_rounds is not None:
        s.max_rounds = max_rounds
    if use_graph is not None:
        s.use_graph = use_graph
    return [s.__next__(region, Lmin, u, Ls, transform, loglike) for _ in range(calls)]


def _same_run(a, b):
    for (ua, pa, La, nca), (ub, pb, Lb, ncb) in zip(a, b):
        assert nca == ncb
        assert (ua is None) == (ub is None)
        if ua is not None:
            assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and La == Lb
    return sum(x[0] is not None for x in a)


def test_population_sampler_with_the_user_rosenbrock():
    from ultranest_amd.regions import DeviceRNG
    d = 7
    rs = np.random.RandomState(3)
    u = 0.5 + 0.04 * rs.normal(size=(300, d))
    region = _region(u)
    R = usermodels.rosenbrock(d)
    Ls = lk.rosenbrock_loglike(lk.rosenbrock_transform(u))
    Lmin = np.sort(Ls)[5]
    builtin = (lk.rosenbrock_transform, lk.rosenbrock_loglike)
    user = (R.transform, R.loglike)
    # host-RNG mode: mlf_walkers_finish_user against mlf_walkers_finish_dev
    a = _walk(*builtin, region, u, Ls, Lmin)
    b = _walk(*user, region, u, Ls, Lmin)
    assert _same_run(a, b) > 20
    # Philox mode, one step per call on both
    a = _walk(*builtin, region, u, Ls, Lmin, DeviceRNG(5), 1, False)
    b = _walk(*user, region, u, Ls, Lmin, DeviceRNG(5), 1, False)
    assert _same_run(a, b) > 20
    # the sampler's defaults (multi-round kernel, graph replay) for the user model: the per-step route, so its points are
    # those of the built-in per-step run, and the evaluations between two points add up to the same count
    c = _walk(*user, region, u, Ls, Lmin, DeviceRNG(5))
    pa = [(x[0], x[1], x[2]) for x in a if x[0] is not None]
    pc = [(x[0], x[1], x[2]) for x in c if x[0] is not None]
    assert len(pa) == len(pc) > 20
    for (ua, va, La), (uc, vc, Lc) in zip(pa, pc):
        assert np.array_equal(ua, uc) and np.array_equal(va, vc) and La == Lc

    def ncs(run):
        out, acc = [], 0
        for x in run:
            acc += x[3]
            if x[0] is not None:
                out.append(acc)
                acc = 0
        return out
    assert ncs(a) == ncs(c)


def test_nested_sampling_evidence_of_the_user_gauss():
    """d = 10 Gaussian (sigma 0.1, normalised, inside the cube): analytic ln Z = 0, region refills on the device"""
    from ultranest_amd import kernels
    from ultranest_amd.harness import StaticNestedSampler
    from ultranest_amd.regions import DeviceRNG
    G = usermodels.gauss(10)
    calls = []
    orig = kernels.DeviceRegion.refill_user

    def counting(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    kernels.DeviceRegion.refill_user = counting
    try:
        s = StaticNestedSampler(10, G.loglike, transform=lk.identity_transform, num_live_points=400, ndraw=4096, seed=2,
                                device_rng=DeviceRNG(21))
        res = s.run(dlogz=0.5)
    finally:
        kernels.DeviceRegion.refill_user = orig
    assert abs(res["logz"]) < 4 * res["logzerr"] + 0.15, res
    assert len(calls) > 10


def test_two_models_alternately_then_destroyed():
    rs = np.random.RandomState(9)
    d = 9
    x = rs.uniform(size=(5000, d))
    alone = []
    for make in (lambda: usermodels.rosenbrock(d), lambda: usermodels.funnel(d)):
        m = make()
        alone.append((m.transform(x), m.loglike(m.transform(x))))
        m.close()
    a, b = usermodels.rosenbrock(d), usermodels.funnel(d)
    for _ in range(3):
        for m, (p0, L0) in zip((a, b), alone):
            p = m.transform(x)
            assert np.array_equal(p, p0) and np.array_equal(m.loglike(p), L0)
    a.close()
    p0, L0 = alone[1]
    assert np.array_equal(b.loglike(b.transform(x)), L0)
    b.close()
