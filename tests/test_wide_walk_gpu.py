"""PopulationSliceSampler's resident walkers above 128 dimensions (csrc/mlf_walk.hip, template parameter WIDE;
dw_direction_wide of csrc/mlf_walk_dev.hpp): the device-side direction draw against the numpy restatement
(tests/randomwalk_reference.py::directions), the host-random mode against the CPU stand-in bit for bit, the device forms
against each other, user models with and without derived parameters, the dimensionality bounds of mlf_walkers_create, and
invariance of the uniform distribution under a hard contour.  Before the wide form existed every test here ended in
MLF_E_DIM."""
import ctypes
import functools
import types

import numpy as np
import pytest

import randomwalk_reference as R
from golden import inputs
from test_wide_walk_restatement import problem as synthetic_problem

pytestmark = pytest.mark.gpu


# ---- the direction draw against the restatement ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _affine_problem(d):
    """(axes, live, std) of the _affine_region recipe (tests/test_randomwalk_device.py) with 400 live points"""
    import ultranest_amd.mlfriends as m
    rs = np.random.RandomState(900 + d)
    u = np.clip(0.5 + 0.15 * rs.normal(size=(400, d)), 0.01, 0.99)
    layer = m.AffineLayer()
    layer.optimize(u, u)
    region = m.MLFriends(u, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    return np.array(region.transformLayer.axes), u, u.std(axis=0)


@functools.lru_cache(maxsize=None)
def _synthetic_problem(d):
    """d = 1024: a synthetic layer (axes, T, ctr from a seeded, well-conditioned matrix) and 64 live points: nothing of size
    N x d^2 is built"""
    axes, live, std = synthetic_problem(d)
    layer = types.SimpleNamespace(axes=axes, T=np.linalg.inv(axes), ctr=live.mean(axis=0))
    return layer.axes, live, std


GRID = 1 << 13      # workgroups of a wide walker launch (wide_walker_grid, csrc/mlf_walk.hip)
DIRECTION_CASES = ([(d, 70, kind, 77) for d in (129, 130, 192, 193, 256) for kind in range(7)]
                   + [(1024, 3, kind, 77) for kind in range(7)]
                   + [(130, GRID + 70, 4, 77), (130, GRID + 70, 6, 77)]       # a workgroup makes a second trip
                   + [(129, 70, 2, 2**32 - 40), (130, 70, 6, 2**32 - 40)])    # the 64-bit counter carries within the call


@pytest.mark.parametrize("d,P,kind,offset", DIRECTION_CASES)
def test_directions_against_the_restatement(d, P, kind, offset):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    axes, live, std = _affine_problem(d) if d <= 256 else _synthetic_problem(d)
    seed, scale, dirscale = 40 + kind, 0.37, 0.8
    w = pop._Walkers(P, 1, d)
    w.set_direction_data(axes=axes, live=live, std=std)
    start = np.arange(P) % len(live)
    w.start(np.arange(P), live[start], np.zeros(P))
    rng = DeviceRNG(seed)
    rng.offset = offset
    w.brackets_philox(scale, kind, dirscale, rng)
    npairs = (d + 1) // 2
    assert rng.offset == offset + P * (npairs + 2) == R.next_offset(offset, P, 1, d)
    st = w.export()
    assert (st["current_left"] == -scale).all() and (st["current_right"] == scale).all()
    assert st["searching_left"].all() and st["searching_right"].all() and (st["currentt"] == 0).all()
    assert np.array_equal(st["allu"][:, 0], live[start]) and (st["generation"] == 0).all()
    got = st["currentv"]
    want = R.directions(seed, offset, kind, dirscale, P, 1, 0, d, axes=axes, live=live, std=std)
    if kind == 6:       # both branches of the coin occur (on the restatement), and each is the restated selection
        from3 = (want == R.directions(seed, offset, 3, dirscale, P, 1, 0, d, axes=axes)).all(axis=1)
        from5 = (want == R.directions(seed, offset, 5, dirscale, P, 1, 0, d, live=live)).all(axis=1)
        assert np.logical_xor(from3, from5).all()
        if P >= 70:
            assert from3.any() and from5.any()
    if kind == 2:       # Box-Muller: a few ulp of a value below 9; the norm of d >= 129 normals is at least 11
        dev = np.abs(got - want).max()
        print("kind 2: largest deviation %.3g, bound %.3g" % (dev, 1e-12 * dirscale))
        assert dev <= 1e-12 * dirscale
    elif kind == 4:     # the rounding bound of a row's sum is d 2^-53 dirscale |axes[r]|_2 (1.1e-13 at d = 1024)
        bound = 1e-12 * dirscale * np.linalg.norm(axes, axis=1)
        ratio = (np.abs(got - want) / bound).max()
        print("kind 4: largest deviation / bound = %.3g" % ratio)
        assert ratio <= 1.0
    else:
        assert np.array_equal(got, want), np.abs(got - want).max()


# ---- host-random mode against the CPU stand-in -----------------------------------------------------------------------

def _host_region(d, u=None):
    """a region object of plain attributes (as test_popstepsampler's traces use): nothing of it is built on the GPU"""
    if u is None:
        u = inputs.live_points(940 + d, 300, d)
    axes = synthetic_problem(d, seed=3)[0]
    layer = types.SimpleNamespace(axes=axes, T=np.linalg.inv(axes), ctr=u.mean(axis=0))
    return types.SimpleNamespace(u=u, transformLayer=layer, maxradiussq=float(d))


@pytest.mark.parametrize("d", [130, 200])
@pytest.mark.parametrize("name", ["generate_mixture_random_direction", "generate_cube_oriented_direction"])
def test_host_random_mode_equals_the_cpu_stand_in(monkeypatch, d, name):
    """Same np.random seed, same region object, same callbacks: once through OracleWalkers (tests/oracle_backend.py), once
    through the HIP walkers -- every (u, p, L, nc), the final chain state, the scale and the numpy stream's position."""
    import oracle_backend
    import ultranest_amd.popstepsampler as pop
    region = _host_region(d)
    u = region.u
    Ls = inputs.walker_loglike(u)
    order = np.argsort(Ls)

    def run():
        np.random.seed(950)
        sampler = pop.PopulationSliceSampler(popsize=13, nsteps=5, generate_direction=getattr(pop, name), scale=0.8)
        out, nfound = [], 0
        for it in range(300):
            Lmin = Ls[order[min(nfound // 3, len(order) - 50)]]
            res = sampler.__next__(region, Lmin, u, Ls, inputs.walker_transform, inputs.walker_loglike)
            nfound += res[0] is not None
            out.append(res)
        return out, sampler.state(), sampler.scale, np.random.uniform(), type(sampler._walkers).__name__

    with monkeypatch.context() as mp:
        oracle_backend.install_stepfuncs(mp)
        want, want_state, want_scale, want_next, cls = run()
        assert cls == "OracleWalkers"
    got, got_state, got_scale, got_next, cls = run()
    assert cls == "_Walkers"
    nfound = 0
    for it, ((ua, pa, La, nca), (ub, pb, Lb, ncb)) in enumerate(zip(got, want)):
        assert nca == ncb and (ua is None) == (ub is None), it
        if ua is not None:
            nfound += 1
            assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and La == Lb, it
    assert nfound > 10
    assert np.array_equal(got_state["generation"], want_state["generation"])
    assert np.array_equal(got_state["allL"], want_state["allL"], equal_nan=True)
    assert got_scale == want_scale and got_next == want_next


# ---- the device forms against each other -----------------------------------------------------------------------------

def _ball_problem(d, nlive, seed):
    """test_popstepsampler's: {L > Lmin} is a ball of radius R around 0.5; live points uniform in it"""
    rs = np.random.RandomState(seed)
    Rb = 0.3
    z = rs.normal(size=(nlive, d))
    z *= (Rb * rs.uniform(size=(nlive, 1))**(1. / d)) / np.linalg.norm(z, axis=1).reshape((-1, 1))
    sigma = 0.1
    return 0.5 + z, sigma, -0.5 * (Rb / sigma)**2, Rb


@functools.lru_cache(maxsize=None)
def _gpu_region(d, nlive, seed):
    import ultranest_amd.mlfriends as m
    u = _ball_problem(d, nlive, seed)[0]
    layer = m.AffineLayer()
    layer.optimize(u, u)
    region = m.MLFriends(u, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    return region


def _same_runs(a, b, least):
    nfound = 0
    for (ua, pa, La, nca), (ub, pb, Lb, ncb) in zip(a, b):
        assert nca == ncb and (ua is None) == (ub is None)
        if ua is not None:
            nfound += 1
            assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and La == Lb
    assert nfound > least, nfound


@pytest.mark.parametrize("d", [130, 200])
@pytest.mark.parametrize("direction", ["generate_mixture_random_direction", "generate_region_random_direction"])
def test_graph_replay_equals_kernel_by_kernel_launches(d, direction):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods
    from ultranest_amd.regions import DeviceRNG
    region = _gpu_region(d, 300, 21)
    u = region.u
    sigma = 0.1
    loglike = likelihoods.GaussLikelihood(0.5, sigma, d)
    Ls = loglike(u)
    thresholds = np.sort(Ls)
    runs = []
    for graph in (True, False):
        sampler = pop.PopulationSliceSampler(popsize=96, nsteps=8, generate_direction=getattr(pop, direction), scale=0.3,
                                             device_rng=DeviceRNG(77))
        sampler.use_graph = graph
        sampler.max_rounds = 1
        out, nfound = [], 0
        for it in range(400):
            Lcut = thresholds[min(nfound // 4, 200)]          # rising threshold: step_back and restarts happen
            res = sampler.__next__(region, Lcut, u, Ls, likelihoods.identity_transform, loglike)
            nfound += res[0] is not None
            out.append(res)
        runs.append((out, sampler.scale, sampler.ringindex, sampler.device_rng.offset, sampler.state()))
    (a, scale_a, ring_a, off_a, st_a), (b, scale_b, ring_b, off_b, st_b) = runs
    assert scale_a == scale_b and ring_a == ring_b and off_a == off_b
    _same_runs(a, b, 30)
    for key in st_a:
        assert np.array_equal(st_a[key], st_b[key], equal_nan=True), key


@pytest.mark.parametrize("d,direction,max_rounds", [
    (130, "generate_mixture_random_direction", 4), (130, "generate_region_random_direction", -4),
    (200, "generate_region_random_direction", 4), (200, "generate_mixture_random_direction", -4),
    (130, "generate_cube_oriented_direction", 4), (200, "generate_random_direction", -4)])
def test_rounds_equal_single_steps(d, direction, max_rounds):
    """mlf_walkers_rounds_dev above 128 dimensions (the memory form, whichever sign max_rounds has) against one
    mlf_walkers_step_dev call per round, driven as test_popstepsampler's test of this name drives them: same points,
    likelihoods, counts, scale, ring index, Philox offset, per-round statistics and resident state, bit for bit."""
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods
    from ultranest_amd.regions import DeviceRNG
    region = _gpu_region(d, 300, 21)
    u = region.u
    loglike, transform = likelihoods.GaussLikelihood(0.5, 0.1, d), likelihoods.identity_transform
    Ls = loglike(u)
    thresholds = np.sort(Ls)
    runs = []
    for mr in (1, max_rounds):
        sampler = pop.PopulationSliceSampler(popsize=64, nsteps=7, generate_direction=getattr(pop, direction), scale=0.4,
                                             device_rng=DeviceRNG(31))
        sampler.max_rounds = mr
        out = []
        for it in range(40):
            Lcut = thresholds[min(it // 3, len(Ls) // 2)]
            nc_total, calls = 0, 0
            while True:
                unew, pnew, Lnew, nc = sampler.__next__(region, Lcut, u, Ls, transform, loglike)
                nc_total += nc
                calls += 1
                assert calls < 5000
                if unew is not None:
                    break
            out.append((unew, pnew, Lnew, nc_total))
        runs.append((out, sampler.scale, sampler.ringindex, sampler.device_rng.offset, np.array(sampler.logstat), sampler.state()))
    (a, scale_a, ring_a, off_a, log_a, st_a), (b, scale_b, ring_b, off_b, log_b, st_b) = runs
    for (ua, pa, La, nca), (ub, pb, Lb, ncb) in zip(a, b):
        assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and La == Lb and nca == ncb
    assert scale_a == scale_b and ring_a == ring_b and off_a == off_b
    assert log_a.shape == log_b.shape and np.array_equal(log_a, log_b)
    for key in st_a:
        assert np.array_equal(st_a[key], st_b[key], equal_nan=True), key


@pytest.mark.parametrize("d", [130, 200])
def test_resident_likelihood_equals_host_callbacks(d):
    """Same numpy stream, once with numpy callbacks and once with the device-evaluated Rosenbrock pair: transformed points bit
    for bit, likelihoods to 1e-12, so the trajectories coincide."""
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods
    rs = np.random.RandomState(3)
    u = 0.5 + 0.04 * rs.normal(size=(300, d))
    region = _host_region(d, u)

    def host_transform(x):
        return x * 20 - 10

    def host_loglike(theta):
        a, b = theta[:, :-1], theta[:, 1:]
        return -2 * (100 * (b - a**2)**2 + (1 - a)**2).sum(axis=1)

    Ls = host_loglike(host_transform(u))
    Lmin = np.sort(Ls)[5]
    runs = []
    for transform, loglike in [(host_transform, host_loglike),
                               (likelihoods.rosenbrock_transform, likelihoods.rosenbrock_loglike)]:
        np.random.seed(8)
        sampler = pop.PopulationSliceSampler(popsize=32, nsteps=6, generate_direction=pop.generate_mixture_random_direction,
                                             scale=0.5)
        runs.append([sampler.__next__(region, Lmin, u, Ls, transform, loglike) for _ in range(300)])
    nfound = 0
    for (ua, pa, La, nca), (ub, pb, Lb, ncb) in zip(*runs):
        assert nca == ncb and (ua is None) == (ub is None)
        if ua is not None:
            nfound += 1
            assert np.array_equal(ua, ub) and np.array_equal(pa, pb)
            assert abs(La - Lb) <= 1e-12 * abs(La)
    assert nfound > 20


def _philox_walk(transform, loglike, region, u, Ls, Lmin, calls=300):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    s = pop.PopulationSliceSampler(popsize=32, nsteps=6, generate_direction=pop.generate_mixture_random_direction, scale=0.5,
                                   device_rng=DeviceRNG(5))
    s.max_rounds, s.use_graph = 1, False         # one step per call, the route a user model takes
    return [s.__next__(region, Lmin, u, Ls, transform, loglike) for _ in range(calls)], s.device_rng.offset


@pytest.mark.parametrize("d", [130, 200])
def test_user_gauss_equals_the_builtin_pair(d):
    """usermodels.gauss(d) through mlf_walkers_step_user against the built-in Gaussian pair through mlf_walkers_step_dev, Philox
    mode: the same records (above 128 dimensions both evaluate a row on one thread, terms in ascending order)."""
    from ultranest_amd import likelihoods as lk, usermodels
    G = usermodels.gauss(d)
    builtin = lk.GaussLikelihood(usermodels.gauss_centers(d), 0.1, d)
    rs = np.random.RandomState(4)
    u = np.clip(usermodels.gauss_centers(d) + 0.08 * rs.normal(size=(300, d)), 0.01, 0.99)
    region = _host_region(d, u)
    Ls = builtin(u)
    Lmin = np.sort(Ls)[5]
    a, off_a = _philox_walk(lk.identity_transform, builtin, region, u, Ls, Lmin)
    b, off_b = _philox_walk(G.transform, G.loglike, region, u, Ls, Lmin)
    assert off_a == off_b
    _same_runs(a, b, 20)


def test_derived_parameters_at_130_dimensions():
    """a user model with derived parameters returns p rows d + Q wide whose first d columns are the model's without them"""
    from ultranest_amd import usermodels
    d, Q = 130, 3
    m, g = usermodels.gauss_derived(d), usermodels.gauss(d)
    rs = np.random.RandomState(4)
    u = np.clip(usermodels.gauss_centers(d) + 0.08 * rs.normal(size=(300, d)), 0.01, 0.99)
    region = _host_region(d, u)
    Ls = g.loglike(g.transform(u))
    Lmin = np.sort(Ls)[5]
    (wide, off_w), (narrow, off_n) = (_philox_walk(x.transform, x.loglike, region, u, Ls, Lmin, calls=150) for x in (m, g))
    assert off_w == off_n
    nfound = 0
    for (ua, pa, La, nca), (ub, pb, Lb, ncb) in zip(wide, narrow):
        assert nca == ncb and (ua is None) == (ub is None)
        if ua is None:
            continue
        nfound += 1
        assert np.array_equal(ua, ub) and La == Lb
        assert pa.shape == (d + Q,) and pb.shape == (d,)
        assert np.array_equal(pa[:d], pb) and np.array_equal(pa[d:], usermodels.gauss_derived_columns(pb[None, :])[0])
    assert nfound > 5


def test_dimensionality_bounds_of_create():
    from ultranest_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.mlf_walkers_create(ctypes.byref(h), 3, 2, 1025) == 2        # MLF_E_DIM
    assert not h.value and b"1024" in L.mlf_last_error()
    for _ in range(2):
        h = ctypes.c_void_p()
        assert L.mlf_walkers_create(ctypes.byref(h), 3, 2, 1024) == 0 and h.value
        assert L.mlf_walkers_destroy(h) == 0


# ---- invariance ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", ["generate_region_random_direction", "generate_mixture_random_direction"])
def test_slice_sampling_is_uniform_under_the_threshold_at_130_dimensions(direction):
    from scipy import stats
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods
    from ultranest_amd.regions import DeviceRNG
    d = 130
    region = _gpu_region(d, 400, 11)
    u, sigma, Lmin, Rb = _ball_problem(d, 400, 11)
    loglike = likelihoods.GaussLikelihood(0.5, sigma, d)
    norm = -0.5 * np.log(2 * np.pi * sigma**2) * d
    Ls = loglike(u)
    sampler = pop.PopulationSliceSampler(popsize=256, nsteps=8, generate_direction=getattr(pop, direction), scale=0.3,
                                         device_rng=DeviceRNG(5))
    pts, Lout = [], []
    for _ in range(6000):
        unew, pnew, Lnew, nc = sampler.__next__(region, Lmin + norm, u, Ls, likelihoods.identity_transform, loglike)
        if unew is not None:
            pts.append(unew)
            Lout.append(Lnew)
            assert np.array_equal(unew, pnew)
        if len(pts) >= 1500:
            break
    pts, Lout = np.array(pts), np.array(Lout)
    assert len(pts) >= 1500, len(pts)
    assert (Lout > Lmin + norm).all()
    assert np.allclose(Lout, loglike(pts), rtol=1e-12, atol=1e-12)
    r = np.linalg.norm(pts - 0.5, axis=1) / Rb
    assert r.max() < 1
    p = stats.kstest(r[::3]**d, "uniform").pvalue       # thinned: walkers that shared a start point are correlated
    print("KS p-value of r^d against uniform: %.3g" % p)
    assert p > 1e-3
    # a coordinate that never moves is caught here
    assert (np.abs(pts - 0.5).max(axis=0) > 1e-6).all()
    assert (pts.max(axis=0) > pts.min(axis=0)).all()
    # ... and so is one that only ever keeps its start value (every direction of these two kinds moves every coordinate)
    fresh = np.array([(~np.isin(pts[:, k], u[:, k])).any() for k in range(d)])
    assert fresh.all(), np.flatnonzero(~fresh)
