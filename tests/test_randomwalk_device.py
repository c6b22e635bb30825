"""PopulationRandomWalkSampler's device route (csrc/mlf_rwalk.hip): routing and the truncated-normal formula on the CPU; on
the GPU one step against the numpy restatement (tests/randomwalk_reference.py), the two forms bit for bit, a user model
against the built-in pair, the Philox stream discipline, invariance of the uniform distribution under a hard contour, the
sampler's bookkeeping against the host path's formulas, and nested sampling end to end."""
import io
import types

import numpy as np
import pytest

import randomwalk_reference as R


# ---- CPU -------------------------------------------------------------------------------------------------------------

def test_routing_of_the_refill():
    """device_rng x generate_direction x model -> device or host, decided in PopulationRandomWalkSampler._device_route."""
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods as lk, usermodels
    from ultranest_amd.regions import DeviceRNG

    def foreign_direction(ui, region, scale=1):
        return pop.generate_random_direction(ui, region, scale)

    m = usermodels.rosenbrock(7)
    gauss = lk.GaussLikelihood(0.5, 0.1, 7)
    models = {
        "builtin": (lk.rosenbrock_transform, lk.rosenbrock_loglike),
        "builtin-gauss": (lk.identity_transform, gauss),
        "user": (m.transform, m.loglike),
        "user-identity": (lk.identity_transform, m.loglike),
        "callback": (lambda u: u, lambda p: -(p**2).sum(axis=1)),
        "builtin-transform-only": (lk.rosenbrock_transform, lambda p: -(p**2).sum(axis=1)),
        "user-with-foreign-transform": (lk.rosenbrock_transform, m.loglike),
        "user-transform-with-foreign-loglike": (m.transform, lk.rosenbrock_loglike),
    }
    on_device = {"builtin", "builtin-gauss", "user", "user-identity"}
    for with_rng in (False, True):
        for direction in (pop.generate_mixture_random_direction, foreign_direction):
            s = pop.PopulationRandomWalkSampler(popsize=8, nsteps=3, generate_direction=direction, scale=0.5,
                                                device_rng=DeviceRNG(3) if with_rng else None)
            for name, (transform, loglike) in models.items():
                route = s._device_route(transform, loglike)
                want = with_rng and direction is not foreign_direction and name in on_device
                assert (route is not None) == want, (with_rng, direction.__name__, name, route)
                if route is None:
                    continue
                kind, tspec, lspec, user = route
                assert kind == 6
                if name.startswith("user"):
                    assert tspec is None and lspec is None and user == (m, name == "user")
                else:
                    assert user is None and tspec == transform.device_spec and lspec[0] == loglike.device_spec[0]
    s = pop.PopulationRandomWalkSampler(popsize=8, nsteps=3, generate_direction=pop.generate_random_direction, scale=0.5,
                                        device_rng=DeviceRNG(3))
    assert s._device_route(*models["builtin"], 128) is not None and s._device_route(*models["builtin"], 129) is None
    with pytest.raises(TypeError):
        pop.PopulationRandomWalkSampler(popsize=8, nsteps=3, generate_direction=pop.generate_random_direction, scale=0.5,
                                        device_rng=np.random.RandomState(1))
    # without device_rng the constructor leaves what it always set
    s = pop.PopulationRandomWalkSampler(5, 4, pop.generate_random_direction, 0.7, scale_adapt_factor=0.8, scale_min=1e-3,
                                        scale_max=3, log=True, logfile=None)
    had = dict(popsize=5, nsteps=4, generate_direction=pop.generate_random_direction, scale=0.7, scale_adapt_factor=0.8,
               scale_min=1e-3, scale_max=3, nrejects=0, ncalls=0, log=True, logfile=None, logstat=[], prepared_samples=[],
               logstat_labels=['accept_rate', 'efficiency', 'scale', 'far_enough', 'mean_rel_jump'])
    for k, v in had.items():
        assert getattr(s, k) == v, k
    assert s.device_rng is None
    assert str(s) == 'PopulationRandomWalkSampler(popsize=5, nsteps=4, generate_direction=%s, scale=0.7)' % (
        pop.generate_random_direction)


def test_truncated_normal_formula_against_scipy():
    """The restated inverse CDF (what the kernel implements) against scipy.stats.truncnorm.ppf: 2 10^5 draws, a < 0 < b with
    magnitudes from 0.1 to 10^6.  Measured with these draws: 2.3e-13 absolute at most (up to 6.9e-12 with others: scipy's own
    path and 1 - q condition differently in the far tail); asserted <= 1e-10 and containment in [a, b]."""
    from scipy import stats
    rs = np.random.RandomState(7)
    n = 200000
    a = -10.0**rs.uniform(-1, 6, size=n)
    b = 10.0**rs.uniform(-1, 6, size=n)
    q = rs.uniform(size=n)
    t = R.truncnorm_icdf(a, b, q)
    want = stats.truncnorm.ppf(q, a, b)
    assert np.isfinite(t).all() and np.isfinite(want).all()
    assert (t >= a).all() and (t <= b).all()
    dev = np.abs(t - want).max()
    print("largest deviation from scipy.stats.truncnorm.ppf: %.3g" % dev)
    assert dev <= 1e-10, dev


# ---- GPU -------------------------------------------------------------------------------------------------------------

def _np_gauss(centers, sigma):
    def loglike(p):
        return -0.5 * (((p - centers) / sigma)**2).sum(axis=1) - 0.5 * np.log(2 * np.pi * sigma**2) * p.shape[1]
    return loglike


def _np_rosenbrock(p):
    a, b = p[:, :-1], p[:, 1:]
    return -2 * (100 * (b - a**2)**2 + (1 - a)**2).sum(axis=1)


def _np_eggbox(p):
    return (2 + np.cos(p / 2.0).prod(axis=1))**5


def _problem(name, d, nlive, seed):
    """(live points, device transform, device loglike, numpy transform, numpy loglike)"""
    from ultranest_amd import likelihoods as lk
    rs = np.random.RandomState(seed)
    if name == "gauss":
        centers = np.full(d, 0.5)
        u = np.clip(0.5 + 0.15 * rs.normal(size=(nlive, d)), 0.01, 0.99)
        return u, lk.identity_transform, lk.GaussLikelihood(0.5, 0.1, d), (lambda x: np.array(x)), _np_gauss(centers, 0.1)
    if name == "rosenbrock":
        u = np.clip(0.5 + 0.04 * rs.normal(size=(nlive, d)), 0.01, 0.99)
        return u, lk.rosenbrock_transform, lk.rosenbrock_loglike, (lambda x: x * 20 + -10.0), _np_rosenbrock
    assert name == "eggbox"
    u = rs.uniform(0.02, 0.98, size=(nlive, d))
    return u, lk.eggbox_transform, lk.eggbox_loglike, (lambda x: (x * 10.0) * np.pi), _np_eggbox


def _affine_region(u):
    import ultranest_amd.mlfriends as m
    layer = m.AffineLayer()
    layer.optimize(u, u)
    region = m.MLFriends(u, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    return region


def _scaling_region(u):
    import ultranest_amd.mlfriends as m
    layer = m.ScalingLayer(mean=u.mean(axis=0), std=u.std(axis=0))
    return types.SimpleNamespace(u=u, transformLayer=layer, maxradiussq=0.5)


def _walkers(region, us, Ls, P, nsteps, kind):
    """A population handle with the region's copies and the live points on the device, as _refill_on_device sets it up."""
    import ultranest_amd.popstepsampler as pop
    w = pop._RandomWalkers(P, nsteps, us.shape[1])
    pop._sync_region_copies(w, dict(region=None, layer=None, r2=None, calls=0), region, us.shape[1], kind, skip_live=True)
    w.set_live(us, Ls)
    return w


PER_WALKER = ("u", "p", "L", "start", "ever", "last", "tleft", "tright")
COUNTS = ("nrejects", "nlast", "nfar", "sumlog", "nnever")


def _same(a, b):
    for k in PER_WALKER:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in COUNTS:
        assert a[k] == b[k], (k, a[k], b[k])


ONE_STEP = [("gauss", 2, 3, 2, 31), ("rosenbrock", 5, 1100, 2, 32), ("gauss", 50, 70, 4, 33), ("rosenbrock", 66, 70, 2, 34),
            ("gauss", 66, 70, 6, 35)] + [("gauss" if k % 2 else "rosenbrock", 6, 70, k, 40 + k) for k in range(7)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,d,P,kind,seed", ONE_STEP)
def test_one_step_against_the_restatement(name, d, P, kind, seed):
    """nsteps = 1: start rows exact; tleft, tright and the accepted proposals within 1e-12 max(1, |t|) |v|_inf (evaluating
    on the smaller tail bounds p / phi(t) by 1.25, so a few ulp in Phi and Phi^-1 give |dt| of order 1e-15; the bound leaves
    two to three decades); accept masks equal wherever the restated |Lnew - Lmin| > 1e-9 max(1, |Lmin|), at most 1 % of the
    walkers excluded; the counts follow from the masks."""
    from ultranest_amd.regions import DeviceRNG
    us, transform, loglike, np_transform, np_loglike = _problem(name, d, 400, seed)
    region = _affine_region(us)
    Ls = np_loglike(np_transform(us))
    Lmin = np.sort(Ls)[100]
    scale = {0: 0.02, 1: 0.3, 2: 0.05, 3: 0.5, 4: 0.5, 5: 0.5, 6: 0.5}[kind]
    if name == "rosenbrock":
        scale *= 0.3
    layer = region.transformLayer
    ref = R.refill(seed, 77, us, Ls, Lmin, kind, scale, P, 1, np_transform, np_loglike, axes=layer.axes,
                   std=us.std(axis=0), whiten=layer.transform, maxradiussq=region.maxradiussq)
    st = ref["steps"][0]
    undecided = np.logical_and(st["inside"], np.abs(st["Lnew"] - Lmin) <= 1e-9 * max(1.0, abs(Lmin)))
    assert undecided.sum() <= 0.01 * P, undecided.sum()       # (the restatement alone: holds for the seeds chosen here)

    rng = DeviceRNG(seed)
    rng.offset = 77
    w = _walkers(region, us, Ls, P, 1, kind)
    got = w.refill(Lmin, kind, scale, rng, transform.device_spec, loglike.device_spec)
    assert rng.offset == ref["next_offset"]
    assert got["chain_form"] == (d % 2 == 1 or d > 64)
    assert np.array_equal(got["start"], ref["start"])
    vmax = np.abs(st["v"]).max(axis=1)
    for side in ("tleft", "tright"):
        bound = 1e-12 * np.maximum(1.0, np.abs(st[side])) * vmax
        dev = np.abs(got[side] - st[side])
        print("%s: largest deviation / bound = %.3g" % (side, (dev / bound).max()))
        assert (dev <= bound).all(), (side, (dev / bound).max())
    decided = ~undecided
    assert np.array_equal(got["last"][decided], st["accepted"][decided])
    assert np.array_equal(got["ever"], got["last"])
    both = np.logical_and(got["last"], st["accepted"])
    if P >= 70:
        assert both.any() and (~got["last"]).any()          # the case exercises both outcomes
    bound = (1e-12 * np.maximum(1.0, np.abs(st["t"])) * vmax)[:, None]
    dev = np.abs(got["u"] - st["unew"])[both]
    if both.any():
        print("unew: largest deviation / bound = %.3g" % (dev / bound[both]).max())
    assert (dev <= bound[both]).all()
    assert np.array_equal(got["p"][both], np_transform(got["u"][both]))
    assert np.allclose(got["L"][both], st["Lnew"][both], rtol=1e-12, atol=1e-9)
    # walkers that did not move keep their start row, its likelihood, and no transformed point
    stay = ~got["last"]
    assert np.array_equal(got["u"][stay], us[got["start"][stay]]) and np.array_equal(got["L"][stay], Ls[got["start"][stay]])
    assert np.isnan(got["p"][stay]).all()
    # counts from the device's own masks
    assert got["nrejects"] == int(stay.sum()) and got["nlast"] == int(got["last"].sum()) and got["nnever"] == int(stay.sum())
    d2 = ((layer.transform(us[got["start"][got["last"]]]) - layer.transform(got["u"][got["last"]]))**2).sum(axis=1)
    r2 = region.maxradiussq
    close = int((np.abs(d2 - r2) <= 1e-9 * r2).sum())
    assert abs(got["nfar"] - (d2 > r2).sum()) <= close
    assert np.isclose(got["sumlog"], np.log(np.sqrt(d2) / np.sqrt(r2) + 1e-10).sum(), rtol=1e-9, atol=1e-9)


FORMS = [("eggbox", 2, 1, 2, "affine"), ("eggbox", 2, 70, 5, "affine"), ("gauss", 10, 70, 6, "affine"),
         ("gauss", 10, 1, 5, "none"), ("rosenbrock", 50, 70, 2, "affine"), ("eggbox", 50, 70, 6, "affine"),
         ("rosenbrock", 50, 1, 5, "affine"), ("rosenbrock", 7, 70, 6, "affine"), ("gauss", 10, 70, 5, "scaling")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,d,P,kind,layer", FORMS)
def test_fused_form_equals_chain_form(name, d, P, kind, layer):
    """nsteps = 7, once as the shape chooses (one launch where the fused form covers it) and once forced through the chain
    form: every output array, the counts and the returned offset are equal bit for bit.  Odd d and the scaling layer take the
    chain form in both runs."""
    from ultranest_amd.regions import DeviceRNG
    us, transform, loglike, np_transform, np_loglike = _problem(name, d, 300, 50 + d)
    region = _scaling_region(us) if layer == "scaling" else _affine_region(us)
    if layer == "none":
        region.maxradiussq = None
    Ls = np_loglike(np_transform(us))
    Lmin = np.sort(Ls)[60]
    scale = 0.5 if kind != 2 else 0.05
    runs = []
    for force_chain in (False, True):
        rng = DeviceRNG(9)
        rng.offset = 12345
        w = _walkers(region, us, Ls, P, 7, kind)
        runs.append((w.refill(Lmin, kind, scale, rng, transform.device_spec, loglike.device_spec, force_chain=force_chain),
                     rng.offset))
    (a, off_a), (b, off_b) = runs
    assert a["chain_form"] == (d % 2 == 1 or layer == "scaling") and b["chain_form"]
    _same(a, b)
    assert off_a == off_b == R.next_offset(12345, P, 7, d)
    if P >= 70:
        assert a["ever"].any() and a["nrejects"] > 0
    if layer == "none":
        assert a["nfar"] == 0 and a["sumlog"] == 0


@pytest.mark.gpu
def test_user_model_equals_the_builtin_pair():
    """The Rosenbrock DeviceModel of usermodels.py (with its transform) against the built-in pair at d = 7, where
    tests/test_devicemodel_gpu.py shows the two likelihoods bit-identical; nsteps = 5: all outputs identical."""
    from ultranest_amd import usermodels
    from ultranest_amd.regions import DeviceRNG
    d, P = 7, 70
    us, transform, loglike, np_transform, np_loglike = _problem("rosenbrock", d, 300, 61)
    region = _affine_region(us)
    Ls = loglike(transform(us))
    Lmin = np.sort(Ls)[60]
    m = usermodels.rosenbrock(d)
    runs = []
    for user in (None, (m, True)):
        rng = DeviceRNG(10)
        w = _walkers(region, us, Ls, P, 5, 6)
        runs.append(w.refill(Lmin, 6, 0.3, rng, transform.device_spec, loglike.device_spec, user))
    _same(*runs)
    assert runs[0]["ever"].any() and runs[0]["nrejects"] > 0 and runs[1]["chain_form"]


@pytest.mark.gpu
def test_stream_discipline():
    """Same seed and offset: identical results; the offset advances by P nsteps ((d + 1) / 2 + 2); the next refill differs;
    and since every draw is a function of (seed, offset, walker, step) only, popsize 64 and 65 give the same first 64
    walkers."""
    from ultranest_amd.regions import DeviceRNG
    d, nsteps, kind = 10, 4, 6
    us, transform, loglike, np_transform, np_loglike = _problem("gauss", d, 300, 62)
    region = _affine_region(us)
    Ls = np_loglike(us)
    Lmin = np.sort(Ls)[60]
    args = (Lmin, kind, 0.5)
    specs = (transform.device_spec, loglike.device_spec)
    w = _walkers(region, us, Ls, 64, nsteps, kind)
    rng = DeviceRNG(11)
    a = w.refill(*args, rng, *specs)
    assert rng.offset == 64 * nsteps * ((d + 1) // 2 + 2)
    b = w.refill(*args, rng, *specs)
    assert rng.offset == 2 * 64 * nsteps * ((d + 1) // 2 + 2)
    assert not np.array_equal(a["u"], b["u"]) and not np.array_equal(a["start"], b["start"])
    rng2 = DeviceRNG(11)
    _same(a, w.refill(*args, rng2, *specs))
    _same(b, w.refill(*args, rng2, *specs))
    for force_chain in (False, True):
        c = _walkers(region, us, Ls, 65, nsteps, kind).refill(*args, DeviceRNG(11), *specs, force_chain=force_chain)
        for k in PER_WALKER:
            assert np.array_equal(c[k][:64], a[k], equal_nan=True), (k, force_chain)


def _ball_problem(d, nlive, seed):
    """Gaussian shell threshold: {L > Lmin} is a ball of radius R around 0.5; live points uniform in it
    (the problem of tests/test_popstepsampler.py)."""
    rs = np.random.RandomState(seed)
    R_ = 0.3
    z = rs.normal(size=(nlive, d))
    z *= (R_ * rs.uniform(size=(nlive, 1))**(1. / d)) / np.linalg.norm(z, axis=1).reshape((-1, 1))
    sigma = 0.1
    return 0.5 + z, sigma, -0.5 * (R_ / sigma)**2, R_


@pytest.mark.gpu
@pytest.mark.parametrize("direction,scale", [("generate_random_direction", 0.05), ("generate_region_random_direction", 0.4)])
def test_walk_is_uniform_under_the_threshold(direction, scale):
    """A hard likelihood contour (the ball problem, d = 3, 400 live points): several refills of 256 walkers x 20 steps return
    points with L > Lmin whose radii are uniform in the ball (the KS bound of the slice sampler's test).  The steps are short
    against the distance to the cube's faces, so the truncation of the normal (which alone breaks the proposal's symmetry)
    stays below 4 sigma."""
    from scipy import stats
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods
    from ultranest_amd.regions import DeviceRNG
    d = 3
    u, sigma, Lmin, R_ = _ball_problem(d, 400, 11)
    region = _affine_region(u)
    loglike = likelihoods.GaussLikelihood(0.5, sigma, d)
    norm = -0.5 * np.log(2 * np.pi * sigma**2) * d
    Ls = loglike(u)
    sampler = pop.PopulationRandomWalkSampler(popsize=256, nsteps=20, generate_direction=getattr(pop, direction),
                                              scale=scale, device_rng=DeviceRNG(5))
    pts, Lout = [], []
    for _ in range(6 * 256):
        unew, pnew, Lnew, nc = sampler.__next__(region, Lmin + norm, u, Ls, likelihoods.identity_transform, loglike)
        pts.append(unew)
        Lout.append(Lnew)
        assert np.array_equal(unew, pnew)
    pts, Lout = np.array(pts), np.array(Lout)
    assert len(sampler.logstat) == 6
    assert (Lout > Lmin + norm).all()
    assert np.allclose(Lout, loglike(pts), rtol=1e-12, atol=1e-12)
    r = np.linalg.norm(pts - 0.5, axis=1) / R_
    assert r.max() < 1
    assert stats.kstest(r[::3]**d, "uniform").pvalue > 1e-3
    assert np.abs((pts - 0.5).mean(axis=0)).max() < 0.03
    assert 0 <= sampler.far_enough_fraction <= 1 and np.isfinite(sampler.mean_jump_distance)


@pytest.mark.gpu
def test_sampler_bookkeeping_follows_the_host_formulas():
    """After a device refill nrejects, the logstat row (six entries), the logfile line and the adapted scale are what the
    host path's expressions give from the device's counts; prepared_samples hands out popsize triples, nc = nsteps popsize
    on the refilling call and 0 afterwards."""
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    d, P, nsteps = 6, 50, 8
    us, transform, loglike, np_transform, np_loglike = _problem("rosenbrock", d, 300, 63)
    region = _affine_region(us)
    Ls = np_loglike(np_transform(us))
    Lmin = Ls.min() - 1.0        # (every walker starts above the threshold: none rejects all its moves, restated on the CPU)
    log = io.StringIO()
    s = pop.PopulationRandomWalkSampler(popsize=P, nsteps=nsteps, generate_direction=pop.generate_mixture_random_direction,
                                        scale=0.4, scale_adapt_factor=0.8, logfile=log, device_rng=DeviceRNG(6))
    scale, nrejects = s.scale, 0
    for refill in range(3):
        for j in range(P):
            unew, pnew, Lnew, nc = s.__next__(region, Lmin, us, Ls, transform, loglike)
            assert nc == (nsteps * P if j == 0 else 0)
            if j == 0:
                out = s.last_refill
                assert len(s.prepared_samples) == P - 1
            assert np.array_equal(unew, out["u"][j]) and np.array_equal(pnew, out["p"][j]) and Lnew == out["L"][j]
            assert Lnew > Lmin
        assert not s.prepared_samples
        nmoves = nsteps * P
        target = nmoves * (1 - 0.234)
        expected = nrejects + target
        nrejects += out["nrejects"]
        assert s.nrejects == nrejects
        row = [out["last"].mean(), 1 - (nrejects - (expected - target)) / nmoves, scale, nsteps,
               out["nfar"] / out["nlast"], np.exp(out["sumlog"] / out["nlast"])]
        assert len(s.logstat) == refill + 1 and s.logstat[-1] == row, (s.logstat[-1], row)
        line = "rescale\t%.4f\t%.4f\t%g\t%.4f%g\n" % (row[0], row[1], row[2], row[4], row[5])
        assert log.getvalue().splitlines(True)[-1] == line
        if nrejects > expected and scale > s.scale_min:
            scale *= 0.8
        elif nrejects < expected and scale < s.scale_max:
            scale /= 0.8
        assert s.scale == scale
        assert out["nlast"] == out["last"].sum() and out["nrejects"] + out["ever"].sum() <= nmoves


@pytest.mark.gpu
def test_walkers_that_never_moved_raise_the_host_assertion():
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    us, transform, loglike, np_transform, np_loglike = _problem("gauss", 4, 100, 64)
    region = _affine_region(us)
    Ls = np_loglike(us)
    s = pop.PopulationRandomWalkSampler(popsize=20, nsteps=3, generate_direction=pop.generate_random_direction, scale=0.1,
                                        device_rng=DeviceRNG(7))
    with pytest.raises(AssertionError, match="some walkers never moved! Double nsteps of PopulationRandomWalkSampler."):
        s.__next__(region, 1e300, us, Ls, transform, loglike)
    assert s.last_refill["nnever"] == 20 and s.nrejects == 60 and not s.last_refill["ever"].any()


def _truncated_gauss_logz(centers, sigma):
    from scipy.special import ndtr
    return float(np.log(ndtr((1 - centers) / sigma) - ndtr(-centers / sigma)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["builtin", "user"])
def test_nested_sampling_with_the_random_walk_sampler(model):
    """End to end: static nested sampling of a 4-d Gaussian with random-walk replacements on the device recovers the
    analytic evidence within 3 logzerr, with the built-in likelihood and with the same Gaussian as a user DeviceModel (at
    even d the two likelihoods differ in their last bits, so the runs are compared with the truth, not with each other).

    scale: the sampler steers its scale towards 23 % acceptance, where a walker rejects all 16 moves with probability 1.4 %
    ("some walkers never moved").  0.02 is the largest start at which the scale (x 1 / 0.9 per refill, about 13 refills)
    stays below the final contour's radius (0.06), so that acceptance stays above 40 %; smaller scales mix worse.  Sixteen
    steps are a short walk: restated in numpy (randomwalk_reference.refill inside a plain nested-sampling loop) ln Z scatters
    by several logzerr between seeds and scales (-8.6 ... +6.3 over 16 runs at 0.012-0.03), -1.1 at these."""
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods, usermodels
    from ultranest_amd.harness import StaticNestedSampler
    from ultranest_amd.regions import DeviceRNG
    d, sigma = 4, 0.05
    if model == "builtin":
        loglike = likelihoods.GaussLikelihood.docs_gauss(d, sigma)
        centers = loglike.centers
    else:
        m = usermodels.gauss(d, sigma)
        loglike, centers = m.loglike, usermodels.gauss_centers(d, sigma)
    step = pop.PopulationRandomWalkSampler(popsize=256, nsteps=16, generate_direction=pop.generate_random_direction,
                                           scale=0.02, device_rng=DeviceRNG(4))
    s = StaticNestedSampler(d, loglike, transform=likelihoods.identity_transform, num_live_points=200, seed=2,
                            stepsampler=step)
    res = s.run(dlogz=0.2)
    truth = _truncated_gauss_logz(centers, sigma)
    print("logz %.4f +- %.4f, truth %.4f, %d likelihood calls" % (res["logz"], res["logzerr"], truth, res["ncall"]))
    assert abs(res["logz"] - truth) < 3 * res["logzerr"], (res, truth)
    assert step._device_route(likelihoods.identity_transform, loglike) is not None and len(step.logstat) > 3
