"""PopulationRandomWalkSampler's and PopulationSimpleSliceSampler's device refills above 128 dimensions (the wide propose
kernels of csrc/mlf_rwalk.hip and csrc/mlf_sslice.hip, opt-in through ``device_max_dim``): the create bounds, one random-walk
step and a simple-slice refill against the numpy restatements (the cases of tests/test_wide_population_restatement.py, which
decide every comparison on the CPU), the exact parts bit for bit, user models against the built-in pair, the samplers'
bookkeeping and invariance of the uniform distribution at d = 130.

Tolerances.  Where the direction is a selection (kinds 0, 1, 3, 5 and both branches of 6) the bounds are those of the narrow
tests: 1e-12 max(1, |t|) |v|_inf.  Where it is a sum (kinds 2 and 4) the device's direction may differ from the restated one
by what tests/test_wide_walk_gpu.py asserts for dw_direction_wide -- dv = 1e-12 dirscale per coordinate for kind 2,
1e-12 dirscale |axes[r]|_2 for kind 4 -- and the bounds are widened by what that propagates to first order: a bound of the line
t1 = (-(u - 0.5) -+ 0.5) / v at its limiting coordinate k* moves by |t| dv[k*] / |v[k*]| (and by du / |v[k*]| where the point
itself carries an allowance du from earlier steps); a proposal u + t v by |t| max dv + |v|_inf dt."""
import ctypes
import io

import numpy as np
import pytest

import randomwalk_reference as R
import simpleslice_reference as S
import test_randomwalk_device as T
import test_simpleslice_device as SS
import test_wide_population_restatement as W

pytestmark = pytest.mark.gpu


# ---- 1. create bounds -----------------------------------------------------------------------------------------------------

def test_dimensionality_bounds_of_create():
    from ultranest_amd import _lib
    L = _lib.lib()
    head = (3, 2)                                                      # popsize, nsteps
    for create, destroy, tail in ((L.mlf_rwalk_create, L.mlf_rwalk_destroy, ()), (L.mlf_sslice_create, L.mlf_sslice_destroy, (5,))):
        h = ctypes.c_void_p()
        assert create(ctypes.byref(h), *head, 1025, *tail) == 2        # MLF_E_DIM
        assert not h.value and b"1024" in L.mlf_last_error()
        for d in (129, 1024):
            for _ in range(2):
                h = ctypes.c_void_p()
                assert create(ctypes.byref(h), *head, d, *tail) == 0 and h.value
                assert destroy(h) == 0


# ---- the allowances of the summing kinds ----------------------------------------------------------------------------------

def _dv(kind, dirscale, axes, d):
    """per coordinate: what test_wide_walk_gpu.py allows dw_direction_wide against the restatement"""
    if kind == 2:
        return np.full(d, 1e-12 * dirscale)
    if kind == 4:
        return 1e-12 * dirscale * np.linalg.norm(np.asarray(axes), axis=1)
    return np.zeros(d)


def _line_allowance(u, v, dv, du=None):
    """(allowance of tleft, of tright, |tleft|, |tright| of the cube intersection) per row: |t| dv[k*] / |v[k*]| (+ du /
    |v[k*]|) at the restatement's limiting coordinates"""
    P = len(u)
    if not dv.any():
        tl, tr = R.line_intersection(u, v)
        return np.zeros(P), np.zeros(P), np.abs(tl), np.abs(tr)
    with np.errstate(all="ignore"):
        m = 1.0 / v
        nn = m * (u - 0.5)
        kk = np.abs(m) * 0.5
        t1, t2 = -nn - kk, -nn + kk
    rows = np.arange(P)
    kl, kr = np.nanargmax(t1, axis=1), np.nanargmin(t2, axis=1)
    tl, tr = np.abs(t1[rows, kl]), np.abs(t2[rows, kr])
    du = np.zeros(P) if du is None else du
    return (tl * dv[kl] + du) / np.abs(v[rows, kl]), (tr * dv[kr] + du) / np.abs(v[rows, kr]), tl, tr


# ---- 2. one random-walk step against the restatement ----------------------------------------------------------------------

@pytest.mark.parametrize("case", W.RW_CASES, ids=W.rw_id)
def test_one_random_walk_step_against_the_restatement(case):
    """The assertions of test_randomwalk_device.py::test_one_step_against_the_restatement with the module's tolerances;
    dt of the truncated-normal draw = the sum of the two bounds' added terms (|dt / dlo| + |dt / dhi| of the inverse CDF on
    the smaller tail are each at most of order one)."""
    from ultranest_amd.regions import DeviceRNG
    name, d, P, kind, seed = case[:5]
    us, Ls, Lmin, region, scale, transform, loglike, np_transform, ref = W.rw_case(case)
    st = ref["steps"][0]
    undecided = W.rw_undecided(ref, Lmin)
    layer = region.transformLayer

    rng = DeviceRNG(seed)
    rng.offset = W.RW_OFFSET
    w = T._walkers(region, us, Ls, P, 1, kind)
    got = w.refill(Lmin, kind, scale, rng, transform.device_spec, loglike.device_spec)
    assert rng.offset == ref["next_offset"]
    assert got["chain_form"]
    assert np.array_equal(got["start"], ref["start"])
    dv = _dv(kind, scale, layer.axes, d)
    add_l, add_r, _, _ = _line_allowance(us[ref["start"]], st["v"], dv)
    vmax = np.abs(st["v"]).max(axis=1)
    for side, add in (("tleft", add_l), ("tright", add_r)):
        bound = 1e-12 * np.maximum(1.0, np.abs(st[side])) * vmax + add
        dev = np.abs(got[side] - st[side])
        print("%s: largest deviation / bound = %.3g" % (side, (dev / bound).max()))
        assert (dev <= bound).all(), (side, (dev / bound).max())
    decided = ~undecided
    assert np.array_equal(got["last"][decided], st["accepted"][decided])
    assert np.array_equal(got["ever"], got["last"])
    both = np.logical_and(got["last"], st["accepted"])
    if P >= 70:
        assert both.any() and (~got["last"]).any()
    bound = (1e-12 * np.maximum(1.0, np.abs(st["t"])) * vmax + np.abs(st["t"]) * dv.max() + vmax * (add_l + add_r))[:, None]
    dev = np.abs(got["u"] - st["unew"])[both]
    if both.any():
        print("unew: largest deviation / bound = %.3g" % (dev / bound[both]).max())
    assert (dev <= bound[both]).all()
    assert np.array_equal(got["p"][both], np_transform(got["u"][both]))
    assert np.allclose(got["L"][both], st["Lnew"][both], rtol=1e-12, atol=1e-9)
    stay = ~got["last"]
    assert np.array_equal(got["u"][stay], us[got["start"][stay]]) and np.array_equal(got["L"][stay], Ls[got["start"][stay]])
    assert np.isnan(got["p"][stay]).all()
    assert got["nrejects"] == int(stay.sum()) and got["nlast"] == int(got["last"].sum()) and got["nnever"] == int(stay.sum())
    d2 = ((layer.transform(us[got["start"][got["last"]]]) - layer.transform(got["u"][got["last"]]))**2).sum(axis=1)
    r2 = region.maxradiussq
    close = int((np.abs(d2 - r2) <= 1e-9 * r2).sum())
    assert abs(got["nfar"] - (d2 > r2).sum()) <= close
    assert np.isclose(got["sumlog"], np.log(np.sqrt(d2) / np.sqrt(r2) + 1e-10).sum(), rtol=1e-9, atol=1e-9)


# ---- 3. a simple-slice refill against the restatement ---------------------------------------------------------------------

def _slice_allowances(case, ref, us, axes):
    """What the summing kinds add to the bounds, accumulated over the steps of the case: per step the allowance dt[k] of
    point k's slice ends (a proposal t = lo + width q, q in [0, 1], and a shrunk end t / shrink with shrink >= 1 carry at
    most the larger of the two ends' allowances), and after the last step the allowance du[k] of the point itself
    (du <- du + max |t| max dv + |v|_inf dt per step).  All zero for the selecting kinds."""
    d, P, nsteps, limit, shrink, kind, layer, sigma, scale, seed = case
    dirscale = scale * (1.0 + 0.25 * np.arange(nsteps))
    u = us[ref["start"]].copy()
    du = np.zeros(P)
    dts = []
    for s, step in enumerate(ref["steps"]):
        v = step["v"]
        dv = _dv(kind, dirscale[s], axes, d)
        add_l, add_r, tl, tr = _line_allowance(u, v, dv, du)
        dt = np.maximum(add_l, add_r)
        dts.append(dt)
        if dv.any():
            du = du + np.maximum(tl, tr) * dv.max() + np.abs(v).max(axis=1) * dt
        for it in step["its"]:
            got = it["taken"] >= 0
            u[got] = it["unew"][it["taken"][got]]
    return dts, du


def _slice_against_the_restatement(case, got, offset, ref, us, region):
    """test_simpleslice_device.py::_against_the_restatement with the module's tolerances: discrete results exact; tleft /
    tright of the last step, the per-step median widths (a median moves by at most the largest change of an element), u, p
    and L (the Gaussian's gradient times du) within their bounds."""
    d, P, nsteps = case[:3]
    sigma = case[7]
    dts, du = _slice_allowances(case, ref, us, region.transformLayer.axes)
    last = ref["steps"][-1]
    assert offset == ref["next_offset"]
    assert np.array_equal(got["start"], ref["start"])
    assert np.array_equal(got["iters"], ref["iters"]), (got["iters"], ref["iters"])
    assert np.array_equal(got["taken"], ref["taken"]) and np.array_equal(got["taken_it"], ref["taken_it"])
    assert np.array_equal(got["taken"] >= 0, last["its"][-1]["status"] == 1)
    assert got["discarded"] == ref["discarded"] and got["niter"] == ref["niter"] and got["nnan"] == ref["nnan"]
    vmax = np.abs(last["v"]).max(axis=1)
    worst = {}
    for side in ("tleft", "tright"):
        bound = 1e-12 * np.maximum(1.0, np.abs(ref[side])) * vmax + dts[-1]
        worst[side] = (np.abs(got[side] - ref[side]) / bound).max()
    med_got, med_ref = np.median(got["widths"], axis=1), np.median(ref["widths"], axis=1)
    worst["median width"] = 0.0
    for s in range(nsteps):
        bound = 1e-12 * max(1.0, abs(med_ref[s])) * np.abs(ref["steps"][s]["v"]).max() + 2 * dts[s].max()
        worst["median width"] = max(worst["median width"], abs(med_got[s] - med_ref[s]) / bound)
    t = np.maximum(np.abs(ref["tleft"]), np.abs(ref["tright"]))
    moved = ref["taken"] >= 0
    for k in np.flatnonzero(moved):
        t[k] = abs(last["its"][ref["taken_it"][k]]["t"][ref["taken"][k]])
    bound = (1e-12 * np.maximum(1.0, t) * vmax + du)[:, None]
    for name in ("u", "p"):
        fin = np.isfinite(ref[name])
        assert np.array_equal(fin, np.isfinite(got[name]))
        worst[name] = (np.abs(np.where(fin, got[name] - ref[name], 0.0)) / bound).max()
    bound = 1e-12 * np.maximum(1.0, np.abs(ref["L"])) + (np.abs(ref["u"] - 0.5) / sigma**2).sum(axis=1) * du
    worst["L"] = (np.abs(got["L"] - ref["L"]) / bound).max()
    for name, frac in worst.items():
        print("%s: largest deviation / bound = %.3g" % (name, frac))
    assert max(worst.values()) <= 1.0, worst
    tl = region.transformLayer
    d2 = ((tl.transform(us[got["start"]]) - tl.transform(got["u"]))**2).sum(axis=1)
    r2 = region.maxradiussq
    close = int((np.abs(d2 - r2) <= 1e-9 * r2).sum())
    assert abs(got["nfar"] - (d2 > r2).sum()) <= close
    assert np.isclose(got["sumlog"], np.log(np.sqrt(d2) / np.sqrt(r2) + 1e-10).sum(), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("case", W.SS_CASES, ids=W.ss_id)
def test_simple_slice_refill_against_the_restatement(case):
    us, Ls, Lmin, region, dirscale, ref = SS._case(case)
    got, offset = SS._device_refill(case)
    _slice_against_the_restatement(case, got, offset, ref, us, region)


# ---- 4. exact parts, bit for bit ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [130, 193])
@pytest.mark.parametrize("kind", [0, 1, 3, 5])
def test_line_cube_intersection_is_exact_for_the_selecting_kinds(d, kind):
    """A selected direction is the restatement's, double for double, the start rows are the live points', and the
    intersection's max / min are exact (no contraction: the library is built with -ffp-contract=off): tleft and tright of a
    step are the restated ones bit for bit.  A difference is a stride or tree error of line_cube_wave_wide."""
    from ultranest_amd.regions import DeviceRNG
    case = ("gauss", d, 70, kind, 270 + kind)
    us, Ls, Lmin, region, scale, transform, loglike, np_transform, ref = W.rw_case(case)
    rng = DeviceRNG(case[4])
    rng.offset = W.RW_OFFSET
    got = T._walkers(region, us, Ls, 70, 1, kind).refill(Lmin, kind, scale, rng, transform.device_spec, loglike.device_spec)
    assert np.array_equal(got["start"], ref["start"])
    tl, tr = R.line_intersection(us[got["start"]], ref["steps"][0]["v"])
    assert np.array_equal(got["tleft"], tl) and np.array_equal(got["tright"], tr)
    assert np.isfinite(tl).all() and np.isfinite(tr).all() and (tl < 0).all() and (tr > 0).all()


def test_stream_discipline_of_the_random_walk():
    """d = 130, kind 6, nsteps 4: same seed and offset give identical outputs, the second refill differs, the offset
    advances by P nsteps ((d + 1) / 2 + 2), popsize 64 and 65 give the same first 64 walkers."""
    from ultranest_amd.regions import DeviceRNG
    d, nsteps, kind = 130, 4, 6
    us, transform, loglike, np_transform, np_loglike = T._problem("gauss", d, 400, 262)
    region = SS._region(us, "affine")
    Ls = np_loglike(us)
    Lmin = np.sort(Ls)[100]
    args = (Lmin, kind, 0.5)
    specs = (transform.device_spec, loglike.device_spec)
    per = 64 * nsteps * ((d + 1) // 2 + 2)
    w = T._walkers(region, us, Ls, 64, nsteps, kind)
    rng = DeviceRNG(11)
    a = w.refill(*args, rng, *specs)
    assert rng.offset == per == R.next_offset(0, 64, nsteps, d)
    b = w.refill(*args, rng, *specs)
    assert rng.offset == 2 * per
    assert not np.array_equal(a["u"], b["u"]) and not np.array_equal(a["start"], b["start"])
    assert a["chain_form"] and a["ever"].any() and a["nrejects"] > 0
    rng2 = DeviceRNG(11)
    T._same(a, w.refill(*args, rng2, *specs))
    T._same(b, w.refill(*args, rng2, *specs))
    c = T._walkers(region, us, Ls, 65, nsteps, kind).refill(*args, DeviceRNG(11), *specs)
    for k in T.PER_WALKER:
        assert np.array_equal(c[k][:64], a[k], equal_nan=True), k


def test_stream_discipline_of_the_simple_slice():
    """d = 130, kind 6, nsteps 4: same seed and offset give identical outputs, the second refill differs, the offset
    advances by max(P nsteps ((d + 1) / 2 + 2), P (1 + nsteps max_it)) -- both branches of the maximum."""
    from ultranest_amd import likelihoods as lk
    from ultranest_amd.regions import DeviceRNG
    d, P, nsteps, kind = 130, 64, 4, 6
    case = (d, P, nsteps, 0, 1.0, kind, "affine", 0.1, 1.0, 263)
    specs = (lk.identity_transform.device_spec, lk.GaussLikelihood(0.5, 0.1, d).device_spec)
    for mi, per in ((3, P * nsteps * ((d + 1) // 2 + 2)), (SS.MAX_IT, P * (1 + nsteps * SS.MAX_IT))):
        us, Ls, Lmin, region, dirscale, ref = SS._case(case, mi)
        args = (Lmin, kind, dirscale, 0, 1.0)
        w = SS._walkers(region, us, Ls, P, nsteps, kind, mi)
        rng = DeviceRNG(11)
        a = w.refill(*args, rng, *specs)
        assert rng.offset == per == S.next_offset(0, P, nsteps, d, mi)
        b = w.refill(*args, rng, *specs)
        assert rng.offset == 2 * per
        assert not np.array_equal(a["u"], b["u"]) and not np.array_equal(a["start"], b["start"])
        w2 = SS._walkers(region, us, Ls, P, nsteps, kind, mi)
        rng2 = DeviceRNG(11)
        SS._same(a, w2.refill(*args, rng2, *specs))
        SS._same(b, w2.refill(*args, rng2, *specs))
        assert rng2.offset == 2 * per


def test_simple_slice_results_do_not_depend_on_the_batch_size():
    """d = 130: one slot per poll, the policy, and all nsteps * max_it slots in one batch give identical bits."""
    case = W.SS_BATCH_CASE
    runs = [SS._device_refill(case, slots_per_poll=n) for n in (1, 0, 4 * SS.MAX_IT)]
    for got, offset in runs[1:]:
        SS._same(runs[0][0], got)
        assert offset == runs[0][1] == S.next_offset(77, case[1], case[2], case[0], SS.MAX_IT)
    assert runs[0][0]["niter"] >= 8 and runs[0][0]["nnan"] == 0


def test_max_it_caps_a_wide_simple_slice_step():
    """max_it = 2 at d = 130 leaves points without a successor (restated: 70 in the last step, 3 that never moved): the
    outputs equal the restatement with the same cap."""
    case = W.SS_CAP_CASE
    us, Ls, Lmin, region, dirscale, ref = SS._case(case, 2)
    assert (ref["taken"] < 0).any() and list(ref["iters"]) == [2, 2, 2]
    got, offset = SS._device_refill(case, max_it=2)
    assert len(got["iters"]) == case[2] and got["niter"] == 2 * case[2]
    _slice_against_the_restatement(case, got, offset, ref, us, region)


# ---- 5. user models -------------------------------------------------------------------------------------------------------

def _gauss_problem(d, sigma, seed):
    from ultranest_amd import usermodels
    centers = usermodels.gauss_centers(d, sigma)
    rs = np.random.RandomState(seed)
    us = np.clip(centers + sigma * rs.normal(size=(400, d)), 0.01, 0.99)
    Ls = T._np_gauss(centers, sigma)(us)
    return centers, us, Ls, SS._region(us, "affine")


@pytest.mark.parametrize("d", [129, 130])
def test_user_gauss_equals_the_builtin_pair_in_both_samplers(d):
    """Above 128 dimensions the built-in Gaussian evaluates a row on one thread, terms ascending, as the user model does
    (tests/test_devicemodel_gpu.py: bit-identical), so every output array and count of both refills is identical."""
    from ultranest_amd import likelihoods as lk, usermodels
    from ultranest_amd.regions import DeviceRNG
    sigma, P, nsteps, kind = 0.1, 70, 3, 6
    centers, us, Ls, region = _gauss_problem(d, sigma, 300 + d)
    m = usermodels.gauss(d, sigma)
    builtin = lk.GaussLikelihood.docs_gauss(d, sigma)
    assert np.array_equal(builtin.centers, centers)
    specs = (lk.identity_transform.device_spec, builtin.device_spec)
    Lmin = np.sort(Ls)[100]
    runs = []
    for user in (None, (m, False)):
        rng = DeviceRNG(12)
        runs.append((T._walkers(region, us, Ls, P, nsteps, kind).refill(Lmin, kind, 0.5, rng, *specs, user), rng.offset))
    T._same(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]
    assert runs[0][0]["ever"].any() and runs[0][0]["nrejects"] > 0 and runs[0][0]["chain_form"] and runs[1][0]["chain_form"]
    Lmin = Ls.min() - 0.1
    dirscale = np.array([1.0, 1.25, 1.5])
    runs = []
    for user in (None, (m, False)):
        rng = DeviceRNG(9)
        runs.append((SS._walkers(region, us, Ls, P, nsteps, kind).refill(Lmin, kind, dirscale, 0, 1.5, rng, *specs, user),
                     rng.offset))
    SS._same(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1]
    assert runs[0][0]["nnan"] == 0 and runs[0][0]["niter"] >= nsteps


def _drain(sampler, region, Lmin, us, Ls, model, n):
    return [sampler.__next__(region, Lmin, us, Ls, model.transform, model.loglike) for _ in range(n)]


@pytest.mark.parametrize("which", ["randomwalk", "simpleslice"])
def test_derived_parameters_at_130_dimensions(which):
    """usermodels.gauss_derived(130) through __next__ with device_max_dim = 1024: p rows d + 3 wide whose first d columns are
    those of the model without derived parameters and whose derived columns are numpy's."""
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import usermodels
    from ultranest_amd.regions import DeviceRNG
    d, Q, P = 130, 3, 50
    centers, us, Ls, region = _gauss_problem(d, 0.1, 4)
    Lmin = Ls.min() - 1.0        # (restated on the CPU: no walker rejects all four moves at this scale)
    runs = []
    for model in (usermodels.gauss_derived(d), usermodels.gauss(d)):
        if which == "randomwalk":
            s = pop.PopulationRandomWalkSampler(P, 4, pop.generate_mixture_random_direction, 0.2, device_rng=DeviceRNG(8),
                                                device_max_dim=1024)
        else:
            s = pop.PopulationSimpleSliceSampler(P, 3, pop.generate_mixture_random_direction, device_rng=DeviceRNG(8),
                                                 device_max_dim=1024)
        runs.append(_drain(s, region, Lmin, us, Ls, model, P))
        assert s.last_refill["u"].shape == (P, d)
    for (ua, pa, La, nca), (ub, pb, Lb, ncb) in zip(*runs):
        assert nca == ncb and np.array_equal(ua, ub) and La == Lb
        assert pa.shape == (d + Q,) and pb.shape == (d,)
        assert np.array_equal(pa[:d], pb) and np.array_equal(pa[d:], usermodels.gauss_derived_columns(pb[None, :])[0])
    assert runs[0][0][3] > 0


# ---- 6. the samplers' bookkeeping at d = 130 ------------------------------------------------------------------------------

def _host_loop_has_no_refill_record(sampler, *args):
    state = np.random.get_state()
    np.random.seed(1)
    try:
        u, p, L, nc = sampler.__next__(*args)
    finally:
        np.random.set_state(state)
    assert nc > 0 and not hasattr(sampler, "last_refill")


def test_random_walk_bookkeeping_at_130_dimensions():
    """test_randomwalk_device.py::test_sampler_bookkeeping_follows_the_host_formulas at d = 130 (P = 50, nsteps 4, three
    refills; scale 0.1: restated on the CPU, no walker rejects all its moves), and the same call without device_max_dim takes
    the host loop."""
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    d, P, nsteps = 130, 50, 4
    us, transform, loglike, np_transform, np_loglike = T._problem("rosenbrock", d, 300, 63)
    region = SS._region(us, "affine")
    Ls = np_loglike(np_transform(us))
    Lmin = Ls.min() - 1.0
    log = io.StringIO()
    make = lambda **kw: pop.PopulationRandomWalkSampler(      # noqa: E731
        popsize=P, nsteps=nsteps, generate_direction=pop.generate_mixture_random_direction, scale=0.1, scale_adapt_factor=0.8,
        device_rng=DeviceRNG(6), **kw)
    s = make(logfile=log, device_max_dim=1024)
    scale, nrejects = s.scale, 0
    for refill in range(3):
        for j in range(P):
            unew, pnew, Lnew, nc = s.__next__(region, Lmin, us, Ls, transform, loglike)
            assert nc == (nsteps * P if j == 0 else 0)
            if j == 0:
                out = s.last_refill
                assert len(s.prepared_samples) == P - 1 and out["chain_form"] and out["u"].shape == (P, d)
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
    _host_loop_has_no_refill_record(make(), region, Lmin, us, Ls, transform, loglike)


def test_simple_slice_bookkeeping_at_130_dimensions():
    """test_simpleslice_device.py::test_sampler_bookkeeping_follows_the_host_formulas at d = 130 (P = 50, nsteps 4, three
    refills), and the same call without device_max_dim takes the host loop."""
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods as lk
    from ultranest_amd.regions import DeviceRNG
    d, P, nsteps = 130, 50, 4
    case = (d, P, nsteps, 0, 1.0, 6, "affine", 0.1, 1.0, 264)
    us, Ls, Lmin, region = SS._case(case)[:4]
    loglike = lk.GaussLikelihood(0.5, 0.1, d)
    jitters = list(1.0 + 0.1 * np.arange(3 * nsteps))
    calls = []

    def jitter():
        calls.append(jitters[len(calls)])
        return calls[-1]

    make = lambda **kw: pop.PopulationSimpleSliceSampler(      # noqa: E731
        P, nsteps, pop.generate_mixture_random_direction, scale_adapt_factor=0.8, adapt_slice_scale_target=2.0, scale=0.9,
        shrink_factor=1.5, device_rng=DeviceRNG(6), **kw)
    s = make(scale_jitter_func=jitter, device_max_dim=1024)
    scale, ncalls, discarded = 0.9, 0, 0
    for refill in range(3):
        recorded = DeviceRNG(6)
        recorded.offset = s.device_rng.offset
        for j in range(P):
            unew, pnew, Lnew, nc = s.__next__(region, Lmin, us, Ls, lk.identity_transform, loglike)
            if j == 0:
                out = s.last_refill
                assert nc == P * out["iters"].sum() == P * out["niter"] and len(s.prepared_samples) == P - 1
            else:
                assert nc == 0
            assert np.array_equal(unew, out["u"][j]) and np.array_equal(pnew, out["p"][j]) and Lnew == out["L"][j]
            assert Lnew > Lmin
        assert not s.prepared_samples
        assert calls == jitters[:(refill + 1) * nsteps]
        lengths = np.array([scale * x for x in jitters[refill * nsteps:(refill + 1) * nsteps]])
        again = SS._walkers(region, us, Ls, P, nsteps, 6).refill(Lmin, 6, lengths, 0, 1.5, recorded,
                                                                 lk.identity_transform.device_spec, loglike.device_spec)
        SS._same(out, again)
        assert recorded.offset == s.device_rng.offset
        ncalls += P * out["niter"]
        discarded += out["discarded"]
        assert s.ncalls == ncalls and s.discarded == discarded
        row = [P / (P * out["niter"]), scale, nsteps, out["nfar"] / P, np.exp(out["sumlog"] / P)]
        assert len(s.logstat) == refill + 1 and s.logstat[-1] == row, (s.logstat[-1], row)
        width_sum = 0.
        for widths in out["widths"]:
            width_sum += np.median(widths)
        if width_sum / nsteps >= 1. / 2.0:
            scale *= 1. / 0.8
        else:
            scale *= 0.8
        assert s.scale == scale
    _host_loop_has_no_refill_record(make(), region, Lmin, us, Ls, lk.identity_transform, loglike)


# ---- 7. invariance --------------------------------------------------------------------------------------------------------

def test_simple_slices_are_uniform_under_the_threshold_at_130_dimensions():
    """The ball problem and the assertions of test_wide_walk_gpu.py::
    test_slice_sampling_is_uniform_under_the_threshold_at_130_dimensions: 1500 points from six refills of 256 points x 8
    steps.  The coordinate checks catch a stride that never reaches the coordinates from 128 on."""
    from scipy import stats
    import ultranest_amd.popstepsampler as pop
    import test_wide_walk_gpu as WW
    from ultranest_amd import likelihoods
    from ultranest_amd.regions import DeviceRNG
    d = 130
    region = WW._gpu_region(d, 400, 11)
    u, sigma, Lmin, Rb = WW._ball_problem(d, 400, 11)
    loglike = likelihoods.GaussLikelihood(0.5, sigma, d)
    norm = -0.5 * np.log(2 * np.pi * sigma**2) * d
    Ls = loglike(u)
    sampler = pop.PopulationSimpleSliceSampler(popsize=256, nsteps=8, generate_direction=pop.generate_region_random_direction,
                                               device_rng=DeviceRNG(5), device_max_dim=1024)
    pts, Lout = [], []
    for _ in range(1500):
        unew, pnew, Lnew, nc = sampler.__next__(region, Lmin + norm, u, Ls, likelihoods.identity_transform, loglike)
        pts.append(unew)
        Lout.append(Lnew)
        assert np.array_equal(unew, pnew)
    pts, Lout = np.array(pts), np.array(Lout)
    assert len(sampler.logstat) == 6 and sampler._sslice is not None
    assert (Lout > Lmin + norm).all()
    assert np.allclose(Lout, loglike(pts), rtol=1e-12, atol=1e-12)
    r = np.linalg.norm(pts - 0.5, axis=1) / Rb
    assert r.max() < 1
    p = stats.kstest(r[::3]**d, "uniform").pvalue       # thinned: points that shared a start point are correlated
    print("KS p-value of r^d against uniform: %.3g" % p)
    assert p > 1e-3
    assert (np.abs(pts - 0.5).max(axis=0) > 1e-6).all()
    assert (pts.max(axis=0) > pts.min(axis=0)).all()
    fresh = np.array([(~np.isin(pts[:, k], u[:, k])).any() for k in range(d)])
    assert fresh.all(), np.flatnonzero(~fresh)
