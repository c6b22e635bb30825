"""The whole-population samplers above 128 dimensions, on the CPU: the cases of tests/test_wide_population_gpu.py restated in
numpy (tests/randomwalk_reference.py, tests/simpleslice_reference.py) decide every comparison that test makes, and the routing
of ``device_max_dim``.  The case tables and their restatements live here and are shared with the GPU file."""
import functools

import numpy as np
import pytest

import randomwalk_reference as R
import test_randomwalk_device as T       # (its problems)
import test_simpleslice_device as SS     # (its host-only region, its case recipe)

# ---- the cases ---------------------------------------------------------------------------------------------------------
# d = 129 (odd, first above the narrow form), 130, 192 (exactly three strides), 193, 256, 1024 (the LDS bound; P = 3), and
# one population above the 8192-workgroup grid of the wide kernels (8262 walkers at d = 130)

# (name, d, P, kind, seed[, scale]); one step, offset 77
RW_CASES = [("rosenbrock" if k % 2 == 0 else "gauss", 130, 70, k, 240 + k) for k in range(7)] + [
    ("gauss", 129, 70, 2, 251), ("gauss", 129, 70, 4, 252), ("rosenbrock", 129, 70, 6, 253),
    ("gauss", 193, 70, 4, 254), ("rosenbrock", 256, 70, 2, 255), ("gauss", 256, 70, 5, 256),
    ("gauss", 1024, 3, 4, 257), ("gauss", 1024, 3, 5, 258),
    ("gauss", 130, 8262, 6, 259, 0.5), ("gauss", 130, 8262, 4, 260, 0.5)]
RW_SCALES = {0: 0.02, 1: 0.3, 2: 0.05, 3: 0.5, 4: 0.5, 5: 0.5, 6: 0.5}      # (test_one_step_against_the_restatement's table)
RW_OFFSET = 77

# (d, P, nsteps, limit, shrink, kind, layer, sigma, scale, seed): the tuple of test_simpleslice_device.CASES
SS_CASES = [
    (129, 70, 2, 0, 1.0, 2, "affine", 0.1, 1.0, 201),
    (130, 70, 3, 1, 1.5, 4, "affine", 0.05, 0.5, 202),
    (130, 200, 2, 0, 1.5, 6, "scaling", 0.1, 1.0, 203),
    (192, 70, 1, 0, 1.0, 0, "affine", 0.1, 1.0, 204),
    (193, 70, 2, 1, 1.5, 1, "scaling", 0.05, 5.0, 205),
    (256, 70, 1, 0, 1.5, 3, "affine", 0.1, 1.0, 206),
    (256, 70, 2, 0, 1.0, 5, "affine", 0.1, 1.0, 207),
    (1024, 3, 1, 0, 1.5, 4, "scaling", 0.1, 1.0, 208),
    (1024, 3, 2, 1, 1.0, 2, "scaling", 0.1, 1.0, 209),
    (130, 8262, 1, 0, 1.5, 6, "affine", 0.1, 1.0, 210),
    (130, 8262, 1, 0, 1.0, 4, "affine", 0.1, 1.0, 211),
]
SS_BATCH_CASE = (130, 200, 4, 0, 1.5, 6, "affine", 0.1, 1.0, 220)      # results do not depend on slots_per_poll
SS_CAP_CASE = (130, 200, 3, 0, 1.0, 6, "affine", 0.1, 1.0, 225)        # max_it = 2


def rw_id(case):
    return "%s-d%d-P%d-kind%d" % case[:4]


def ss_id(case):
    return "d%d-P%d-n%d-lim%d-shr%g-kind%d-%s" % case[:7]


@functools.lru_cache(maxsize=None)
def rw_case(case, nsteps=1):
    """(live points, likelihoods, Lmin, region, scale, device transform, device loglike, numpy transform, the restated refill)
    of one random-walk case, computed once and shared.  400 live points (1100 at d = 1024: an affine layer needs more points
    than dimensions); Lmin = the 25th-percentile likelihood; a host-only region."""
    name, d, P, kind, seed = case[:5]
    nlive = 1100 if d == 1024 else 400
    us, transform, loglike, np_transform, np_loglike = T._problem(name, d, nlive, seed)
    region = SS._region(us, "affine")
    Ls = np_loglike(np_transform(us))
    Lmin = np.sort(Ls)[nlive // 4]
    scale = case[5] if len(case) > 5 else RW_SCALES[kind] * (0.3 if name == "rosenbrock" else 1.0)
    layer = region.transformLayer
    ref = R.refill(seed, RW_OFFSET, us, Ls, Lmin, kind, scale, P, nsteps, np_transform, np_loglike, axes=layer.axes,
                   std=us.std(axis=0), whiten=layer.transform, maxradiussq=region.maxradiussq)
    for a in (us, Ls):
        a.setflags(write=False)
    return us, Ls, Lmin, region, scale, transform, loglike, np_transform, ref


def rw_undecided(ref, Lmin):
    st = ref["steps"][0]
    return np.logical_and(st["inside"], np.abs(st["Lnew"] - Lmin) <= 1e-9 * max(1.0, abs(Lmin)))


# ---- the restatement alone ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", RW_CASES, ids=rw_id)
def test_the_random_walk_cases_decide_every_comparison(case):
    """At most 1 % of the walkers undecided (inside the cube with |Lnew - Lmin| <= 1e-9 max(1, |Lmin|)); for P >= 70 both
    outcomes occur."""
    P = case[2]
    us, Ls, Lmin, region, scale, transform, loglike, np_transform, ref = rw_case(case)
    undecided = rw_undecided(ref, Lmin)
    acc = ref["steps"][0]["accepted"]
    print(case, "undecided %d, accepted %d, rejected %d" % (undecided.sum(), acc.sum(), (~acc).sum()))
    assert undecided.sum() <= 0.01 * P, undecided.sum()
    if P >= 70:
        assert acc.any() and (~acc).any()


@pytest.mark.parametrize("case", SS_CASES, ids=ss_id)
def test_the_simple_slice_cases_decide_every_comparison(case):
    """No proposal's L within 1e-7 max(1, |Lmin|) of the threshold, no t within 1e-9 max(1, |t|) of a bound it is compared
    with, every point moved."""
    ref = SS._case(case)[5]
    print(case, "min |L - Lmin| margin %.3g, min t margin %.3g, iterations %s" % (
        ref["min_L_margin"], ref["min_t_margin"], list(ref["iters"])))
    assert ref["min_L_margin"] > 1e-7 and ref["min_t_margin"] > 1e-9, case
    assert ref["nnan"] == 0


def test_the_capped_simple_slice_case_decides_every_comparison():
    """max_it = 2 leaves points without a successor; the margins hold with the cap too."""
    ref = SS._case(SS_CAP_CASE, 2)[5]
    print("min |L - Lmin| margin %.3g, min t margin %.3g, without a successor %d, never moved %d" % (
        ref["min_L_margin"], ref["min_t_margin"], (ref["taken"] < 0).sum(), ref["nnan"]))
    assert ref["min_L_margin"] > 1e-7 and ref["min_t_margin"] > 1e-9
    assert (ref["taken"] < 0).any() and list(ref["iters"]) == [2, 2, 2]


# ---- routing --------------------------------------------------------------------------------------------------------------

def _samplers(rng=True, **kw):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    return (pop.PopulationRandomWalkSampler(8, 3, pop.generate_random_direction, 0.5, device_rng=DeviceRNG(3) if rng else None, **kw),
            pop.PopulationSimpleSliceSampler(8, 3, pop.generate_random_direction, device_rng=DeviceRNG(3) if rng else None, **kw))


def test_routing_of_device_max_dim():
    """Default samplers keep the host loop above 128 dimensions; device_max_dim = 1024 routes 129 and 1024 to the device and
    1025 to the host loop; anything but an integer in [1, 1024] is a ValueError; without device_rng nothing is routed."""
    from ultranest_amd import likelihoods as lk
    model = (lk.identity_transform, lk.GaussLikelihood(0.5, 0.1, 7))
    for s in _samplers():
        assert s.device_max_dim == 128
        assert s._device_route(*model, 128) is not None and s._device_route(*model, 129) is None
    for s in _samplers(device_max_dim=1024):
        assert s.device_max_dim == 1024
        for ndim in (7, 128, 129, 1024):
            assert s._device_route(*model, ndim) is not None, ndim
        assert s._device_route(*model, 1025) is None
        assert s._device_route(*model, 129) == s._device_route(*model, 7)
    for s in _samplers(device_max_dim=64):
        assert s._device_route(*model, 64) is not None and s._device_route(*model, 65) is None
    for bad in (0, 1025, 1.5, -1, None, "128", True):
        with pytest.raises(ValueError):
            _samplers(device_max_dim=bad)
    for kw in ({}, dict(device_max_dim=1024)):
        for s in _samplers(rng=False, **kw):
            for ndim in (None, 7, 129, 1024):
                assert s._device_route(*model, ndim) is None
    rw, sl = _samplers(device_max_dim=1024)
    assert str(rw) == str(_samplers()[0]) and str(sl) == str(_samplers()[1])
