"""The summed form of a user model (DeviceModel(..., nterms=K)) on the GPU: the documented summation order bit for bit against
its numpy restatement, the cross-check against the default-form twin, independence of the row's position and of the
membership mask, the transform, non-finite terms, every device route against the twin (staircase_sum: integer terms, so the
two forms are bit-identical and whole runs are compared with ==), variant mismatches and model lifetimes.

The restatement (`_contract`): lane l adds term(l), term(l + 64), ... one by one from 0.0; then six exchange steps
s = s + s[lane ^ m], m = 32, 16, 8, 4, 2, 1.  numpy's own sum is pairwise and is not used anywhere here."""
import functools
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_devicemodel_gpu as G  # noqa: E402   (its MLFriends region of a live set and its run comparison)
import test_tregion_refill_gpu as TR  # noqa: E402   (a bootstrapped WrappingEllipsoid and its quadratic form)
from ultranest_amd import devicemodel as dm  # noqa: E402
from ultranest_amd import usermodels  # noqa: E402

SENTINEL = 7.25


def _contract(t):
    """L of the order contract for the term rows t (n, K): sequential additions per lane, then the xor steps"""
    n, K = t.shape
    s = np.zeros((n, 64))
    for k0 in range(0, K, 64):          # lane l takes k0 + l: one addition per lane and pass, k ascending
        w = min(64, K - k0)
        s[:, :w] = s[:, :w] + t[:, k0:k0 + w]
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ m]
    assert (s == s[:, :1]).all() or np.isnan(s).any()
    return s[:, 0]


def _linear_terms(p, X, y, w):
    """term(k) of linear_sum for the parameter rows p (n, d), bit for bit: m from 0.0 in ascending j, one multiplication
    and one addition each"""
    m = np.zeros((p.shape[0], X.shape[0]))
    for j in range(X.shape[1]):
        m = m + p[:, j:j + 1] * X[:, j]
    r = (y - m) * w
    return -0.5 * r * r


@functools.lru_cache(maxsize=None)
def _linear(d, K, affine=False):
    return usermodels.linear_sum(d, K, seed=d + K, affine=affine), usermodels.linear_data(d, K, seed=d + K)


def _eval_dev(model, u, want_p=False, member=None):
    """eval_dev on resident torch tensors, p and L prefilled with SENTINEL; returns (p or None, L)"""
    import torch
    from ultranest_amd import _lib
    dev = torch.device("cuda")
    n, d = u.shape
    tu = torch.from_numpy(np.ascontiguousarray(u)).to(dev)
    tp = torch.full((n, d), SENTINEL, dtype=torch.float64, device=dev) if want_p else None
    tL = torch.full((n,), SENTINEL, dtype=torch.float64, device=dev)
    tm = None if member is None else torch.from_numpy(np.asarray(member).astype(np.uint8)).to(dev)
    torch.cuda.synchronize()
    model.eval_dev(tu.data_ptr(), n, tp.data_ptr() if want_p else None, tL.data_ptr(), None if tm is None else tm.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().mlf_synchronize())
    return (tp.cpu().numpy() if want_p else None), tL.cpu().numpy()


# ---- the order contract ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("d", [1, 3, 50])
def test_order_contract_bit_for_bit(d, K):
    m, (X, y, w) = _linear(d, K)
    rs = np.random.RandomState(1000 * d + K)
    for n in (1, 5, 64, 130):
        p = rs.normal(size=(n, d))
        want = _contract(_linear_terms(p, X, y, w))
        L = m.loglike(p)
        assert L.shape == (n,) and np.array_equal(L, want), (d, K, n, np.abs(L - want).max())
        assert np.array_equal(_eval_dev(m, p)[1], want), (d, K, n)


def test_order_contract_with_many_terms():
    d, K, n = 3, 100003, 3
    m, (X, y, w) = _linear(d, K)
    p = np.random.RandomState(5).normal(size=(n, d))
    want = _contract(_linear_terms(p, X, y, w))
    assert np.array_equal(m.loglike(p), want)
    assert np.array_equal(_eval_dev(m, p)[1], want)


@pytest.mark.parametrize("d,K", [(3, 200), (50, 65), (10, 1000)])
def test_summed_form_against_its_twin(d, K):
    """the project's 1e-12 * scale class (test_loglike_forms.py), scale = the sum of the terms' magnitudes: the two forms
    add the same K terms in different orders"""
    m, (X, y, w) = _linear(d, K)
    twin = usermodels.linear_twin(d, K, seed=d + K)
    p = np.random.RandomState(K).normal(size=(130, d))
    t = _linear_terms(p, X, y, w)
    scale = np.zeros(len(p))
    for k in range(K):
        scale = scale + np.abs(t[:, k])
    a, b = m.loglike(p), twin.loglike(p)
    print("max |L_sum - L_twin| / scale = %.3g" % (np.abs(a - b) / scale).max())
    assert (np.abs(a - b) <= 1e-12 * scale).all()
    # and the twin is the serial sum of the same terms
    serial = np.zeros(len(p))
    for k in range(K):
        serial = serial + t[:, k]
    assert np.array_equal(b, serial)


def test_position_in_the_batch_does_not_matter():
    d, K = 3, 65
    m, (X, y, w) = _linear(d, K)
    rs = np.random.RandomState(11)
    rows = rs.normal(size=(7, d))
    want = m.loglike(rows)
    assert np.array_equal(want, _contract(_linear_terms(rows, X, y, w)))
    for n in (130, 200):
        for off in (0, 1, 63, 64, 129):
            k = min(7, n - off)
            batch = rs.normal(size=(n, d))
            batch[off:off + k] = rows[:k]
            assert np.array_equal(m.loglike(batch)[off:off + k], want[:k]), (n, off)
            assert np.array_equal(_eval_dev(m, batch)[1][off:off + k], want[:k]), (n, off)


@pytest.mark.parametrize("mask", ["all", "none", "every_third", "only_row_129"])
def test_membership(mask):
    d, K, n = 3, 65, 130
    m, _ = _linear(d, K, affine=True)
    u = np.random.RandomState(12).uniform(size=(n, d))
    member = dict(all=np.ones(n, dtype=bool), none=np.zeros(n, dtype=bool), every_third=np.arange(n) % 3 == 0,
                  only_row_129=np.arange(n) == 129)[mask]
    p0, L0 = _eval_dev(m, u, want_p=True)                 # the unmasked call
    assert np.array_equal(p0, u * 20.0 + -10.0) and np.isfinite(L0).all()
    p, L = _eval_dev(m, u, want_p=True, member=member)
    assert np.isneginf(L[~member]).all() and (p[~member] == SENTINEL).all()
    assert np.array_equal(L[member], L0[member]) and np.array_equal(p[member], p0[member])
    # likelihood only (no p buffer): the same values
    L1 = _eval_dev(m, p0, member=member)[1]
    assert np.isneginf(L1[~member]).all() and np.array_equal(L1[member], L0[member])


@pytest.mark.parametrize("d", [3, 50, 130])
def test_transform(d):
    K, n = 65, 130
    m, (X, y, w) = _linear(d, K, affine=True)
    twin = usermodels.linear_twin(d, K, seed=d + K, affine=True)
    u = np.random.RandomState(13).uniform(size=(n, d))
    p = m.transform(u)
    assert np.array_equal(p, twin.transform(u)) and np.array_equal(p, u * 20.0 + -10.0)
    pd, Ld = _eval_dev(m, u, want_p=True)
    assert np.array_equal(pd, p) and np.array_equal(Ld, _contract(_linear_terms(p, X, y, w)))
    # without a transform and with d_p given, p is a copy of u
    plain, _ = _linear(d, K)
    assert np.array_equal(plain.transform(u), u)
    pd, Ld = _eval_dev(plain, u, want_p=True)
    assert np.array_equal(pd, u) and np.array_equal(Ld, _contract(_linear_terms(u, X, y, w)))


NEG_INF_TERM = r"""
__device__ double mlf_user_loglike_term(const double *p, int d, const double *aux, long long naux, long long k) {
  if (k == aux[0]) return -__builtin_inf();
  return -(p[0] * p[0]);
}
"""


def test_non_finite_terms():
    d, K = 3, 200
    m, _ = _linear(d, K)
    p = np.random.RandomState(14).normal(size=(5, d))
    p[2, 1] = np.nan
    L = m.loglike(p)
    assert np.isnan(L[2]) and np.isfinite(np.delete(L, 2)).all()
    assert np.isnan(_eval_dev(m, p)[1][2])
    for k_inf in (0, 70, 199):      # wherever the term sits: one lane's partial sum is -inf and the exchange spreads it
        minf = dm.DeviceModel(d, NEG_INF_TERM, aux=[float(k_inf)], nterms=K)
        L = minf.loglike(p[:2])
        assert np.isneginf(L).all(), (k_inf, L)
        minf.close()


# ---- the routes, against the default-form twin ------------------------------------------------------------------------------

D, K = 3, 150


@functools.lru_cache(maxsize=None)
def _staircase_pair():
    return usermodels.staircase_sum(D, K, seed=3, affine=True), usermodels.staircase_twin(D, K, seed=3, affine=True)


@functools.lru_cache(maxsize=None)
def _live(n=40):
    u = np.clip(0.5 + 0.1 * np.random.RandomState(21).normal(size=(n, D)), 0.01, 0.99)
    twin = _staircase_pair()[1]
    return u, twin.loglike(twin.transform(u))


def test_staircase_forms_are_bit_identical():
    s, twin = _staircase_pair()
    u = np.random.RandomState(22).uniform(size=(130, D))
    p = s.transform(u)
    c = usermodels.staircase_data(D, K, seed=3, affine=True)
    want = np.zeros(len(p))
    for k in range(K):
        want = want + -np.floor(np.abs(p[:, k % D] - c[k]) * 8.0)
    assert np.array_equal(s.loglike(p), want) and np.array_equal(twin.loglike(p), want)
    assert len(np.unique(want)) > 20


@pytest.mark.parametrize("method", ["sample_from_boundingbox", "sample_from_points"])
@pytest.mark.parametrize("gated", [False, True])
def test_region_refill_equals_the_twin(method, gated):
    from ultranest_amd import kernels
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = np.sort(Ls)[10] + 0.5          # (integer likelihoods: no value sits on the threshold)
    tregion = None
    if gated:
        twin = _staircase_pair()[1]
        tregion = TR._tregion(twin.transform(u))
    out = []
    calls = []
    orig = kernels.DeviceRegion.refill_user

    def counting(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)

    kernels.DeviceRegion.refill_user = counting
    try:
        for model in _staircase_pair():
            region = G._region(u)
            region.device_rng = DeviceRNG(seed=11)
            region.current_sampling_method = getattr(region, method)
            if gated and not out:
                # the gate decides about half of the batch: the enlargement is the median of the quadratic form over
                # the ungated batch's p rows
                probe = region.refill(4096, -1e300, model.transform, model.loglike)
                tregion.enlarge = float(np.median(TR._quadratic_form(tregion, probe[1])))
                region.device_rng = DeviceRNG(seed=11)
                ungated = probe[3]
            got = region.refill(4096, Lmin, model.transform, model.loglike, **(dict(tregion=tregion) if gated else {}))
            out.append(got + (region.device_rng.offset,))
    finally:
        kernels.DeviceRegion.refill_user = orig
    assert len(calls) == (3 if gated else 2)
    (ua, pa, La, nca, oa), (ub, pb, Lb, ncb, ob) = out
    assert nca == ncb > 0 and oa == ob and len(ua) > 10
    assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and np.array_equal(La, Lb) and (La > Lmin).all()
    if gated:
        assert tregion.inside(pa).all() and 0.2 * ungated <= nca <= 0.8 * ungated


def _slice_runs(model, region, u, Ls, Lmin, device_rng, calls=40):
    import ultranest_amd.popstepsampler as pop
    np.random.seed(8)
    # (one slice step per point and a short first bracket: walkers finish within the 40 calls)
    s = pop.PopulationSliceSampler(popsize=16, nsteps=1, generate_direction=pop.generate_mixture_random_direction, scale=0.2,
                                   device_rng=device_rng)
    return [s.__next__(region, Lmin, u, Ls, model.transform, model.loglike) for _ in range(calls)]


@pytest.mark.parametrize("philox", [False, True])
def test_population_slice_sampler_equals_the_twin(philox):
    """host-RNG mode (mlf_walkers_finish_user) and Philox mode (mlf_walkers_step_user)"""
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = Ls.min() - 0.5
    region = G._region(u)
    s, twin = _staircase_pair()
    a = _slice_runs(twin, region, u, Ls, Lmin, DeviceRNG(5) if philox else None)
    b = _slice_runs(s, region, u, Ls, Lmin, DeviceRNG(5) if philox else None)
    assert G._same_run(a, b) >= 1          # (calls that returned a point)
    assert sum(x[3] for x in a) == sum(x[3] for x in b) > 0


def _host_region(u):
    import ultranest_amd.mlfriends as m
    tl = m.AffineLayer()
    tl.optimize(u, u)
    return types.SimpleNamespace(u=u, transformLayer=tl, maxradiussq=float(u.shape[1]))


def _same_refill(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _same_prepared(a, b):
    assert len(a) == len(b) > 0
    for (ua, pa, La), (ub, pb, Lb) in zip(a, b):
        assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and La == Lb


def test_random_walk_refill_equals_the_twin():
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = Ls.min() - 0.5
    region = _host_region(u)
    done = []
    for model in _staircase_pair():
        s = pop.PopulationRandomWalkSampler(64, 4, pop.generate_mixture_random_direction, 0.05, device_rng=DeviceRNG(6))
        first = s.__next__(region, Lmin, u, Ls, model.transform, model.loglike)
        done.append((s, first))
    (sa, fa), (sb, fb) = done
    assert fa[3] == fb[3] == 64 * 4 and np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]) and fa[2] == fb[2]
    _same_refill(sa.last_refill, sb.last_refill)
    out = sa.last_refill
    assert out["nnever"] == 0 and (out["L"] > Lmin).all() and 0 <= out["nrejects"] < 64 * 4
    _same_prepared(sa.prepared_samples, sb.prepared_samples)
    assert len(sa.prepared_samples) == 63 and sa.scale == sb.scale and sa.nrejects == sb.nrejects
    assert sa.logstat == sb.logstat and sa.device_rng.offset == sb.device_rng.offset > 0


def test_simple_slice_refill_equals_the_twin():
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = Ls.min() - 0.5
    region = _host_region(u)
    done = []
    for model in _staircase_pair():
        s = pop.PopulationSimpleSliceSampler(64, 4, pop.generate_mixture_random_direction, scale_adapt_factor=0.8, max_it=20,
                                             device_rng=DeviceRNG(7))
        first = s.__next__(region, Lmin, u, Ls, model.transform, model.loglike)
        done.append((s, first))
    (sa, fa), (sb, fb) = done
    assert fa[3] == fb[3] > 0 and np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]) and fa[2] == fb[2]
    _same_refill(sa.last_refill, sb.last_refill)
    out = sa.last_refill
    assert out["nnan"] == 0 and (out["L"] > Lmin).all() and fa[3] == 64 * out["niter"] and out["niter"] >= 4
    assert sa.ncalls == sb.ncalls == fa[3] and sa.discarded == sb.discarded == out["discarded"]
    _same_prepared(sa.prepared_samples, sb.prepared_samples)
    assert len(sa.prepared_samples) == 63 and sa.scale == sb.scale and sa.scale != 1.0
    assert sa.logstat == sb.logstat and sa.device_rng.offset == sb.device_rng.offset > 0


# ---- variants and lifetimes ----------------------------------------------------------------------------------------------

def test_a_summed_model_of_the_other_variant_is_refused():
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    s = _staircase_pair()[0]
    region = G._region(u)
    region.device_rng = DeviceRNG(41)
    region.current_sampling_method = region.sample_from_wrapping_ellipsoid
    tregion = TR._tregion(s.transform(u))
    got = region.refill(4096, -1e300, s.transform, s.loglike, tregion=tregion)
    assert got[3] > 0
    handle = region._dev.handle       # the t-region is set on it
    with pytest.raises(ValueError, match="the region has a t-region"):
        handle.refill_user(1, 4096, 41, 0, -1e300, s.handle(True))
    handle.clear_tregion()
    with pytest.raises(ValueError, match="the region has no t-region"):
        handle.refill_user(1, 4096, 41, 0, -1e300, s.handle(True, gated=True))
    # a code object loaded as a variant it was not compiled as has no such entry
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(s.code, D, True, s.aux, gated=True, nterms=K)
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(dm.compile_model(s.source, True, gated=True, summed=True), D, True, s.aux, nterms=K)
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(s.code, D, True, s.aux)                                       # a summed program as a default model
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(_staircase_pair()[1].code, D, True, s.aux, nterms=K)          # and the reverse
    assert len(handle.refill_user(1, 4096, 41, 0, -1e300, s.handle(True))[0]) >= got[3]     # the handle still works, ungated


def test_two_summed_models_alternately_then_destroyed():
    rs = np.random.RandomState(9)
    d = 9
    x = rs.uniform(size=(500, d))
    alone = []
    makes = (lambda: usermodels.linear_sum(d, 200, seed=4, affine=True), lambda: usermodels.staircase_sum(d, 70, seed=5))
    for make in makes:
        m = make()
        alone.append((m.transform(x), m.loglike(m.transform(x))))
        m.close()
    a, b = makes[0](), makes[1]()
    for _ in range(3):
        for m, (p0, L0) in zip((a, b), alone):
            p = m.transform(x)
            assert np.array_equal(p, p0) and np.array_equal(m.loglike(p), L0)
    a.close()
    p0, L0 = alone[1]
    assert np.array_equal(b.loglike(b.transform(x)), L0)
    b.close()
