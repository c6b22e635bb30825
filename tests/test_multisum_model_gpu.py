"""Several sums and a final function (DeviceModel(..., nterms=K, nsums=M)) on the GPU: the extended order contract bit for bit
against its numpy restatement (multisum_reference.contract: every accumulator in the single-sum order, then finish),
amplitude_sum against a long-double reference, staircase3_sum against its default-form twin bit for bit (exact sums), independence
of the row's position and of the membership mask, a NaN that stays in its accumulator, every device route against the twin,
variant mismatches and model lifetimes.

A program depends on the source, the transform flag, the gate and M only (d and K are run-time arguments), so the models of this
file share a dozen programs."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import multisum_reference as MR  # noqa: E402
import test_devicemodel_gpu as G  # noqa: E402   (its MLFriends region of a live set and its run comparison)
import test_summed_model_gpu as S  # noqa: E402   (eval_dev on resident tensors, the host region, the refill comparisons)
import test_tregion_refill_gpu as TR  # noqa: E402   (a bootstrapped WrappingEllipsoid and its quadratic form)
from ultranest_amd import devicemodel as dm  # noqa: E402
from ultranest_amd import usermodels  # noqa: E402

SENTINEL = S.SENTINEL


@functools.lru_cache(maxsize=None)
def _generated(M, d, K):
    x = MR.generated_data(K)
    return dm.DeviceModel(d, MR.generated_source(M), aux=x, nterms=K, nsums=M, name="generated%d_%dx%d" % (M, d, K)), x


# ---- the order contract ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_order_contract_bit_for_bit(M, d, K):
    m, x = _generated(M, d, K)
    p = np.random.RandomState(1000 * d + 10 * K + M).normal(size=(130, d))
    want = MR.generated_L(M, p, x)
    assert np.isfinite(want).all() and len(np.unique(want)) > 100
    L = m.loglike(p)
    assert L.shape == (130,) and np.array_equal(L, want), (M, d, K, np.abs(L - want).max())
    assert np.array_equal(S._eval_dev(m, p)[1], want), (M, d, K)


def test_order_contract_with_forty_passes_and_a_remainder():
    M, d, K = 3, 3, 64 * 40 + 7
    m, x = _generated(M, d, K)
    p = np.random.RandomState(5).normal(size=(130, d))
    want = MR.generated_L(M, p, x)
    assert np.array_equal(m.loglike(p), want)
    assert np.array_equal(S._eval_dev(m, p)[1], want)


# ---- amplitude_sum against a high-precision reference ------------------------------------------------------------------

@pytest.mark.parametrize("d,K", MR.AMPLITUDE_SHAPES)
def test_amplitude_sum_against_the_long_double_reference(d, K):
    """tolerance: 1e-12 * (sum_j |dL/ds_j| sum_k |t_jk| + |L|) (multisum_reference.amplitude_reference; that the bound is not
    vacuous and holds for the numpy restatement is checked without a GPU in test_multisum_model_compile.py)"""
    p, (X, y, w) = MR.amplitude_rows(d, K)
    m = usermodels.amplitude_sum(d, K, seed=d + K)
    twin = usermodels.amplitude_twin(d, K, seed=d + K)
    ref, tol, s2 = MR.amplitude_reference(p, X, y, w)
    assert (s2 >= K / 10.0).all()
    L, Lt = m.loglike(p), twin.loglike(p)
    print("max |L - ref| / tol: multi-sum %.3g, twin %.3g" % ((np.abs(L - ref) / tol).max(), (np.abs(Lt - ref) / tol).max()))
    assert (np.abs(L - ref) <= tol).all()
    assert (np.abs(Lt - ref) <= tol).all()
    # the sums are the contract's bit for bit, so L is the restatement's up to the device's log (the only operation of the
    # finish that numpy need not round the same way): one part in 1e15 of |log s2| and of |L|
    mine = MR.amplitude_finish(MR.contract(MR.amplitude_terms(p, X, y, w)))
    assert (np.abs(L - mine) <= 1e-15 * (np.abs(np.log(s2)) + np.abs(mine))).all()
    for x in (m, twin):
        x.close()


# ---- staircase3: exact sums, so the two forms agree bit for bit ------------------------------------------------------------

K3 = 150


@pytest.mark.parametrize("d,affine", [(3, False), (50, False), (130, True)])
def test_staircase3_forms_are_bit_identical(d, affine):
    s = usermodels.staircase3_sum(d, K3, seed=3, affine=affine)
    twin = usermodels.staircase3_twin(d, K3, seed=3, affine=affine)
    u = np.random.RandomState(22 + d).uniform(size=(300, d))
    p = s.transform(u)
    assert np.array_equal(p, twin.transform(u)) and np.array_equal(p, u * 20.0 + -10.0 if affine else u)
    c = usermodels.staircase_data(d, K3, seed=3, affine=affine)
    a = np.abs(p[:, np.arange(K3) % d] - c)
    s0, s1, s2 = (-np.floor(a * 8.0)).sum(axis=1), np.floor(a * 4.0).sum(axis=1), (-np.floor(a * 2.0)).sum(axis=1)   # (integers)
    want = s0 - s1 * s1 / (1.0 - s2)
    La, Lb = s.loglike(p), twin.loglike(p)
    assert np.array_equal(La, Lb) and np.array_equal(La, want)
    assert len(np.unique(want)) > 20
    pd, Ld = S._eval_dev(s, u, want_p=True)
    pt, Lt = S._eval_dev(twin, u, want_p=True)
    assert np.array_equal(pd, p) and np.array_equal(pt, p) and np.array_equal(Ld, want) and np.array_equal(Lt, want)
    for x in (s, twin):
        x.close()


# ---- position, mask, non-finite values ---------------------------------------------------------------------------------

def test_position_in_the_batch_does_not_matter():
    M, d, K = 3, 3, 65
    m, x = _generated(M, d, K)
    rs = np.random.RandomState(11)
    row = rs.normal(size=(1, d))
    want = MR.generated_L(M, row, x)
    for n in (130, 200):
        for at in (0, 63, 64, 129):
            batch = rs.normal(size=(n, d))
            batch[at] = row[0]
            assert np.array_equal(m.loglike(batch)[at:at + 1], want), (n, at)
            assert np.array_equal(S._eval_dev(m, batch)[1][at:at + 1], want), (n, at)


@functools.lru_cache(maxsize=None)
def _staircase_pair():
    return usermodels.staircase3_sum(D, K3, seed=3, affine=True), usermodels.staircase3_twin(D, K3, seed=3, affine=True)


@pytest.mark.parametrize("mask", ["all", "none", "every_third", "only_row_129"])
def test_membership(mask):
    n = 130
    m = _staircase_pair()[0]
    u = np.random.RandomState(12).uniform(size=(n, D))
    member = dict(all=np.ones(n, dtype=bool), none=np.zeros(n, dtype=bool), every_third=np.arange(n) % 3 == 0,
                  only_row_129=np.arange(n) == 129)[mask]
    p0, L0 = S._eval_dev(m, u, want_p=True)                 # the unmasked call
    assert np.array_equal(p0, u * 20.0 + -10.0) and np.isfinite(L0).all()
    p, L = S._eval_dev(m, u, want_p=True, member=member)
    assert np.isneginf(L[~member]).all() and (p[~member] == SENTINEL).all()
    assert np.array_equal(L[member], L0[member]) and np.array_equal(p[member], p0[member])
    # likelihood only (no p buffer): the same values
    L1 = S._eval_dev(m, p0, member=member)[1]
    assert np.isneginf(L1[~member]).all() and np.array_equal(L1[member], L0[member])


NAN_IN_ONE_SUM = r"""
__device__ void mlf_user_loglike_terms(const double *p, int d, const double *aux, long long naux, long long k, double *t) {
  t[0] = p[0] * 0.5;
  t[1] = k == (long long)aux[0] ? __builtin_nan("") : 1.0;
  t[2] = p[1];
}
__device__ double mlf_user_loglike_finish(const double *s, int nsums, const double *p, int d, const double *aux, long long naux) {
  if (aux[1] != 0.0) return s[0] + s[1] + s[2];
  return s[0] - s[2];      // s[1] is not looked at
}
"""


def test_a_nan_stays_in_its_accumulator():
    d, K = 3, 200
    p = np.random.RandomState(14).normal(size=(5, d))
    t = np.stack([np.repeat(p[:, :1] * 0.5, K, axis=1), np.ones((5, K)), np.repeat(p[:, 1:2], K, axis=1)], axis=1)
    s = MR.contract(t)
    for k_nan in (0, 70, 199):      # wherever the term sits
        ignoring = dm.DeviceModel(d, NAN_IN_ONE_SUM, aux=[float(k_nan), 0.0], nterms=K, nsums=3)
        L = ignoring.loglike(p)
        assert np.isfinite(L).all() and np.array_equal(L, s[:, 0] - s[:, 2]), (k_nan, L)
        using = dm.DeviceModel(d, NAN_IN_ONE_SUM, aux=[float(k_nan), 1.0], nterms=K, nsums=3)
        assert np.isnan(using.loglike(p)).all(), k_nan
        for x in (ignoring, using):
            x.close()
    clean = dm.DeviceModel(d, NAN_IN_ONE_SUM, aux=[-1.0, 1.0], nterms=K, nsums=3)     # no NaN term: all three sums are used
    assert np.array_equal(clean.loglike(p), s[:, 0] + s[:, 1] + s[:, 2])
    clean.close()


# ---- the routes, against the default-form twin ------------------------------------------------------------------------------

D = 3


@functools.lru_cache(maxsize=None)
def _live(n=100):
    u = np.clip(0.5 + 0.1 * np.random.RandomState(21).normal(size=(n, D)), 0.01, 0.99)
    twin = _staircase_pair()[1]
    return u, twin.loglike(twin.transform(u))


@pytest.mark.parametrize("method", ["sample_from_boundingbox", "sample_from_points"])
@pytest.mark.parametrize("gated", [False, True])
def test_region_refill_equals_the_twin(method, gated):
    from ultranest_amd import kernels
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = np.sort(Ls)[5]           # (a low threshold: the draws of a region around the live points are mostly worse than they)
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
                probe = region.refill(2048, -1e300, model.transform, model.loglike)
                tregion.enlarge = float(np.median(TR._quadratic_form(tregion, probe[1])))
                region.device_rng = DeviceRNG(seed=11)
                ungated = probe[3]
            got = region.refill(2048, Lmin, model.transform, model.loglike, **(dict(tregion=tregion) if gated else {}))
            out.append(got + (region.device_rng.offset,))
    finally:
        kernels.DeviceRegion.refill_user = orig
    assert len(calls) == (3 if gated else 2)
    (ua, pa, La, nca, oa), (ub, pb, Lb, ncb, ob) = out
    assert nca == ncb > 0 and oa == ob and 0 < len(ua) < nca       # (the threshold keeps some and drops some)
    assert np.array_equal(ua, ub) and np.array_equal(pa, pb) and np.array_equal(La, Lb) and (La > Lmin).all()
    if gated:
        assert tregion.inside(pa).all() and 0.2 * ungated <= nca <= 0.8 * ungated


def _slice_runs(model, region, u, Ls, Lmin, device_rng, calls=20):
    import ultranest_amd.popstepsampler as pop
    np.random.seed(8)
    s = pop.PopulationSliceSampler(popsize=64, nsteps=1, generate_direction=pop.generate_mixture_random_direction, scale=0.2,
                                   device_rng=device_rng)
    return [s.__next__(region, Lmin, u, Ls, model.transform, model.loglike) for _ in range(calls)]


@pytest.mark.parametrize("philox", [False, True])
def test_population_slice_sampler_equals_the_twin(philox):
    """host-RNG mode (mlf_walkers_finish_user) and Philox mode (mlf_walkers_step_user): 20 calls, record by record"""
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = Ls.min() - 0.5
    region = G._region(u)
    s, twin = _staircase_pair()
    a = _slice_runs(twin, region, u, Ls, Lmin, DeviceRNG(5) if philox else None)
    b = _slice_runs(s, region, u, Ls, Lmin, DeviceRNG(5) if philox else None)
    assert len(a) == len(b) == 20 and G._same_run(a, b) >= 1          # (calls that returned a point)
    assert sum(x[3] for x in a) == sum(x[3] for x in b) > 0


def test_random_walk_refill_equals_the_twin():
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = Ls.min() - 0.5
    region = S._host_region(u)
    done = []
    for model in _staircase_pair():
        s = pop.PopulationRandomWalkSampler(64, 5, pop.generate_mixture_random_direction, 0.05, device_rng=DeviceRNG(6))
        first = s.__next__(region, Lmin, u, Ls, model.transform, model.loglike)
        done.append((s, first))
    (sa, fa), (sb, fb) = done
    assert fa[3] == fb[3] == 64 * 5 and np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]) and fa[2] == fb[2]
    S._same_refill(sa.last_refill, sb.last_refill)
    assert (sa.last_refill["L"] > Lmin).all()
    S._same_prepared(sa.prepared_samples, sb.prepared_samples)
    assert len(sa.prepared_samples) == 63 and sa.scale == sb.scale and sa.nrejects == sb.nrejects
    assert sa.logstat == sb.logstat and sa.device_rng.offset == sb.device_rng.offset > 0


def test_simple_slice_refill_equals_the_twin():
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    Lmin = Ls.min() - 0.5
    region = S._host_region(u)
    done = []
    for model in _staircase_pair():
        s = pop.PopulationSimpleSliceSampler(64, 5, pop.generate_mixture_random_direction, scale_adapt_factor=0.8, max_it=20,
                                             device_rng=DeviceRNG(7))
        first = s.__next__(region, Lmin, u, Ls, model.transform, model.loglike)
        done.append((s, first))
    (sa, fa), (sb, fb) = done
    assert fa[3] == fb[3] > 0 and np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]) and fa[2] == fb[2]
    S._same_refill(sa.last_refill, sb.last_refill)
    assert (sa.last_refill["L"] > Lmin).all() and sa.ncalls == sb.ncalls == fa[3]
    S._same_prepared(sa.prepared_samples, sb.prepared_samples)
    assert len(sa.prepared_samples) == 63 and sa.scale == sb.scale
    assert sa.logstat == sb.logstat and sa.device_rng.offset == sb.device_rng.offset > 0


# ---- variants and lifetimes ----------------------------------------------------------------------------------------------

def test_a_multisum_model_of_the_other_variant_is_refused():
    from ultranest_amd.regions import DeviceRNG
    u, Ls = _live()
    s = _staircase_pair()[0]
    region = G._region(u)
    region.device_rng = DeviceRNG(41)
    region.current_sampling_method = region.sample_from_wrapping_ellipsoid
    tregion = TR._tregion(s.transform(u))
    got = region.refill(2048, -1e300, s.transform, s.loglike, tregion=tregion)
    assert got[3] > 0
    handle = region._dev.handle       # the t-region is set on it
    with pytest.raises(ValueError, match="the region has a t-region"):            # MLF_E_STATE
        handle.refill_user(1, 2048, 41, 0, -1e300, s.handle(True))
    handle.clear_tregion()
    with pytest.raises(ValueError, match="the region has no t-region"):
        handle.refill_user(1, 2048, 41, 0, -1e300, s.handle(True, gated=True))
    # the library's own check, for the launches that have no region in front of them
    from ultranest_amd import _lib
    L = np.empty(4)
    rows = np.full((4, D), 0.5)
    assert _lib.lib().mlf_usermodel_eval(s.handle(True, gated=True), _lib.ptr(rows), 4, None, _lib.ptr(L)) == 4     # MLF_E_STATE
    # a code object loaded as a variant it was not compiled as has no such entry
    gated_code = dm.compile_model(s.source, True, gated=True, summed=True, nsums=3)
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(s.code, D, True, s.aux, gated=True, nterms=K3, nsums=3)
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(gated_code, D, True, s.aux, nterms=K3, nsums=3)
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(s.code, D, True, s.aux, nterms=K3)                             # a multi-sum program as a single-sum model
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(s.code, D, True, s.aux)                                        # ... as a default model
    with pytest.raises(ValueError, match="no entry of this variant"):
        dm._Handle(_staircase_pair()[1].code, D, True, s.aux, nterms=K3, nsums=3)   # and the reverse
    assert len(handle.refill_user(1, 2048, 41, 0, -1e300, s.handle(True))[0]) >= got[3]     # the handle still works, ungated


def test_two_multisum_models_of_different_m_alternately_then_destroyed():
    rs = np.random.RandomState(9)
    d = 3
    p = rs.normal(size=(500, d))
    xs = {M: MR.generated_data(70 + M) for M in (2, 8)}
    want = {M: MR.generated_L(M, p, xs[M]) for M in (2, 8)}
    make = lambda M: dm.DeviceModel(d, MR.generated_source(M), aux=xs[M], nterms=70 + M, nsums=M)   # noqa: E731
    for M in (2, 8):
        m = make(M)
        assert np.array_equal(m.loglike(p), want[M])
        m.close()
    a, b = make(2), make(8)
    for _ in range(3):
        for m, M in ((a, 2), (b, 8)):
            assert np.array_equal(m.transform(p), p) and np.array_equal(m.loglike(p), want[M])
    a.close()
    assert np.array_equal(b.loglike(p), want[8])
    b.close()
