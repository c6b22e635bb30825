"""Derived parameters of a user model (DeviceModel(..., nderived=Q, derived_source=...): mlf_user_derived, compiled into its own
program with -DMLF_USER_DERIVED=1), CPU side: hiprtc compiles the derive program for gfx950 without a GPU -- one kernel,
mlf_user_derive_rows, no spills, no private segment -- while the model's main programs stay those of the model without nderived
(the same source string, cache keys and code objects); the choice of form and its LDS size; the argument checks; which entry
point every route takes (device entry points replaced by recorders)."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import test_devicemodel_compile as C     # (its metadata reader, the recording region and the stand-in walkers)
import test_tregion_routing as R         # (the same region with a t-region, and a host-built t-region)
from ultranest_amd import devicemodel as dm
from ultranest_amd import usermodels

HEADER_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mlfriends_hip.h")


def test_gauss_derived_compiles_one_more_program():
    g = usermodels.gauss(5)
    n = dm.compile_calls
    m = usermodels.gauss_derived(5)
    assert dm.compile_calls == n + 1                         # the derive program; the main program comes from the cache
    assert m.code is g.code and m.code == g.code and m.source == g.source
    assert m.nderived == 3 and m.nparams == 8 and m.ndim == 5 and g.nderived is None and g.nparams == 5
    assert m.derive_code[:4] == b"\x7fELF" and m.derive_code != m.code
    assert "mlf_user_derive_rows" in C._symbols(m.derive_code) and "mlf_user_rows" not in C._symbols(m.derive_code)
    assert usermodels.gauss_derived(5).derive_code is m.derive_code and dm.compile_calls == n + 1
    # with nterms / nsums: no more programs than the summed model's own and the one derive program
    src = usermodels.amplitude_sum(3, 65).source
    s = dm.DeviceModel(3, src, aux=np.arange(400.0), nterms=65, nsums=3)
    n = dm.compile_calls
    sd = dm.DeviceModel(3, src, aux=np.arange(400.0), nterms=65, nsums=3, nderived=3, derived_source=usermodels.GAUSS_DERIVED)
    assert dm.compile_calls == n + 1 and sd.code is s.code and sd.nparams == 6 and sd.summed


def _parents_key(source, has_transform, gated=False, summed=False, nsums=None):
    """the recipe of the cache key as it was before nderived existed, restated"""
    h = hashlib.sha256()
    with open(dm.HEADER, "rb") as fh:
        header = fh.read()
    options = repr((("--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off"), bool(has_transform)))
    if gated:
        options += " tregion"
        with open(dm.GATE_HEADER, "rb") as fh:
            header += fh.read()
    if summed:
        options += " sum"
    if nsums is not None:
        options += " sums=%d" % nsums
    for part in (source.encode(), b"\0", options.encode(), b"\0", header):
        h.update(part)
    return h.hexdigest()


def _derive_key(source):
    return dm._cache_key(source, dm.Form(False, derived="derive"))


def test_existing_cache_keys_are_what_they_were():
    m = usermodels.gauss_derived(5, affine=True)
    keys = set()
    for source in (m.source, usermodels.amplitude_sum(3, 65).source):
        for tr in (False, True):
            for gated in (False, True):
                for summed in (False, True):
                    assert dm._cache_key(source, tr, gated, summed) == _parents_key(source, tr, gated, summed)
                    keys.add(dm._cache_key(source, tr, gated, summed))
                for nsums in (1, 3, 8):
                    assert dm._cache_key(source, tr, gated, True, nsums=nsums) == _parents_key(source, tr, gated, True, nsums)
                    keys.add(dm._cache_key(source, tr, gated, True, nsums=nsums))
    assert len(keys) == 2 * 2 * 2 * 5
    # the derive program has a key of its own, over the source it is compiled from
    full = m.source + "\n" + usermodels.GAUSS_DERIVED
    assert _derive_key(full) not in keys and _derive_key(full) != _derive_key(m.source)
    assert _derive_key(full) != _parents_key(full, False)
    assert dm._code_cache[_derive_key(full)] is m.derive_code
    assert dm._code_cache[dm._cache_key(m.source, True)] is m.code


def _lds(d, nq):
    return dm._lib.lib().mlf_usermodel_derive_lds_bytes(d, nq)


@pytest.mark.parametrize("d,nq,staged", [(5, 3, True), (2, 1, True), (50, 3, True), (123, 3, True), (124, 3, False),
                                         (1, 125, True), (1, 126, False), (1000, 24, False)])
def test_derive_lds_bytes_either_side_of_the_budget(d, nq, staged):
    """64 * (d + nq + 2) * 8 bytes where that fits the 65536-byte budget (d + nq <= 126), else 0: the direct form"""
    assert (64 * (d + nq + 2) * 8 <= 65536) == staged
    assert _lds(d, nq) == (64 * (d + nq + 2) * 8 if staged else 0)


@pytest.mark.skipif(C.LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("d", [5, 124])
def test_derive_program_is_one_kernel_without_spills(d, tmp_path):
    """one program serves both forms (picked from d and nq at run time): checked at a staged and a direct pair"""
    assert (_lds(d, 3) != 0) == (d == 5)
    m = usermodels.gauss_derived(d)
    notes = C._notes(m.derive_code, tmp_path, "derive%d" % d)
    assert re.findall(r"\.name:\s+(\w+)", notes) == ["mlf_user_derive_rows"]
    assert len(re.findall(r"\.value_kind:\s+(?:global_buffer|by_value)", notes)) == 7
    for field in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        assert [int(x) for x in re.findall(r"\.%s:\s+(\d+)" % field, notes)] == [0], field


# ---- argument checks --------------------------------------------------------------------------------------------------

def _no_library(monkeypatch):
    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)


def test_nderived_and_derived_source_go_together(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="derived_source"):
        dm.DeviceModel(3, usermodels.ROSENBROCK_LOGLIKE, nderived=3)
    with pytest.raises(ValueError, match="nderived"):
        dm.DeviceModel(3, usermodels.ROSENBROCK_LOGLIKE, derived_source=usermodels.GAUSS_DERIVED)


@pytest.mark.parametrize("nderived", [0, -1, True, 2.0, "3"])
def test_bad_nderived_is_refused_before_any_library_call(nderived, monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="nderived"):
        dm.DeviceModel(3, usermodels.ROSENBROCK_LOGLIKE, nderived=nderived, derived_source=usermodels.GAUSS_DERIVED)


def test_too_many_columns_are_refused_before_any_library_call(monkeypatch):
    _no_library(monkeypatch)
    with pytest.raises(ValueError, match="nderived"):
        dm.DeviceModel(1000, usermodels.ROSENBROCK_LOGLIKE, nderived=25, derived_source=usermodels.GAUSS_DERIVED)
    with pytest.raises(ValueError, match="nderived"):
        dm.DeviceModel(1024, usermodels.ROSENBROCK_LOGLIKE, nderived=1, derived_source=usermodels.GAUSS_DERIVED)


def test_the_limit_itself_compiles():
    assert dm.DeviceModel(1000, usermodels.ROSENBROCK_LOGLIKE, nderived=24, derived_source=usermodels.GAUSS_DERIVED).nparams == 1024


def test_a_source_without_the_derived_function_does_not_compile():
    with pytest.raises(dm.DeviceModelCompileError) as ei:
        dm.DeviceModel(3, usermodels.ROSENBROCK_LOGLIKE, nderived=2, derived_source="// nothing here\n")
    assert "mlf_user_derived" in ei.value.log


def test_helpers_of_the_model_source_are_visible_to_the_derived_source():
    helper = "__device__ inline double mlf_twice(double x) { return x + x; }\n" + usermodels.ROSENBROCK_LOGLIKE
    derived = ("__device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux) {\n"
               "  q[0] = mlf_twice(p[0]);\n}\n")
    m = dm.DeviceModel(3, helper, usermodels.ROSENBROCK_TRANSFORM, nderived=1, derived_source=derived)
    assert m.code is dm.compile_model(helper + "\n" + usermodels.ROSENBROCK_TRANSFORM, True) and m.derive_code[:4] == b"\x7fELF"


def test_shapes_are_checked_before_any_library_call(monkeypatch):
    m = usermodels.gauss_derived(5)
    g = usermodels.gauss(5)
    _no_library(monkeypatch)
    for bad in (np.zeros((4, 6)), np.zeros((4, 9)), np.zeros(5)):
        with pytest.raises(ValueError, match="expects"):
            m.loglike(bad)
    for bad in (np.zeros((4, 8)), np.zeros((4, 4))):
        with pytest.raises(ValueError, match="expects"):
            m.derive(bad)
        with pytest.raises(ValueError, match="expects"):
            m.transform(bad)
    with pytest.raises(ValueError, match="expects"):
        g.loglike(np.zeros((4, 8)))                         # a model without nderived takes its own width only
    with pytest.raises(ValueError, match="nderived"):
        g.derive(np.zeros((4, 5)))
    assert m.derive(np.zeros((0, 5))).shape == (0, 8) and m.loglike(np.zeros((0, 8))).shape == (0,)


def test_library_entry_points_check_their_arguments():
    from ultranest_amd import _lib
    L = _lib.lib()
    m = usermodels.gauss_derived(5)
    size = ctypes.c_size_t(0)
    log = ctypes.create_string_buffer(256)
    full = (m.source + "\n" + usermodels.GAUSS_DERIVED).encode()
    assert L.mlf_usermodel_compile_variant(full, dm.INCLUDE_DIR.encode(), 0, 6, None, 0, ctypes.byref(size), log, 256) == 0
    assert size.value == len(m.derive_code)
    assert L.mlf_usermodel_compile_variant(full, dm.INCLUDE_DIR.encode(), 0, 7, None, 0, ctypes.byref(size), log, 256) == 1
    h = ctypes.c_void_p()
    aux = m.aux
    code = m.derive_code
    assert L.mlf_usermodel_create_derived(code, len(code), 5, 0, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert L.mlf_usermodel_create_derived(code, len(code), 0, 3, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert L.mlf_usermodel_create_derived(code, len(code), 1000, 25, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 2     # MLF_E_DIM
    assert L.mlf_usermodel_create_derived(b"not a code object" * 8, 136, 5, 3, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert L.mlf_usermodel_create_derived(code, len(code), 5, 3, None, 4, ctypes.byref(h)) == 1
    assert not h.value
    assert L.mlf_usermodel_derive(None, None, 0, None) == 1 and L.mlf_usermodel_derive_dev(None, None, 0, None, None) == 1


def test_abi_version_is_five():
    from ultranest_amd import _lib
    with open(HEADER_H) as fh:
        assert re.search(r"^#define MLF_ABI_VERSION 5$", fh.read(), re.M)
    assert _lib.ABI_VERSION == 5 and _lib.lib().mlf_abi_version() == 5
    with open(HEADER_H) as fh:
        assert re.search(r"^#define MLF_USERMODEL_DERIVED 6$", fh.read(), re.M)
    assert dm.VARIANT_DERIVED == 6


# ---- routing ---------------------------------------------------------------------------------------------------------

def _recording_region(calls, monkeypatch, cpu_region, d):
    from ultranest_amd import regions
    region = cpu_region(calls, monkeypatch, d=d)

    def refill_user_derived(self, region, use_scan, method, nsamples, Lmin, model):
        calls.append(("refill_user_derived", method, nsamples, Lmin, model))
        return np.zeros((1, d)), np.zeros((1, model.nparams)), np.zeros(1), 1

    monkeypatch.setattr(regions._DeviceState, "refill_user_derived", refill_user_derived)
    return region


def test_region_refill_takes_the_derived_entry(monkeypatch):
    from ultranest_amd import likelihoods as lk
    calls = []
    region = _recording_region(calls, monkeypatch, C._cpu_region, 7)
    m = usermodels.gauss_derived(7, affine=True)
    got = region.refill(100, -1.0, m.transform, m.loglike)
    assert calls[-1] == ("refill_user_derived", 0, 100, -1.0, m) and got[1].shape == (1, 10)
    # paired with identity_transform the host route yields no derived columns: the plain entry, d-wide rows
    got = region.refill(100, -2.0, lk.identity_transform, m.loglike)
    assert calls[-1] == ("refill_user", 0, 100, -2.0, m, False) and got[1].shape == (1, 7)
    assert dm.device_route(lk.identity_transform, m.loglike) == (m, False)
    assert dm.device_route(m.transform, m.loglike) == (m, True)
    # a model without nderived keeps its entry
    g = usermodels.gauss(7, affine=True)
    region.refill(100, -1.0, g.transform, g.loglike)
    assert calls[-1] == ("refill_user", 0, 100, -1.0, g, True)
    # a wrapper around the transform is a foreign callback, as before
    n = len(calls)
    assert region.refill(100, -1.0, lambda u: m.transform(u), m.loglike) is None and len(calls) == n


def test_region_refill_with_a_tregion_is_the_host_sequence(monkeypatch):
    calls = []
    region = _recording_region(calls, monkeypatch, R._cpu_region, R.D)
    m = usermodels.gauss_derived(R.D, affine=True)
    for t in (R._tregion(d=R.D + 3), R._tregion()):          # over all nparams columns (the driver's), and one over ndim
        assert region.refill(100, -1.0, m.transform, m.loglike, tregion=t) is None
    assert not calls
    # without one the batch goes to the derived entry (harness.refill_samples passes on what refill returns: it has no branch
    # of its own; it is not imported here, so that the modules that stub its kernels still import it first)
    got = region.refill(100, -1.0, m.transform, m.loglike, tregion=None)
    assert calls == [("refill_user_derived", 0, 100, -1.0, m)] and got[1].shape == (1, R.D + 3)


def test_population_slice_sampler_takes_the_user_route(monkeypatch):
    from ultranest_amd import likelihoods as lk
    from ultranest_amd.regions import DeviceRNG
    m = usermodels.gauss_derived(7, affine=True)
    assert C._sampler_call(monkeypatch, m.transform, m.loglike) == [("finish_user", -1.0, m, True, 0)]
    assert C._sampler_call(monkeypatch, lk.identity_transform, m.loglike) == [("finish_user", -1.0, m, False, 0)]
    assert C._sampler_call(monkeypatch, m.transform, m.loglike, DeviceRNG(5)) == [("step_user", -1.0, 6, m, True)]
    assert C._sampler_call(monkeypatch, lk.identity_transform, m.loglike, DeviceRNG(5)) == [("step_user", -1.0, 6, m, False)]


def test_whole_refill_samplers_take_the_user_route():
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods as lk
    from ultranest_amd.regions import DeviceRNG
    m = usermodels.gauss_derived(7, affine=True)
    rw = pop.PopulationRandomWalkSampler(8, 3, pop.generate_mixture_random_direction, 1.0, device_rng=DeviceRNG(3))
    assert rw._device_route(m.transform, m.loglike, 7) == (6, None, None, (m, True))
    assert rw._device_route(lk.identity_transform, m.loglike, 7) == (6, None, None, (m, False))
    ss = pop.PopulationSimpleSliceSampler(8, 3, pop.generate_mixture_random_direction, device_rng=DeviceRNG(3))
    assert ss._device_route(m.transform, m.loglike, 7) == (6, 0, None, None, (m, True))
    assert ss._device_route(lk.identity_transform, m.loglike, 7) == (6, 0, None, None, (m, False))


def test_harvested_rows_are_extended_only_where_the_host_route_would(monkeypatch):
    m = usermodels.gauss_derived(4, affine=True)
    g = usermodels.gauss(4, affine=True)
    seen = []

    def derive(p):
        seen.append(np.shape(p))
        return np.hstack([p, usermodels.gauss_derived_columns(p)])

    monkeypatch.setattr(m, "derive", derive)
    rows = np.arange(12.0).reshape(3, 4)
    wide = dm.extend_derived((m, True), rows)
    assert wide.shape == (3, 7) and np.array_equal(wide[:, :4], rows) and seen == [(3, 4)]
    one = dm.extend_derived((m, True), rows[1])
    assert one.shape == (7,) and np.array_equal(one, wide[1]) and seen[-1] == (1, 4)
    n = len(seen)
    assert dm.extend_derived((m, False), rows) is rows and dm.extend_derived((g, True), rows) is rows
    assert dm.extend_derived(None, rows) is rows and len(seen) == n
    # the walkers' record keeps nparams == d; p grows when a point is harvested, and only then
    import ultranest_amd.popstepsampler as pop
    row = rows[0]
    rec = dict(found=False, p=row)
    assert pop._Walkers._harvest_derived(rec, m, True)["p"] is row and len(seen) == n
    rec = dict(found=True, p=row)
    assert pop._Walkers._harvest_derived(rec, m, True)["p"].shape == (7,) and len(seen) == n + 1
    rec = dict(found=True, p=row)
    assert pop._Walkers._harvest_derived(rec, m, False)["p"] is row and len(seen) == n + 1


def test_model_handle_keys_the_derive_program_separately(monkeypatch):
    made = []

    class H(object):
        def __init__(self, code, ndim, has_transform, aux, gated=False, derived=None, nderived=None):
            assert (has_transform, gated, derived) == (False, False, "derive")
            made.append((code, ndim, nderived))
            self.handle = 100 + len(made)
            self.closed = False

        def close(self):
            self.closed = True

    monkeypatch.setattr(dm, "_Handle", H)
    m = usermodels.gauss_derived(5)
    a = m.derive_handle()
    assert m.derive_handle() == a and made == [(m.derive_code, 5, 3)]
    h = m._handles[dm.Form(False, derived="derive")]
    m.close()
    assert h.closed and m._handles == {}
    with pytest.raises(ValueError, match="nderived"):
        usermodels.gauss(5).derive_handle()


def test_numpy_restatement_of_the_derived_columns():
    p = np.random.RandomState(4).normal(size=(50, 6)) * 10.0 ** np.random.RandomState(5).uniform(-6, 6, size=(50, 6))
    q = usermodels.gauss_derived_columns(p)
    s = np.zeros(50)
    for k in range(6):
        s = s + p[:, k]
    assert q.shape == (50, 3) and np.array_equal(q[:, 2], s) and np.array_equal(q[:, 0], p[:, 0] + p[:, 1])
    assert np.array_equal(q[:, 1], p[:, 0] * p[:, 1])
