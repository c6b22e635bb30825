"""The summed form of a user model (DeviceModel(..., nterms=K): one wave per row around mlf_user_loglike_term, compiled with
-DMLF_USER_SUM=1), CPU side: hiprtc compiles its four programs for gfx950 without a GPU, each its own code object under its own
cache key with one kernel of the documented name and parameter count, no spills, no private segment, no static LDS and no
fused multiply-add; the default-form twins are what default models were; the argument checks need no device; every route
recognises a summed model as it does a default one (device entry points replaced by recorders)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import test_devicemodel_compile as C     # (its routing helpers: the recording region and the stand-in walkers)
import test_tregion_routing as R         # (the same region with a t-region, and a host-built t-region)
from ultranest_amd import devicemodel as dm
from ultranest_amd import usermodels

LLVM_BIN = next((p for p in ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin") if os.path.exists(os.path.join(p, "llvm-readelf"))),
                None)

MODELS = {
    "linear_sum": lambda affine: usermodels.linear_sum(3, 65, affine=affine),
    "staircase_sum": lambda affine: usermodels.staircase_sum(3, 150, affine=affine),
}
TWINS = {
    "linear_twin": lambda: usermodels.linear_twin(3, 65),
    "staircase_twin": lambda: usermodels.staircase_twin(3, 150, affine=True),
}


def _tool(name, code, tmp_path, tag, *args):
    path = os.path.join(str(tmp_path), tag + ".co")
    with open(path, "wb") as fh:
        fh.write(code)
    return subprocess.run([os.path.join(LLVM_BIN, name)] + list(args) + [path], capture_output=True, text=True, check=True).stdout


def _ints(field, notes):
    return [int(x) for x in re.findall(r"\.%s:\s+(\d+)" % field, notes)]


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("which", sorted(MODELS))
@pytest.mark.parametrize("with_transform", [True, False])
@pytest.mark.parametrize("gated", [False, True])
def test_summed_programs_are_one_kernel_each_without_spills(which, with_transform, gated, tmp_path):
    m = MODELS[which](with_transform)
    assert m.summed and m.nterms in (65, 150) and m.has_transform == with_transform
    before = dm.compile_calls
    code = dm.compile_model(m.source, with_transform, gated=gated, summed=True)
    assert code[:4] == b"\x7fELF"
    if not gated:
        assert code is m.code                                             # what the constructor compiled
    others = [dm.compile_model(m.source, with_transform, gated=g, summed=True) for g in (False, True) if g != gated]
    # the same source as a default-form program has no mlf_user_loglike: the other three variants of the summed program's
    # cache key are told apart by the key alone
    keys = {dm._cache_key(m.source, with_transform, g, s) for g in (False, True) for s in (False, True)}
    assert len(keys) == 4 and all(code != o for o in others)
    twin = TWINS[which.replace("_sum", "_twin")]()                        # the same terms as a default-form program
    assert all(code != dm.compile_model(twin.source, twin.has_transform, gated=g) for g in (False, True))
    n = dm.compile_calls
    assert dm.compile_model(m.source, with_transform, gated=gated, summed=True) is code and dm.compile_calls == n
    assert n <= before + 4
    notes = _tool("llvm-readelf", code, tmp_path, "sum", "--notes")
    assert re.findall(r"\.name:\s+(\w+)", notes) == ["mlf_user_rows_sum_tregion" if gated else "mlf_user_rows_sum"]
    assert len(re.findall(r"\.value_kind:\s+(?:global_buffer|by_value)", notes)) == (14 if gated else 9)
    for field in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        assert _ints(field, notes) == [0], field


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-objdump of ROCm not found")
@pytest.mark.parametrize("gated", [False, True])
def test_linear_sum_forms_no_fma(gated, tmp_path):
    m = usermodels.linear_sum(3, 65, affine=True)
    asm = _tool("llvm-objdump", dm.compile_model(m.source, True, gated=gated, summed=True), tmp_path, "lin", "-d")
    assert "v_mul_f64" in asm and "v_add_f64" in asm
    assert not re.search(r"\bv_fma_f64\b|\bv_fmac_f64\b", asm)


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("which", sorted(TWINS))
def test_default_form_twins_are_one_mlf_user_rows_with_eight_parameters(which, tmp_path):
    m = TWINS[which]()
    assert not m.summed and m.nterms is None
    notes = _tool("llvm-readelf", m.code, tmp_path, "twin", "--notes")
    assert re.findall(r"\.name:\s+(\w+)", notes) == ["mlf_user_rows"]
    assert len(re.findall(r"\.value_kind:\s+(?:global_buffer|by_value)", notes)) == 8
    for field in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        assert _ints(field, notes) == [0], field
    gated = _tool("llvm-readelf", dm.compile_model(m.source, m.has_transform, gated=True), tmp_path, "twing", "--notes")
    assert re.findall(r"\.name:\s+(\w+)", gated) == ["mlf_user_rows_tregion"]
    assert len(re.findall(r"\.value_kind:\s+(?:global_buffer|by_value)", gated)) == 13


def test_the_summed_and_the_default_program_of_one_source_differ():
    """A source with both functions compiles in all four variants: four cache keys, four programs."""
    both = (usermodels.LINEAR_TERM % 65 + usermodels.SUMMED_LOGLIKE % dict(name="mlf_linear_term")
            + usermodels.TWIN_LOGLIKE % dict(name="mlf_linear_term", K="MLF_LINEAR_K"))
    codes = [dm.compile_model(both, False, gated=g, summed=s) for g in (False, True) for s in (False, True)]
    assert all(c[:4] == b"\x7fELF" for c in codes) and len(set(codes)) == 4
    assert dm.DeviceModel(3, both).code is codes[0] and dm.DeviceModel(3, both, nterms=65).code is codes[1]


# ---- argument checks, all without a device ------------------------------------------------------------------------------

@pytest.mark.parametrize("nterms", [0, -3, 2.5, "4"])
def test_bad_nterms_is_refused_before_any_library_call(nterms, monkeypatch):
    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)
    source = usermodels.LINEAR_TERM % 65 + usermodels.SUMMED_LOGLIKE % dict(name="mlf_linear_term")
    with pytest.raises(ValueError, match="nterms"):
        dm.DeviceModel(3, source, nterms=nterms)


def test_a_source_without_the_term_function_does_not_compile():
    with pytest.raises(dm.DeviceModelCompileError) as ei:
        dm.DeviceModel(7, usermodels.ROSENBROCK_LOGLIKE, nterms=5)          # a default-form source
    assert "mlf_user_loglike_term" in ei.value.log
    with pytest.raises(dm.DeviceModelCompileError) as ei:                   # and the reverse
        dm.DeviceModel(3, usermodels.LINEAR_TERM % 65 + usermodels.SUMMED_LOGLIKE % dict(name="mlf_linear_term"))
    assert "mlf_user_loglike" in ei.value.log


def test_library_entry_points_check_their_arguments():
    from ultranest_amd import _lib
    L = _lib.lib()
    size = ctypes.c_size_t(0)
    log = ctypes.create_string_buffer(256)
    m = usermodels.linear_sum(3, 65)
    src = m.source.encode()
    assert L.mlf_usermodel_compile_variant(src, dm.INCLUDE_DIR.encode(), 0, 7, None, 0, ctypes.byref(size), log, 256) == 1
    assert b"variant" in L.mlf_last_error()
    for variant in (2, 3):     # a size query of each summed variant
        assert L.mlf_usermodel_compile_variant(src, dm.INCLUDE_DIR.encode(), 0, variant, None, 0, ctypes.byref(size), log, 256) == 0
        assert size.value > 64
    aux = m.aux
    h = ctypes.c_void_p()
    assert L.mlf_usermodel_create_variant(m.code, len(m.code), 3, 0, 2, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert b"mlf_usermodel_create_sum" in L.mlf_last_error() and not h.value
    assert L.mlf_usermodel_create_variant(m.code, len(m.code), 3, 0, 3, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert not h.value
    for variant, nterms in ((0, 65), (1, 65), (7, 65), (2, 0), (3, 0)):
        assert L.mlf_usermodel_create_sum(m.code, len(m.code), 3, 0, variant, nterms, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
        assert not h.value, (variant, nterms)
    # the other checks of create_variant come before the device as well
    assert L.mlf_usermodel_create_sum(m.code, len(m.code), 0, 0, 2, 65, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert L.mlf_usermodel_create_sum(b"not a code object" * 8, 136, 3, 0, 2, 65, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert L.mlf_usermodel_create_sum(m.code, len(m.code), 3, 0, 2, 65, None, 5, ctypes.byref(h)) == 1
    assert not h.value


# ---- routing ---------------------------------------------------------------------------------------------------------

def test_region_refill_takes_the_user_route(monkeypatch):
    from ultranest_amd import likelihoods as lk
    calls = []
    region = C._cpu_region(calls, monkeypatch)
    m = usermodels.linear_sum(7, 65, affine=True)
    assert region.refill(100, -1.0, m.transform, m.loglike) is not None
    assert calls[-1] == ("refill_user", 0, 100, -1.0, m, True)
    region.refill(100, -2.0, lk.identity_transform, m.loglike)
    assert calls[-1] == ("refill_user", 0, 100, -2.0, m, False)
    n = len(calls)
    assert region.refill(100, -1.0, lk.rosenbrock_transform, m.loglike) is None and len(calls) == n


def test_region_refill_with_a_tregion_takes_the_user_route(monkeypatch):
    calls = []
    region = R._cpu_region(calls, monkeypatch)
    m = usermodels.staircase_sum(R.D, 150, affine=True)
    t = R._tregion()
    got = R._harness().refill_samples(region, t, m.transform, m.loglike, -1.0, 100)
    assert len(got) == 4 and calls[-1] == ("refill_user", 0, 100, -1.0, m, True, dict(tregion=t))
    region.refill(100, -1.0, m.transform, m.loglike, tregion=t)
    assert calls[-1] == ("refill_user", 0, 100, -1.0, m, True, dict(tregion=t))


def test_population_slice_sampler_takes_the_user_route(monkeypatch):
    from ultranest_amd import likelihoods as lk
    from ultranest_amd.regions import DeviceRNG
    m = usermodels.staircase_sum(7, 150, affine=True)
    assert C._sampler_call(monkeypatch, m.transform, m.loglike) == [("finish_user", -1.0, m, True, 0)]
    assert C._sampler_call(monkeypatch, lk.identity_transform, m.loglike) == [("finish_user", -1.0, m, False, 0)]
    assert C._sampler_call(monkeypatch, lk.rosenbrock_transform, m.loglike) == [("finish", -1.0, 0)]
    assert C._sampler_call(monkeypatch, m.transform, m.loglike, DeviceRNG(5)) == [("step_user", -1.0, 6, m, True)]
    assert C._sampler_call(monkeypatch, lk.identity_transform, m.loglike, DeviceRNG(5)) == [("step_user", -1.0, 6, m, False)]


def test_whole_refill_samplers_take_the_user_route():
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods as lk
    from ultranest_amd.regions import DeviceRNG
    m = usermodels.staircase_sum(7, 150, affine=True)
    rw = pop.PopulationRandomWalkSampler(8, 3, pop.generate_mixture_random_direction, 1.0, device_rng=DeviceRNG(3))
    assert rw._device_route(m.transform, m.loglike, 7) == (6, None, None, (m, True))
    assert rw._device_route(lk.identity_transform, m.loglike, 7) == (6, None, None, (m, False))
    assert rw._device_route(lk.rosenbrock_transform, m.loglike, 7) is None
    ss = pop.PopulationSimpleSliceSampler(8, 3, pop.generate_mixture_random_direction, device_rng=DeviceRNG(3))
    assert ss._device_route(m.transform, m.loglike, 7) == (6, 0, None, None, (m, True))
    assert ss._device_route(lk.identity_transform, m.loglike, 7) == (6, 0, None, None, (m, False))
    for s in (pop.PopulationRandomWalkSampler(8, 3, pop.generate_mixture_random_direction, 1.0),
              pop.PopulationSimpleSliceSampler(8, 3, pop.generate_mixture_random_direction)):
        assert s._device_route(m.transform, m.loglike, 7) is None            # no device_rng: the host loop


def test_model_handle_keys_the_summed_variants_separately(monkeypatch):
    made = []

    class H(object):
        def __init__(self, code, ndim, has_transform, aux, gated=False, nterms=None):
            made.append((code, has_transform, gated, nterms))
            self.handle = len(made)

        def close(self):
            pass

    monkeypatch.setattr(dm, "_Handle", H)
    m = usermodels.linear_sum(3, 65, affine=True)
    a, b, c, e = m.handle(True), m.handle(True, gated=True), m.handle(False, gated=True), m.handle(False)
    assert len({a, b, c, e}) == 4 and m.handle(True, gated=True) == b and m.handle(True) == a and len(made) == 4
    assert made[0] == (m.code, True, False, 65)
    assert made[1] == (dm.compile_model(m.source, True, gated=True, summed=True), True, True, 65)
    assert made[2] == (dm.compile_model(m.source, False, gated=True, summed=True), False, True, 65)
    assert made[3] == (dm.compile_model(m.source, False, summed=True), False, False, 65)
    assert len({x[0] for x in made}) == 4
    # a default model's handles are made as they were (no nterms in the call)
    t = usermodels.linear_twin(3, 65, affine=True)
    t.handle(True, gated=True)
    assert made[-1] == (dm.compile_model(t.source, True, gated=True), True, True, None)
    m.close()
    t.close()


def test_numpy_restatement_is_not_a_pairwise_sum():
    """The order contract in numpy (the GPU tests use it): sequential additions per lane, then the six exchange steps."""
    rs = np.random.RandomState(3)
    t = rs.normal(size=200) * 10.0 ** rs.uniform(-8, 8, size=200)
    s = np.zeros(64)
    for k in range(200):
        s[k % 64] += t[k]
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[np.arange(64) ^ m]
    assert (s == s[0]).all()                                   # IEEE addition commutes: every lane holds the same bits
    assert abs(s[0] - np.sum(t)) <= 1e-12 * np.abs(t).sum()
