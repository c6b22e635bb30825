"""Several sums and a final function (DeviceModel(..., nterms=K, nsums=M): mlf_user_loglike_terms / mlf_user_loglike_finish,
compiled with -DMLF_USER_SUM=1 -DMLF_USER_NSUMS=M), CPU side: hiprtc compiles the programs for gfx950 without a GPU, each its own
code object under its own cache key with one kernel of the documented name and parameter count, no spills, no private segment,
no static LDS and no fused multiply-add; without nsums every key and program is what it was; the argument checks need no
library; every route recognises such a model as it does a summed one (device entry points replaced by recorders)."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import multisum_reference as MR           # (sources and numpy restatements shared with the GPU tests)
import test_devicemodel_compile as C     # (its routing helpers: the recording region and the stand-in walkers)
import test_tregion_routing as R         # (the same region with a t-region, and a host-built t-region)
from ultranest_amd import devicemodel as dm
from ultranest_amd import usermodels

LLVM_BIN = next((p for p in ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin") if os.path.exists(os.path.join(p, "llvm-readelf"))),
                None)

MODELS = {
    "amplitude_sum": lambda affine: usermodels.amplitude_sum(3, 65, affine=affine),
    "staircase3_sum": lambda affine: usermodels.staircase3_sum(3, 150, affine=affine),
}


def _tool(name, code, tmp_path, tag, *args):
    path = os.path.join(str(tmp_path), tag + ".co")
    with open(path, "wb") as fh:
        fh.write(code)
    return subprocess.run([os.path.join(LLVM_BIN, name)] + list(args) + [path], capture_output=True, text=True, check=True).stdout


def _ints(field, notes):
    return [int(x) for x in re.findall(r"\.%s:\s+(\d+)" % field, notes)]


def _one_kernel_without_spills(code, gated, tmp_path):
    assert code[:4] == b"\x7fELF"
    notes = _tool("llvm-readelf", code, tmp_path, "sums", "--notes")
    assert re.findall(r"\.name:\s+(\w+)", notes) == ["mlf_user_rows_sums_tregion" if gated else "mlf_user_rows_sums"]
    assert len(re.findall(r"\.value_kind:\s+(?:global_buffer|by_value)", notes)) == (14 if gated else 9)
    for field in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        assert _ints(field, notes) == [0], field


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("which", sorted(MODELS))
@pytest.mark.parametrize("with_transform", [True, False])
@pytest.mark.parametrize("gated", [False, True])
def test_multisum_programs_are_one_kernel_each_without_spills(which, with_transform, gated, tmp_path):
    m = MODELS[which](with_transform)
    assert m.summed and m.nsums == 3 and m.nterms in (65, 150) and m.has_transform == with_transform
    code = dm.compile_model(m.source, with_transform, gated=gated, summed=True, nsums=3)
    if not gated:
        assert code is m.code                                             # what the constructor compiled
    other = dm.compile_model(m.source, with_transform, gated=not gated, summed=True, nsums=3)
    assert other != code
    n = dm.compile_calls
    assert dm.compile_model(m.source, with_transform, gated=gated, summed=True, nsums=3) is code and dm.compile_calls == n
    _one_kernel_without_spills(code, gated, tmp_path)


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("gated", [False, True])
def test_eight_sums_stay_in_registers(gated, tmp_path):
    m = dm.DeviceModel(3, MR.generated_source(8), usermodels.AFFINE_TRANSFORM, aux=np.arange(70.0), nterms=70, nsums=8)
    assert m.nsums == 8
    _one_kernel_without_spills(dm.compile_model(m.source, True, gated=gated, summed=True, nsums=8), gated, tmp_path)


# amplitude_sum's terms and sums with a finish of + - * only: this program has nothing the compiler expands into fused operations
PLAIN_FINISH = usermodels.AMPLITUDE_TERMS % 65 + r"""
__device__ void mlf_user_loglike_terms(const double *p, int d, const double *aux, long long naux, long long k, double *t) {
  mlf_amplitude_terms(p, d, aux, k, t);
}
__device__ double mlf_user_loglike_finish(const double *s, int nsums, const double *p, int d, const double *aux, long long naux) {
  return -0.5 * (s[0] - s[1] * s[1] * s[2]) - 0.5 * s[2];
}
""" + usermodels.AFFINE_TRANSFORM


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-objdump of ROCm not found")
@pytest.mark.parametrize("gated", [False, True])
def test_amplitude_sum_forms_no_fma(gated, tmp_path):
    """No multiply and add of the user's code, the transform, the accumulation or the exchange is fused.

    amplitude_sum's finish divides and takes a logarithm, and the compiler expands an IEEE binary64 division and log() into
    sequences that are built from v_fma_f64 (v_div_scale / v_rcp / v_fma ... / v_div_fmas / v_div_fixup): a few
    v_fma_f64 / v_fmac_f64 (printed below), every one behind the last exchange step.  So "no v_fma_f64 anywhere in amplitude_sum"
    cannot hold for any program with this finish; what -ffp-contract=off promises is checked in two parts that together ask the
    same of every operation the user wrote: (a) everything up to and including the last exchange step of amplitude_sum
    (transform, gate, term loop, accumulation, the six steps) has no fused operation, and what follows has the division's and
    the logarithm's expansions; (b) the same terms with a finish of + - * only (whose multiply-subtract pairs are candidates
    for contraction as much as amplitude_sum's) have none in the whole program."""
    fused = r"\bv_fmac?_f64"                                                # (v_fma_f64, v_fmac_f64_e32, ...)
    m = usermodels.amplitude_sum(3, 65, affine=True)
    asm = _tool("llvm-objdump", dm.compile_model(m.source, True, gated=gated, summed=True, nsums=3), tmp_path, "amp", "-d")
    assert "v_mul_f64" in asm and "v_add_f64" in asm
    last_exchange = asm.rindex("ds_bpermute_b32")
    assert asm.count("ds_bpermute_b32") == 6 * 3 * 2                       # six steps, three sums, two halves each
    assert not re.search(fused, asm[:last_exchange])
    tail = asm[last_exchange:]
    print("fused operations behind the last exchange step:", len(re.findall(fused, tail)))
    assert "v_div_fixup_f64" in tail and "v_div_fmas_f64" in tail and "v_frexp_mant_f64" in tail    # the division, the log
    plain = _tool("llvm-objdump", dm.compile_model(PLAIN_FINISH, True, gated=gated, summed=True, nsums=3), tmp_path, "plain", "-d")
    assert "v_mul_f64" in plain and "v_add_f64" in plain and plain.count("ds_bpermute_b32") == 36
    assert not re.search(fused, plain)


# ---- cache keys ----------------------------------------------------------------------------------------------------------

def _todays_key(source, has_transform, gated=False, summed=False):
    """the recipe of the cache key as it was before nsums existed, restated"""
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
    for part in (source.encode(), b"\0", options.encode(), b"\0", header):
        h.update(part)
    return h.hexdigest()


ALL_FORMS = (usermodels.LINEAR_TERM % 65 + usermodels.SUMMED_LOGLIKE % dict(name="mlf_linear_term")
             + usermodels.AMPLITUDE_TERMS % 65 + usermodels.MULTISUM_LOGLIKE % dict(name="mlf_amplitude"))


def test_nsums_keys_and_programs():
    """One source that defines the term function, the terms function and finish: nsums 1, 3 and None are three keys and three
    programs, a repeated compile hits the cache, and without nsums the key is today's."""
    keys = [dm._cache_key(ALL_FORMS, False, False, True, nsums=n) for n in (1, 3, None)]
    assert len(set(keys)) == 3
    codes = [dm.compile_model(ALL_FORMS, False, summed=True, nsums=n) for n in (1, 3, None)]
    assert all(c[:4] == b"\x7fELF" for c in codes) and len(set(codes)) == 3
    n = dm.compile_calls
    again = [dm.compile_model(ALL_FORMS, False, summed=True, nsums=k) for k in (1, 3, None)]
    assert all(a is b for a, b in zip(again, codes)) and dm.compile_calls == n
    for tr in (False, True):
        for gated in (False, True):
            for summed in (False, True):
                want = _todays_key(ALL_FORMS, tr, gated, summed)
                assert dm._cache_key(ALL_FORMS, tr, gated, summed) == want
                assert dm._cache_key(ALL_FORMS, tr, gated=gated, summed=summed, nsums=None) == want
            assert dm._cache_key(ALL_FORMS, tr, gated, True, nsums=3) != _todays_key(ALL_FORMS, tr, gated, True)
    # compile_model with its present arguments returns what the present entry point returns
    assert dm.compile_model(ALL_FORMS, False, False, True) is codes[2]
    L = dm._lib.lib()
    size = ctypes.c_size_t(0)
    log = ctypes.create_string_buffer(1 << 12)
    buf = ctypes.create_string_buffer(1 << 20)
    assert L.mlf_usermodel_compile_variant(ALL_FORMS.encode(), dm.INCLUDE_DIR.encode(), 0, 2, buf, 1 << 20, ctypes.byref(size), log,
                                           len(log)) == 0
    assert buf.raw[:size.value] == codes[2]
    # the models carry the attribute; a model without nsums is the summed model it was
    assert dm.DeviceModel(3, ALL_FORMS, nterms=65).nsums is None and dm.DeviceModel(3, ALL_FORMS, nterms=65).code is codes[2]
    assert dm.DeviceModel(3, ALL_FORMS, nterms=65, nsums=3).code is codes[1]
    one = dm.DeviceModel(3, ALL_FORMS, nterms=65, nsums=1)
    assert one.nsums == 1 and one.summed and one.code is codes[0]


# ---- argument checks --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nsums", [0, -1, 9, 2.5, "3", True])
def test_bad_nsums_is_refused_before_any_library_call(nsums, monkeypatch):
    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)
    with pytest.raises(ValueError, match="nsums"):
        dm.DeviceModel(3, ALL_FORMS, nterms=65, nsums=nsums)
    with pytest.raises(ValueError, match="nsums"):
        dm.compile_model(ALL_FORMS, False, summed=True, nsums=nsums)


def test_nsums_without_nterms_is_refused_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)
    with pytest.raises(ValueError, match="nsums"):
        dm.DeviceModel(3, ALL_FORMS, nsums=3)
    with pytest.raises(ValueError, match="nsums"):
        dm.compile_model(ALL_FORMS, False, nsums=3)


def test_sources_that_must_not_compile():
    only_term = usermodels.LINEAR_TERM % 65 + usermodels.SUMMED_LOGLIKE % dict(name="mlf_linear_term")
    with pytest.raises(dm.DeviceModelCompileError) as ei:
        dm.DeviceModel(3, only_term, nterms=65, nsums=2)
    assert "mlf_user_loglike_terms" in ei.value.log
    source = usermodels.AMPLITUDE_TERMS % 65 + usermodels.MULTISUM_LOGLIKE % dict(name="mlf_amplitude")
    no_finish = source[:source.index("__device__ double mlf_user_loglike_finish")]
    assert "mlf_user_loglike_terms" in no_finish
    with pytest.raises(dm.DeviceModelCompileError) as ei:
        dm.DeviceModel(3, no_finish, nterms=65, nsums=3)
    assert "mlf_user_loglike_finish" in ei.value.log
    # and a multi-sum source is no single-sum one
    with pytest.raises(dm.DeviceModelCompileError) as ei:
        dm.DeviceModel(3, source, nterms=65)
    assert "mlf_user_loglike_term" in ei.value.log


def test_library_entry_points_check_their_arguments():
    from ultranest_amd import _lib
    L = _lib.lib()
    size = ctypes.c_size_t(0)
    log = ctypes.create_string_buffer(256)
    m = usermodels.amplitude_sum(3, 65)
    src, inc = m.source.encode(), dm.INCLUDE_DIR.encode()
    for variant in (0, 1, 2, 3, 6):
        assert L.mlf_usermodel_compile_sums(src, inc, 0, variant, 3, None, 0, ctypes.byref(size), log, 256) == 1, variant
        assert b"variant" in L.mlf_last_error()
    for nsums in (0, -1, 9):
        assert L.mlf_usermodel_compile_sums(src, inc, 0, 4, nsums, None, 0, ctypes.byref(size), log, 256) == 1, nsums
        assert b"nsums" in L.mlf_last_error()
    for variant in (4, 5):
        assert L.mlf_usermodel_compile_variant(src, inc, 0, variant, None, 0, ctypes.byref(size), log, 256) == 1
        assert b"mlf_usermodel_compile_sums" in L.mlf_last_error()
        assert L.mlf_usermodel_compile_sums(src, inc, 0, variant, 3, None, 0, ctypes.byref(size), log, 256) == 0   # a size query
        assert size.value > 64
    aux = m.aux
    h = ctypes.c_void_p()
    for variant in (4, 5):
        assert L.mlf_usermodel_create_variant(m.code, len(m.code), 3, 0, variant, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
        assert b"mlf_usermodel_create_sum" in L.mlf_last_error() and not h.value
        assert L.mlf_usermodel_create_sum(m.code, len(m.code), 3, 0, variant, 0, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
        assert L.mlf_usermodel_create_sum(m.code, len(m.code), 0, 0, variant, 65, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
        assert L.mlf_usermodel_create_sum(b"not a code object" * 8, 136, 3, 0, variant, 65, _lib.ptr(aux), len(aux),
                                          ctypes.byref(h)) == 1
        assert not h.value
    assert L.mlf_usermodel_create_sum(m.code, len(m.code), 3, 0, 6, 65, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert not h.value


# ---- routing ---------------------------------------------------------------------------------------------------------

def test_region_refill_takes_the_user_route(monkeypatch):
    from ultranest_amd import likelihoods as lk
    calls = []
    region = C._cpu_region(calls, monkeypatch)
    m = usermodels.amplitude_sum(7, 65, affine=True)
    assert region.refill(100, -1.0, m.transform, m.loglike) is not None
    assert calls[-1] == ("refill_user", 0, 100, -1.0, m, True)
    region.refill(100, -2.0, lk.identity_transform, m.loglike)
    assert calls[-1] == ("refill_user", 0, 100, -2.0, m, False)
    n = len(calls)
    assert region.refill(100, -1.0, lk.rosenbrock_transform, m.loglike) is None and len(calls) == n


def test_region_refill_with_a_tregion_takes_the_user_route(monkeypatch):
    calls = []
    region = R._cpu_region(calls, monkeypatch)
    m = usermodels.staircase3_sum(R.D, 150, affine=True)
    t = R._tregion()
    got = R._harness().refill_samples(region, t, m.transform, m.loglike, -1.0, 100)
    assert len(got) == 4 and calls[-1] == ("refill_user", 0, 100, -1.0, m, True, dict(tregion=t))
    region.refill(100, -1.0, m.transform, m.loglike, tregion=t)
    assert calls[-1] == ("refill_user", 0, 100, -1.0, m, True, dict(tregion=t))


def test_population_slice_sampler_takes_the_user_route(monkeypatch):
    from ultranest_amd import likelihoods as lk
    from ultranest_amd.regions import DeviceRNG
    m = usermodels.staircase3_sum(7, 150, affine=True)
    assert C._sampler_call(monkeypatch, m.transform, m.loglike) == [("finish_user", -1.0, m, True, 0)]
    assert C._sampler_call(monkeypatch, lk.identity_transform, m.loglike) == [("finish_user", -1.0, m, False, 0)]
    assert C._sampler_call(monkeypatch, lk.rosenbrock_transform, m.loglike) == [("finish", -1.0, 0)]
    assert C._sampler_call(monkeypatch, m.transform, m.loglike, DeviceRNG(5)) == [("step_user", -1.0, 6, m, True)]
    assert C._sampler_call(monkeypatch, lk.identity_transform, m.loglike, DeviceRNG(5)) == [("step_user", -1.0, 6, m, False)]


def test_whole_refill_samplers_take_the_user_route():
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods as lk
    from ultranest_amd.regions import DeviceRNG
    m = usermodels.staircase3_sum(7, 150, affine=True)
    rw = pop.PopulationRandomWalkSampler(8, 3, pop.generate_mixture_random_direction, 1.0, device_rng=DeviceRNG(3))
    assert rw._device_route(m.transform, m.loglike, 7) == (6, None, None, (m, True))
    assert rw._device_route(lk.identity_transform, m.loglike, 7) == (6, None, None, (m, False))
    assert rw._device_route(lk.rosenbrock_transform, m.loglike, 7) is None
    ss = pop.PopulationSimpleSliceSampler(8, 3, pop.generate_mixture_random_direction, device_rng=DeviceRNG(3))
    assert ss._device_route(m.transform, m.loglike, 7) == (6, 0, None, None, (m, True))
    assert ss._device_route(lk.identity_transform, m.loglike, 7) == (6, 0, None, None, (m, False))


def test_model_handle_keys_the_multisum_variants_separately(monkeypatch):
    made = []

    class H(object):
        def __init__(self, code, ndim, has_transform, aux, gated=False, nterms=None, nsums=None):
            made.append((code, has_transform, gated, nterms, nsums))
            self.handle = len(made)

        def close(self):
            pass

    monkeypatch.setattr(dm, "_Handle", H)
    m = usermodels.amplitude_sum(3, 65, affine=True)
    a, b, c, e = m.handle(True), m.handle(True, gated=True), m.handle(False, gated=True), m.handle(False)
    assert len({a, b, c, e}) == 4 and m.handle(True, gated=True) == b and m.handle(True) == a and len(made) == 4
    assert made[0] == (m.code, True, False, 65, 3)
    assert made[1] == (dm.compile_model(m.source, True, gated=True, summed=True, nsums=3), True, True, 65, 3)
    assert made[2] == (dm.compile_model(m.source, False, gated=True, summed=True, nsums=3), False, True, 65, 3)
    assert made[3] == (dm.compile_model(m.source, False, summed=True, nsums=3), False, False, 65, 3)
    assert len({x[0] for x in made}) == 4
    # the same source with another number of sums: other programs under other keys
    m1 = dm.DeviceModel(3, m.source[:len(m.source)], aux=m.aux, nterms=65, nsums=1)
    m1.handle(False)
    assert made[-1][4] == 1 and made[-1][0] not in {x[0] for x in made[:4]}
    # a single-sum model's handles are made as they were (no nsums in the call)
    s = usermodels.linear_sum(3, 65, affine=True)
    s.handle(True, gated=True)
    assert made[-1] == (dm.compile_model(s.source, True, gated=True, summed=True), True, True, 65, None)
    for x in (m, m1, s):
        x.close()


def test_the_twins_are_default_models():
    for t in (usermodels.amplitude_twin(3, 65), usermodels.staircase3_twin(3, 150, affine=True)):
        assert not t.summed and t.nterms is None and t.nsums is None
        assert t.code is dm.compile_model(t.source, t.has_transform)


def test_numpy_restatement_of_several_sums():
    """The extended order contract in numpy (the GPU tests use it): every accumulator on its own in the single-sum order."""
    rs = np.random.RandomState(3)
    t = rs.normal(size=(3, 200)) * 10.0 ** rs.uniform(-8, 8, size=(3, 200))
    s = np.zeros((3, 64))
    for k in range(200):
        s[:, k % 64] += t[:, k]
    for m in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ m]
    assert (s == s[:, :1]).all()
    for j in range(3):                                           # accumulator j alone gives the same bits
        one = np.zeros(64)
        for k in range(200):
            one[k % 64] += t[j, k]
        for m in (32, 16, 8, 4, 2, 1):
            one = one + one[np.arange(64) ^ m]
        assert one[0] == s[j, 0]


@pytest.mark.parametrize("d,K", MR.AMPLITUDE_SHAPES)
def test_amplitude_bound_is_not_vacuous_and_holds_for_the_restatement(d, K):
    """The bound of the GPU test, checked where no GPU is needed: the seeded data keep s2 at about K / 10 or more (so the
    derivatives in the bound stay moderate), and the numpy restatement of the order contract lies inside the bound around the
    long-double reference."""
    p, (X, y, w) = MR.amplitude_rows(d, K)
    t = MR.amplitude_terms(p, X, y, w)
    L = MR.amplitude_finish(MR.contract(t))
    ref, tol, s2 = MR.amplitude_reference(p, X, y, w)
    print("min s2 / K = %.3g, max |L - ref| / tol = %.3g, max tol / |L| = %.3g" % ((s2 / K).min(), (np.abs(L - ref) / tol).max(),
                                                                              (tol / np.abs(ref)).max()))
    assert (s2 >= K / 10.0).all()
    assert (tol <= 1e-10 * np.abs(ref)).all()            # not vacuous: a few hundred times the scale of L at the most
    assert (np.abs(L - ref) <= tol).all()
