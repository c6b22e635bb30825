"""User models (ultranest_amd.devicemodel), CPU side: hiprtc compiles the example models for gfx950 without a GPU, the
per-process cache, compile errors, register spills of the wrapper kernel, argument checks and the routing of the samplers
(device entry points replaced by recorders)."""
import os
import re
import struct
import subprocess
import types

import numpy as np
import pytest

from ultranest_amd import devicemodel as dm
from ultranest_amd import usermodels

LLVM_BIN = next((p for p in ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin") if os.path.exists(os.path.join(p, "llvm-readelf"))),
                None)


def _symbols(code):
    """names of the defined symbols of an ELF64 little-endian code object (section headers -> .symtab / .dynsym)"""
    shoff, = struct.unpack_from("<Q", code, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", code, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", code, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for name, typ, flags, addr, off, size, link, info, align, entsize in secs:
        if typ not in (2, 11):      # SHT_SYMTAB, SHT_DYNSYM
            continue
        stroff = secs[link][4]
        for k in range(size // 24):
            st_name, st_info, st_other, st_shndx = struct.unpack_from("<IBBH", code, off + k * 24)
            if st_shndx == 0 or st_name == 0:
                continue
            end = code.index(b"\0", stroff + st_name)
            names.add(code[stroff + st_name:end].decode())
    return names


def _notes(code, tmp_path, tag):
    path = os.path.join(str(tmp_path), tag + ".co")
    with open(path, "wb") as fh:
        fh.write(code)
    return subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", path], capture_output=True, text=True,
                          check=True).stdout


MODELS = {
    "R": lambda: usermodels.rosenbrock(7),
    "F": lambda: usermodels.funnel(51),
    "G": lambda: usermodels.gauss(10),
}


@pytest.mark.parametrize("which", sorted(MODELS))
def test_example_models_compile_to_gfx950_code_objects(which):
    m = MODELS[which]()
    code = m.code
    assert code[:4] == b"\x7fELF" and code[4] == 2 and code[5] == 1          # ELF64, little endian
    e_machine, = struct.unpack_from("<H", code, 18)
    assert e_machine == 0xE0                                                  # EM_AMDGPU
    assert "mlf_user_rows" in _symbols(code)
    assert m.loglike.device_spec.model is m and m.transform.device_spec.model is m
    assert not isinstance(m.loglike.device_spec, tuple)


def test_second_compile_comes_from_the_cache():
    src = usermodels.ROSENBROCK_LOGLIKE + "\n// cache probe %d\n" % os.getpid()
    before = dm.compile_calls
    a = dm.DeviceModel(5, src)
    assert dm.compile_calls == before + 1
    b = dm.DeviceModel(5, src)
    assert dm.compile_calls == before + 1
    assert a.code == b.code
    # with a transform it is another program
    dm.DeviceModel(5, src, usermodels.ROSENBROCK_TRANSFORM)
    assert dm.compile_calls == before + 2


def test_compile_errors_carry_the_hiprtc_log():
    bad = ("__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) {\n"
           "  double s = 0.0;\n"
           "  s += p[0]\n"
           "  return s;\n"
           "}\n")
    with pytest.raises(dm.DeviceModelCompileError) as ei:
        dm.DeviceModel(3, bad)
    log = ei.value.log
    assert "error" in log and re.search(r"mlf_user_model\.hip:3:\d+", log), log
    with pytest.raises(dm.DeviceModelCompileError) as ei:
        dm.DeviceModel(3, "__device__ double not_the_likelihood(const double *p) { return p[0]; }\n")
    assert "mlf_user_loglike" in ei.value.log


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("which", ["R", "F"])
@pytest.mark.parametrize("with_transform", [True, False])
def test_wrapper_kernel_has_no_register_spills(which, with_transform, tmp_path):
    """One kernel holds both forms (LDS-staged and direct, picked by d at run time); the identity variant (a route that pairs
    the likelihood with identity_transform) is the other program."""
    m = MODELS[which]()
    code = m.code if with_transform else dm.compile_model(m.source, False)
    notes = _notes(code, tmp_path, which + str(with_transform))
    assert ".name:           mlf_user_rows" in notes or re.search(r"\.name:\s+mlf_user_rows", notes)
    vs = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)]
    ss = [int(x) for x in re.findall(r"\.sgpr_spill_count:\s+(\d+)", notes)]
    assert vs and ss and max(vs) == 0 and max(ss) == 0, notes
    assert [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)] == [0]
    # LDS is dynamic only (sized by the launch from d): nothing static
    assert [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)] == [0]


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-objdump of ROCm not found")
def test_no_fma_is_formed(tmp_path):
    """-ffp-contract=off reaches hiprtc: the Rosenbrock model's code has no fused multiply-add (what makes the bitwise
    agreement with the built-in kernels possible)."""
    path = os.path.join(str(tmp_path), "r.co")
    with open(path, "wb") as fh:
        fh.write(usermodels.rosenbrock(7).code)
    asm = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", path], capture_output=True, text=True, check=True).stdout
    assert "v_mul_f64" in asm and "v_add_f64" in asm
    assert "v_fma_f64" not in asm and "v_fmac_f64" not in asm


def test_shape_checked_before_any_library_call(monkeypatch):
    m = usermodels.rosenbrock(7)

    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)
    with pytest.raises(ValueError):
        m.loglike(np.zeros((4, 6)))
    with pytest.raises(ValueError):
        m.transform(np.zeros(7))


def test_no_cpu_fallback_without_device():
    from ultranest_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    m = usermodels.rosenbrock(7)
    x = np.full((3, 7), 0.5)
    with pytest.raises(_lib.HipLibraryError):
        m.loglike(x)
    with pytest.raises(_lib.HipLibraryError):
        m.transform(x)


# ---- routing ---------------------------------------------------------------------------------------------------------

def _cpu_region(calls, monkeypatch, d=7):
    from ultranest_amd import regions
    from ultranest_amd.regions import DeviceRNG, MLFriends

    def refill(self, region, use_scan, method, nsamples, Lmin, tspec, lspec):
        calls.append(("refill", method, nsamples, Lmin, tspec, lspec))
        return np.zeros((1, d)), np.zeros((1, d)), np.zeros(1), 1

    def refill_user(self, region, use_scan, method, nsamples, Lmin, model, with_transform):
        calls.append(("refill_user", method, nsamples, Lmin, model, with_transform))
        return np.zeros((1, d)), np.zeros((1, d)), np.zeros(1), 1

    monkeypatch.setattr(regions._DeviceState, "refill", refill)
    monkeypatch.setattr(regions._DeviceState, "refill_user", refill_user)
    region = MLFriends.__new__(MLFriends)
    region.device_rng = DeviceRNG(11)
    region._dev = regions._DeviceState()
    region.current_sampling_method = region.sample_from_boundingbox
    return region


def test_region_refill_routing(monkeypatch):
    from ultranest_amd import likelihoods as lk
    calls = []
    region = _cpu_region(calls, monkeypatch)
    m = usermodels.rosenbrock(7)
    other = usermodels.funnel(7)
    assert region.refill(100, -1.0, m.transform, m.loglike) is not None
    assert calls[-1] == ("refill_user", 0, 100, -1.0, m, True)
    region.refill(100, -2.0, lk.identity_transform, m.loglike)
    assert calls[-1] == ("refill_user", 0, 100, -2.0, m, False)
    n = len(calls)
    # a user likelihood with a built-in non-identity transform, a numpy transform or another model's transform; a built-in
    # likelihood with a user transform: host callbacks
    assert region.refill(100, -1.0, lk.rosenbrock_transform, m.loglike) is None
    assert region.refill(100, -1.0, lambda x: x * 20 - 10, m.loglike) is None
    assert region.refill(100, -1.0, other.transform, m.loglike) is None
    assert region.refill(100, -1.0, m.transform, lk.rosenbrock_loglike) is None
    assert region.refill(100, -1.0, m.loglike, m.transform) is None
    assert len(calls) == n
    # built-in pairs: the existing call, the same arguments as before
    region.refill(100, -3.0, lk.rosenbrock_transform, lk.rosenbrock_loglike)
    assert calls[-1] == ("refill", 0, 100, -3.0, lk.rosenbrock_transform.device_spec, lk.rosenbrock_loglike.device_spec)
    region.current_sampling_method = region.sample_from_wrapping_ellipsoid
    region.refill(50, -3.0, lk.identity_transform, lk.eggbox2_loglike)
    assert calls[-1] == ("refill", 1, 50, -3.0, lk.identity_transform.device_spec, lk.eggbox2_loglike.device_spec)
    region.refill(50, -3.0, m.transform, m.loglike)
    assert calls[-1] == ("refill_user", 1, 50, -3.0, m, True)
    region.device_rng = None
    assert region.refill(50, -3.0, m.transform, m.loglike) is None


class _FakeWalkers(object):
    """Stands in for popstepsampler._Walkers: records the entry points the sampler reaches."""
    calls = []

    def __init__(self, popsize, nsteps, ndim):
        self.popsize, self.nsteps, self.ndim, self.nparams = popsize, nsteps, ndim, None

    def _rec(self):
        return dict(found=False, nc=1, nsuccess=0, nmovable=0, ring=0, rounds=1, L=0.0, left=0.0, right=0.0,
                    u=np.zeros(self.ndim), p=np.zeros(self.ndim))

    def begin(self, Lmin):
        return np.zeros(self.popsize, dtype=np.int64), np.zeros(self.popsize, dtype=np.uint8)

    def propose(self, unif=None, rng=None, fetch=True):
        self.calls.append(("propose", fetch))
        return np.empty((0, self.ndim)) if fetch else None

    def finish(self, Lmin, pnew, Lnew, ringindex):
        self.calls.append(("finish", Lmin, ringindex))
        return self._rec()

    def finish_dev(self, Lmin, tspec, lspec, ringindex):
        self.calls.append(("finish_dev", Lmin, tspec, lspec, ringindex))
        return self._rec()

    def finish_user(self, Lmin, model, with_transform, ringindex):
        self.calls.append(("finish_user", Lmin, model, with_transform, ringindex))
        return self._rec()

    def step_dev(self, Lmin, scale, kind, dirscale, rng, tspec, lspec, graph=True):
        self.calls.append(("step_dev", Lmin, kind, tspec, lspec, graph))
        return self._rec()

    def step_user(self, Lmin, scale, kind, dirscale, rng, model, with_transform):
        self.calls.append(("step_user", Lmin, kind, model, with_transform))
        return self._rec()

    def rounds_dev(self, Lmin, scale, kind, dirscale, rng, tspec, lspec, max_rounds):
        self.calls.append(("rounds_dev", Lmin, kind, tspec, lspec, max_rounds))
        return self._rec(), np.zeros((1, 5))

    def __getattr__(self, name):     # set_layer, set_direction_data, set_live, update_live, ...
        return lambda *a, **k: None


def _sampler_call(monkeypatch, transform, loglike, device_rng=None, max_rounds=None, use_graph=None, d=7):
    import ultranest_amd.popstepsampler as pop
    monkeypatch.setattr(pop, "_Walkers", _FakeWalkers)
    _FakeWalkers.calls = []
    s = pop.PopulationSliceSampler(popsize=32, nsteps=6, generate_direction=pop.generate_mixture_random_direction,
                                   device_rng=device_rng)
    if max_rounds is not None:
        s.max_rounds = max_rounds
    if use_graph is not None:
        s.use_graph = use_graph
    u = np.full((40, d), 0.5)
    region = types.SimpleNamespace(u=u, maxradiussq=None,
                                   transformLayer=types.SimpleNamespace(ctr=np.zeros(d), T=np.eye(d), axes=np.eye(d)))
    np.random.seed(1)
    s.__next__(region, -1.0, u, np.zeros(40), transform, loglike)
    return [c for c in _FakeWalkers.calls if c[0] != "propose"]


def test_population_sampler_routing(monkeypatch):
    from ultranest_amd import likelihoods as lk
    from ultranest_amd.regions import DeviceRNG
    m = usermodels.rosenbrock(7)
    # host-RNG mode
    assert _sampler_call(monkeypatch, m.transform, m.loglike) == [("finish_user", -1.0, m, True, 0)]
    assert _sampler_call(monkeypatch, lk.identity_transform, m.loglike) == [("finish_user", -1.0, m, False, 0)]
    assert _sampler_call(monkeypatch, lk.rosenbrock_transform, m.loglike) == [("finish", -1.0, 0)]
    assert _sampler_call(monkeypatch, lambda x: x, m.loglike) == [("finish", -1.0, 0)]
    assert _sampler_call(monkeypatch, m.transform, lk.rosenbrock_loglike) == [("finish", -1.0, 0)]
    assert _sampler_call(monkeypatch, lk.rosenbrock_transform, lk.rosenbrock_loglike) == [
        ("finish_dev", -1.0, lk.rosenbrock_transform.device_spec, lk.rosenbrock_loglike.device_spec, 0)]
    # Philox mode: the user model takes the per-step route whatever max_rounds / use_graph say
    kind = 6
    for max_rounds, graph in [(256, True), (1, False), (1, True)]:
        got = _sampler_call(monkeypatch, m.transform, m.loglike, DeviceRNG(5), max_rounds, graph)
        assert got == [("step_user", -1.0, kind, m, True)], got
    assert _sampler_call(monkeypatch, lk.identity_transform, m.loglike, DeviceRNG(5)) == [("step_user", -1.0, kind, m, False)]
    assert _sampler_call(monkeypatch, lk.rosenbrock_transform, m.loglike, DeviceRNG(5)) == [("finish", -1.0, 0)]
    ts, ls = lk.rosenbrock_transform.device_spec, lk.rosenbrock_loglike.device_spec
    assert _sampler_call(monkeypatch, lk.rosenbrock_transform, lk.rosenbrock_loglike, DeviceRNG(5)) == [
        ("rounds_dev", -1.0, kind, ts, ls, 256)]
    assert _sampler_call(monkeypatch, lk.rosenbrock_transform, lk.rosenbrock_loglike, DeviceRNG(5), 1, True) == [
        ("step_dev", -1.0, kind, ts, ls, True)]
    assert _sampler_call(monkeypatch, lk.rosenbrock_transform, lk.rosenbrock_loglike, DeviceRNG(5), 1, False) == [
        ("step_dev", -1.0, kind, ts, ls, False)]
