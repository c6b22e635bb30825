"""The t-region gate over a user model's derived parameters (DeviceModel(..., nderived=Q, gate_derived=True): the gated programs
compiled with -DMLF_USER_GATE_DERIVED=1 from the model's source followed by its derived source), CPU side: hiprtc compiles the
three programs for gfx950 without a GPU -- one kernel each, no spills, no private segment; the keys of every existing program
are what they were, with and without the flag; the choice between the staged and the direct form and its LDS size; the argument
checks; which entry point a region refill takes (device entry points replaced by recorders); the header and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest

import test_derived_model_compile as DC   # (the restated key recipe of the existing programs)
import test_devicemodel_compile as C     # (its metadata reader)
import test_tregion_routing as R         # (the recording region and a host-built t-region)
from ultranest_amd import devicemodel as dm
from ultranest_amd import usermodels

HEADER_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mlfriends_hip.h")

# nonlinear derived columns: with them the covariance over [p | q] is not singular (those of gauss_derived are linear in p)
NONLINEAR_DERIVED = r"""
__device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux) {
  q[0] = p[0] * p[1];
  if (nq > 1) q[1] = p[d - 1] * p[d - 1];
  if (nq > 2) q[2] = exp(p[0] * 0.125);
}
"""


def _default(d=5, nq=3, flag=True):
    return dm.DeviceModel(d, usermodels.GAUSS_LOGLIKE % 0.1, usermodels.AFFINE_TRANSFORM, aux=usermodels.gauss_centers(d),
                          nderived=nq, derived_source=NONLINEAR_DERIVED, gate_derived=flag)


def _summed(d=4, K=130, flag=True):
    """integer-valued terms (usermodels.staircase_sum): every summation order gives the same bits"""
    source = usermodels.STAIRCASE_TERM % K + usermodels.SUMMED_LOGLIKE % dict(name="mlf_staircase_term")
    return dm.DeviceModel(d, source, usermodels.AFFINE_TRANSFORM, aux=usermodels.staircase_data(d, K, affine=True), nterms=K,
                          nderived=2, derived_source=NONLINEAR_DERIVED, gate_derived=flag)


def _multisum(d=4, K=130, flag=True):
    source = usermodels.STAIRCASE3_TERMS % K + usermodels.MULTISUM_LOGLIKE % dict(name="mlf_staircase3")
    return dm.DeviceModel(d, source, usermodels.AFFINE_TRANSFORM, aux=usermodels.staircase_data(d, K, affine=True), nterms=K,
                          nsums=3, nderived=2, derived_source=NONLINEAR_DERIVED, gate_derived=flag)


CASES = {"default": (_default, "mlf_user_rows_tregion_derived", 15), "summed": (_summed, "mlf_user_rows_sum_tregion_derived", 16),
         "multisum": (_multisum, "mlf_user_rows_sums_tregion_derived", 16)}


# ---- the programs ------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(C.LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("which", sorted(CASES))
@pytest.mark.parametrize("with_transform", [True, False])
def test_gate_derived_program_is_one_kernel_without_spills(which, with_transform, tmp_path):
    make, entry, nargs = CASES[which]
    m = make()
    assert m.source == make(flag=False).source and m.code is make(flag=False).code       # the flag changes no existing program
    code = m.compile_gate_derived(with_transform)
    assert code[:4] == b"\x7fELF" and code != m.code and code != m.derive_code and code != m._compile(with_transform, True)
    assert m.compile_gate_derived(with_transform) is code                              # from the cache
    notes = C._notes(code, tmp_path, "gd_%s%d" % (which, with_transform))
    assert re.findall(r"\.name:\s+(\w+)", notes) == [entry]
    assert len(re.findall(r"\.value_kind:\s+(?:global_buffer|by_value)", notes)) == nargs
    for field in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        assert [int(x) for x in re.findall(r"\.%s:\s+(\d+)" % field, notes)] == [0], field


@pytest.mark.skipif(C.LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
def test_the_direct_form_is_the_same_program_without_spills(tmp_path):
    """one program serves both forms (picked from d, nq and the p buffer at run time): checked at the boundary pair as well"""
    for d in BOUNDARY:
        notes = C._notes(_default(d, 3).compile_gate_derived(True), tmp_path, "gd_direct%d" % d)
        assert re.findall(r"\.name:\s+(\w+)", notes) == ["mlf_user_rows_tregion_derived"]
        for field in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert [int(x) for x in re.findall(r"\.%s:\s+(\d+)" % field, notes)] == [0], field


def test_a_source_without_the_derived_function_fails_at_the_first_gated_use():
    m = dm.DeviceModel(3, usermodels.ROSENBROCK_LOGLIKE, usermodels.ROSENBROCK_TRANSFORM, nderived=1,
                       derived_source=NONLINEAR_DERIVED, gate_derived=True)
    with pytest.raises(dm.DeviceModelCompileError) as ei:
        dm.compile_gate_derived(m.source + "\n// nothing here\n", True)
    assert "mlf_user_derived" in ei.value.log


# ---- cache keys --------------------------------------------------------------------------------------------------------------

def _gate_derived_key(source, has_transform, summed=False, nsums=None):
    return dm._cache_key(source, dm.Form(has_transform, True, summed, nsums, derived="gate"))


def test_existing_cache_keys_are_what_they_were_with_and_without_the_flag():
    keys = set()
    for flag in (False, True):
        for m in (_default(flag=flag), _summed(flag=flag), _multisum(flag=flag)):
            for tr in (False, True):
                for gated in (False, True):
                    for summed in (False, True):
                        assert dm._cache_key(m.source, tr, gated, summed) == DC._parents_key(m.source, tr, gated, summed)
                        keys.add(dm._cache_key(m.source, tr, gated, summed))
                    for nsums in (1, 3, 8):
                        assert dm._cache_key(m.source, tr, gated, True, nsums=nsums) == DC._parents_key(m.source, tr, gated, True, nsums)
                        keys.add(dm._cache_key(m.source, tr, gated, True, nsums=nsums))
            full = m.source + "\n" + NONLINEAR_DERIVED
            assert dm._code_cache[dm._cache_key(m.source, True, False, m.summed, nsums=m.nsums)] is m.code
            assert dm._code_cache[DC._derive_key(full)] is m.derive_code
    assert len(keys) == 3 * 2 * 2 * 5
    # the new programs have keys of their own, over the source they are compiled from
    new = set()
    for m in (_default(), _summed(), _multisum()):
        full = m.source + "\n" + NONLINEAR_DERIVED
        for tr in (False, True):
            k = _gate_derived_key(full, tr, m.summed, m.nsums)
            assert k not in keys and k != DC._derive_key(full) and k != DC._parents_key(full, tr, True, m.summed, m.nsums)
            assert k != _gate_derived_key(m.source, tr, m.summed, m.nsums)
            new.add(k)
        assert dm._code_cache[_gate_derived_key(full, True, m.summed, m.nsums)] is m.compile_gate_derived(True)
    assert len(new) == 6


def test_the_flag_compiles_nothing_until_the_first_gated_use():
    def make(flag):      # (a source of its own: the cache is keyed by the source, not by the model)
        return dm.DeviceModel(7, usermodels.GAUSS_LOGLIKE % 0.375, usermodels.AFFINE_TRANSFORM, aux=usermodels.gauss_centers(7),
                              nderived=2, derived_source=NONLINEAR_DERIVED, gate_derived=flag)

    make(False)
    n = dm.compile_calls
    m = make(True)
    assert dm.compile_calls == n and m.gate_derived is True and make(False).gate_derived is False
    m.compile_gate_derived(True)
    assert dm.compile_calls == n + 1
    m.compile_gate_derived(True)
    assert dm.compile_calls == n + 1


# ---- argument checks ---------------------------------------------------------------------------------------------------------

def test_the_flag_needs_nderived(monkeypatch):
    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)
    with pytest.raises(ValueError, match="gate_derived"):
        dm.DeviceModel(3, usermodels.ROSENBROCK_LOGLIKE, gate_derived=True)
    with pytest.raises(ValueError, match="gate_derived"):
        dm.DeviceModel(3, usermodels.ROSENBROCK_LOGLIKE, usermodels.ROSENBROCK_TRANSFORM, gate_derived=True)


def test_handle_arguments(monkeypatch):
    m = _default()
    with pytest.raises(ValueError, match="gated=True"):
        m.handle(True, derived=True)
    with pytest.raises(ValueError, match="nderived"):
        usermodels.gauss(5).compile_gate_derived()
    made = []

    class H(object):
        def __init__(self, code, ndim, has_transform, aux, gated=False, nterms=None, nsums=None, derived=None, nderived=None):
            assert (gated, derived) == (True, "gate")
            made.append((code, ndim, has_transform, nderived, nterms, nsums))
            self.handle = 200 + len(made)

        def close(self):
            pass

    monkeypatch.setattr(dm, "_Handle", H)
    a = m.handle(True, gated=True, derived=True)
    assert m.handle(True, gated=True, derived=True) == a and made == [(m.compile_gate_derived(True), 5, True, 3, None, None)]
    s = _multisum()
    s.handle(True, gated=True, derived=True)
    assert made[-1] == (s.compile_gate_derived(True), 4, True, 2, 130, 3)
    m._handles = {}
    s._handles = {}


def test_library_entry_points_check_their_arguments():
    from ultranest_amd import _lib
    L = _lib.lib()
    m = _default()
    size = ctypes.c_size_t(0)
    log = ctypes.create_string_buffer(256)
    full = (m.source + "\n" + NONLINEAR_DERIVED).encode()
    inc = dm.INCLUDE_DIR.encode()
    code = m.compile_gate_derived(True)
    assert L.mlf_usermodel_compile_gate_derived(full, inc, 1, 7, 0, None, 0, ctypes.byref(size), log, 256) == 0
    assert size.value == len(code)
    for variant, nsums in [(1, 0), (6, 0), (10, 0), (7, 3), (8, 1), (9, 0), (9, 9)]:
        assert L.mlf_usermodel_compile_gate_derived(full, inc, 1, variant, nsums, None, 0, ctypes.byref(size), log, 256) == 1
    for variant in (7, 8, 9):        # the other compile entries do not take the new variants
        assert L.mlf_usermodel_compile_variant(full, inc, 1, variant, None, 0, ctypes.byref(size), log, 256) == 1
        assert L.mlf_usermodel_compile_sums(full, inc, 1, variant, 3, None, 0, ctypes.byref(size), log, 256) == 1
    h = ctypes.c_void_p()
    aux = m.aux
    create = L.mlf_usermodel_create_gate_derived
    assert create(code, len(code), 5, 1, 7, 0, 0, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1              # no derived column
    assert create(code, len(code), 5, 1, 7, 4, 3, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1              # terms without a sum
    assert create(code, len(code), 5, 1, 8, 0, 3, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1              # a sum without terms
    assert create(code, len(code), 5, 1, 1, 0, 3, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1              # another variant
    assert create(code, len(code), 0, 1, 7, 0, 3, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert create(code, len(code), 1000, 1, 7, 0, 25, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 2          # MLF_E_DIM
    assert create(b"not a code object" * 8, 136, 5, 1, 7, 0, 3, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert create(code, len(code), 5, 1, 7, 0, 3, None, 4, ctypes.byref(h)) == 1
    assert L.mlf_usermodel_create_variant(code, len(code), 5, 1, 7, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert L.mlf_usermodel_create_sum(code, len(code), 5, 1, 8, 4, _lib.ptr(aux), len(aux), ctypes.byref(h)) == 1
    assert not h.value
    assert L.mlf_region_set_tregion_wide(None, 5, None, None, None, 1.0) == 1
    assert L.mlf_region_refill_user_derived_gated(None, 1, 0, 0, 0, 0.0, None, None, None, None, None, 0, None, None, None) == 1


# ---- the choice of form ------------------------------------------------------------------------------------------------------

# mlf_user_rows_gate_derived_lds_bytes(d, nq, p buffer) = 64 * ((p buffer ? 2 : 1) * (d | 1) + (nq | 1)) * 8 where that is at most
# MLF_USER_ROWS_LDS_BUDGET = 65536, i.e. 2 * (d | 1) + (nq | 1) <= 128 with a p buffer.  At nq = 3: 2 * (d | 1) <= 125, d | 1 <= 61
# (odd), so d = 61 is the largest staged dimensionality (2 * 61 + 3 = 125 units of 512 bytes) and d = 62 (2 * 63 + 3 = 129) the
# first direct one.
BOUNDARY = (61, 62)


def _lds(d, nq, p_buffer=True):
    return dm._lib.lib().mlf_usermodel_gate_derived_lds_bytes(d, nq, int(p_buffer))


def test_lds_bytes_either_side_of_the_budget():
    assert _lds(61, 3) == 64 * (2 * 61 + 3) * 8 == 64000 <= 65536
    assert _lds(62, 3) == 0 and 64 * (2 * 63 + 3) * 8 > 65536
    for d, nq, p_buffer in [(2, 1, True), (5, 3, True), (5, 2, True), (4, 2, False), (50, 3, True), (60, 3, True), (61, 3, True),
                            (61, 4, True), (61, 5, True), (61, 6, True), (62, 3, True), (62, 1, True), (123, 3, False),
                            (124, 3, False), (125, 3, False), (1, 125, True), (1, 126, True), (1000, 24, True)]:
        want = 64 * ((2 if p_buffer else 1) * (d | 1) + (nq | 1)) * 8
        assert _lds(d, nq, p_buffer) == (want if want <= 65536 else 0), (d, nq, p_buffer)
        # odd pitches: lane l's 8-byte word of a row sits on banks 2 P l mod 64, distinct over each half of the wave
        for pitch in (d | 1, nq | 1):
            assert len({(2 * pitch * lane) % 64 for lane in range(32)}) == 32
    assert _lds(0, 3) == 0 and _lds(5, 0) == 0 and _lds(2000, 3) == 0


# ---- routing -----------------------------------------------------------------------------------------------------------------

def _recording_region(calls, monkeypatch, d):
    from ultranest_amd import regions
    region = DC._recording_region(calls, monkeypatch, R._cpu_region, d)

    def refill_user_derived_gated(self, region, use_scan, method, nsamples, Lmin, model, tregion):
        calls.append(("refill_user_derived_gated", method, nsamples, Lmin, model, tregion))
        return np.zeros((1, d)), np.zeros((1, model.nparams)), np.zeros(1), 1

    monkeypatch.setattr(regions._DeviceState, "refill_user_derived_gated", refill_user_derived_gated)
    return region


def test_region_refill_takes_the_gated_derived_entry_only_for_the_flag_and_the_wide_tregion(monkeypatch):
    from ultranest_amd import likelihoods as lk
    calls = []
    d, Q = R.D, 3
    region = _recording_region(calls, monkeypatch, d)
    m, plain = _default(d, Q), _default(d, Q, flag=False)
    wide, narrow = R._tregion(d=d + Q), R._tregion(d=d)
    got = region.refill(100, -1.0, m.transform, m.loglike, tregion=wide)
    assert calls == [("refill_user_derived_gated", 0, 100, -1.0, m, wide)] and got[1].shape == (1, d + Q) and got[0].shape == (1, d)
    # the flag with a tregion over the parameters alone, or over another number of columns: the host sequence
    assert region.refill(100, -1.0, m.transform, m.loglike, tregion=narrow) is None
    assert region.refill(100, -1.0, m.transform, m.loglike, tregion=R._tregion(d=d + Q + 1)) is None
    # no flag: the host sequence for either width, as before
    for t in (wide, narrow):
        assert region.refill(100, -1.0, plain.transform, plain.loglike, tregion=t) is None
    assert len(calls) == 1
    # the flag and no tregion: the derived entry, as before
    got = region.refill(100, -2.0, m.transform, m.loglike)
    assert calls[-1] == ("refill_user_derived", 0, 100, -2.0, m) and got[1].shape == (1, d + Q)
    # paired with identity_transform the rows carry no derived columns: the plain gated entry over d columns
    region.refill(100, -3.0, lk.identity_transform, m.loglike, tregion=narrow)
    assert calls[-1] == ("refill_user", 0, 100, -3.0, m, False, dict(tregion=narrow))
    assert region.refill(100, -3.0, lk.identity_transform, m.loglike, tregion=wide) is None
    # a constant derived column is a fixed dimension of the tregion
    fixed = R._tregion(d=d + Q, fixed_last=True)
    assert fixed.variable_dims is not Ellipsis
    region.refill(100, -4.0, m.transform, m.loglike, tregion=fixed)
    assert calls[-1] == ("refill_user_derived_gated", 0, 100, -4.0, m, fixed)


def test_the_device_copy_of_a_wide_tregion_is_told_its_width():
    from ultranest_amd import regions
    d, Q = R.D, 3

    class Handle(R._Handle):
        def set_tregion(self, A, ctr, fixed, enlarge, **kw):
            R._Handle.set_tregion(self, A, ctr, fixed, enlarge)
            self.calls[-1] += (kw,)

    state, h = regions._DeviceState(), Handle()
    t = R._tregion(d=d + Q, fixed_last=True)
    state.sync_tregion(h, t, d + Q, wide=True)
    kind, A, ctr, fixed, enlarge, kw = h.calls[-1]
    assert kind == "set" and kw == dict(width=d + Q) and A.shape == (d + Q, d + Q) and ctr.shape == (d + Q,)
    assert fixed[-1] == 0.25 and np.isnan(fixed[:-1]).all()
    state.sync_tregion(h, t, d + Q, wide=True)
    assert len(h.calls) == 1
    t.update_center(np.append(t.ellipsoid_center + 0.5, 0.25))
    state.sync_tregion(h, t, d + Q, wide=True)
    assert h.calls[-1][0] == "center" and h.calls[-1][1].shape == (d + Q,)
    # a tregion over the region's own columns keeps today's positional call
    state.sync_tregion(h, R._tregion(d=d), d)
    assert h.calls[-1][0] == "set" and h.calls[-1][-1] == {}


# ---- header and binding ------------------------------------------------------------------------------------------------------

def test_header_declares_the_new_entries_and_the_abi_versions_agree():
    from ultranest_amd import _lib
    with open(HEADER_H) as fh:
        text = fh.read()
    for name in ("mlf_usermodel_compile_gate_derived", "mlf_usermodel_create_gate_derived", "mlf_usermodel_gate_derived_lds_bytes",
                 "mlf_region_set_tregion_wide", "mlf_region_refill_user_derived_gated"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    for name, value in (("TREGION_DERIVED", 7), ("SUM_TREGION_DERIVED", 8), ("SUMS_TREGION_DERIVED", 9)):
        assert re.search(r"^#define MLF_USERMODEL_%s %d$" % (name, value), text, re.M)
        assert getattr(dm, "VARIANT_" + name) == value
    version = int(re.search(r"^#define MLF_ABI_VERSION (\d+)$", text, re.M).group(1))
    assert version == _lib.ABI_VERSION == _lib.lib().mlf_abi_version()
