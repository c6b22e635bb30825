"""The covariance form of a user model (DeviceModel(..., ncov=n)), CPU side: hiprtc compiles its programs for gfx950 without a GPU;
each holds the one kernel the header names with its documented parameters, workgroup size and static LDS, no spills and no private
segment; what is no covariance model is refused before any library call; the keys of every other form are what they were; and
every route recognises the model (the recorders of test_devicemodel_compile.py)."""
import hashlib
import re

import numpy as np
import pytest

import test_devicemodel_compile as C
from ultranest_amd import _lib
from ultranest_amd import devicemodel as dm
from ultranest_amd import hotstart, usermodels

NMAX = dm.max_ncov(4, True)


def test_the_cap():
    assert dm.max_ncov(4, False) == dm.max_ncov(4, True) == 199 and dm.max_ncov(1024, True) < dm.max_ncov(1024, False) < 199
    L = _lib.lib()
    for n in (1, 2, 63, 64, 65, 128, NMAX, NMAX + 1):
        assert dm.cov_lds_bytes(n) == L.mlf_covmodel_lds_bytes(n) and dm.cov_lds_bytes(n) % 16 == 0
        # the layout: the packed augmented triangle, the column vector, one word of flags
        assert dm.cov_lds_bytes(n) >= 8 * ((n + 1) * (n + 2) // 2 + n + 1 + 1) > dm.cov_lds_bytes(n) - 16
    for ndim, tr in ((4, True), (4, False), (500, True), (1024, False)):
        n = dm.max_ncov(ndim, tr)
        rows = (2 if tr else 1) * ndim * 8
        assert dm.cov_lds_bytes(n) + rows <= 163840 < dm.cov_lds_bytes(n + 1) + rows
    assert L.mlf_covmodel_lds_bytes(0) == 0 and L.mlf_covmodel_lds_bytes(-3) == 0


@pytest.mark.skipif(C.LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("n", [1, 65, NMAX])
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("transform", [False, True])
def test_programs(n, gated, transform, tmp_path):
    source = usermodels.GP_SQEXP % n + usermodels.GP_COV_LOGLIKE + "\n" + usermodels.GP_TRANSFORM
    code = dm.compile_form(source, dm.Form(transform, gated, ncov=n))
    assert code[:4] == b"\x7fELF"
    notes = C._notes(code, tmp_path, "cov%d%d%d" % (n, gated, transform))
    assert re.findall(r"\.name:\s+(\w+)", notes) == ["mlf_user_rows_cov_tregion" if gated else "mlf_user_rows_cov"]
    explicit = re.findall(r"\.value_kind:\s+(global_buffer|by_value)\b", notes)
    assert len(explicit) == (14 if gated else 9), explicit
    assert [int(x) for x in re.findall(r"\.max_flat_workgroup_size:\s+(\d+)", notes)] == [256]
    assert [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)] == [0]
    assert [int(x) for x in re.findall(r"\.sgpr_spill_count:\s+(\d+)", notes)] == [0]
    assert [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)] == [0]
    assert [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)] == [_lib.lib().mlf_covmodel_lds_bytes(n)]


def test_the_library_refuses_what_is_no_program():
    import ctypes
    L = _lib.lib()
    src = (usermodels.GP_SQEXP % 8 + usermodels.GP_COV_LOGLIKE).encode()
    size = ctypes.c_size_t(0)
    for ncov in (0, -1, 200, 5000):
        assert L.mlf_covmodel_compile(src, dm.INCLUDE_DIR.encode(), 0, 0, ncov, None, 0, ctypes.byref(size), None, 0) == 1
        assert b"ncov" in L.mlf_last_error()
    h = ctypes.c_void_p(1)
    code = dm.compile_form(src.decode(), dm.Form(False, ncov=8))
    assert L.mlf_covmodel_create(code, len(code), 4, 0, 0, 200, None, 0, ctypes.byref(h)) == 1 and not h.value
    # a covariance program is no numbered variant
    assert dm.Form(False, ncov=8).variant not in range(10) and dm.Form(False, True, ncov=8).variant not in range(10)
    assert dm.Form(False, ncov=8).variant != dm.Form(False, True, ncov=8).variant


def test_what_is_no_covariance_model_is_refused_before_any_library_call(monkeypatch):
    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)
    src = usermodels.GP_SQEXP % 8 + usermodels.GP_COV_LOGLIKE
    for bad in (dict(nterms=8), dict(nterms=8, nsums=2)):
        with pytest.raises(ValueError, match="ncov"):
            dm.DeviceModel(4, src, ncov=8, **bad)
    with pytest.raises(ValueError):
        dm.DeviceModel(4, src, ncov=8, nsums=2)
    for bad in (8.0, "8", True, 0, -1):
        with pytest.raises(ValueError, match="ncov"):
            dm.DeviceModel(4, src, ncov=bad)
    for ndim, tr, n in ((4, None, NMAX + 1), (4, usermodels.GP_TRANSFORM, NMAX + 1), (1024, usermodels.GP_TRANSFORM, dm.max_ncov(1024, True) + 1)):
        with pytest.raises(ValueError, match="max_ncov"):
            dm.DeviceModel(ndim, src, tr, ncov=n)
    with pytest.raises(ValueError, match="gate_derived"):
        dm.DeviceModel(4, src, ncov=8, nderived=3, derived_source=usermodels.GAUSS_DERIVED, gate_derived=True)
    for bad in (dict(summed=True), dict(summed=True, nsums=2), dict(gated=True, derived="gate")):
        with pytest.raises(ValueError, match="ncov"):
            dm.Form(True, ncov=8, **bad)
    with pytest.raises(ValueError, match="ncov"):
        dm._Handle(b"", 4, True, (), nterms=5, ncov=8)
    with pytest.raises(ValueError, match="ndata"):
        usermodels.gp_sqexp_twin(13)


def test_hotstart_device_forms_refuse_a_covariance_model():
    m = usermodels.gp_sqexp(8, affine=True)
    rs = np.random.RandomState(1)
    up = rs.uniform(0.3, 0.7, size=(50, 4))
    with pytest.raises(ValueError, match="host callbacks"):
        hotstart.get_auxiliary_contbox_parameterization(["a", "l", "s", "m"], m.loglike, m.transform, up, np.full(50, 1 / 50.))
    with pytest.raises(ValueError, match="host callbacks"):
        hotstart.get_extended_auxiliary_independent_problem(m.loglike, m.transform, np.full(4, 0.5), np.full(4, 0.05), df=2)


def _old_key(source, has_transform, tags, gated):
    """the cache key as it was before Form had ncov"""
    header = b""
    for path in (dm.HEADER, dm.GATE_HEADER) if gated else (dm.HEADER,):
        with open(path, "rb") as fh:
            header += fh.read()
    h = hashlib.sha256()
    for part in (source.encode(), b"\0", (repr((dm.COMPILE_OPTIONS, has_transform)) + tags).encode(), b"\0", header):
        h.update(part)
    return h.hexdigest()


def test_keys_of_the_other_forms_are_what_they_were():
    src = "// any source\n"
    cases = [(dm.Form(False), ""), (dm.Form(True), ""), (dm.Form(True, True), " tregion"), (dm.Form(True, summed=True), " sum"),
             (dm.Form(False, True, True), " tregion sum"), (dm.Form(True, False, True, 3), " sum sums=3"),
             (dm.Form(True, True, True, 8), " tregion sum sums=8"), (dm.DERIVE, " derived"),
             (dm.Form(True, True, derived="gate"), " tregion gate_derived"),
             (dm.Form(True, True, True, 2, "gate"), " tregion gate_derived sum sums=2")]
    for form, tags in cases:
        assert form.ncov is None and form.tags == tags
        assert dm._cache_key(src, form) == _old_key(src, form.has_transform, tags, form.gated), form
    # positional uses stay valid and a form without ncov equals the five-field form it was
    assert dm.Form(True, False, True, 3) == (True, False, True, 3, None, None)
    # a covariance form: its own tag, its own header instead of mlf_user_rows.hpp
    a, b = dm.Form(True, ncov=8), dm.Form(True, ncov=9)
    assert a.tags == " cov=8" and dm.Form(True, True, ncov=8).tags == " tregion cov=8"
    keys = {dm._cache_key(src, f) for f in (a, b, dm.Form(False, ncov=8), dm.Form(True, True, ncov=8), dm.Form(True))}
    assert len(keys) == 5
    assert dm._cache_key(src, a) != _old_key(src, True, " cov=8", False)      # (mlf_user_rows.hpp is not what it hashes)
    # the models of the other forms ask for the forms they asked for
    m = usermodels.linear_sum(3, 65)
    assert m.ncov is None and m._form(False, True) == dm.Form(False, True, True)
    g = usermodels.gp_sqexp(8)
    assert g.ncov == 8 and g._form(False, True) == dm.Form(False, True, ncov=8) and not g.summed and g.nsums is None


def test_prior_library_passes_ncov():
    from ultranest_amd import priors
    pt = priors.PriorTransform([priors.Uniform(-1, 1, name="lna"), priors.Uniform(-1, 2, name="lnl"), priors.Uniform(-2, 0, name="lns"),
                                priors.Normal(0, 1, name="mean")])
    x, y = usermodels.gp_data(8)
    m = pt.model(usermodels.GP_SQEXP % 8 + usermodels.GP_COV_LOGLIKE, aux=np.concatenate([x, y]), ncov=8)
    assert m.ncov == 8 and m.has_transform and "mlf_user_rows_cov" in C._symbols(m.code)


# ---- routing -----------------------------------------------------------------------------------------------------------------------

def test_every_route_recognises_the_model(monkeypatch):
    from ultranest_amd import likelihoods as lk
    from ultranest_amd.regions import DeviceRNG
    m = usermodels.gp_sqexp(8, affine=True)
    assert dm.device_route(m.transform, m.loglike) == (m, True) and dm.device_route(lk.identity_transform, m.loglike) == (m, False)
    calls = []
    region = C._cpu_region(calls, monkeypatch, d=4)
    assert region.refill(100, -1.0, m.transform, m.loglike) is not None
    assert calls[-1] == ("refill_user", 0, 100, -1.0, m, True)
    region.refill(100, -2.0, lk.identity_transform, m.loglike)
    assert calls[-1] == ("refill_user", 0, 100, -2.0, m, False)
    assert C._sampler_call(monkeypatch, m.transform, m.loglike, d=4) == [("finish_user", -1.0, m, True, 0)]
    assert C._sampler_call(monkeypatch, m.transform, m.loglike, DeviceRNG(5), d=4) == [("step_user", -1.0, 6, m, True)]
    assert C._sampler_call(monkeypatch, lk.identity_transform, m.loglike, DeviceRNG(5), d=4) == [("step_user", -1.0, 6, m, False)]


def test_no_cpu_fallback_without_device():
    if _lib.device_count() > 0:      # (with a GPU the calls succeed: test_cov_model_gpu.py)
        return
    m = usermodels.gp_sqexp(8)
    with pytest.raises(_lib.HipLibraryError):
        m.loglike(np.zeros((2, 4)))
    with pytest.raises(_lib.HipLibraryError):
        m.cov_factor(np.zeros((2, 4)))
