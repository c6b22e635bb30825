"""Warm start on the device (ultranest_amd/hotstart.py), CPU side with the compiler: hiprtc compiles forms (a) and (b) over
default, gated, ``nterms``, ``nsums = 3`` and ``nderived`` inner models at d = 1, 2, 50 for gfx950 without a GPU.  Every
program is one kernel without register spills; the inner model's cache keys are untouched; two sample sets at one d share one
code object; every ValueError comes before any compile; ``device_route`` recognises the new model.

Private segment.  The bound is the inner program's private segment plus 8 (d + 1) bytes (one array of d doubles).  Measured
(bytes; every inner program measured 0): at d = 1 and 2 every program 0 (the arrays live in registers).  At d = 50: over an
inner model WITHOUT a transform 0 in both forms (form (a) writes umod straight into the p row, form (b)'s p row is x itself);
over an inner model WITH a transform 408 in every main program of both forms, default, gated, nterms, nsums = 3 and nderived
(400 for the array, the compiler's 4-byte scavenging slot, an 8-byte frame alignment); every derive program 0.
"""
import re

import numpy as np
import pytest

from ultranest_amd import devicemodel as dm
from ultranest_amd import hotstart as hs
from ultranest_amd import likelihoods as lk
from ultranest_amd import usermodels as um
from test_devicemodel_compile import LLVM_BIN, _notes, _symbols
from test_priors_compile import _is_gfx950_object

DIMS = (1, 2, 50)
DERIVED1 = r"""
__device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux) {
  q[0] = p[0] * 2.0;
}
"""


def inner_model(kind, d):
    if kind == "default":
        return um.gauss(d, affine=True)
    if kind == "default_no_transform":
        return um.gauss(d)
    if kind == "nterms":
        return um.linear_sum(d, 100, affine=True)
    if kind == "nsums3":
        return um.amplitude_sum(d, 100, affine=True)
    if kind == "nderived":
        return dm.DeviceModel(d, um.GAUSS_LOGLIKE % 0.1, um.AFFINE_TRANSFORM, aux=um.gauss_centers(d), name="gauss_d1_%d" % d,
                              nderived=1, derived_source=DERIVED1)
    raise KeyError(kind)


def flat_samples(d, seed=1, n=400):
    rs = np.random.RandomState(seed)
    return np.clip(0.5 + 0.05 * rs.normal(size=(n, d)), 0.01, 0.99), np.full(n, 1.0 / n)


def contbox(model, seed=1):
    up, w = flat_samples(model.ndim, seed)
    names, L, T, vec = hs.get_auxiliary_contbox_parameterization(["x%d" % k for k in range(model.ndim)], model.loglike, model.transform, up, w)
    assert vec is True and len(names) == model.ndim + 1 and L.model.loglike is L and L.model.transform is T
    return L.model


def independent(model, df):
    d = model.ndim
    L, T = hs.get_extended_auxiliary_independent_problem(model.loglike, model.transform, np.full(d, 0.5), np.full(d, 0.05), df=df)
    return L.model


def programs(form, kind, d):
    """[(tag, code object, inner code object)] of one auxiliary model: its main program, its gated variant where asked, its
    derive program"""
    inner = inner_model("default" if kind == "gated" else kind, d)
    if form == "a":
        aux = contbox(inner)
    else:
        aux = independent(inner, 1 if form == "b_cauchy" else 4.5)
    if kind == "gated":
        code = dm.compile_model(aux.source, aux.has_transform, gated=True, summed=aux.summed, nsums=aux.nsums)
        return aux, [("gated", code, dm.compile_model(inner.source, True, gated=True))]
    out = [("main", aux.code, inner.code)]
    if aux.nderived is not None:
        out.append(("derive", aux.derive_code, inner.derive_code if inner.nderived is not None else inner.code))
    return aux, out


A_KINDS = ("default", "default_no_transform", "gated", "nterms", "nsums3", "nderived")
B_KINDS = ("default", "default_no_transform", "gated", "nderived")
CASES = [("a", k, d) for k in A_KINDS for d in DIMS] + [(f, k, d) for f in ("b_cauchy", "b_student") for k in B_KINDS for d in DIMS]


def _note_ints(notes, key):
    return [int(x) for x in re.findall(r"\.%s:\s+(\d+)" % key, notes)]


@pytest.mark.parametrize("form,kind,d", CASES)
def test_every_program_is_one_kernel_without_spills(form, kind, d, tmp_path):
    aux, progs = programs(form, kind, d)
    assert aux.ndim == (d + 1 if form == "a" else d)
    for tag, code, inner_code in progs:
        _is_gfx950_object(code)
        kernels = [s for s in _symbols(code) if s.endswith(".kd")]          # one kernel descriptor per kernel
        assert len(kernels) == 1, kernels
        if LLVM_BIN is None:
            continue
        notes = _notes(code, tmp_path, "%s_%s_%d_%s" % (form, kind, d, tag))
        assert len(re.findall(r"\.name:\s+mlf_user_\w+", notes)) == 1
        assert _note_ints(notes, "vgpr_spill_count") == [0] and _note_ints(notes, "sgpr_spill_count") == [0], notes


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("form,kind,d", CASES)
def test_private_segment_within_the_inner_programs_plus_one_array(form, kind, d, tmp_path):
    """Measured: module docstring (0 or 408 bytes at d = 50, 0 below)."""
    aux, progs = programs(form, kind, d)
    for tag, code, inner_code in progs:
        mine = _note_ints(_notes(code, tmp_path, "p_%s" % tag), "private_segment_fixed_size")
        inner = _note_ints(_notes(inner_code, tmp_path, "i_%s" % tag), "private_segment_fixed_size")
        print("MEASURED private segment %s %s d=%d %s: %d bytes (inner %d, bound %d)" % (form, kind, d, tag, mine[0], inner[0],
                                                                                        inner[0] + 8 * (d + 1)))
        assert len(mine) == 1 and mine[0] <= inner[0] + 8 * (d + 1), (form, kind, d, tag, mine, inner)


def test_the_inner_models_cache_keys_are_unchanged():
    inner = um.gauss(6, affine=True)          # (a dimension no other test of this file compiles)
    before = dm.compile_calls
    keys = set(dm._code_cache)
    assert dm._cache_key(inner.source, True) in keys
    aux = contbox(inner)
    assert dm.compile_calls == before + 1 and keys < set(dm._code_cache)
    assert dm._cache_key(inner.source, True) in dm._code_cache and um.gauss(6, affine=True).code == inner.code
    assert dm.compile_calls == before + 1            # the inner model again: still from the cache
    assert aux.source != inner.source and inner.source in aux.source          # the user's text is not edited
    assert aux.source.index("#define mlf_user_loglike mlf_hotstart_inner_loglike") < aux.source.index(inner.source)
    assert hs.header_text() in aux.source


def test_two_sample_sets_share_one_code_object():
    inner = um.gauss(4, affine=True)
    a = contbox(inner, seed=1)
    before = dm.compile_calls
    b = contbox(inner, seed=2)
    assert dm.compile_calls == before and a.source == b.source and a.code == b.code
    assert not np.array_equal(a.aux, b.aux) and np.array_equal(a.aux[:4], inner.aux)
    x = independent(inner, 4.5)
    before = dm.compile_calls
    L, T = hs.get_extended_auxiliary_independent_problem(inner.loglike, inner.transform, np.full(4, 0.4), np.full(4, 0.1), df=7.0)
    assert dm.compile_calls == before and L.model.code == x.code and L.model.logz_offset != x.logz_offset
    assert independent(inner, 1).code != x.code       # df = 1 is the closed Cauchy form: another text


def test_value_errors_come_before_any_compile():
    inner, summed = um.gauss(3, affine=True), um.linear_sum(3, 10)
    up, w = flat_samples(3)
    before = dm.compile_calls
    f, t = inner.loglike, inner.transform
    with pytest.raises(ValueError, match=r"get_auxiliary_contbox_parameterization.*get_extended_auxiliary_independent_problem"):
        hs.get_auxiliary_problem(f, t, np.full(3, 0.5), np.eye(3), 1.0)
    with pytest.raises(ValueError, match=r"get_auxiliary_contbox_parameterization.*get_extended_auxiliary_independent_problem"):
        hs.get_extended_auxiliary_problem(f, t, np.full(3, 0.5), np.eye(3), 1.0)
    with pytest.raises(ValueError, match="get_auxiliary_contbox_parameterization"):
        hs.get_extended_auxiliary_independent_problem(summed.loglike, summed.transform, np.full(3, 0.5), np.full(3, 0.1))
    with pytest.raises(ValueError, match="df"):
        hs.get_extended_auxiliary_independent_problem(f, t, np.full(3, 0.5), np.full(3, 0.1), df=2000)
    with pytest.raises(ValueError, match="df"):
        hs.get_extended_auxiliary_independent_problem(f, t, np.full(3, 0.5), np.full(3, 0.1), df=0.5)
    with pytest.raises(ValueError, match="positive"):
        hs.get_extended_auxiliary_independent_problem(f, t, np.full(3, 0.5), np.array([0.1, 0.0, 0.1]))
    with pytest.raises(ValueError, match="has 3 parameters"):
        hs.get_auxiliary_contbox_parameterization(["a"] * 2, f, t, up[:, :2], w)
    with pytest.raises(ValueError, match="strictly between 0 and 1"):
        hs.get_auxiliary_contbox_parameterization(["a"] * 3, f, t, up + 1.0, w)
    with pytest.raises(ValueError, match="more than 10 samples"):
        hs.get_auxiliary_contbox_parameterization(["a"] * 3, f, t, up[:5], w[:5])
    with pytest.raises(ValueError, match="weighted_samples"):
        hs.from_results(inner, {})
    assert dm.compile_calls == before
    aux = contbox(inner)
    before = dm.compile_calls
    with pytest.raises(ValueError, match="itself a warm-start model"):
        contbox(aux)
    assert dm.compile_calls == before


def test_device_route_recognises_the_new_model():
    inner = um.gauss(3, affine=True)
    for aux in (contbox(inner), independent(inner, 1)):
        assert dm.device_route(aux.transform, aux.loglike) == (aux, True)
        assert dm.device_route(lk.identity_transform, aux.loglike) == (aux, False)
        assert dm.device_route(inner.transform, aux.loglike) is None
    # the pair (identity_transform, inner likelihood) is a device pair too: the inner transform is then left out
    names, L, T, vec = hs.get_auxiliary_contbox_parameterization(["a"] * 3, inner.loglike, lk.identity_transform, *flat_samples(3))
    assert "mlf_hotstart_inner_transform(umod" not in L.model.source and "mlf_hotstart_inner_transform(umod" in contbox(inner).source


def test_region_refill_routes_with_and_without_a_tregion(monkeypatch):
    """form (a) goes to the user entry with and without a t-region; form (b) has derived columns and no gate_derived, so with
    a t-region its refill returns None (the host sequence) and without one it goes to the derived entry"""
    import test_derived_model_compile as DC
    import test_tregion_routing as R
    inner = um.gauss(R.D - 1, affine=True)
    calls = []
    region = DC._recording_region(calls, monkeypatch, R._cpu_region, R.D)
    a = contbox(inner)
    assert a.ndim == R.D and a.nderived is None
    t = R._tregion()
    region.refill(100, -1.0, a.transform, a.loglike)
    assert calls[-1][:6] == ("refill_user", 0, 100, -1.0, a, True) and not calls[-1][6].get("tregion")
    region.refill(100, -1.0, a.transform, a.loglike, tregion=t)
    assert calls[-1][:6] == ("refill_user", 0, 100, -1.0, a, True) and calls[-1][6]["tregion"] is t
    calls = []
    region = DC._recording_region(calls, monkeypatch, R._cpu_region, R.D)
    b = independent(um.gauss(R.D, affine=True), 1)
    assert not b.gate_derived
    for tr in (R._tregion(d=2 * R.D + 1), R._tregion()):
        assert region.refill(100, -1.0, b.transform, b.loglike, tregion=tr) is None
    assert not calls
    got = region.refill(100, -1.0, b.transform, b.loglike)
    assert calls == [("refill_user_derived", 0, 100, -1.0, b)] and got[1].shape == (1, 2 * R.D + 1)


def test_form_b_warns_when_it_drops_the_inner_models_derived_columns():
    inner = inner_model("nderived", 3)
    with pytest.warns(UserWarning, match="does not carry"):
        b = independent(inner, 1)
    assert b.nderived == 4
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        independent(um.gauss(3, affine=True), 1)
        assert contbox(inner).nderived == 1          # form (a) carries them: nothing to warn about


def test_summed_inner_models_become_nsums_models_and_derived_columns_carry_over():
    one, three, der = contbox(inner_model("nterms", 2)), contbox(inner_model("nsums3", 2)), contbox(inner_model("nderived", 2))
    assert (one.nterms, one.nsums) == (100, 1) and (three.nterms, three.nsums) == (100, 3)
    assert der.nderived == 1 and der.nparams == 4 and der.ndim == 3
    b = independent(inner_model("default", 2), 4.5)
    assert b.nderived == 3 and b.nparams == 5 and b.has_transform
    assert b.logz_offset == pytest.approx(2 * np.log(np.diff(__import__("scipy.stats").stats.t(4.5, 0.5, 0.05).cdf([0, 1]))[0]))


def test_from_results_builds_form_a():
    inner = um.gauss(2, affine=True)
    up, w = flat_samples(2)
    w2 = np.concatenate([w * 3.0, [0.0]])
    names, L, T, vec = hs.from_results(inner, {"weighted_samples": {"upoints": np.vstack([up, [[0.5, 0.5]]]), "weights": w2},
                                               "paramnames": ["a", "b"]})
    assert names == ["a", "b", "aux_logweight"] and np.allclose(L.model.aux, contbox(inner).aux, rtol=1e-12, atol=0)
    assert L.model.code == contbox(inner).code


def test_header_keeps_the_user_model_contract():
    text = hs.header_text()
    code = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("//"))
    assert "asm" not in code and "__builtin" not in code and "#include" not in code and "__noinline__" not in code
    assert code.count("__device__ __forceinline__") == code.count("__device__") == 7
