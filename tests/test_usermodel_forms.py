"""The forms of a user-model program in one place (devicemodel.Form in Python, the variant table of csrc/mlf_user.hip, the table in
include/mlfriends_hip.h), CPU side: every Form a DeviceModel can produce maps to the header's variant number, has a cache key of its
own and compiles to the one kernel the header's table names; what is no form is refused; and every exported compile and create
entry accepts exactly the variants the header's table gives it (checked from outside, over the numbers -1 .. 10)."""
import ctypes
import os
import re

import pytest

import test_devicemodel_compile as C     # (llvm-readelf of ROCm and the notes reader)
from ultranest_amd import _lib
from ultranest_amd import devicemodel as dm
from ultranest_amd import usermodels

HEADER_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mlfriends_hip.h")
MLF_E_BADARG = 1

# one source that defines the functions of every form: default, one sum, several sums (any M: the terms function writes t[0..3)),
# the transform and the derived columns
MAIN = (usermodels.GAUSS_LOGLIKE % 0.1 + usermodels.LINEAR_TERM % 65 + usermodels.SUMMED_LOGLIKE % dict(name="mlf_linear_term")
        + usermodels.AMPLITUDE_TERMS % 65 + usermodels.MULTISUM_LOGLIKE % dict(name="mlf_amplitude") + "\n" + usermodels.AFFINE_TRANSFORM)
SOURCE = MAIN + "\n" + usermodels.GAUSS_DERIVED

SUMS = [(False, None), (True, None), (True, 1), (True, 3), (True, 8)]
FORMS = ([dm.Form(tr, gated, summed, nsums) for tr in (False, True) for gated in (False, True) for summed, nsums in SUMS]
         + [dm.Form(False, derived="derive")]
         + [dm.Form(tr, True, summed, nsums, "gate") for tr in (False, True) for summed, nsums in SUMS])


def _header_table():
    """{variant name: (number, kernel, compile entry, create entry)} from the header's table and its #defines"""
    with open(HEADER_H) as fh:
        text = fh.read()
    numbers = {name: int(value) for name, value in re.findall(r"^#define MLF_USERMODEL_(\w+) (\d+)$", text, re.M) if name != "MAX_SUMS"}
    rows = re.findall(r"^ \*   MLF_USERMODEL_(\w+)\s+(mlf_user\w+)\s+(compile_\w+)\s+(create_\w+)$", text, re.M)
    assert sorted(r[0] for r in rows) == sorted(numbers) and sorted(numbers.values()) == list(range(10))
    return {name: (numbers[name], kernel, "mlf_usermodel_" + comp, "mlf_usermodel_" + create) for name, kernel, comp, create in rows}


def _name(form):
    """the header's name of a form's variant, spelled from the form's facts"""
    if form.derived == "derive":
        return "DERIVED"
    parts = (["SUMS"] if form.nsums is not None else ["SUM"] if form.summed else []) + (["TREGION"] if form.gated else [])
    return "_".join(parts + (["DERIVED"] if form.derived == "gate" else [])) or "DEFAULT"


def test_the_forms_a_model_can_produce():
    assert len(FORMS) == len(set(FORMS)) == 2 * 2 * 5 + 1 + 2 * 5
    table = _header_table()
    for form in FORMS:
        assert form.variant == table[_name(form)][0] == getattr(dm, "VARIANT_" + _name(form)), form
    assert {f.variant for f in FORMS} == set(range(10))
    assert len({dm._cache_key(SOURCE, f) for f in FORMS}) == len(FORMS)
    # a model asks for these and no others
    m = dm.DeviceModel(3, MAIN, aux=usermodels.linear_aux(3, 65), nterms=65, nsums=3, nderived=3,
                       derived_source=usermodels.GAUSS_DERIVED, gate_derived=True)
    assert m._form(False, True) == dm.Form(False, True, True, 3) and m._form(False, True, "gate") == dm.Form(False, True, True, 3, "gate")
    assert m._form(False, False, "derive") == dm.Form(False, derived="derive") == dm.DERIVE
    assert dm.Form(1, 0, 1, 3) == dm.Form(True, False, True, 3) and hash(dm.Form(1, 0, 1, 3)) == hash(dm.Form(True, False, True, 3))


@pytest.mark.skipif(C.LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
def test_every_form_compiles_to_the_one_kernel_the_header_names(tmp_path):
    table = _header_table()
    for k, form in enumerate(FORMS):
        code = dm.compile_form(SOURCE, form)
        assert code[:4] == b"\x7fELF" and dm._code_cache[dm._cache_key(SOURCE, form)] is code
        assert re.findall(r"\.name:\s+(\w+)", C._notes(code, tmp_path, "form%d" % k)) == [table[_name(form)][1]], form
    # the public compile functions are these forms
    assert dm.compile_model(SOURCE, True, True, True, 3) is dm.compile_form(SOURCE, dm.Form(True, True, True, 3))
    assert dm.compile_derived(SOURCE) is dm.compile_form(SOURCE, dm.DERIVE)
    assert dm.compile_gate_derived(SOURCE, True, True, 3) is dm.compile_form(SOURCE, dm.Form(True, True, True, 3, "gate"))


def test_what_is_no_form_is_refused(monkeypatch):
    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)
    for bad in (dict(nsums=3), dict(gated=True, nsums=1), dict(summed=True, nsums=0), dict(summed=True, nsums=9),
                dict(summed=True, nsums=True), dict(summed=True, nsums=2.0)):
        with pytest.raises(ValueError, match="nsums"):
            dm.Form(True, **bad)
    for bad in (dict(derived="gate"), dict(summed=True, nsums=3, derived="gate")):
        with pytest.raises(ValueError, match="gated=True"):
            dm.Form(True, **bad)
    for bad in (dict(derived="derive"), dict(derived=True), dict(derived="q")):
        with pytest.raises(ValueError, match="derived"):
            dm.Form(True, **bad)
    for bad in (dict(gated=True), dict(summed=True)):
        with pytest.raises(ValueError, match="derived"):
            dm.Form(False, derived="derive", **bad)
    with pytest.raises(ValueError, match="nsums"):
        dm.compile_model(SOURCE, True, nsums=3)
    with pytest.raises(ValueError, match="nsums"):
        dm.compile_gate_derived(SOURCE, True, nsums=3)
    with pytest.raises(ValueError, match="nsums"):
        dm._Handle(b"", 3, True, (), nsums=3)


# ---- the owner columns, from outside -------------------------------------------------------------------------------------------

def _compile_calls(L):
    """{entry: call(variant, nsums)}: a size query with otherwise valid arguments"""
    src, inc = SOURCE.encode(), dm.INCLUDE_DIR.encode()
    size = ctypes.c_size_t(0)
    log = ctypes.create_string_buffer(256)
    tail = (None, 0, ctypes.byref(size), log, 256)
    return {"mlf_usermodel_compile_variant": lambda v, nsums: L.mlf_usermodel_compile_variant(src, inc, 1, v, *tail),
            "mlf_usermodel_compile_sums": lambda v, nsums: L.mlf_usermodel_compile_sums(src, inc, 1, v, nsums or 3, *tail),
            "mlf_usermodel_compile_gate_derived": lambda v, nsums: L.mlf_usermodel_compile_gate_derived(src, inc, 1, v, nsums, *tail)}


def test_each_compile_entry_takes_exactly_its_variants():
    L = _lib.lib()
    table = _header_table()
    owner = {number: comp for number, kernel, comp, create in table.values()}
    multi = {table[name][0] for name in table if name.startswith("SUMS")}
    assert set(owner.values()) == set(_compile_calls(L))
    for entry, call in _compile_calls(L).items():
        for v in range(-1, 11):
            rc = call(v, 3 if v in multi else 0)
            if owner.get(v) == entry:
                assert rc == 0, (entry, v, L.mlf_last_error())
            else:
                assert rc == MLF_E_BADARG and b"variant" in L.mlf_last_error(), (entry, v)
                if v in owner:      # the message names the entry that takes it
                    assert owner[v].encode() in L.mlf_last_error(), (entry, v)
    assert L.mlf_usermodel_compile(SOURCE.encode(), dm.INCLUDE_DIR.encode(), 1, None, 0, ctypes.byref(ctypes.c_size_t(0)), None, 0) == 0


def test_each_create_entry_refuses_every_variant_but_its_own():
    """(a create call of an owned variant needs the GPU: the GPU tests make those)"""
    L = _lib.lib()
    table = _header_table()
    owner = {number: create for number, kernel, comp, create in table.values()}
    summed = {table[name][0] for name in table if name.startswith("SUM")}
    code = dm.compile_form(SOURCE, dm.Form(True))
    aux = usermodels.linear_aux(3, 65)
    h = ctypes.c_void_p(1)
    head, tail = (code, len(code), 3, 1), (_lib.ptr(aux), len(aux), ctypes.byref(h))
    calls = {"mlf_usermodel_create_variant": lambda v: L.mlf_usermodel_create_variant(*head, v, *tail),
             "mlf_usermodel_create_sum": lambda v: L.mlf_usermodel_create_sum(*head, v, 65, *tail),
             "mlf_usermodel_create_gate_derived": lambda v: L.mlf_usermodel_create_gate_derived(*head, v, 65 if v in summed else 0, 3,
                                                                                                *tail)}
    assert set(owner.values()) == set(calls) | {"mlf_usermodel_create_derived"}      # (which takes no variant number)
    for entry, call in calls.items():
        for v in range(-1, 11):
            if owner.get(v) == entry:
                continue
            h.value = 1
            assert call(v) == MLF_E_BADARG and b"variant" in L.mlf_last_error() and not h.value, (entry, v)
            if v in owner:
                assert owner[v].encode() in L.mlf_last_error(), (entry, v)
