"""Run-time priors (``priors.Ref``, ``priors.Tabulated``), CPU side with the compiler: hiprtc compiles every Ref-capable
family, tables of 2 and of 4096 knots and a mixed model for gfx950 without a GPU (default, gated and summed programs), the
wrapper kernel keeps no spills, no stack and no LDS, a transform at the knot cap compiles, lists of constant priors keep the
source text they had before Ref and Tabulated existed (tests/golden/g18_prior_sources.json), the new header's text appears
exactly when it is needed, and the header keeps the user-model contract."""
import hashlib
import json
import os
import re
import sys
import time

import numpy as np
import pytest

import prior_reference as PR
import prior_rt_reference as RT
from ultranest_amd import devicemodel as dm
from ultranest_amd import priors as P
from ultranest_amd.priors import Ref
from test_devicemodel_compile import LLVM_BIN, _notes, _symbols
from test_priors_compile import GAUSS, SUMMED, _is_gfx950_object

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARK = "MLF_PRIORS_RT_DEV_HPP"


def mixed_rt_priors():
    """12 columns mixing constants, Refs (one of them to a Tabulated column, one to a block column) and tables.  The truncated
    normal reads mu / 10: with mu itself, 30 sigma from the window, there is no probability between the bounds in binary64
    and the column is NaN by the run-time contract"""
    return [P.Normal(0.0, 10.0, name="mu"), P.LogUniform(0.01, 10.0, name="tau"), P.Normal(Ref("mu"), Ref("tau"), name="theta"),
            P.Tabulated([0.5, 1.0, 1.0, 3.0], [0.0, 0.25, 0.5, 1.0], name="tab"), P.Exponential(Ref("tab"), name="rate"),
            P.Uniform(Ref("late", offset=-20.0), Ref("tab", scale=2.0, offset=1.0), name="between"),
            P.TruncatedNormal(Ref("mu", scale=0.1), Ref("tau", scale=2.0, offset=0.1), -3.0, 4.0, name="late"),
            P.OrderedUniform(1.0, 2.0, 2, name="o"), P.Triangular(0.0, Ref("o_0"), Ref("o_1", offset=1.0)),
            RT.make_table(1025, 2, "steps"), P.StudentT(4.0, Ref("theta"), Ref("tau"))]


def ref_family_lists():
    """{name: list}: every Ref-capable family with all its Ref parameters read from Fixed parents (first setting)"""
    out = {}
    for name, params in sorted(RT.REF_FAMILIES.items()):
        out[name] = RT.ref_list(name, params(PR.family(name)[0]))
    for name, settings in sorted(RT.SPECIAL_REF_FAMILIES.items()):
        lead, args = settings[0]
        out[name] = RT.ref_list(name, args, lead)
    return out


def _no_spills_no_stack(code, tmp_path, tag):
    notes = _notes(code, tmp_path, tag)
    assert re.search(r"\.name:\s+mlf_user_rows", notes)
    vs = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)]
    ss = [int(x) for x in re.findall(r"\.sgpr_spill_count:\s+(\d+)", notes)]
    assert vs and ss and max(vs) == 0 and max(ss) == 0, notes
    assert [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)] == [0]
    assert [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)] == [0]


def _every_form(priors, tmp_path, tag):
    pt = P.PriorTransform(priors)
    d = pt.ndim
    m = pt.model(GAUSS, aux=np.zeros(d))
    _is_gfx950_object(m.code)
    gated = dm.compile_model(m.source, True, gated=True)
    s = pt.model(SUMMED, aux=np.zeros(2 * d), nterms=2 * d)
    assert "mlf_user_rows" in _symbols(m.code) and "mlf_user_rows_tregion" in _symbols(gated)
    assert "mlf_user_rows_sum" in _symbols(s.code)
    if LLVM_BIN is not None:
        for form, code in (("default", m.code), ("gated", gated), ("summed", s.code)):
            _no_spills_no_stack(code, tmp_path, "%s_%s" % (tag, form))
    return pt


@pytest.mark.parametrize("name", sorted(ref_family_lists()))
def test_every_ref_capable_family_compiles_in_every_form(name, tmp_path):
    pt = _every_form(ref_family_lists()[name], tmp_path, name)
    assert MARK in pt.source and pt.parents[-1] == tuple(range(pt.ndim - 1))


@pytest.mark.parametrize("n", [2, 4096])
def test_a_table_compiles_in_every_form(n, tmp_path):
    pt = _every_form([RT.make_table(n, 1), P.Normal(0.0, 1.0)], tmp_path, "table%d" % n)
    assert "static __device__ const double mlf_prior_tab0[%d] = {" % (3 * n - 1) in pt.source


def test_the_mixed_list_compiles_in_every_form(tmp_path):
    pt = _every_form(mixed_rt_priors(), tmp_path, "mixed")
    assert pt.ndim == 12 and pt.parents[5] == (3, 6) and pt.parents[9] == (7, 8)
    assert [pt.paramnames[k] for k in (3, 7, 8)] == ["tab", "o_0", "o_1"]


def test_a_transform_at_the_knot_cap_compiles():
    pt = P.PriorTransform([RT.make_table(4096, seed) for seed in range(4)])
    assert sum(p.n for p in pt.priors) == P.MAX_TABLE_KNOTS
    t0 = time.perf_counter()
    m = pt.model(P.CONSTANT_LOGLIKE)
    dt = time.perf_counter() - t0
    _is_gfx950_object(m.code)
    print("MEASURED compile of 4 x 4096 knots: %.2f s, source %d bytes, code object %d bytes" % (dt, len(pt.source), len(m.code)))


def test_lists_of_constant_priors_keep_their_source_text():
    sys.path.insert(0, GOLDEN)
    try:
        import make_prior_sources
    finally:
        sys.path.remove(GOLDEN)
    with open(os.path.join(GOLDEN, "g18_prior_sources.json")) as fh:
        want = json.load(fh)
    lists = make_prior_sources.lists()
    assert set(lists) == set(want) and len(want) == 24
    for name, priors in sorted(lists.items()):
        src = P.PriorTransform(priors).source
        assert hashlib.sha256(src.encode()).hexdigest() == want[name], name
        assert MARK not in src


def test_the_new_header_appears_exactly_when_it_is_needed():
    rt = P.rt_header_text()
    const = [P.Normal(0.0, 1.0), P.Uniform(0.0, 1.0)]
    assert rt not in P.PriorTransform(const).source
    with_ref = P.PriorTransform(const + [P.Normal(Ref(0), 1.0)]).source
    with_tab = P.PriorTransform(const + [P.Tabulated([0.0, 1.0], [0.0, 1.0])]).source
    assert with_ref.startswith(P.header_text() + rt) and with_tab.startswith(P.header_text() + rt)
    assert with_ref.count(rt) == 1 and "static" not in with_ref.split(rt)[1]
    both = P.PriorTransform(const + [P.Gamma(2.0, Ref(1, scale=0.5, offset=3.0)), RT.make_table(5, 1)]).source
    assert both.startswith(P.header_text() + P.special_header_text() + rt) and both.count("mlf_prior_tab3[14]") == 1


def test_source_is_deterministic_and_sensitive_to_the_last_bit():
    a, b = P.PriorTransform(mixed_rt_priors()), P.PriorTransform(mixed_rt_priors())
    assert a.source == b.source
    body = a.source[a.source.index(MARK + "\n\nstatic"):]
    assert not re.search(r"(?<![\w.+-])\d+\.\d+(?![\w.])", body)          # every constant a hexadecimal literal
    pri = mixed_rt_priors()
    pri[6] = P.TruncatedNormal(Ref("mu", scale=0.1), Ref("tau", scale=np.nextafter(2.0, 3.0), offset=0.1), -3.0, 4.0, name="late")
    c = P.PriorTransform(pri)
    assert c.source != a.source and len(c.source) == len(a.source)
    pri = mixed_rt_priors()
    x = pri[3].x.copy()
    x[-1] = np.nextafter(x[-1], 4.0)
    pri[3] = P.Tabulated(x, pri[3].cdf, name="tab")
    e = P.PriorTransform(pri)
    assert e.source != a.source and len(e.source) == len(a.source)
    ma = a.model(GAUSS, aux=np.zeros(12))
    before = dm.compile_calls
    assert b.model(GAUSS, aux=np.ones(12)).code == ma.code and dm.compile_calls == before
    c.model(GAUSS, aux=np.zeros(12))
    assert dm.compile_calls == before + 1


def test_header_keeps_the_user_model_contract():
    text = P.rt_header_text()
    code = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("//"))
    assert "asm" not in code and "__builtin" not in code and "#include" not in code
    leaves = re.findall(r"__device__ __noinline__ double (mlf_prior_\w+)\(", code)
    assert leaves == ["mlf_prior_rt_uniform", "mlf_prior_rt_loguniform", "mlf_prior_rt_truncnormal", "mlf_prior_rt_triangular",
                      "mlf_prior_table"]
    inl = re.findall(r"__device__ __forceinline__ double (mlf_prior_\w+)\(", code)
    assert inl == ["mlf_prior_rt_loc", "mlf_prior_rt_scale", "mlf_prior_rt_pos"] and code.count("__device__") == 8
    # leaf functions: none of them names another mlf_prior_ function
    for body in re.split(r"__device__ __noinline__", code)[1:]:
        assert len(re.findall(r"mlf_prior_\w+\(", body.split("\n}\n")[0])) == 1
    # the two earlier headers are what they were
    assert len(re.findall(r"__device__ __noinline__ double mlf_prior_\w+\(", P.header_text())) == 20


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
def test_the_table_lies_in_read_only_data(tmp_path):
    import subprocess
    m = P.PriorTransform([RT.make_table(1024, 1)]).model(P.CONSTANT_LOGLIKE)
    path = os.path.join(str(tmp_path), "tab.co")
    with open(path, "wb") as fh:
        fh.write(m.code)
    out = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "-S", "-W", path], capture_output=True, text=True, check=True).stdout
    ro = re.search(r"\.rodata\s+PROGBITS\s+\w+\s+\w+\s+(\w+)", out)
    assert ro and int(ro.group(1), 16) >= 8 * (3 * 1024 - 1), out


def test_routing_takes_the_device_route():
    from ultranest_amd import likelihoods as lk
    pt = P.PriorTransform(mixed_rt_priors())
    m = pt.model(GAUSS, aux=np.zeros(12))
    assert dm.device_route(m.transform, m.loglike) == (m, True)
    assert dm.device_route(lk.identity_transform, m.loglike) == (m, False)
    assert dm.device_route(pt.transform, lambda p: -0.5 * (p ** 2).sum(axis=1)) is None
