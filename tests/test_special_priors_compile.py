"""The iterative prior families (ultranest_amd.priors: Gamma, ChiSquared, InverseGamma, Beta, StudentT, Dirichlet), CPU side:
hiprtc compiles each of them and the Dirichlet block for gfx950 without a GPU (default, gated and summed programs), the
wrapper kernel of a mixed model keeps its registers and needs no stack, a wide model compiles to calls, the closed-form header
and every closed-form source text are unchanged, and the argument checks, properties and routing."""
import os
import re
import subprocess

import numpy as np
import pytest

import special_prior_reference as SR
from ultranest_amd import devicemodel as dm
from ultranest_amd import priors as P
from test_devicemodel_compile import LLVM_BIN, _notes, _symbols
from test_priors_compile import GAUSS, SUMMED, _is_gfx950_object, mixed_priors

TRANSFORM_HEAD = "\n__device__ void mlf_user_transform("


def special_mixed():
    """9 columns: every new device function beside closed-form families and a Dirichlet block"""
    return [P.Gamma(2.5, 3.0, name="rate"), P.Normal(0.0, 2.0), P.ChiSquared(5.0), P.InverseGamma(3.0, 2.0, name="var"),
            P.Beta(2.0, 3.0, name="frac"), P.Uniform(-1.0, 1.0, circular=True), P.StudentT(5.0, 1.0, 0.5, name="loc"),
            P.Dirichlet([0.5, 2.0], name="w")]


FAMILY_MODELS = {
    "Gamma": lambda: [P.Gamma(0.1, 1.0), P.Gamma(2.5, 3.0), P.Gamma(1000.0, 0.01)],
    "ChiSquared": lambda: [P.ChiSquared(0.2), P.ChiSquared(5.0), P.ChiSquared(2000.0)],
    "InverseGamma": lambda: [P.InverseGamma(0.1, 1.0), P.InverseGamma(3.0, 2.0), P.InverseGamma(1000.0, 5.0)],
    "Beta": lambda: [P.Beta(0.1, 0.1), P.Beta(2.5, 40.0), P.Beta(1000.0, 1000.0)],
    "StudentT": lambda: [P.StudentT(1.0), P.StudentT(2.5, -3.0, 0.5), P.StudentT(1000.0)],
    "Dirichlet1": lambda: [P.Dirichlet(SR.dirichlet_alpha(1))],
    "Dirichlet5": lambda: [P.Dirichlet(SR.dirichlet_alpha(5))],
    "Dirichlet64": lambda: [P.Dirichlet(SR.dirichlet_alpha(64))],
}


@pytest.mark.parametrize("name", sorted(FAMILY_MODELS))
def test_every_family_compiles_in_every_form(name):
    pt = P.PriorTransform(FAMILY_MODELS[name]())
    d = pt.ndim
    m = pt.model(GAUSS, aux=np.zeros(d))
    _is_gfx950_object(m.code)
    assert "mlf_user_rows" in _symbols(m.code)
    assert "mlf_user_rows_tregion" in _symbols(dm.compile_model(m.source, True, gated=True))
    s = pt.model(SUMMED, aux=np.zeros(2 * d), nterms=2 * d)
    assert "mlf_user_rows_sum" in _symbols(s.code)
    assert "mlf_user_rows_sum_tregion" in _symbols(dm.compile_model(s.source, True, gated=True, summed=True))
    # straight-line code and no table
    assert "[]" not in pt.source.split("mlf_user_transform")[1] and "static" not in pt.source


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("gated", [False, True])
def test_wrapper_kernel_of_a_mixed_model_has_no_register_spills_and_no_stack(gated, tmp_path):
    """the method of test_priors_compile.py: the iterative quantile functions are leaf functions too (their shared pieces are
    inlined), so the kernel needs no stack; no table and no indexed local array, so no scratch"""
    m = P.PriorTransform(special_mixed()).model(GAUSS, aux=np.zeros(9))
    code = dm.compile_model(m.source, True, gated=True) if gated else m.code
    notes = _notes(code, tmp_path, "special%d" % gated)
    assert re.search(r"\.name:\s+mlf_user_rows", notes)
    vs = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)]
    ss = [int(x) for x in re.findall(r"\.sgpr_spill_count:\s+(\d+)", notes)]
    assert vs and ss and max(vs) == 0 and max(ss) == 0, notes
    assert [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)] == [0]
    assert [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)] == [0]


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-objdump of ROCm not found")
def test_a_wide_model_compiles_to_calls(tmp_path):
    """256 Gamma columns: 256 calls of one function, not 256 inlined copies of the iteration; the code object stays below
    8 times that of a 3-column model (the library's existing ratio)"""
    wide = P.PriorTransform([P.Gamma(0.5 + 0.1 * k, 1.0 + k) for k in range(256)]).model(P.CONSTANT_LOGLIKE)
    small = P.PriorTransform([P.Gamma(0.5 + 0.1 * k, 1.0 + k) for k in range(3)]).model(P.CONSTANT_LOGLIKE)
    _is_gfx950_object(wide.code)
    assert "mlf_prior_gamma" in "".join(_symbols(wide.code))
    path = os.path.join(str(tmp_path), "wide.co")
    with open(path, "wb") as fh:
        fh.write(wide.code)
    asm = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", path], capture_output=True, text=True, check=True).stdout
    assert asm.count("s_swappc_b64") >= 256
    assert len(wide.code) < 8 * len(small.code), (len(wide.code), len(small.code))


def test_closed_form_header_and_sources_are_unchanged():
    """header_text() is the closed-form header alone, and a list without an iterative family gives today's text: the header,
    then the body, nothing of the new header (so no cache key and no code object of an existing model moves)"""
    import hashlib
    text = P.header_text()
    assert hashlib.sha256(text.encode()).hexdigest() == "8dfd47566b5af6171b87f1a03d5921e97613d7f005b043e97b682ef5e74d7285"
    assert "mlf_priors_special" not in text and "MLF_PRIOR_SPECIAL" not in text
    pt = P.PriorTransform(mixed_priors())
    assert pt.source.startswith(text + TRANSFORM_HEAD)
    assert "special" not in pt.source.lower() and "mlf_psp_" not in pt.source and "mlf_prior_gamma" not in pt.source
    body = pt.source[len(text):]
    assert body.startswith(TRANSFORM_HEAD) and body.count("__device__") == 1
    sp = P.PriorTransform(special_mixed())
    assert sp.source.startswith(text + P.special_header_text() + TRANSFORM_HEAD)


def test_special_header_keeps_the_user_model_contract():
    text = P.special_header_text()
    code = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("//"))
    assert "asm" not in code and "__builtin" not in code and "#include" not in code
    assert "static" not in code and "[" not in code                 # no table, no array
    names = re.findall(r"__device__ __noinline__ double (mlf_prior_\w+)\(", code)
    assert names == ["mlf_prior_gamma", "mlf_prior_invgamma", "mlf_prior_beta", "mlf_prior_studentt"]
    helpers = re.findall(r"__device__ __forceinline__ \w+ (\w+)\(", code)
    assert code.count("__device__") == len(names) + len(helpers) and len(helpers) >= 5
    # leaf functions: no __noinline__ function is called from the header itself
    for n in names:
        assert len(re.findall(r"\b%s\(" % n, code)) == 1
    # every loop has a compile-time cap
    loops = re.findall(r"for \(([^)]*)\)", code)
    assert loops and all("MLF_PRIOR_SPECIAL_MAX_STEPS" in c or "MLF_PRIOR_SPECIAL_MAX_TERMS" in c for c in loops)
    assert "while" not in code and "goto" not in code


def test_source_text_is_deterministic_and_sensitive_to_the_last_bit():
    a = P.PriorTransform(special_mixed())
    b = P.PriorTransform(special_mixed())
    assert a.source == b.source
    head = P.header_text() + P.special_header_text()
    body = a.source[len(head):]
    assert not re.search(r"(?<![\w.+-])\d+\.\d+(?![\w.])", body)    # every constant is a hexadecimal floating literal
    pri = special_mixed()
    pri[0] = P.Gamma(np.nextafter(2.5, 3.0), 3.0, name="rate")
    c = P.PriorTransform(pri)
    assert c.source != a.source
    pri[0] = P.Gamma(2.5, np.nextafter(3.0, 4.0), name="rate")
    assert P.PriorTransform(pri).source not in (a.source, c.source)
    ma = a.model(GAUSS, aux=np.zeros(9))
    before = dm.compile_calls
    mb = b.model(GAUSS, aux=np.ones(9))
    assert dm.compile_calls == before and mb.code == ma.code        # the per-process code cache hits
    c.model(GAUSS, aux=np.zeros(9))
    assert dm.compile_calls == before + 1


NAN, INF = float("nan"), float("inf")
BAD = [
    lambda: P.Gamma(0.0999), lambda: P.Gamma(1000.5), lambda: P.Gamma(NAN), lambda: P.Gamma(INF), lambda: P.Gamma(-1.0),
    lambda: P.Gamma(2.0, 0.0), lambda: P.Gamma(2.0, -1.0), lambda: P.Gamma(2.0, INF), lambda: P.Gamma("a"),
    lambda: P.Gamma([1.0, 2.0]),
    lambda: P.ChiSquared(0.19), lambda: P.ChiSquared(2001.0), lambda: P.ChiSquared(NAN), lambda: P.ChiSquared([2.0, 3.0]),
    lambda: P.InverseGamma(0.05), lambda: P.InverseGamma(1e4), lambda: P.InverseGamma(2.0, 0.0), lambda: P.InverseGamma(NAN, 1.0),
    lambda: P.InverseGamma(2.0, NAN),
    lambda: P.Beta(0.05, 1.0), lambda: P.Beta(1.0, 0.05), lambda: P.Beta(1001.0, 1.0), lambda: P.Beta(1.0, 1001.0),
    lambda: P.Beta(NAN, 1.0), lambda: P.Beta(1.0, INF), lambda: P.Beta(0.0, 0.0), lambda: P.Beta([1.0], 2.0),
    lambda: P.StudentT(0.99), lambda: P.StudentT(1000.5), lambda: P.StudentT(NAN), lambda: P.StudentT(5.0, INF, 1.0),
    lambda: P.StudentT(5.0, 0.0, 0.0), lambda: P.StudentT(5.0, 0.0, -2.0), lambda: P.StudentT(5.0, 0.0, NAN),
    lambda: P.Dirichlet([]), lambda: P.Dirichlet(2.0), lambda: P.Dirichlet([[1.0, 2.0]]), lambda: P.Dirichlet([1.0, 0.05]),
    lambda: P.Dirichlet([1.0, 2000.0]), lambda: P.Dirichlet([1.0, NAN]), lambda: P.Dirichlet([1.0, "x"]),
    lambda: P.Dirichlet(np.ones(P.MAX_BLOCK + 1)),
    lambda: P.PriorTransform([P.Dirichlet(np.ones(P.MAX_BLOCK))] * (dm.MAX_DIM // P.MAX_BLOCK) + [P.Dirichlet([1.0, 1.0])]),
]


@pytest.mark.parametrize("k", range(len(BAD)))
def test_argument_checks_come_before_any_compile(k, monkeypatch):
    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)
    with pytest.raises(ValueError):
        BAD[k]()


def test_the_range_is_stated_in_the_error():
    for make, lo, hi in ((lambda: P.Gamma(0.01), "0.1", "1000"), (lambda: P.ChiSquared(0.1), "0.2", "2000"),
                         (lambda: P.Beta(0.01, 1.0), "0.1", "1000"), (lambda: P.StudentT(0.5), "1", "1000")):
        with pytest.raises(ValueError) as err:
            make()
        assert "[%s, %s]" % (lo, hi) in str(err.value)
    # the ends of every range are accepted
    P.Gamma(0.1), P.Gamma(1000.0), P.ChiSquared(0.2), P.ChiSquared(2000.0), P.InverseGamma(0.1), P.InverseGamma(1000.0)
    P.Beta(0.1, 1000.0), P.Beta(1000.0, 0.1), P.StudentT(1.0), P.StudentT(1000.0), P.Dirichlet([0.1, 1000.0])


def test_properties():
    pt = P.PriorTransform(special_mixed())
    assert pt.ndim == 9 and not pt.is_affine and pt.wrapped_dims == [5]
    assert pt.paramnames == ["rate", "p1", "p2", "var", "frac", "p5", "loc", "w_0", "w_1"]
    for one in (P.Gamma(2.0), P.ChiSquared(3.0), P.InverseGamma(2.0), P.Beta(2.0, 2.0), P.StudentT(4.0), P.Dirichlet([1.0, 1.0])):
        assert not P.PriorTransform([one]).is_affine and not P.PriorTransform([one, P.Uniform(0.0, 1.0)]).is_affine
    assert P.PriorTransform([P.Dirichlet([1.0] * 3)]).paramnames == ["p0_0", "p0_1", "p0_2"]
    assert P.Dirichlet(np.ones(P.MAX_BLOCK)).size == P.MAX_BLOCK
    c = P.ChiSquared(5.0)
    assert (c.shape, c.scale) == (2.5, 2.0) and c.call("u[0]") == P.Gamma(2.5, 2.0).call("u[0]")
    for name in ("Gamma", "ChiSquared", "InverseGamma", "Beta", "StudentT", "Dirichlet"):
        assert name in P.__all__


def test_routing_takes_the_device_route():
    from ultranest_amd import likelihoods as lk
    pt = P.PriorTransform(special_mixed())
    m = pt.model(GAUSS, aux=np.zeros(9))
    assert dm.device_route(m.transform, m.loglike) == (m, True)
    assert dm.device_route(lk.identity_transform, m.loglike) == (m, False)
    assert dm.device_route(pt.transform, lambda p: -0.5 * (p ** 2).sum(axis=1)) is None
