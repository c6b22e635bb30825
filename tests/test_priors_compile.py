"""Prior library (ultranest_amd.priors), CPU side: hiprtc compiles every family, both blocks and a mixed model for gfx950
without a GPU (default, gated and summed programs), the wrapper kernel keeps its registers, a wide model compiles, the source
text is a deterministic function of the parameter bits, and the argument checks, properties and routing."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import prior_reference as PR
from ultranest_amd import devicemodel as dm
from ultranest_amd import priors as P
from ultranest_amd import usermodels
from test_devicemodel_compile import LLVM_BIN, _notes, _symbols

GAUSS = usermodels.GAUSS_LOGLIKE % 0.5
SUMMED = r"""
__device__ double mlf_user_loglike_term(const double *p, int d, const double *aux, long long naux, long long k) {
  const double z = p[(int)(k % d)] - aux[k];
  return -0.5 * z * z;
}
"""


def mixed_priors():
    """12 columns: every kind of statement the generator writes (inline constant, call, both blocks)"""
    return [P.Uniform(-1.0, 1.0, circular=True, name="phase"), P.LogUniform(1e-3, 10.0, name="scale"), P.Normal(0.0, 2.0),
            P.TruncatedNormal(0.0, 1.0, -1.0, 2.0), P.Exponential(2.0), P.Sine(name="incl"), P.Fixed(0.25, name="pinned"),
            P.MultivariateNormal([0.0, 1.0], [[2.0, 0.5], [0.5, 1.0]], name="ab"), P.OrderedUniform(0.0, 1.0, 3, name="t")]


def _is_gfx950_object(code):
    assert code[:4] == b"\x7fELF" and code[4] == 2 and code[5] == 1
    e_machine, = struct.unpack_from("<H", code, 18)
    assert e_machine == 0xE0


@pytest.mark.parametrize("name", sorted(PR.FAMILIES))
def test_every_family_compiles(name):
    pt = P.PriorTransform(PR.family(name))
    assert pt.ndim == 3
    m = pt.model(GAUSS, aux=np.zeros(3))
    _is_gfx950_object(m.code)
    assert "mlf_user_rows" in _symbols(m.code)


@pytest.mark.parametrize("block", ["mvn1", "mvn8", "mvn64", "ordered1", "ordered5"])
def test_both_blocks_compile(block):
    if block.startswith("mvn"):
        n = int(block[3:])
        A = np.random.RandomState(n).normal(size=(n, n))
        cov = A.dot(A.T) + n * np.eye(n)
        prior = P.MultivariateNormal(np.arange(n), 0.5 * (cov + cov.T))
    else:
        n = int(block[7:])
        prior = P.OrderedUniform(-1.0, 3.0, n)
    pt = P.PriorTransform([prior])
    assert pt.ndim == n
    _is_gfx950_object(pt.model(GAUSS, aux=np.zeros(n)).code)
    # straight-line code: the factor matrix is in the instruction stream, not in a table
    assert "[]" not in pt.source.split("mlf_user_transform")[1] and "static" not in pt.source


def test_mixed_model_compiles_in_every_form():
    pt = P.PriorTransform(mixed_priors())
    assert pt.ndim == 12
    m = pt.model(GAUSS, aux=np.zeros(12))
    _is_gfx950_object(m.code)
    gated = dm.compile_model(m.source, True, gated=True)
    _is_gfx950_object(gated)
    assert "mlf_user_rows_tregion" in _symbols(gated)
    s = pt.model(SUMMED, aux=np.zeros(24), nterms=24)
    _is_gfx950_object(s.code)
    assert "mlf_user_rows_sum" in _symbols(s.code)
    sg = dm.compile_model(s.source, True, gated=True, summed=True)
    assert "mlf_user_rows_sum_tregion" in _symbols(sg)
    assert s.nterms == 24 and s.transform.device_spec.model is s


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("gated", [False, True])
def test_wrapper_kernel_of_the_mixed_model_has_no_register_spills(gated, tmp_path):
    """the method of test_devicemodel_compile.py::test_wrapper_kernel_has_no_register_spills.  The quantile functions are
    leaf functions (none of them calls another __noinline__ function), so the kernel needs no stack either."""
    m = P.PriorTransform(mixed_priors()).model(GAUSS, aux=np.zeros(12))
    code = dm.compile_model(m.source, True, gated=True) if gated else m.code
    notes = _notes(code, tmp_path, "mixed%d" % gated)
    assert re.search(r"\.name:\s+mlf_user_rows", notes)
    vs = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)]
    ss = [int(x) for x in re.findall(r"\.sgpr_spill_count:\s+(\d+)", notes)]
    assert vs and ss and max(vs) == 0 and max(ss) == 0, notes
    assert [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)] == [0]
    assert [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)] == [0]


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-objdump of ROCm not found")
def test_a_wide_model_compiles_to_calls(tmp_path):
    """256 Normal columns: 256 calls of one function, not 256 inlined copies of normcdfinv -- what __noinline__ is for.  The
    code object stays within a few times that of a 3-column model."""
    wide = P.PriorTransform([P.Normal(0.1 * k, 1.0 + k) for k in range(256)]).model(P.CONSTANT_LOGLIKE)
    small = P.PriorTransform([P.Normal(0.1 * k, 1.0 + k) for k in range(3)]).model(P.CONSTANT_LOGLIKE)
    _is_gfx950_object(wide.code)
    assert "mlf_prior_normal" in "".join(_symbols(wide.code))
    path = os.path.join(str(tmp_path), "wide.co")
    with open(path, "wb") as fh:
        fh.write(wide.code)
    asm = subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", path], capture_output=True, text=True, check=True).stdout
    assert asm.count("s_swappc_b64") >= 256
    assert len(wide.code) < 8 * len(small.code), (len(wide.code), len(small.code))


def test_source_text_is_deterministic_and_sensitive_to_the_last_bit():
    a = P.PriorTransform(mixed_priors())
    b = P.PriorTransform(mixed_priors())
    assert a.source == b.source
    assert a.source.startswith(P.header_text()) and "__device__ void mlf_user_transform(" in a.source
    # every constant is a hexadecimal floating literal: no decimal literal in the generated part
    body = a.source[len(P.header_text()):]
    assert not re.search(r"(?<![\w.+-])\d+\.\d+(?![\w.])", body) and "0x1.0000000000000p+1" in body
    pri = mixed_priors()
    pri[2] = P.Normal(0.0, np.nextafter(2.0, 3.0))
    c = P.PriorTransform(pri)
    assert c.source != a.source and len(c.source) == len(a.source)
    ma = a.model(GAUSS, aux=np.zeros(12))
    before = dm.compile_calls
    mb = b.model(GAUSS, aux=np.ones(12))
    assert dm.compile_calls == before and mb.code == ma.code        # the per-process code cache hits
    c.model(GAUSS, aux=np.zeros(12))
    assert dm.compile_calls == before + 1


def test_header_keeps_the_user_model_contract():
    text = P.header_text()
    code = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("//"))
    assert "asm" not in code and "__builtin" not in code and "#include" not in code
    n = len(re.findall(r"__device__ __noinline__ double mlf_prior_\w+\(", code))
    assert n == 20 and code.count("__device__") == n + 1          # one inlined helper, mlf_prior_z_leaf


BAD = [
    lambda: P.Fixed(float("nan")), lambda: P.Fixed(float("inf")),
    lambda: P.Uniform(1.0, 1.0), lambda: P.Uniform(2.0, 1.0), lambda: P.Uniform(0.0, float("inf")),
    lambda: P.Uniform(-1e308, 1e308),
    lambda: P.LogUniform(0.0, 1.0), lambda: P.LogUniform(-1.0, 1.0), lambda: P.LogUniform(2.0, 1.0),
    lambda: P.Normal(0.0, 0.0), lambda: P.Normal(0.0, -1.0), lambda: P.Normal(float("nan"), 1.0),
    lambda: P.Normal(0.0, float("inf")),
    lambda: P.TruncatedNormal(0.0, 1.0, 1.0, 1.0), lambda: P.TruncatedNormal(0.0, 0.0, -1.0, 1.0),
    lambda: P.TruncatedNormal(0.0, 1.0, -1.0, float("inf")), lambda: P.TruncatedNormal(0.0, 1.0, 50.0, 60.0),
    lambda: P.LogNormal(0.0, 0.0), lambda: P.HalfNormal(0.0), lambda: P.HalfNormal(float("nan")),
    lambda: P.Exponential(-1.0), lambda: P.Rayleigh(0.0), lambda: P.Weibull(1.0, 0.0), lambda: P.Weibull(0.0, 1.0),
    lambda: P.Pareto(0.0, 1.0), lambda: P.Pareto(1.0, -2.0), lambda: P.Cauchy(0.0, 0.0), lambda: P.Cauchy(float("inf"), 1.0),
    lambda: P.HalfCauchy(0.0), lambda: P.Laplace(0.0, 0.0), lambda: P.Logistic(0.0, -1.0), lambda: P.Gumbel(0.0, 0.0),
    lambda: P.Triangular(0.0, 2.0, 1.0), lambda: P.Triangular(1.0, 1.0, 1.0), lambda: P.Triangular(0.0, float("nan"), 1.0),
    lambda: P.MultivariateNormal([0.0, 0.0], [[1.0, 2.0], [2.0, 1.0]]),            # not positive definite
    lambda: P.MultivariateNormal([0.0, 0.0], [[1.0, 0.5], [0.4, 1.0]]),            # not symmetric
    lambda: P.MultivariateNormal([0.0, 0.0], [[1.0, 1.0], [1.0, 1.0]]),            # singular
    lambda: P.MultivariateNormal([0.0, float("nan")], np.eye(2)), lambda: P.MultivariateNormal([0.0, 0.0], np.eye(3)),
    lambda: P.MultivariateNormal(np.zeros(65), np.eye(65)), lambda: P.MultivariateNormal([], np.zeros((0, 0))),
    lambda: P.OrderedUniform(1.0, 0.0, 3), lambda: P.OrderedUniform(0.0, 1.0, 0), lambda: P.OrderedUniform(0.0, 1.0, 2.5),
    lambda: P.PriorTransform([]), lambda: P.PriorTransform([P.Normal(0.0, 1.0), "Normal"]),
    lambda: P.PriorTransform([P.Uniform(0.0, 1.0)] * (dm.MAX_DIM + 1)),
    lambda: P.PriorTransform([P.OrderedUniform(0.0, 1.0, dm.MAX_DIM), P.Fixed(1.0)]),
]


@pytest.mark.parametrize("k", range(len(BAD)))
def test_argument_checks_come_before_any_compile(k, monkeypatch):
    def no_library():
        raise AssertionError("library called")

    monkeypatch.setattr(dm._lib, "lib", no_library)
    with pytest.raises(ValueError):
        BAD[k]()


def test_properties():
    pt = P.PriorTransform(mixed_priors())
    assert pt.ndim == 12
    assert pt.paramnames == ["phase", "scale", "p2", "p3", "p4", "incl", "pinned", "ab_0", "ab_1", "t_0", "t_1", "t_2"]
    assert pt.wrapped_dims == [0] and not pt.is_affine
    aff = P.PriorTransform([P.Uniform(0.0, 2.0), P.Fixed(3.0), P.Uniform(-1.0, 1.0, circular=True),
                            P.Uniform(0.0, 6.0, circular=True)])
    assert aff.is_affine and aff.wrapped_dims == [2, 3] and aff.ndim == 4 and aff.paramnames == ["p0", "p1", "p2", "p3"]
    assert not P.PriorTransform([P.Uniform(0.0, 2.0), P.Normal(0.0, 1.0)]).is_affine
    assert P.PriorTransform([P.OrderedUniform(0.0, 1.0, dm.MAX_DIM)]).ndim == dm.MAX_DIM
    import ultranest_amd
    assert ultranest_amd.priors is P


def test_model_passes_its_keywords_through():
    pt = P.PriorTransform([P.Normal(0.0, 1.0), P.Uniform(0.0, 1.0)])
    m = pt.model(GAUSS, aux=[0.1, 0.2], name="named", nderived=3, derived_source=usermodels.GAUSS_DERIVED, gate_derived=True)
    assert isinstance(m, dm.DeviceModel) and m.name == "named" and m.ndim == 2 and m.nparams == 5 and m.gate_derived
    assert m.has_transform and m.source.endswith(pt.source) and list(m.aux) == [0.1, 0.2]
    s = pt.model(usermodels.AMPLITUDE_TERMS % 4 + usermodels.MULTISUM_LOGLIKE % dict(name="mlf_amplitude"),
                 aux=usermodels.linear_aux(2, 4), nterms=4, nsums=3)
    assert s.nterms == 4 and s.nsums == 3


def test_routing_takes_the_device_route():
    from ultranest_amd import likelihoods as lk
    pt = P.PriorTransform(mixed_priors())
    m = pt.model(GAUSS, aux=np.zeros(12))
    assert dm.device_route(m.transform, m.loglike) == (m, True)
    assert dm.device_route(lk.identity_transform, m.loglike) == (m, False)
    # the stand-alone callback of a host likelihood is a host callback pair: no device route
    assert dm.device_route(pt.transform, lambda p: -0.5 * (p ** 2).sum(axis=1)) is None


def test_gauss_normal_prior_evidence_is_the_quadrature_of_its_factors():
    """ln Z = sum_k ln of the integral of N(x; c_k, sigma) N(x; m_k, t) dx: a trapezoid sum over +-12 sigma around each centre
    (the integrand is analytic and vanishes at the ends to 1e-31 of its peak: the trapezoid rule converges geometrically)"""
    sigma, t = 0.1, 1.0
    model, lnz = usermodels.gauss_normal_prior(4, sigma=sigma, prior_sigma=t)
    c = usermodels.gauss_centers(4, sigma)
    assert model.ndim == 4 and model.has_transform and np.array_equal(model.aux, c)
    total = 0.0
    for ck in c:
        x = np.linspace(ck - 12 * sigma, ck + 12 * sigma, 20001)
        f = (np.exp(-0.5 * ((x - ck) / sigma) ** 2) / (sigma * np.sqrt(2 * np.pi))
             * np.exp(-0.5 * ((x - 0.5) / t) ** 2) / (t * np.sqrt(2 * np.pi)))
        total += np.log(np.sum(0.5 * (f[1:] + f[:-1])) * (x[1] - x[0]))
    assert abs(total - lnz) < 1e-10, (total, lnz)
    assert np.abs(c - 0.5).max() < 0.3 * t          # the posterior sits in the prior's bulk
