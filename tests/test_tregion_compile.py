"""The gated variant of the user-model wrapper kernel (the tregion test between transform and likelihood, -DMLF_USER_TREGION=1),
CPU side: hiprtc compiles it for gfx950 without a GPU, as its own code object under its own cache key; it spills nothing, uses
no private segment and forms no fused multiply-add; the default variant of the same sources is what it was."""
import os
import re
import subprocess

import pytest

from ultranest_amd import devicemodel as dm
from ultranest_amd import usermodels

LLVM_BIN = next((p for p in ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin") if os.path.exists(os.path.join(p, "llvm-readelf"))),
                None)

MODELS = {
    "rosenbrock7": lambda: usermodels.rosenbrock(7),       # staged form with the p buffer
    "funnel51": lambda: usermodels.funnel(51),             # staged, near the LDS budget
    "rosenbrock70": lambda: usermodels.rosenbrock(70),     # direct form
}


def _tool(name, code, tmp_path, tag, *args):
    path = os.path.join(str(tmp_path), tag + ".co")
    with open(path, "wb") as fh:
        fh.write(code)
    return subprocess.run([os.path.join(LLVM_BIN, name)] + list(args) + [path], capture_output=True, text=True, check=True).stdout


def _fma_count(asm):
    return len(re.findall(r"\bv_fma_f64\b|\bv_fmac_f64\b", asm))


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("which", sorted(MODELS))
@pytest.mark.parametrize("with_transform", [True, False])
def test_gated_variant_compiles_without_spills_or_fma(which, with_transform, tmp_path):
    """The gate's own arithmetic has no fused multiply-add anywhere: the Rosenbrock models, whose default code has none, have
    none in the gated variant either.  The funnel's likelihood calls pow, log and a division, which the device library
    expands with fused multiply-adds in the DEFAULT variant already (122 of them); there the gated variant must not have one
    more."""
    m = MODELS[which]()
    tr = with_transform and m.has_transform
    before = dm.compile_calls
    code = dm.compile_model(m.source, tr, gated=True)
    default = dm.compile_model(m.source, tr)
    assert code[:4] == b"\x7fELF" and code != default
    assert dm.compile_model(m.source, tr, gated=True) is code          # cached under its own key
    assert dm.compile_calls <= before + 2
    notes = _tool("llvm-readelf", code, tmp_path, "gated", "--notes")
    assert re.findall(r"\.name:\s+(\w+)", notes) == ["mlf_user_rows_tregion"]     # its own entry: never loaded as the default
    assert [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", notes)] == [0]
    assert [int(x) for x in re.findall(r"\.sgpr_spill_count:\s+(\d+)", notes)] == [0]
    assert [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)] == [0]
    assert [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", notes)] == [0]
    # the five parameters of the gate behind the eight of the default kernel
    assert len(re.findall(r"\.value_kind:\s+(?:global_buffer|by_value)", notes)) == 13
    asm = _tool("llvm-objdump", code, tmp_path, "gated", "-d")
    asm_default = _tool("llvm-objdump", default, tmp_path, "default", "-d")
    assert "v_mul_f64" in asm and "v_add_f64" in asm
    assert _fma_count(asm) == _fma_count(asm_default)
    if which != "funnel51":
        assert _fma_count(asm) == 0


TRIVIAL_LOGLIKE = r"""
__device__ double mlf_user_loglike(const double *p, int d, const double *aux, long long naux) { return p[0]; }
"""


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
def test_gated_funnel_transform_and_gate_form_no_fma(tmp_path):
    """The funnel's fused multiply-adds all come from the pow, log and division of its likelihood.  Its transform under the
    gated variant with a likelihood that computes nothing leaves the transform and the gate alone: not one."""
    code = dm.compile_model(TRIVIAL_LOGLIKE + "\n" + usermodels.FUNNEL_TRANSFORM, True, gated=True)
    asm = _tool("llvm-objdump", code, tmp_path, "funnel_gate", "-d")
    assert "v_mul_f64" in asm and "v_add_f64" in asm
    assert _fma_count(asm) == 0


@pytest.mark.skipif(LLVM_BIN is None, reason="llvm-readelf of ROCm not found")
@pytest.mark.parametrize("which", sorted(MODELS))
def test_default_variant_is_one_kernel_with_the_old_parameters(which, tmp_path):
    m = MODELS[which]()
    notes = _tool("llvm-readelf", m.code, tmp_path, "default", "--notes")
    assert re.findall(r"\.name:\s+(\w+)", notes) == ["mlf_user_rows"]
    assert [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)] == [0]
    assert len(re.findall(r"\.value_kind:\s+(?:global_buffer|by_value)", notes)) == 8


def test_variant_entry_points_check_their_arguments():
    import ctypes
    from ultranest_amd import _lib
    L = _lib.lib()
    size = ctypes.c_size_t(0)
    log = ctypes.create_string_buffer(256)
    src = usermodels.ROSENBROCK_LOGLIKE.encode()
    assert L.mlf_usermodel_compile_variant(src, dm.INCLUDE_DIR.encode(), 0, 7, None, 0, ctypes.byref(size), log, 256) == 1
    assert b"variant" in L.mlf_last_error()
    h = ctypes.c_void_p()
    code = usermodels.rosenbrock(7).code
    assert L.mlf_usermodel_create_variant(code, len(code), 7, 1, 7, None, 0, ctypes.byref(h)) == 1
    assert not h.value
    assert L.mlf_region_clear_tregion(None) == 1 and L.mlf_region_set_tregion_center(None, None) == 1
