"""Register spills of the built kernels, read from the code objects' metadata (scripts/spill_report.py).  The kernels of the
headline step must not spill at all -- a spill inside their loops is silent and costs 10 % (round 6: three diagnostic stamps in
k_prep_sweep spilled 25 registers and every timing taken with them was wrong) -- and no other kernel may spill more than it is
known to (k_prep4 at d >= 50, k_boot above 64 dimensions, the narrow k_sweep instances)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = {"k_prep4<50>": 6, "k_prep4<52>": 6, "k_prep4<56>": 9, "k_prep4<60>": 26, "k_prep4<64>": 29,
         "k_boot<80>": 12, "k_boot<96>": 10, "k_boot<112>": 10, "k_boot<128>": 13,
         "k_sweep<4, 2, true, 1>": 5, "k_sweep<4, 2, false, 1>": 5, "k_sweep<2, 4, true, 1>": 2, "k_sweep<2, 4, false, 1>": 2}
HEADLINE = ("k_prep_sweep<", "k_sweep_min<", "k_uncertain<", "k_scan<", "k_inside_mid<", "k_inside_small<", "k_filter<", "k_boot_sym<",
            "k_walk_", "k_loglike")


def test_no_new_register_spills():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import spill_report
    finally:
        sys.path.pop(0)
    if not os.path.exists(os.path.join(spill_report.LLVM, "llvm-objdump")):
        pytest.skip("no ROCm LLVM tools here")
    ks = spill_report.kernels()
    if not ks:
        pytest.skip("no object files under ultranest_amd/csrc/build (the library was built elsewhere)")
    assert len(ks) >= 925, len(ks)      # 924 and k_generate_around_points_wide
    names = subprocess.run(["c++filt"], input="\n".join(ks), capture_output=True, text=True).stdout.splitlines()
    assert sum("k_generate_around_points_wide(" in name for name in names) == 1
    for mangled, name in zip(ks, names):
        spilled = ks[mangled].get("vgpr_spill_count", 0)
        short = name.replace("void mlf::", "").replace("mlf::", "").split("(")[0]
        if short.startswith(HEADLINE):
            assert spilled == 0, (name, spilled)
        assert spilled <= KNOWN.get(short, 0), (name, spilled, KNOWN.get(short, 0))
