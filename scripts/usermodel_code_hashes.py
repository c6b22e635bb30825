#!/usr/bin/env python3
"""sha256 of the code object of every user-model program form (ultranest_amd.devicemodel), one line ``name sha256`` each.

    python scripts/usermodel_code_hashes.py > profiles/usermodel_code_hashes_after.txt
    python scripts/usermodel_code_hashes.py --resources > profiles/user_wrapper_resources_after.txt

Needs no GPU (hiprtc compiles for gfx950 anywhere).  It goes through the module's public compile functions only, so the same
script runs on any commit that has them: two commits whose outputs are identical files hand hiprtc the same source and options
for every form, and launch the same machine code.  The models: usermodels.gauss_derived(5, affine=True) (default form, with
the derive program and the gate over derived parameters), linear_sum(3, 65, affine=True) (one sum), amplitude_sum(3, 65,
affine=True) (three sums; the source is also compiled with nsums = 1 and 8) and funnel(70); every main program with and without
its transform, gated and not; and the covariance form of usermodels.gp_sqexp at n = 8, with and without its transform, gated
and not.

--resources: behind the hash, what the code object's notes say of its one kernel (llvm-readelf of ROCm): the kernel's name,
VGPRs, SGPRs, private segment, static group segment and kernel-argument size in bytes.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("name", "vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size")


def resources(code):
    readelf = next(os.path.join(p, "llvm-readelf") for p in ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin")
                   if os.path.exists(os.path.join(p, "llvm-readelf")))
    with tempfile.NamedTemporaryFile(suffix=".co") as fh:
        fh.write(code)
        fh.flush()
        notes = subprocess.run([readelf, "--notes", fh.name], capture_output=True, text=True, check=True).stdout
    out = []
    for f in FIELDS:
        found = re.findall(r"\.%s:\s+(\w+)" % f, notes)
        assert len(found) == 1, (f, found)      # one kernel per program
        out.append("%s=%s" % (f.replace("_fixed_size", "").replace("_segment_size", "").replace("_count", ""), found[0]))
    return " ".join(out)


def main():
    from ultranest_amd import devicemodel as dm
    from ultranest_amd import usermodels
    models = [usermodels.gauss_derived(5, affine=True), usermodels.linear_sum(3, 65, affine=True),
              usermodels.amplitude_sum(3, 65, affine=True), usermodels.funnel(70)]
    out = []
    for m in models:
        full = m.source + "\n" + usermodels.GAUSS_DERIVED
        out.append((m.name + " constructor", m.code))
        for tr in (True, False):
            for nsums in ([None] if m.nsums is None else [m.nsums, 1, 8]):
                tag = "%s tr=%d%s%s" % (m.name, tr, " sum" if m.summed else "", "" if nsums is None else " sums=%d" % nsums)
                for gated in (False, True):
                    out.append((tag + (" tregion" if gated else ""), dm.compile_model(m.source, tr, gated, m.summed, nsums)))
                if m is not models[-1]:
                    out.append((tag + " tregion gate_derived", dm.compile_gate_derived(full, tr, summed=m.summed, nsums=nsums)))
        if m is not models[-1]:
            out.append((m.name + " derived", dm.compile_derived(full)))
    g = models[0]
    out.append((g.name + " model derive_code", g.derive_code))
    out.append((g.name + " model compile_gate_derived", g.compile_gate_derived(True)))
    cov = usermodels.GP_SQEXP % 8 + usermodels.GP_COV_LOGLIKE + "\n" + usermodels.GP_TRANSFORM
    for tr in (True, False):
        for gated in (False, True):
            out.append(("gp_sqexp8 tr=%d cov%s" % (tr, " tregion" if gated else ""), dm.compile_form(cov, dm.Form(tr, gated, ncov=8))))
    for name, code in out:
        assert code[:4] == b"\x7fELF", name
        print(name.replace(" ", "_"), hashlib.sha256(code).hexdigest(), *([resources(code)] if "--resources" in sys.argv[1:] else []))


if __name__ == "__main__":
    main()
