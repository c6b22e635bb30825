#!/usr/bin/env python3
"""sha256 of the code object of every user-model program form (ultranest_amd.devicemodel), one line ``name sha256`` each.

    python scripts/usermodel_code_hashes.py > profiles/usermodel_code_hashes_after.txt

Needs no GPU (hiprtc compiles for gfx950 anywhere).  It goes through the module's public compile functions only, so the same
script runs on any commit that has them: two commits whose outputs are identical files hand hiprtc the same source and options
for every form, and launch the same machine code.  The models: usermodels.gauss_derived(5, affine=True) (default form, with
the derive program and the gate over derived parameters), linear_sum(3, 65, affine=True) (one sum), amplitude_sum(3, 65,
affine=True) (three sums; the source is also compiled with nsums = 1 and 8) and funnel(70); every main program with and without
its transform, gated and not.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    for name, code in out:
        assert code[:4] == b"\x7fELF", name
        print(name.replace(" ", "_"), hashlib.sha256(code).hexdigest())


if __name__ == "__main__":
    main()
