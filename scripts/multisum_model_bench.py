#!/usr/bin/env python3
"""A user model of several sums and a final function against its default-form twin and against the single-sum form, measured on
one GPU in one process; writes profiles/multisum_model_bench.json.

    python scripts/multisum_model_bench.py [--reps 20] [--out profiles/multisum_model_bench.json]

Three models at d = 10 under the prior u * 20 - 10, on the data of usermodels.linear_data:

  multisum  usermodels.amplitude_sum   DeviceModel(..., nterms=K, nsums=3): one wave per row, three accumulators, a finish with
                                       one division and one logarithm
  twin      usermodels.amplitude_twin  the same terms and finish in the default form: one thread per row walks the K terms
  single    usermodels.linear_sum      the single-sum form on the same data: one accumulator, no finish

The method is that of scripts/summed_model_bench.py, whose timing function this script calls: DeviceModel.eval_dev on resident
rows with p and L written, device events around `inner` launches on one stream (`inner` sized in the warm-up so that a window
is a few milliseconds), three warm-up windows, then `reps` windows in which the three models take turns, the launches of a
window walking through a ring of input buffers; median and minimum of the per-launch time.

Per shape: "twin_over_multisum" (what the form buys), "multisum_over_single" (what two more accumulators and the finish cost).
"crossover" names, per K, the row counts between which twin / multisum passes 1, or says that it does not within the measured
range.  The multi-sum model's L is compared with the twin's on the first rows (relative to |L|: the forms add the same terms in
different orders).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import summed_model_bench as SB  # noqa: E402   (kernel_timing, crossover, D and the window constants)

ROWS = (256, 1024, 4096, 16384)
TERMS = (1024, 16384)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multisum_model_bench.json"))
    args = ap.parse_args()
    import torch
    from ultranest_amd import _lib, usermodels
    from csrc_build import source_hash
    if _lib.device_count() == 0:
        raise SystemExit("no GPU visible: nothing is measured")
    D = SB.D
    res = dict(device=_lib.device_name(), source_hash=source_hash(), d=D, reps=args.reps,
               model="usermodels.amplitude_sum / amplitude_twin / linear_sum, affine prior",
               timing="device events around `inner` eval_dev launches (p and L written), inputs rotated through `buffers` buffers, "
                      "the three models taking turns",
               kernel=[])
    for K in TERMS:
        models = dict(multisum=usermodels.amplitude_sum(D, K, seed=1, affine=True),
                      twin=usermodels.amplitude_twin(D, K, seed=1, affine=True),
                      single=usermodels.linear_sum(D, K, seed=1, affine=True))
        ratios = []
        for rows in ROWS:
            ms, inner, nbuf, L, _ = SB.kernel_timing(torch, models, rows, args.reps)
            c = min(rows, 256)
            entry = dict(rows=rows, nterms=K, nsums=3, buffers=nbuf, input_bytes_in_rotation=nbuf * rows * D * 8, rows_compared=c,
                         max_relative_difference_multisum_twin=float((np.abs(L["multisum"][:c] - L["twin"][:c])
                                                                      / np.abs(L["twin"][:c])).max()))
            for name in models:
                entry[name] = dict(ms_median=float(np.median(ms[name])), ms_min=float(np.min(ms[name])), inner=inner[name])
            entry["twin_over_multisum"] = entry["twin"]["ms_median"] / entry["multisum"]["ms_median"]
            entry["multisum_over_single"] = entry["multisum"]["ms_median"] / entry["single"]["ms_median"]
            ratios.append(entry["twin_over_multisum"])
            res["kernel"].append(entry)
            print(json.dumps(entry, sort_keys=True), flush=True)
        res["crossover_nterms_%d" % K] = SB.crossover(ROWS, ratios)
        for m in models.values():
            m.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
