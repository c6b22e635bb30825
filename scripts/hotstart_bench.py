#!/usr/bin/env python3
"""What the warm start's contbox deformation (ultranest_amd.hotstart, form (a)) costs inside the device refill, measured on one
GPU in one process; writes profiles/hotstart_bench.json.

    python scripts/hotstart_bench.py [--reps 20] [--warmup 5] [--out profiles/hotstart_bench.json]

The method of scripts/prior_transform_bench.py: shape C5 (N = 4000 live points, d = 50), region.refill of 2^20 draws from the
wrapping ellipsoid with Lmin = 1e300, so that no row is kept and what is left is the device work.  The models:
  (a) inner    usermodels.gauss (sigma 0.1) under 50 Normal(0.5, 1) priors of the prior library
  (b) contbox  its contbox model (hotstart.get_auxiliary_contbox_parameterization) from 400 samples around the centres: d + 1 = 51
               cube coordinates, the same likelihood and prior text behind the deformation
Each model has its own region of its own dimension (50 and 51: the live points of (b) are those of (a) with one more column),
so the two calls differ in the region's work as well as in the model's: the ratio is that of the whole calls.  `warmup` rounds,
then `reps` rounds in which the models take turns; wall clock around each call (every one synchronises), medians.  No threshold:
the ratio is recorded, not asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--draws", type=int, default=2 ** 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hotstart_bench.json"))
    args = ap.parse_args()
    from ultranest_amd import _lib, hotstart, usermodels
    from ultranest_amd.regions import DeviceRNG
    import ultranest_amd.mlfriends as M
    from csrc_build import source_hash
    N, d, n = 4000, 50, args.draws
    if _lib.device_count() < 1:
        raise SystemExit("hotstart_bench needs a GPU: nothing is measured without one")
    res = dict(device=_lib.device_name(), source_hash=source_hash(), nlive=N, d=d, draws=n,
               method="sample_from_wrapping_ellipsoid", reps=args.reps, warmup=args.warmup, Lmin=1e300)
    rs = np.random.RandomState(1)
    live = np.clip(0.5 + 0.1 * rs.normal(size=(N, d + 1)), 1e-6, 1 - 1e-6)

    def make_region(points):
        layer = M.AffineLayer()
        layer.optimize(points, points)
        region = M.MLFriends(points.copy(), layer)
        region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=30, rng=np.random.RandomState(2))
        region.create_ellipsoid()
        return region

    t0 = time.perf_counter()
    inner, _ = usermodels.gauss_normal_prior(d)
    res["compile_inner_s"] = time.perf_counter() - t0
    upoints = np.clip(0.5 + 0.05 * rs.normal(size=(400, d)), 1e-6, 1 - 1e-6)
    t0 = time.perf_counter()
    aux = hotstart.get_auxiliary_contbox_parameterization(["x%d" % k for k in range(d)], inner.loglike, inner.transform, upoints,
                                                          np.full(400, 1.0 / 400))[1].model
    res["compile_contbox_s"] = time.perf_counter() - t0
    models = dict(a_inner=(inner, make_region(live[:, :d])), b_contbox=(aux, make_region(live)))
    ms = {k: [] for k in models}
    evaluated = {}
    for r in range(args.warmup + args.reps):
        for k, (m, reg) in models.items():
            reg.device_rng = DeviceRNG(7)
            reg.current_sampling_method = reg.sample_from_wrapping_ellipsoid
            t0 = time.perf_counter()
            got = reg.refill(n, 1e300, m.transform, m.loglike)
            t1 = time.perf_counter()
            assert got is not None and len(got[0]) == 0, k
            if r >= args.warmup:
                ms[k].append((t1 - t0) * 1e3)
            evaluated[k] = int(got[3])
    for k, v in ms.items():
        res[k] = dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)), evaluated=evaluated[k])
    res["b_over_a"] = res["b_contbox"]["ms_median"] / res["a_inner"]["ms_median"]
    res["b_over_a_per_member_row"] = res["b_over_a"] * evaluated["a_inner"] / max(evaluated["b_contbox"], 1)
    inner.close()
    aux.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
