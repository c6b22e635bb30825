#!/usr/bin/env python3
"""The tregion gate inside the device refill, measured on one GPU in one process; writes profiles/tregion_refill_bench.json.

    python scripts/tregion_refill_bench.py [--reps 10] [--out profiles/tregion_refill_bench.json]

Shape C5 (N = 4000 live points, d = 50), 2^20 draws from the wrapping ellipsoid (method 1), Rosenbrock under the prior
u * 20 - 10, as a user model and as the built-in pair.  For each of the two, on the same region, tregion and Philox
position:
  (a) the gated device refill       region.refill(..., tregion=tregion)
  (b) the ungated device refill     region.refill(...)
  (c) the host sequence harness.refill_samples runs where the region has no device refill for the tregion: region.sample ->
      transform callback -> tregion.inside -> likelihood callback on the accepted rows -> cut
(a) runs on one region object, (b) and (c) on a second one of identical state, so that the handle of (a) keeps its tregion from
call to call as it does in the driver (on one shared region every ungated call would clear the device copy and every timed
gated call would pay the full upload of the d x d matrix again); recorded as "tregion_sync".  Three warm-up rounds, then `reps` rounds in which (a), (b), (c) take turns (a drift of the clocks meets all three alike); wall
clock around each call (every one of them synchronises), medians.  Recorded: (a) / (c) and (a) - (b), the share of the batch
the region and the tregion accept, the device name and the kernel-source hash.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--draws", type=int, default=2 ** 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tregion_refill_bench.json"))
    args = ap.parse_args()
    from ultranest_amd import _lib, harness, likelihoods, usermodels
    from ultranest_amd.regions import DeviceRNG
    import ultranest_amd.mlfriends as M
    from csrc_build import source_hash
    N, d, n = 4000, 50, args.draws
    res = dict(device=_lib.device_name(), source_hash=source_hash(), nlive=N, d=d, draws=n,
               method="sample_from_wrapping_ellipsoid", reps=args.reps)
    rs = np.random.RandomState(1)
    live = np.clip(0.55 + 0.01 * rs.normal(size=(N, d)), 1e-6, 1 - 1e-6)      # around the Rosenbrock's maximum p = 1

    def make_region():
        layer = M.AffineLayer()
        layer.optimize(live, live)
        region = M.MLFriends(live.copy(), layer)
        region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=30, rng=np.random.RandomState(2))
        region.create_ellipsoid()
        return region

    gated_region, region = make_region(), make_region()
    assert gated_region.maxradiussq == region.maxradiussq and gated_region.enlarge == region.enlarge
    res["tregion_sync"] = ("outside the timed calls: the gated refills run on their own region object, whose handle keeps "
                           "the tregion; the timed call finds it unchanged and sends nothing")
    p_live = likelihoods.rosenbrock_transform(live)
    tregion = M.WrappingEllipsoid(p_live)
    tregion.enlarge = tregion.compute_enlargement(nbootstraps=30, rng=np.random.RandomState(3))
    tregion.create_ellipsoid()
    Lmin = float(np.quantile(likelihoods.rosenbrock_loglike(p_live), 0.1))
    R = usermodels.rosenbrock(d)
    host_only = types.SimpleNamespace(sample=region.sample)      # no `refill`: refill_samples runs its host sequence

    for name, transform, loglike in (("user", R.transform, R.loglike),
                                     ("builtin", likelihoods.rosenbrock_transform, likelihoods.rosenbrock_loglike)):
        routes = dict(
            a_gated=lambda: gated_region.refill(n, Lmin, transform, loglike, tregion=tregion),
            b_ungated=lambda: region.refill(n, Lmin, transform, loglike),
            c_host=lambda: harness.refill_samples(host_only, tregion, transform, loglike, Lmin, n))
        ms = {k: [] for k in routes}
        out = {}
        for r in range(3 + args.reps):
            for k, call in routes.items():
                for reg in (gated_region, region):
                    reg.device_rng = DeviceRNG(7)
                    reg.current_sampling_method = reg.sample_from_wrapping_ellipsoid
                t0 = time.perf_counter()
                got = call()
                t1 = time.perf_counter()
                if r >= 3:
                    ms[k].append((t1 - t0) * 1e3)
                out[k] = got
        same = (out["a_gated"][3] == out["c_host"][3] and np.array_equal(out["a_gated"][0], out["c_host"][0])
                and np.array_equal(out["a_gated"][1], out["c_host"][1]))
        entry = {k: dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)), kept=int(len(out[k][0])),
                         evaluated=int(out[k][3])) for k, v in ms.items()}
        entry["gated_over_host"] = entry["a_gated"]["ms_median"] / entry["c_host"]["ms_median"]
        entry["gated_minus_ungated_ms"] = entry["a_gated"]["ms_median"] - entry["b_ungated"]["ms_median"]
        entry["region_accepts"] = entry["b_ungated"]["evaluated"] / float(n)
        entry["tregion_accepts_of_those"] = entry["a_gated"]["evaluated"] / float(max(entry["b_ungated"]["evaluated"], 1))
        entry["gated_rows_equal_host_rows"] = bool(same)
        res[name] = entry
    res["anchor"] = "H3 over a 2^20 x 50 batch as its own launch: about 0.15 ms (round 6)"
    R.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
