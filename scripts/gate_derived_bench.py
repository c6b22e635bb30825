#!/usr/bin/env python3
"""The t-region gate over a user model's derived parameters (DeviceModel(..., gate_derived=True)), measured on one GPU in one
process; writes profiles/gate_derived_bench.json.

    python scripts/gate_derived_bench.py [--reps 20] [--warmup 5] [--out profiles/gate_derived_bench.json]

Shape C5 (N = 4000 live points, d = 50), 2^20 draws from the wrapping ellipsoid (method 1), a Gaussian (sigma 2 around 0) under
the prior u * 20 - 10 with three NONLINEAR derived columns (p0 p1, p49^2, exp(p0 / 8)), and the driver's t-region built over
all 53 columns of the transformed live points.  On the same region state, t-region and Philox position:
  (a) the gated derived refill      region.refill(..., tregion=tregion) of the model with gate_derived=True
                                    (mlf_region_refill_user_derived_gated: derived columns of every member row, gate, likelihood
                                    in one launch)
  (b) the host sequence of harness.refill_samples for the same model: region.sample -> transform callback (with the derived
      columns) -> tregion.inside -> likelihood callback on the accepted rows -> cut.  Without the flag this is the only path of
      such a batch, and the baseline of the speed-up
  (c) the ungated derived refill    region.refill(...) without a t-region (mlf_region_refill_user_derived): the floor
(a) runs on one region object, (b) and (c) on a second one of identical state, so that the handle of (a) keeps its t-region from
call to call as it does in the driver.  `warmup` rounds, then `reps` rounds in which (a), (b), (c) take turns (a drift of the
clocks meets all three alike); wall clock around each call (every one of them synchronises), medians.  Recorded: a / b and a / c,
the share of the batch the region and the t-region accept, whether (a) returned the rows of (b), the device name and the
kernel-source hash.
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

DERIVED = r"""
__device__ void mlf_user_derived(const double *p, int d, double *q, int nq, const double *aux, long long naux) {
  q[0] = p[0] * p[1];
  q[1] = p[d - 1] * p[d - 1];
  q[2] = exp(p[0] * 0.125);
}
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--draws", type=int, default=2 ** 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_derived_bench.json"))
    args = ap.parse_args()
    from ultranest_amd import _lib, harness, usermodels
    from ultranest_amd.devicemodel import DeviceModel
    from ultranest_amd.regions import DeviceRNG
    import ultranest_amd.mlfriends as M
    from csrc_build import source_hash
    N, d, n = 4000, 50, args.draws
    res = dict(device=_lib.device_name(), source_hash=source_hash(), nlive=N, d=d, nderived=3, draws=n,
               method="sample_from_wrapping_ellipsoid", reps=args.reps, warmup=args.warmup)
    rs = np.random.RandomState(1)
    live = np.clip(0.5 + 0.1 * rs.normal(size=(N, d)), 1e-6, 1 - 1e-6)      # p = u * 20 - 10: about N(0, 2) per column

    def make_region():
        layer = M.AffineLayer()
        layer.optimize(live, live)
        region = M.MLFriends(live.copy(), layer)
        region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=30, rng=np.random.RandomState(2))
        region.create_ellipsoid()
        return region

    gated_region, region = make_region(), make_region()
    assert gated_region.maxradiussq == region.maxradiussq and gated_region.enlarge == region.enlarge
    G = DeviceModel(d, usermodels.GAUSS_LOGLIKE % 2.0, usermodels.AFFINE_TRANSFORM, aux=np.zeros(d), name="gauss_nonlinear50",
                    nderived=3, derived_source=DERIVED, gate_derived=True)
    p_live = G.transform(live)
    tregion = M.WrappingEllipsoid(p_live)
    tregion.enlarge = tregion.compute_enlargement(nbootstraps=30, rng=np.random.RandomState(3))
    tregion.create_ellipsoid()
    assert np.shape(tregion.u)[1] == d + 3
    Lmin = float(np.quantile(G.loglike(p_live), 0.1))
    host_only = types.SimpleNamespace(sample=region.sample)      # no `refill`: refill_samples runs its host sequence
    routes = dict(
        a_gated=lambda: gated_region.refill(n, Lmin, G.transform, G.loglike, tregion=tregion),
        b_host=lambda: harness.refill_samples(host_only, tregion, G.transform, G.loglike, Lmin, n),
        c_ungated=lambda: region.refill(n, Lmin, G.transform, G.loglike))
    ms = {k: [] for k in routes}
    out = {}
    for r in range(args.warmup + args.reps):
        for k, call in routes.items():
            for reg in (gated_region, region):
                reg.device_rng = DeviceRNG(7)
                reg.current_sampling_method = reg.sample_from_wrapping_ellipsoid
            t0 = time.perf_counter()
            got = call()
            t1 = time.perf_counter()
            assert got is not None, k
            if r >= args.warmup:
                ms[k].append((t1 - t0) * 1e3)
            out[k] = got
    same = (out["a_gated"][3] == out["b_host"][3] and np.array_equal(out["a_gated"][0], out["b_host"][0])
            and np.array_equal(out["a_gated"][1], out["b_host"][1]))
    for k, v in ms.items():
        res[k] = dict(ms_median=float(np.median(v)), ms_min=float(np.min(v)), ms_max=float(np.max(v)), kept=int(len(out[k][0])),
                      evaluated=int(out[k][3]), p_width=int(np.shape(out[k][1])[1]))
    res["a_over_b"] = res["a_gated"]["ms_median"] / res["b_host"]["ms_median"]
    res["a_over_c"] = res["a_gated"]["ms_median"] / res["c_ungated"]["ms_median"]
    res["region_accepts"] = res["c_ungated"]["evaluated"] / float(n)
    res["tregion_accepts_of_those"] = res["a_gated"]["evaluated"] / float(max(res["c_ungated"]["evaluated"], 1))
    res["gated_rows_equal_host_rows"] = bool(same)
    G.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
