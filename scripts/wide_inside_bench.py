"""MLFriends.inside above 128 dimensions, device-resident: the f16 matrix-core pre-filter (mlf_wide_filter.hip, the default
route) against the exact scan alone ("filter" = 0, the route of every batch before the pre-filter existed), alternating in
one process.  Writes profiles/wide_inside_bench.json.

    python scripts/wide_inside_bench.py [--dims 129,200,256,512,1024] [--sizes 16384,262144,1048576] [--reps 5]
                                        [--small 257,1024,4096] [--tree DIR] [--routes both|default] [--parent-json FILE]
                                        [--blocked]

N = 4000 live points at 0.5 + 0.05 N(0, 1), layer and ellipsoid from cov (d + 2), r2 = the 0.8-quantile of the nearest-
neighbour distances among the first 150 whitened live points.  Proposals, built in the whitened space and taken back to the
cube: half jittered live points (spread x U(0.05, 1.2): neighbours for most), a quarter a Gaussian of the live set's width
(inside the ellipsoid, no neighbour: the exact scan's whole sweep), a quarter a shell across the ellipsoid's surface.
--small: batch sizes for the routing threshold (below which batch size does the exact scan win?).
--tree: the checkout whose library is measured (default: this one); --routes default: one route only (a checkout without the
pre-filter); --parent-json: results of such a run, kept under "parent_commit" in the output."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--dims", default="129,200,256,512,1024")
ap.add_argument("--sizes", default="16384,262144,1048576")
ap.add_argument("--small", default="257,1024,4096")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--nlive", type=int, default=4000)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--routes", default="both", choices=("both", "default"))
ap.add_argument("--parent-json", default=None)
ap.add_argument("--blocked", action="store_true", help="all repeats of one route, then all of the other, instead of alternating")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.tree)
from ultranest_amd import _lib, kernels  # noqa: E402

dev = torch.device("cuda:0")
stream = torch.cuda.current_stream().cuda_stream
dims = [int(x) for x in args.dims.split(",") if x]
sizes = [int(x) for x in args.sizes.split(",") if x]
small = [int(x) for x in args.small.split(",") if x]
routes = (1, 0) if args.routes == "both" else (1,)


def build(d, n):
    rs = np.random.RandomState(4100 + d)
    u = 0.5 + 0.05 * rs.normal(size=(n, d))
    ctr = u.mean(axis=0)
    cov = np.cov(u, rowvar=0) * (d + 2) + 1e-6 * np.eye(d)
    ev, evec = np.linalg.eigh(cov)
    T = evec * ev ** -0.5
    invT = (evec * ev ** 0.5).T
    inv = np.linalg.inv(cov)
    tl = kernels.affine_transform(u, ctr, T)
    dd = ((tl[:150, None, :] - tl[None, :150, :]) ** 2).sum(axis=2)
    np.fill_diagonal(dd, np.inf)
    r2 = float(np.quantile(dd.min(axis=1), 0.8))
    reg = kernels.DeviceRegion()
    reg.set(u, 0, ctr, T, None, ctr, inv, 2.0 * d, r2, live_space=1)
    return reg, tl, invT, ctr


def proposals(d, p, tl, invT, ctr):
    g = torch.Generator(device=dev)
    g.manual_seed(4200 + d)
    tl_d = torch.from_numpy(tl).to(dev)
    invT_d = torch.from_numpy(np.ascontiguousarray(invT)).to(dev)
    ctr_d = torch.from_numpy(ctr).to(dev)
    sd = float(tl.std())
    pts = torch.empty((p, d), dtype=torch.float64, device=dev)
    for r0 in range(0, p, 65536):
        m = min(65536, p - r0)
        z = torch.randn((m, d), dtype=torch.float64, device=dev, generator=g)
        s = torch.rand((m, 1), dtype=torch.float64, device=dev, generator=g)
        idx = torch.randint(len(tl), (m,), device=dev, generator=g)
        which = (torch.arange(r0, r0 + m, device=dev) % 4).unsqueeze(1)
        a = tl_d[idx] + sd * z * (0.05 + 1.15 * s)
        b = 1.3 * sd * z
        c = z / z.norm(dim=1, keepdim=True) * torch.sqrt(2.0 * d * (0.9 + 0.2 * s))
        t = torch.where(which <= 1, a, torch.where(which == 2, b, c))
        pts[r0:r0 + m] = t @ invT_d + ctr_d
    torch.cuda.synchronize()
    return pts


def run(reg, pts, p, mask):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reg.inside_dev(pts.data_ptr(), p, mask.data_ptr(), stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(reg, pts, p, reps):
    name = {1: "default", 0: "exact_scan"}
    masks = {f: torch.empty(p, dtype=torch.uint8, device=dev) for f in routes}
    ms = {f: [] for f in routes}
    row = {"filter_active": bool(reg.filter_info(p)[0])}
    for f in routes:                                   # warm-up: allocations, LDS grants
        reg.set_option("filter", f)
        run(reg, pts, p, masks[f])
    order = [f for f in routes for _ in range(reps)] if args.blocked else [f for _ in range(reps) for f in routes]   # default: alternating
    for f in order:
        reg.set_option("filter", f)
        ms[f].append(run(reg, pts, p, masks[f]))
    for f in routes:                                   # per-stage / per-launch times of one timed call
        reg.set_option("filter", f)
        reg.inside_dev_timed(pts.data_ptr(), p, masks[f].data_ptr(), stream)
        torch.cuda.synchronize()
        _, prep, scan, rest = reg.timing_collect()
        row[name[f] + "_stage_ms"] = {"per_proposal_stage": prep, "neighbour_test": scan, "tail": rest}
        if f == 1:
            row["default_filter_launch_ms"] = [float(x) for x in reg.timing_filter_launch_ms()]   # quantise, sweep
            reg.timing_filter_launches()
            st = reg.debug_stats()       # every query the pre-filter left to the exact scan: guard cases + minimum in the band
            row["route2_share"] = st["exact_scan_queries"] / p if row["filter_active"] else None
            row["band_share"] = st["uncertain_queries"] / p if row["filter_active"] else None
    reg.set_option("filter", None)
    for f in routes:
        v = np.array(ms[f])
        row[name[f] + "_ms"] = [round(float(x), 4) for x in v]
        row[name[f] + "_median_ms"] = float(np.median(v))
        row[name[f] + "_spread"] = float((v.max() - v.min()) / np.median(v))
        row[name[f] + "_proposals_per_s"] = p / (float(np.median(v)) * 1e-3)
    row["accepted"] = float(masks[1].float().mean().item())
    if len(routes) == 2:
        row["masks_equal"] = bool((masks[0] == masks[1]).all().item())
        assert row["masks_equal"], "masks differ"
        row["speedup"] = row["exact_scan_median_ms"] / row["default_median_ms"]
    return row


out = {"device": _lib.device_name(), "nlive": args.nlive, "reps": args.reps, "order": "blocked" if args.blocked else "alternating", "shapes": {}, "small": {}}
for d in dims:
    reg, tl, invT, ctr = build(d, args.nlive)
    pmax = max(sizes + small)
    pts = proposals(d, pmax, tl, invT, ctr)
    for p in sizes:
        out["shapes"]["d%d_P%d" % (d, p)] = row = measure(reg, pts, p, args.reps)
        print("d", d, "P", p, json.dumps(row), flush=True)
    for p in small:
        out["small"]["d%d_P%d" % (d, p)] = row = measure(reg, pts, p, args.reps)
        print("d", d, "P", p, json.dumps(row), flush=True)
    reg.close()
    del pts
    torch.cuda.empty_cache()
if args.parent_json:
    with open(args.parent_json) as fh:
        out["parent_commit"] = json.load(fh)
if len(routes) == 2:   # the conditions this route is held to, against "filter" = 0 (the route of the batches before the pre-filter)
    rows = dict(out["shapes"], **out["small"])
    out["conditions"] = {
        "no_shape_slower_than_filter_0_beyond_the_spread": {
            k: r["speedup"] for k, r in rows.items() if r["speedup"] < 1.0 - max(r["default_spread"], r["exact_scan_spread"])},
        "below_2x_at_d_ge_200_and_P_ge_2^18": {
            k: r["speedup"] for k, r in out["shapes"].items()
            if int(k[1:].split("_P")[0]) >= 200 and int(k.split("_P")[1]) >= 262144 and r["speedup"] < 2.0}}
    print("conditions (empty = met):", json.dumps(out["conditions"]), flush=True)
dst = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wide_inside_bench.json")
with open(dst, "w") as fh:
    json.dump(out, fh, indent=1)
print("wrote", dst)
