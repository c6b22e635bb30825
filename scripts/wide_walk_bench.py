#!/usr/bin/env python3
"""PopulationSliceSampler above 128 dimensions, measured on one GPU in one process; writes profiles/wide_walk_bench.json.

    python scripts/wide_walk_bench.py [--reps 7] [--dims 128,256,512,1024] [--out profiles/wide_walk_bench.json]
                                      [--walk-bench parent=a.json,b.json,c.json:this=d.json,e.json,f.json]

Philox mode, popsize 1024, nsteps 16, one round per call (max_rounds = 1: a call is one likelihood evaluation of every walker,
whatever the walker under the ring index does), at d = 128 (the narrow direction draw, the anchor of every ratio) and
256, 512, 1024 (the wide one):
  models      builtin  identity transform + GaussLikelihood (above 128 dimensions: one thread per row)
              user     usermodels.gauss (the user-model wrapper kernel; one step per call, no graph replay)
  directions  region-random (a d x d matrix-vector product per new slice), mixture, cube-oriented
  step        milliseconds per __next__: five warm-up calls, then `reps` rounds in which all samplers take turns, 20 calls
              each per round (a drift of the clocks meets all alike); wall clock (every call ends in a synchronisation);
              median and minimum over the rounds
  direction   the direction kernel alone (mlf_walkers_brackets_philox on a population of 1024 walkers without a slice, nsteps
              1): reset, synchronise, then the launch and a synchronisation on the clock; all seven kinds
The region is a synthetic affine layer (a seeded well-conditioned matrix), so nothing of size N x d^2 is built at d = 1024; 400
live points around the Gaussian's centre, threshold at their 10 % quantile.  Every number is recorded, and its ratio to the
d = 128 number of the same run.

--walk-bench folds in runs of scripts/walk_bench.py (its walk_bench_device.json files) of the parent commit and of this tree,
made alternately in one session: per (mode, popsize) the parent's median and spread (max - min over its runs) and this tree's
median; `beyond_spread` lists the rows where this tree's median lies above the parent's slowest run.
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

POPSIZE, NSTEPS, NLIVE, CALLS = 1024, 16, 400, 20
DIRECTIONS = ("generate_region_random_direction", "generate_mixture_random_direction", "generate_cube_oriented_direction")


def problem(d):
    from ultranest_amd import usermodels
    rs = np.random.RandomState(1000 + d)
    axes = 0.05 * (np.eye(d) + 0.3 * rs.normal(size=(d, d)) / np.sqrt(d))
    centers = usermodels.gauss_centers(d)
    u = np.clip(centers + 0.05 * rs.normal(size=(NLIVE, d)), 1e-3, 1 - 1e-3)
    layer = types.SimpleNamespace(axes=axes, T=np.linalg.inv(axes), ctr=u.mean(axis=0))
    return types.SimpleNamespace(u=u, transformLayer=layer, maxradiussq=float(d)), centers


def summary(ms):
    return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), ms_max=float(np.max(ms)))


def bench_steps(dims, reps):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import likelihoods, usermodels
    from ultranest_amd.regions import DeviceRNG
    runs = []
    for d in dims:
        region, centers = problem(d)
        builtin = (likelihoods.identity_transform, likelihoods.GaussLikelihood(centers, 0.1, d))
        G = usermodels.gauss(d)
        Ls = builtin[1](region.u)
        Lmin = float(np.quantile(Ls, 0.1))
        for model, (transform, loglike) in (("builtin", builtin), ("user", (G.transform, G.loglike))):
            for direction in DIRECTIONS:
                s = pop.PopulationSliceSampler(popsize=POPSIZE, nsteps=NSTEPS, generate_direction=getattr(pop, direction),
                                               scale=0.3, device_rng=DeviceRNG(7))
                s.max_rounds = 1
                runs.append(dict(d=d, model=model, direction=direction, sampler=s, ms=[], nc=0, found=0,
                                 args=(region, Lmin, region.u, Ls, transform, loglike)))
    for r in range(1 + reps):
        for run in runs:
            s, args = run["sampler"], run["args"]
            n = 5 if r == 0 else CALLS
            t0 = time.perf_counter()
            for _ in range(n):
                res = s.__next__(*args)
                run["nc"] += res[3]
                run["found"] += res[0] is not None
            t1 = time.perf_counter()
            if r > 0:
                run["ms"].append((t1 - t0) * 1e3 / n)
    rows = []
    for run in runs:
        row = dict(d=run["d"], model=run["model"], direction=run["direction"], found=run["found"],
                   likelihood_evals_per_call=run["nc"] / (5 + reps * CALLS), **summary(run["ms"]))
        rows.append(row)
    for row in rows:
        anchor = [x for x in rows if x["d"] == 128 and x["model"] == row["model"] and x["direction"] == row["direction"]]
        row["over_d128"] = row["ms_median"] / anchor[0]["ms_median"] if anchor else None
    return rows


def bench_direction_kernel(dims, reps):
    import ultranest_amd.popstepsampler as pop
    from ultranest_amd import _lib
    from ultranest_amd.regions import DeviceRNG
    L = _lib.lib()
    rows = []
    for d in dims:
        region, _ = problem(d)
        w = pop._Walkers(POPSIZE, 1, d)
        w.set_direction_data(axes=region.transformLayer.axes, live=region.u, std=region.u.std(axis=0))
        rng = DeviceRNG(9)
        for kind in range(7):
            ms = []
            for r in range(2 + reps):
                _lib.check(L.mlf_walkers_reset(w._h))
                _lib.check(L.mlf_synchronize())
                t0 = time.perf_counter()
                w.brackets_philox(0.3, kind, 1.0, rng)
                _lib.check(L.mlf_synchronize())
                t1 = time.perf_counter()
                if r >= 2:
                    ms.append((t1 - t0) * 1e3)
            assert np.isfinite(w.export()["currentv"]).all()
            rows.append(dict(d=d, kind=kind, **summary(ms)))
    for row in rows:
        anchor = [x for x in rows if x["d"] == 128 and x["kind"] == row["kind"]]
        row["over_d128"] = row["ms_median"] / anchor[0]["ms_median"] if anchor else None
    return rows


def fold_walk_bench(spec):
    """parent=a.json,b.json:this=c.json,d.json -> per (mode, popsize) the two sides' ms_per_call"""
    sides = {}
    for part in spec.split(":"):
        name, files = part.split("=")
        sides[name] = [json.load(open(f)) for f in files.split(",")]
    out = []
    for i, first in enumerate(sides["parent"][0]):
        parent = [run[i]["ms_per_call"] for run in sides["parent"]]
        this = [run[i]["ms_per_call"] for run in sides["this"]]
        out.append(dict(mode=first["mode"], popsize=first["popsize"], d=first["d"], parent_ms=parent, this_ms=this,
                        parent_median=float(np.median(parent)), parent_spread=float(np.max(parent) - np.min(parent)),
                        this_median=float(np.median(this)), this_over_parent=float(np.median(this) / np.median(parent)),
                        beyond_spread=bool(np.median(this) > np.max(parent))))
    return dict(script="scripts/walk_bench.py device", runs_per_side=len(sides["parent"]), rows=out,
                beyond_spread=[(r["mode"], r["popsize"]) for r in out if r["beyond_spread"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dims", default="128,256,512,1024")
    ap.add_argument("--walk-bench", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_walk_bench.json"))
    args = ap.parse_args()
    dims = [int(x) for x in args.dims.split(",")]
    from ultranest_amd import _lib
    from csrc_build import source_hash
    res = dict(device=_lib.device_name(), source_hash=source_hash(), reps=args.reps, popsize=POPSIZE, nsteps=NSTEPS, nlive=NLIVE,
               calls_per_round=CALLS, mode="Philox, one round per call", dims=dims)
    res["direction_kernel"] = bench_direction_kernel(dims, args.reps)
    res["step"] = bench_steps(dims, args.reps)
    if args.walk_bench:
        res["narrow_path_walk_bench"] = fold_walk_bench(args.walk_bench)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
