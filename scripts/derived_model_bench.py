#!/usr/bin/env python3
"""What derived parameters cost on the device routes, measured on one GPU in one process; writes
profiles/derived_model_bench.json.

    python scripts/derived_model_bench.py [--reps 20] [--warmup 5] [--out profiles/derived_model_bench.json]

usermodels.gauss_derived (three derived columns, DeviceModel(..., nderived=3)) against usermodels.gauss, the same model without
them.  Every timed call ends in a synchronisation of the library's stream (the calls return host arrays), so a host clock
around the call measures the call; the variants of a comparison take turns inside every repetition, after `warmup` calls each;
medians over `reps` calls.

  a  MLFriends.refill(2^20) at N = 4000, d = 50, wrapping-ellipsoid method: "derived" (mlf_region_refill_user_derived) against
     "narrow" (mlf_region_refill_user), and against "host_wrapper", what a user had before nderived existed: gauss's callbacks
     with the transform wrapped in a Python function that appends the three numpy columns -- a foreign callback, so the batch
     takes the host sequence of harness.refill_samples (fewer repetitions: it is slow)
  b  the PopulationSimpleSliceSampler device refill at d = 10, popsize 1024, nsteps 40, with and without derived columns (one
     DeviceModel.derive call over the 1024 prepared rows per refill)
  c  one PopulationSliceSampler.__next__ at popsize 1024, d = 10, Philox mode, with and without derived columns: the two
     samplers run in lockstep under equal seeds (identical sequences); a call that harvests a point makes one small synchronous
     derive call, the others nothing, so the calls that harvest are reported on their own
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


def _stats(ts):
    if len(ts) == 0:
        return dict(ms_median=float("nan"), ms_min=float("nan"), ms_max=float("nan"), calls=0)
    ts = np.asarray(ts) * 1e3
    return dict(ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), ms_max=float(np.max(ts)), calls=int(len(ts)))


def _take_turns(fns, warmup, reps):
    """fns: name -> callable; every repetition calls each once, in order; returns name -> seconds per timed call"""
    out = {k: [] for k in fns}
    for r in range(warmup + reps):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            if r >= warmup:
                out[name].append(t1 - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derived_model_bench.json"))
    args = ap.parse_args()
    from ultranest_amd import _lib, harness, usermodels
    from ultranest_amd.regions import DeviceRNG
    import ultranest_amd.mlfriends as M
    import ultranest_amd.popstepsampler as pop
    from csrc_build import source_hash
    if _lib.device_count() == 0:
        raise SystemExit("no GPU visible: nothing is measured")
    res = dict(device=_lib.device_name(), source_hash=source_hash(), reps=args.reps, warmup=args.warmup,
               timing="host clock around calls that end in a stream synchronisation; variants take turns in every repetition")
    columns = usermodels.gauss_derived_columns

    # ---- (a) ------------------------------------------------------------------------------------------------------------
    N, d = 4000, 50
    wide, narrow = usermodels.gauss_derived(d), usermodels.gauss(d)
    rs = np.random.RandomState(1)
    live = np.clip(usermodels.gauss_centers(d) + 0.03 * rs.normal(size=(N, d)), 1e-6, 1 - 1e-6)
    layer = M.AffineLayer()
    layer.optimize(live, live)
    region = M.MLFriends(live, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=30, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    region.device_rng = DeviceRNG(7)
    Lmin = float(np.quantile(narrow.loglike(live), 0.1))
    kept = {}

    def wrapper(u):
        p = narrow.transform(u)
        return np.hstack([p, columns(p)])

    def host_loglike(p):
        return narrow.loglike(p[:, :d])

    def refill(name, transform, loglike):
        def call():
            region.current_sampling_method = region.sample_from_wrapping_ellipsoid
            u, p, L, nc = harness.refill_samples(region, None, transform, loglike, Lmin, 2 ** 20)
            kept[name] = (len(u), p.shape[1], nc)
        return call

    fns = dict(narrow=refill("narrow", narrow.transform, narrow.loglike), derived=refill("derived", wide.transform, wide.loglike))
    ts = _take_turns(fns, args.warmup, args.reps)
    host_reps = max(3, args.reps // 4)
    ts.update(_take_turns(dict(host_wrapper=refill("host_wrapper", wrapper, host_loglike)), 2, host_reps))
    a = {k: _stats(v) for k, v in ts.items()}
    for k, (nk, width, nc) in kept.items():
        a[k].update(kept=nk, p_columns=width, evaluated=nc)
    a.update(draws=2 ** 20, nlive=N, d=d, nderived=3, method="sample_from_wrapping_ellipsoid",
             derived_over_narrow=a["derived"]["ms_median"] / a["narrow"]["ms_median"],
             host_wrapper_over_derived=a["host_wrapper"]["ms_median"] / a["derived"]["ms_median"])
    res["a_region_refill"] = a
    print(json.dumps(a, sort_keys=True), flush=True)
    for m in (wide, narrow):
        m.close()

    # ---- (b), (c) -------------------------------------------------------------------------------------------------------
    d, P, nlive = 10, 1024, 1000
    wide, narrow = usermodels.gauss_derived(d, affine=True), usermodels.gauss(d, affine=True)
    us = np.clip(0.5 + 0.02 * np.random.RandomState(3).normal(size=(nlive, d)), 0.01, 0.99)
    Ls = narrow.loglike(narrow.transform(us))
    Lmin = float(Ls.min() - 1.0)
    tl = M.AffineLayer()
    tl.optimize(us, us)
    host_region = types.SimpleNamespace(u=us, transformLayer=tl, maxradiussq=float(d))
    samplers = {k: pop.PopulationSimpleSliceSampler(P, 40, pop.generate_mixture_random_direction, device_rng=DeviceRNG(7))
                for k in ("narrow", "derived")}
    models = dict(narrow=narrow, derived=wide)
    fns = {k: (lambda k=k: samplers[k]._refill(host_region, Lmin, us, Ls, models[k].transform, models[k].loglike))
           for k in samplers}
    b = {k: _stats(v) for k, v in _take_turns(fns, args.warmup, args.reps).items()}
    b.update(d=d, popsize=P, nsteps=40, nlive=nlive, nderived=3,
             p_columns={k: int(len(s.prepared_samples[0][1])) for k, s in samplers.items()},
             derived_over_narrow=b["derived"]["ms_median"] / b["narrow"]["ms_median"])
    res["b_simple_slice_refill"] = b
    print(json.dumps(b, sort_keys=True), flush=True)

    region = M.MLFriends(us, tl)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=10, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    slicers = {k: pop.PopulationSliceSampler(P, 10, pop.generate_mixture_random_direction, scale=0.2, device_rng=DeviceRNG(5))
               for k in ("narrow", "derived")}
    every = {k: [] for k in slicers}
    harvest = {k: [] for k in slicers}
    calls = 0
    while calls < 4000 and len(harvest["derived"]) < args.reps:
        found = {}
        for k, s in slicers.items():
            t0 = time.perf_counter()
            got = s.__next__(region, Lmin, us, Ls, models[k].transform, models[k].loglike)
            t1 = time.perf_counter()
            found[k] = got[0] is not None
            if calls >= args.warmup:
                (harvest if found[k] else every)[k].append(t1 - t0)
        assert found["narrow"] == found["derived"]
        calls += 1
    c = dict(d=d, popsize=P, nsteps=10, nlive=nlive, nderived=3, mode="Philox (mlf_walkers_step_user)", calls_per_sampler=calls)
    for k in slicers:
        c[k] = dict(harvesting_calls=_stats(harvest[k]), other_calls=_stats(every[k]))
    c["derived_over_narrow_harvesting_call"] = (c["derived"]["harvesting_calls"]["ms_median"]
                                                / c["narrow"]["harvesting_calls"]["ms_median"])
    c["derived_over_narrow_other_call"] = c["derived"]["other_calls"]["ms_median"] / c["narrow"]["other_calls"]["ms_median"]
    c["note_threshold"] = "above 1.25 on the harvesting call: derive inside step_user instead of one synchronous call per point"
    res["c_slice_sampler_next"] = c
    print(json.dumps(c, sort_keys=True), flush=True)
    for m in (wide, narrow):
        m.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "ultranest_amd", "csrc"))
    import importlib
    sys.modules["csrc_build"] = importlib.import_module("build")
    main()
