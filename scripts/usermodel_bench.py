#!/usr/bin/env python3
"""User models (ultranest_amd.devicemodel) measured on one GPU, one process; writes profiles/usermodel_bench.json.

    python scripts/usermodel_bench.py [--reps 20] [--out profiles/usermodel_bench.json]

(a) the fused wrapper kernel (mlf_usermodel_eval_dev) on 10^6 x 50 resident rows: the Gaussian restated as a user model with
    the affine transform u * 20 - 10 (transform + likelihood, one launch: read u, write p, write L), next to the built-in pair
    on the same rows -- the elementwise affine (one torch elementwise launch with the traffic of k_elementwise_affine: read u,
    write p; the library has no stand-alone entry for k_elementwise_affine) + mlf_loglike_dev(kind 0);
(b) MLFriends.refill(2^20) at N = 4000, d = 50 (wrapping ellipsoid) with the user Gaussian and with the built-in one
    (identity transform on both);
(c) the funnel (examples/testfunnel.py) at d = 50: rows per second of the fused kernel.
Times: median over `reps` runs (torch events on the stream the work is enqueued on; wall clock for refill, which
synchronises).
"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _notes(code):
    llvm = next((p for p in ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin") if os.path.exists(os.path.join(p, "llvm-readelf"))),
                None)
    if llvm is None:
        return {}
    with tempfile.NamedTemporaryFile(suffix=".co") as fh:
        fh.write(code)
        fh.flush()
        text = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", fh.name], capture_output=True, text=True).stdout
    out = {}
    for key in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size"):
        m = re.search(r"\.%s:\s+(\d+)" % key, text)
        if m:
            out[key] = int(m.group(1))
    return out


def _time_events(torch, fn, reps):
    stream = torch.cuda.current_stream()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "usermodel_bench.json"))
    args = ap.parse_args()
    import torch
    from ultranest_amd import _lib, likelihoods, usermodels
    from ultranest_amd.devicemodel import compile_model
    from ultranest_amd.regions import DeviceRNG
    import ultranest_amd.mlfriends as M
    from csrc_build import source_hash
    L = _lib.lib()
    dev = torch.device("cuda")
    s = torch.cuda.current_stream().cuda_stream
    res = dict(device=_lib.device_name(), source_hash=source_hash())

    # ---- (a) ------------------------------------------------------------------------------------------------------------
    n, d = 10 ** 6, 50
    G = usermodels.gauss(d, affine=True)
    u = torch.rand((n, d), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    p = torch.empty_like(u)
    Lu = torch.empty(n, dtype=torch.float64, device=dev)
    p2 = torch.empty_like(u)
    Lb = torch.empty(n, dtype=torch.float64, device=dev)
    centers = torch.from_numpy(usermodels.gauss_centers(d)).to(dev)
    minus10 = torch.tensor(-10.0, dtype=torch.float64, device=dev)

    def fused():
        G.eval_dev(u.data_ptr(), n, p.data_ptr(), Lu.data_ptr(), None, s)

    def affine():
        torch.add(minus10, u, alpha=20.0, out=p2)

    def loglike():
        _lib.check(L.mlf_loglike_dev(0, ctypes.c_void_p(p2.data_ptr()), d, n, ctypes.c_void_p(centers.data_ptr()), 0.1,
                                     ctypes.c_void_p(Lb.data_ptr()), ctypes.c_void_p(s)))

    def pair():
        affine()
        loglike()

    t_fused, t_fused_min = _time_events(torch, fused, args.reps)
    t_pair, t_pair_min = _time_events(torch, pair, args.reps)
    t_aff, _ = _time_events(torch, affine, args.reps)
    t_ll, _ = _time_events(torch, loglike, args.reps)
    torch.cuda.synchronize()
    agree = float((p - p2).abs().max().item()), float(((Lu - Lb).abs() / Lb.abs()).max().item())
    bytes_fused = n * d * 8 * 2 + n * 8
    lds = 2 * 64 * (d + 1) * 8
    res["a_fused_eval_dev"] = dict(
        rows=n, d=d, ms_median=t_fused, ms_min=t_fused_min, bytes=bytes_fused, tb_per_s=bytes_fused / (t_fused * 1e-3) / 1e12,
        builtin_pair_ms_median=t_pair, builtin_pair_ms_min=t_pair_min, builtin_affine_ms=t_aff, builtin_loglike_ms=t_ll,
        builtin_pair_bytes=n * d * 8 * 3 + n * 8, ratio_fused_over_pair=t_fused / t_pair,
        max_abs_diff_p=agree[0], max_rel_diff_L=agree[1],
        lds_bytes_per_wave=lds, waves_per_cu_by_lds=(160 * 1024) // lds, kernel_notes=_notes(G.code),
        target="fused >= 3 TB/s and <= 1.25 x the built-in pair")

    # ---- (b) ------------------------------------------------------------------------------------------------------------
    N = 4000
    rs = np.random.RandomState(1)
    ctr = usermodels.gauss_centers(d)
    live = np.clip(ctr + 0.03 * rs.normal(size=(N, d)), 1e-6, 1 - 1e-6)
    layer = M.AffineLayer()
    layer.optimize(live, live)
    region = M.MLFriends(live, layer)
    region.maxradiussq, region.enlarge = region.compute_enlargement(nbootstraps=30, rng=np.random.RandomState(2))
    region.create_ellipsoid()
    Gu = usermodels.gauss(d)
    Gb = likelihoods.GaussLikelihood.docs_gauss(d)
    Lmin = float(np.quantile(Gb(live), 0.1))
    refill = {}
    for name, ll in (("user", Gu.loglike), ("builtin", Gb)):
        region.device_rng = DeviceRNG(7)
        ts, kept, ncs = [], [], []
        for r in range(3 + args.reps // 2):
            region.current_sampling_method = region.sample_from_wrapping_ellipsoid
            t0 = time.perf_counter()
            uu, pp, LL, nc = region.refill(2 ** 20, Lmin, likelihoods.identity_transform, ll)
            t1 = time.perf_counter()
            if r >= 3:
                ts.append((t1 - t0) * 1e3)
                kept.append(len(uu))
                ncs.append(nc)
        refill[name] = dict(ms_median=float(np.median(ts)), ms_min=float(np.min(ts)), kept_mean=float(np.mean(kept)),
                            evaluated_mean=float(np.mean(ncs)))
    refill["ratio_user_over_builtin"] = refill["user"]["ms_median"] / refill["builtin"]["ms_median"]
    refill.update(draws=2 ** 20, nlive=N, d=d, method="sample_from_wrapping_ellipsoid", target="user <= 1.2 x builtin")
    res["b_refill"] = refill

    # ---- (c) ------------------------------------------------------------------------------------------------------------
    F = usermodels.funnel(d)
    pf = torch.empty_like(u)
    Lf = torch.empty(n, dtype=torch.float64, device=dev)

    def funnel():
        F.eval_dev(u.data_ptr(), n, pf.data_ptr(), Lf.data_ptr(), None, s)

    t_f, t_f_min = _time_events(torch, funnel, args.reps)
    res["c_funnel"] = dict(rows=n, d=d, ms_median=t_f, ms_min=t_f_min, rows_per_s=n / (t_f * 1e-3),
                           tb_per_s=bytes_fused / (t_f * 1e-3) / 1e12, kernel_notes=_notes(F.code))
    res["identity_variant_notes"] = _notes(compile_model(Gu.source, False))
    for m in (G, Gu, F):
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
