#!/usr/bin/env python3
"""How wide is the pre-filter's band at the benchmark's shape, term by term?  A numpy model, no GPU.

    python scripts/band_model.py > profiles/band_model.json

The benchmark's live points (bench.py: RandomState(1), 4000 x 50), an eigen-whitening of their covariance, the radius of 30
bootstrap rounds (largest distance of a left-out point to its nearest selected one), 2 x 10^5 proposals uniform in the sphere
that wraps the whitened points (enlarged by the bootstraps' largest left-out norm), sigma from the library's rule (the power
of two that brings the largest centred coordinate into [0.5, 1)), and an ASSUMED zeta of 3 x 10^-5 for the whitening chain.
For each proposal the EXACT minimum squared distance is set against the band [T_lo, T_hi] of four bounds:

    today        filter_thresholds4: 2^-11 (1 + 2^-9) (namax + nbn) + 2 sqrt(K) 2^-24 for the operands, E with 2^-15
    live side    the live points' term replaced by ea_max, the largest measured |ah - sigma a'|
    query side   ... and the proposal's by its own measured |bh - bq|
    c(K)         ... and E's coefficient 2^-18 (1 + 2^-9) (K = 64)                  = filter_thresholds4r

The model is not the library's region (its ellipsoid and radius differ in detail) and it looks at the exact minimum, not at
the computed Dt: the shares differ from the device's count, the RATIOS are what it is for."""
import json

import numpy as np

N, D, P, ROUNDS, ZETA, K = 4000, 50, 200000, 30, 3e-5, 64


def f16_residue(x):
    return np.linalg.norm(x.astype(np.float32).astype(np.float16).astype(np.float64) - x, axis=-1)


def main():
    rs = np.random.RandomState(1)
    u = 0.5 + 0.05 * rs.normal(size=(N, D))
    ctr = u.mean(axis=0)
    eigval, eigvec = np.linalg.eigh(np.cov(u, rowvar=False))
    t = (u - ctr) @ (eigvec * eigval**-0.5)
    n2 = (t**2).sum(axis=1)
    d2 = n2[:, None] + n2[None, :] - 2.0 * t @ t.T
    r2 = grow = 0.0
    for _ in range(ROUNDS):
        sel = np.zeros(N, dtype=bool)
        sel[rs.randint(N, size=N)] = True
        r2 = max(r2, d2[~sel][:, sel].min(axis=1).max())
        grow = max(grow, n2[~sel].max() / n2[sel].max())
    big_r = np.sqrt(n2.max() * max(grow, 1.0))
    z = rs.normal(size=(P, D))
    b = z / np.linalg.norm(z, axis=1, keepdims=True) * (big_r * rs.uniform(size=(P, 1)) ** (1.0 / D))
    smin = np.empty(P)
    for lo in range(0, P, 10000):
        bb = b[lo:lo + 10000]
        smin[lo:lo + 10000] = ((bb**2).sum(axis=1)[:, None] + n2[None, :] - 2.0 * bb @ t.T).min(axis=1)

    c = t.mean(axis=0)
    sigma = 2.0 ** -np.frexp(np.abs(t - c).max())[1]
    xa = sigma * (t - c)
    namax = np.linalg.norm(xa, axis=1).max()
    ea = f16_residue(xa)
    xb = sigma * (b - c)
    nbn = np.linalg.norm(xb, axis=1)
    eb = f16_residue(xb)
    worst = 2.0**-11 * (1 + 2.0**-9)
    w0 = namax + nbn
    common = 2.0**-40 * w0 + (1 + 2.0**-10) * ZETA
    sr = sigma * np.sqrt(r2)

    def share(delta, ck):
        w = w0 + 2.0**-8
        e = ck * w * w + 2.0**-22 + 2.0**-18 * nbn**2
        lo = np.maximum(sr * (1 - 2.0**-30) - delta, 0.0)
        hi = sr * (1 + 2.0**-30) + delta
        dt = sigma**2 * smin
        return float(((dt > lo * lo - e) & (dt <= hi * hi + e)).mean())

    rows = [("today", share(worst * w0 + 2 * np.sqrt(K) * 2.0**-24 + common, 2.0**-15)),
            ("live side measured", share(ea.max() + worst * nbn + np.sqrt(K) * 2.0**-24 + common, 2.0**-15)),
            ("+ query side measured", share(ea.max() + eb + common, 2.0**-15)),
            ("+ c(K = 64)", share(ea.max() + eb + common, 2.0**-18 * (1 + 2.0**-9)))]
    out = {"what": "share of proposals whose exact minimum distance lies in the band; model of scripts/band_model.py",
           "n_live": N, "d": D, "proposals": P, "sigma": sigma, "sigma_r": sr, "zeta_assumed": ZETA, "namax": namax,
           "ea_max_over_2^-11_namax": float(ea.max() / (2.0**-11 * namax)),
           "eb_over_2^-11_nbn": {"mean": float((eb / (2.0**-11 * nbn)).mean()), "max": float((eb / (2.0**-11 * nbn)).max())},
           "rows": [{"bound": name, "uncertain_share": s, "ratio": s / rows[0][1]} for name, s in rows]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
