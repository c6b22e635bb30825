"""TEST INFRASTRUCTURE -- numpy restatement of one whole device step of PopulationSliceSampler's resident walkers
(csrc/mlf_walk.hip, csrc/mlf_walk_api.hip: mlf_walkers_step_dev / _step_graph / _step_user, and mlf_walkers_rounds_dev;
reference ultranest/popstepsampler.py:443-697 and ultranest/stepfuncs.pyx:99-334).  A plain module: it imports nothing of
ultranest_amd.

The state is a dict with the keys of _Walkers.export() (allu, allL, generation, currentt, currentv, current_left,
current_right, searching_left, searching_right; optionally currentp) plus the ring index, which travels beside it.

Counter layout of one call (seed, offset; P walkers, d dimensions, npairs = (d + 1) // 2):
  stream 4  restart of walker i: blocks offset + 64 i + attempt, attempt < 64; the four words of a block in order, each
            through below(word, nlive); the first candidate with Ls > Lmin (strictly) wins; after 256 candidates the first
            live row with Ls > Lmin in index order; none: the walker stays unstarted
  stream 2  direction of walker i: block group i of (npairs + 2) blocks (randomwalk_reference.directions with nsteps = 1)
  stream 3  slice uniform of walker i: block offset + i, words 0 and 1
  next offset = offset + P * max(npairs + 2, 64); round r of a several-rounds call draws at offset + r * that stride
"""
import numpy as np

import loglike_reference as LR
import randomwalk_reference as RW
from oracle import philox

KEYS = ("allu", "allL", "generation", "currentt", "currentv", "current_left", "current_right", "searching_left",
        "searching_right")


def per_call(P, d):
    """Philox counters one whole step (one round) consumes"""
    return P * max((d + 1) // 2 + 2, 64)


def next_offset(offset, P, d, rounds=1):
    return offset + rounds * per_call(P, d)


def fresh_state(P, nsteps, d):
    """the state after mlf_walkers_create / mlf_walkers_reset"""
    G = nsteps + 1
    return dict(allu=np.full((P, G, d), np.nan), allL=np.full((P, G), np.nan), generation=np.full(P, -1, dtype=np.int64),
                currentt=np.full(P, np.nan), currentv=np.full((P, d), np.nan), current_left=np.zeros(P),
                current_right=np.zeros(P), searching_left=np.zeros(P, dtype=bool), searching_right=np.zeros(P, dtype=bool),
                currentp=np.full((P, d), np.nan))


def copy_state(state):
    s = {k: np.array(state[k]) for k in KEYS}
    s["searching_left"] = s["searching_left"].astype(bool)
    s["searching_right"] = s["searching_right"].astype(bool)
    P, d = s["currentv"].shape
    s["currentp"] = np.array(state["currentp"]) if state.get("currentp") is not None else np.full((P, d), np.nan)
    return s


# ---- models ----------------------------------------------------------------------------------------------------------
def builtin_transform(tspec):
    """the built-in prior transform (kind, a, b) in binary64, each operation rounded: 0 identity, 1 x * a + b, 2 (x * a) * b"""
    kind, a, b = tspec

    def transform(x):
        x = np.asarray(x, dtype=np.float64)
        if kind == 1:
            return x * a + b
        if kind == 2:
            return (x * a) * b
        return x.copy()
    return transform


def reference_loglike(kind, centers=None, sigma=None):
    """p -> (L, band): the high-precision likelihood of loglike_reference (long double, or mpmath rounded to binary64 where
    the platform has no extended long double) and the band RTOL * scale(x) inside which two correct binary64 evaluations
    may disagree"""
    def loglike(p):
        p = np.asarray(p, dtype=np.float64)
        if len(p) == 0:
            return np.empty(0), np.empty(0)
        if LR.HAVE_LONGDOUBLE:
            L = LR.ref_longdouble(kind, p, centers, sigma)
        else:
            L = np.array([float(v) for v in LR.ref_mpmath(kind, p, centers, sigma)])
        return L, LR.RTOL * LR.scale(kind, p, centers, sigma, L) + LR.ATOL[kind]
    return loglike


def binary64_loglike(fn):
    """a numpy callback as a model of the restatement: no band"""
    def loglike(p):
        L = np.asarray(fn(p), dtype=np.float64)
        return L, np.zeros(len(L))
    return loglike


# ---- the stages ------------------------------------------------------------------------------------------------------
def step_back(state, Lmin):
    """stage 1, per walker over all G slots (a NaN slot is never below the threshold): chain slots go from the end until no
    below-threshold entry is left"""
    allL, gen, t = state["allL"], state["generation"], state["currentt"]
    G = allL.shape[1]
    with np.errstate(invalid="ignore"):
        nbelow = (allL < Lmin).sum(axis=1)
    for i in np.flatnonzero(nbelow):
        nb = int(nbelow[i])
        while nb > 0:
            g = int(gen[i])
            if g < 0 or g >= G:
                break
            gen[i] = g - 1
            t[i] = np.nan
            if allL[i, g] < Lmin:
                nb -= 1
            allL[i, g] = np.nan


def restart_rows(seed, offset, walkers, Ls, Lmin):
    """stage 2's draw: (row, branch) per walker of `walkers`; row -1: no live point above the threshold; branch 0 = by
    rejection, 1 = the linear fallback, -1 = none"""
    Ls = np.asarray(Ls, dtype=np.float64)
    nlive = len(Ls)
    walkers = np.asarray(walkers, dtype=np.int64)
    row = np.full(len(walkers), -1, dtype=np.int64)
    branch = np.full(len(walkers), -1, dtype=np.int64)
    for attempt in range(64):
        open_ = np.flatnonzero(row < 0)
        if not len(open_):
            break
        ctr = np.uint64(offset) + walkers[open_].astype(np.uint64) * np.uint64(64) + np.uint64(attempt)
        cand = RW.below(philox.blocks(seed, 4, ctr), nlive)          # (n, 4)
        ok = Ls[cand] > Lmin
        first = np.argmax(ok, axis=1)
        hit = ok.any(axis=1)
        row[open_[hit]] = cand[hit, first[hit]]
        branch[open_[hit]] = 0
    open_ = np.flatnonzero(row < 0)
    above = np.flatnonzero(Ls > Lmin)
    if len(open_) and len(above):
        row[open_] = above[0]
        branch[open_] = 1
    return row, branch


def slice_uniforms(seed, offset, P):
    w = philox.blocks(seed, 3, np.uint64(offset) + np.arange(P, dtype=np.uint64))
    return philox.u01(w[:, 0], w[:, 1])


def _round(state, seed, offset, Lmin, scale, kind, dirscale, live, Ls, transform, loglike, whiten=None, r2=None, axes=None,
           std=None, v_override=None):
    """stages 1-6 of one round for every walker, in place; returns what the round did"""
    P, G, d = state["allu"].shape
    live, Ls = np.asarray(live, dtype=np.float64), np.asarray(Ls, dtype=np.float64)
    gen, t = state["generation"], state["currentt"]
    left, right, sl, sr = state["current_left"], state["current_right"], state["searching_left"], state["searching_right"]
    step_back(state, Lmin)
    # 2. restarts
    was_starting = gen < 0
    idx = np.flatnonzero(was_starting)
    start = np.full(P, -1, dtype=np.int64)
    branch = np.full(P, -1, dtype=np.int64)
    if len(idx):
        start[idx], branch[idx] = restart_rows(seed, offset, idx, Ls, Lmin)
        got = idx[start[idx] >= 0]
        state["allu"][got, 0] = live[start[got]]
        state["allL"][got, 0] = Ls[start[got]]
        gen[got] = 0
    # 3. new slices (every walker whose slice coordinate is not finite, started or not)
    newslice = ~np.isfinite(t)
    v_restated = None
    if newslice.any():
        v_restated = RW.directions(seed, offset, kind, dirscale, P, 1, 0, d, axes=axes, live=live, std=std)
        rows = v_restated if v_override is None else np.asarray(v_override, dtype=np.float64)
        state["currentv"][newslice] = rows[newslice]
        left[newslice], right[newslice] = -scale, scale
        sl[newslice] = sr[newslice] = True
        t[newslice] = 0.0
    # 4. proposal
    movable = np.logical_and(gen >= 0, gen < G - 1)
    bisecting = np.logical_and(movable, ~np.logical_or(sl, sr))
    unif = slice_uniforms(seed, offset, P)
    span = right - left
    scaled = span * unif
    t[bisecting] = (left + scaled)[bisecting]
    tuse = np.where(sl, left, np.where(sr, right, t))
    m = np.flatnonzero(movable)
    u0 = state["allu"][m, gen[m]]
    stepv = state["currentv"][m] * tuse[m][:, None]
    unew = np.full((P, d), np.nan)
    unew[m] = u0 + stepv
    acceptable = np.zeros(P, dtype=bool)
    with np.errstate(invalid="ignore"):
        acceptable[m] = np.logical_and(unew[m] > 0, unew[m] < 1).all(axis=1)
    # 5. transform and likelihood of the acceptable proposals
    pnew = np.full((P, d), np.nan)
    Lnew = np.full(P, np.nan, dtype=np.longdouble if LR.HAVE_LONGDOUBLE else np.float64)
    band = np.zeros(P)
    if acceptable.any():
        pnew[acceptable] = transform(unew[acceptable])
        L, b = loglike(pnew[acceptable])
        Lnew[acceptable] = L
        band[acceptable] = b
    with np.errstate(invalid="ignore"):
        hit = np.logical_and(acceptable, Lnew > Lmin)
        undecided = np.logical_and(acceptable, np.abs(Lnew - Lmin).astype(np.float64) <= band)
    # 6. evolve_update and advance
    sright = np.logical_and(~sl, sr)
    bis = ~np.logical_or(sl, sr)
    grow_l = np.logical_and(movable, np.logical_and(hit, sl))
    grow_r = np.logical_and(movable, np.logical_and(hit, sright))
    stop_l = np.logical_and(movable, np.logical_and(~hit, sl))
    stop_r = np.logical_and(movable, np.logical_and(~hit, sright))
    left[grow_l] *= 2
    right[grow_r] *= 2
    sl[stop_l] = False
    sr[stop_r] = False
    b = np.logical_and(movable, bis)
    neg = np.logical_and(b, t < 0)
    pos = np.logical_and(b, ~(t < 0))
    left[neg] = t[neg]
    right[pos] = t[pos]
    success = np.logical_and(b, hit)
    t[success] = np.nan
    s = np.flatnonzero(success)
    uorig = state["allu"][s, gen[s]]
    gen[s] += 1
    state["allu"][s, gen[s]] = unew[s]
    state["allL"][s, gen[s]] = Lnew[s].astype(np.float64)
    state["currentp"][s] = pnew[s]
    d2 = np.full(P, np.nan)
    if r2 is not None and len(s):
        d2[s] = ((whiten(uorig) - whiten(unew[s]))**2).sum(axis=1)
    return dict(was_starting=was_starting, start=start, branch=branch, newslice=newslice, v_restated=v_restated, movable=movable,
                bisecting=bisecting, unif=unif, tuse=tuse, unew=unew, acceptable=acceptable, pnew=pnew, Lnew=Lnew, band=band,
                hit=hit, undecided=undecided, success=success, slot=np.where(success, gen, -1), d2=d2)


def statistics(rnd, r2):
    """stage 7: (nc, nmovable, nsuccess, nfar, sumlog) of one round"""
    nfar, sumlog = 0.0, 0.0
    d2 = rnd["d2"][rnd["success"]]
    if r2 is not None and len(d2):
        nfar = float((d2 > r2).sum())
        sumlog = float(np.log(d2**0.5 / r2**0.5 + 1e-10).sum())
    return dict(nc=int(rnd["acceptable"].sum()), nmovable=int(rnd["movable"].sum()), nsuccess=int(rnd["success"].sum()), nfar=nfar,
                sumlog=sumlog)


def ring_shift(ring, was_starting):
    """setup_start's shift of the ring index as k_walk_harvest makes it: only when some but not all walkers were starting"""
    P = len(was_starting)
    n = int(was_starting.sum())
    if 0 < n < P:
        for _ in range(P):
            if not was_starting[ring]:
                break
            ring = (ring + 1) % P
    return ring


def harvest(state, ring):
    """stage 8 after the ring shift: the found test, the record, the clearing of the harvested walker, the next ring index"""
    P, G, d = state["allu"].shape
    found = bool(state["generation"][ring] == G - 1)
    rec = dict(found=found, L=np.nan, left=float(state["current_left"][ring]), right=float(state["current_right"][ring]), u=None,
               p=None, walker=ring)
    if found:
        rec["L"] = float(state["allL"][ring, G - 1])
        rec["u"] = state["allu"][ring, G - 1].copy()
        rec["p"] = state["currentp"][ring].copy()
        state["allu"][ring] = np.nan
        state["allL"][ring] = np.nan
        state["generation"][ring] = -1
        state["currentt"][ring] = np.nan
        ring = (ring + 1) % P
    rec["ring"] = ring
    return rec


def step(state, ring, seed, offset, Lmin, scale, kind, dirscale, live, Ls, transform, loglike, whiten=None, r2=None, axes=None,
         std=None, v_override=None):
    """One call of mlf_walkers_step_dev from `state` (not modified) and ring index `ring`.  transform: u rows -> p rows in
    binary64; loglike: p rows -> (L, band) (reference_loglike, binary64_loglike); whiten, r2: the layer of the move
    diagnostics (r2 None: no layer); v_override: (P, d) rows taken instead of the restated directions where a walker draws.
    Returns dict(state, record, next_offset, round): `record` has the fields of _Walkers._record, "walker" (the ring index
    the harvest looked at) and "ring" (the index after the call); `round` is what _round reports."""
    st = copy_state(state)
    P, G, d = st["allu"].shape
    rnd = _round(st, seed, offset, Lmin, scale, kind, dirscale, live, Ls, transform, loglike, whiten, r2, axes, std, v_override)
    stats = statistics(rnd, r2)
    rec = harvest(st, ring_shift(ring, rnd["was_starting"]))
    rec.update(stats)
    return dict(state=st, record=rec, next_offset=next_offset(offset, P, d), round=rnd)


def rounds(state, ring, seed, offset, Lmin, scale, kind, dirscale, live, Ls, transform, loglike, max_rounds, whiten=None,
           r2=None, axes=None, std=None):
    """One call of mlf_walkers_rounds_dev (max_rounds: its absolute value): round r draws at offset + r * per_call, the ring
    index is fixed after round 0, the ring walker stops when finished or at max_rounds (that gives R), everybody makes
    rounds 0 ... R - 1, one statistics row per round.  Returns dict(state, record (with "rounds"), rows, next_offset,
    rounds: the list of what each round did)."""
    st = copy_state(state)
    P, G, d = st["allu"].shape
    max_rounds = abs(int(max_rounds))
    stride = per_call(P, d)
    made, rows = [], []
    walker = ring
    for r in range(max_rounds):
        if r > 0 and st["generation"][walker] == G - 1:
            break
        rnd = _round(st, seed, offset + r * stride, Lmin, scale, kind, dirscale, live, Ls, transform, loglike, whiten, r2, axes, std)
        if r == 0:
            walker = ring_shift(ring, rnd["was_starting"])
        made.append(rnd)
        rows.append(statistics(rnd, r2))
    R = len(made)
    rec = harvest(st, walker)
    rec["rounds"] = R
    return dict(state=st, record=rec, rows=rows, next_offset=next_offset(offset, P, d, R), rounds=made)

