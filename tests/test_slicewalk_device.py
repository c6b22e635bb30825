"""PopulationSliceSampler's device steps (csrc/mlf_walk.hip, csrc/mlf_walk_api.hip) against the numpy restatement of a whole
step (tests/slicewalk_reference.py), call by call and teacher-forced: before every device call the resident state is
exported, after it again, the restatement makes that one call from the state before, and the two are compared -- start
rows, chain points, slice coordinates, brackets, flags, counts, the record, the ring index, the Philox offset and the number
of rounds bit for bit; likelihoods, Box-Muller directions and the move diagnostics within the bounds the project already
uses for them.  The cases (tests/test_slicewalk_restatement.py: CASES) cover mlf_walkers_step_dev and _step_graph
(alternating within a run), mlf_walkers_rounds_dev in its register and memory forms with the hand-shake launch and the
two-launch split, the wide form, mlf_walkers_step_user, and the restart edges.

A walker whose proposal lies within loglike_reference.RTOL * scale of the threshold is undecided: it is left out of that
call's comparison (at most 1 % of a case's evaluations, never the walker under the ring index; a case that breaks either
cap FAILS).  The free-running restatement meets both caps on its own (test_free_run_stays_within_the_caps).

Largest deviation / bound over all cases, as measured on the MI355X (every test prints its own; 0 of 0.9 million
walker-evaluations were undecided):
  directions of kind 2, 1e-12 dirscale                          2.8e-4 single steps (carry), 4.2e-4 rounds (two-launches-mem)
  directions of kind 4, 1e-12 dirscale |axes[r]|_2              4.3e-4 single steps (kind-4), 2.3e-4 rounds (wide-rounds-4)
  stored likelihoods, loglike_reference.RTOL * scale            1.0e-3 (hand-shake-1500; eggbox 9e-4, rosenbrock 4e-4, gauss 1e-5)
  nfar, within the successes with |d2 - r2| <= 1e-9 r2          equal in every call of every case (no such success occurred)
  sumlog, rtol = 1e-9, atol = 1e-9                              9.2e-6 (kind-0)
  allu in rounds with kinds 2 and 4, sum |t| * direction bound  0.32 (two-launches-mem); 0.016 and below in the other three
The last bound has no term for the rounding of u + v * t itself (half an ulp of a coordinate, 5.6e-17 near 0.5), which is what
fills it where a bisected slice has shrunk to |t| of order 1e-4: the direction's own share is the 4e-4 of the rows above.
"""
import numpy as np
import pytest

import slicewalk_reference as S
import test_slicewalk_restatement as T

pytestmark = pytest.mark.gpu

G = T.NSTEPS + 1


def _walkers(case, prob):
    """A population handle with the region's copies and the live points on the device, as __next__ sets it up."""
    import ultranest_amd.popstepsampler as pop
    w = pop._Walkers(case.P, T.NSTEPS, case.d)
    pop._sync_region_copies(w, dict(region=None, layer=None, r2=None, calls=0), prob.region, case.d, case.kind, skip_live=True)
    w.set_live(prob.us, prob.Ls)
    return w


def _direction_bound(case, prob):
    """per coordinate: kind 2: 1e-12 dirscale; kind 4: 1e-12 dirscale |axes[r]|_2 (tests/test_wide_walk_gpu.py); else exact"""
    if case.kind == 2:
        return np.full(case.d, 1e-12 * case.dirscale)
    if case.kind == 4:
        return 1e-12 * case.dirscale * np.linalg.norm(prob.axes, axis=1)
    return np.zeros(case.d)


def _note(ratios, name, dev, bound):
    dev, bound = np.asarray(dev, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    if dev.size == 0:
        return
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(dev == 0, 0.0, dev / bound)
    ratios[name] = max(ratios.get(name, 0.0), float(np.nanmax(ratio)))


def _same(a, b, what):
    assert np.array_equal(a, b, equal_nan=True), what


def _within(got, want, bound, what, ratios, name):
    """NaN where the other has NaN, and |got - want| <= bound elsewhere (bound 0: equal)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bound = np.broadcast_to(bound, got.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    dev = np.abs(got[ok] - want[ok])
    loose = bound[ok] > 0
    _note(ratios, name, dev[loose], bound[ok][loose])
    assert (dev <= bound[ok]).all(), (what, float(dev.max()), int(np.argmax(dev - bound[ok])))


def _compare(case, prob, call, before, after, rec, rows, want, ratios, tally):
    """One call: the device's state after it, its record and its statistics rows (one per round) against the restatement's."""
    P, d = case.P, case.d
    rounds = T.rounds_of(want)
    ws, wrec = want["state"], want["record"]
    where = "%s call %d" % (case.id, call)
    dirb = _direction_bound(case, prob)
    single = case.mode != "rounds"
    # what this call wrote, and how far the device may be from it
    excluded = np.zeros(P, dtype=bool)
    drew = np.zeros(P, dtype=bool)
    uerr = np.zeros((P, d))
    ubound, Lbound = np.zeros((P, G, d)), np.zeros((P, G))
    for r, rnd in enumerate(rounds):
        excluded |= rnd["undecided"]
        tally["evaluations"] += int(rnd["acceptable"].sum())
        drew |= rnd["newslice"]
        if r == 0:
            uerr[rnd["was_starting"]] = 0
        s = np.flatnonzero(rnd["success"])
        if not single:      # (a single step takes the device's own direction rows: exact from there on)
            uerr[s] += np.abs(rnd["tuse"][s])[:, None] * dirb[None, :] * drew[s][:, None]
        ubound[s, rnd["slot"][s]] = uerr[s]
        Lbound[s, rnd["slot"][s]] = rnd["band"][s]
    tally["excluded"] += int(sum(rnd["undecided"].sum() for rnd in rounds))
    walker = wrec["walker"]
    assert not excluded[walker], "%s: the walker under the ring index (%d) is undecided: |Lref - Lmin| within the band %g" % (
        where, walker, max(float(rnd["band"][walker]) for rnd in rounds))
    keep = ~excluded
    clean = not excluded.any()

    # directions
    if single and case.kind in (2, 4):
        new = rounds[0]["newslice"]
        if new.any():
            dev = np.abs(after["currentv"][new] - rounds[0]["v_restated"][new])
            _note(ratios, "direction kind %d" % case.kind, dev, np.broadcast_to(dirb, dev.shape))
            assert (dev <= dirb).all(), (where, "direction", float((dev / dirb).max()))
        _same(after["currentv"], ws["currentv"], where + " currentv")
    else:
        _within(after["currentv"], ws["currentv"], drew[:, None] * dirb[None, :], where + " currentv", ratios,
                "direction kind %d (rounds)" % case.kind)
    # the discrete state and the slice
    for key in ("generation", "currentt", "current_left", "current_right", "searching_left", "searching_right"):
        _same(np.asarray(after[key])[keep], np.asarray(ws[key])[keep], "%s %s" % (where, key))
    # chain points: allu[g + 1] == allu[g] + currentv * t in binary64 (start rows among them)
    _within(after["allu"][keep], ws["allu"][keep], ubound[keep], where + " allu", ratios, "allu (rounds, kinds 2 and 4)")
    _within(after["allL"][keep], ws["allL"][keep], Lbound[keep], where + " allL", ratios, "stored likelihood")
    _same(after["allL"][keep, 0], ws["allL"][keep, 0], where + " likelihood of the start rows")

    # the record
    assert rec["found"] == wrec["found"] and rec["ring"] == wrec["ring"], (where, rec["found"], wrec["found"], rec["ring"], wrec["ring"])
    assert rec["left"] == wrec["left"] and rec["right"] == wrec["right"], where
    if wrec["found"]:
        _within(rec["u"], wrec["u"], ubound[walker, G - 1], where + " record u", ratios, "allu (rounds, kinds 2 and 4)")
        _within(rec["L"], wrec["L"], Lbound[walker, G - 1], where + " record L", ratios, "stored likelihood")
        _same(rec["p"], prob.transform(rec["u"][None, :])[0], where + " record p")
    else:
        assert np.isnan(rec["L"]), where
    # statistics, one row per round
    assert len(rows) == len(want_rows(want)), (where, len(rows), len(want_rows(want)))
    for r, (got, exp, rnd) in enumerate(zip(rows, want_rows(want), rounds)):
        assert got["nc"] == exp["nc"] and got["nmovable"] == exp["nmovable"], (where, r, got, exp)
        if not clean:
            continue
        assert got["nsuccess"] == exp["nsuccess"], (where, r, got, exp)
        if prob.r2 is None:
            assert got["nfar"] == 0 and got["sumlog"] == 0, (where, r, got)
            continue
        d2 = rnd["d2"][rnd["success"]]
        close = int((np.abs(d2 - prob.r2) <= 1e-9 * prob.r2).sum())
        assert abs(got["nfar"] - exp["nfar"]) <= close, (where, r, got["nfar"], exp["nfar"], close)
        tally["nfar off"] = max(tally["nfar off"], abs(got["nfar"] - exp["nfar"]))
        tol = 1e-9 + 1e-9 * abs(exp["sumlog"])
        _note(ratios, "sumlog", abs(got["sumlog"] - exp["sumlog"]), tol)
        assert np.isclose(got["sumlog"], exp["sumlog"], rtol=1e-9, atol=1e-9), (where, r, got["sumlog"], exp["sumlog"])


def want_rows(want):
    return want["rows"] if "rows" in want else [want["record"]]


def _drive(case):
    from ultranest_amd.regions import DeviceRNG
    prob = T.problem(case)
    w = _walkers(case, prob)
    rng = DeviceRNG(case.seed)
    rng.offset = case.offset
    model = None
    if case.mode == "user":
        from ultranest_amd import usermodels
        assert np.array_equal(usermodels.gauss_centers(case.d), T.gauss_centers(case.d))
        model = usermodels.gauss(case.d)
    args = T.model_args(case, prob)
    ring, scale, nfound = 0, case.scale, 0
    ratios, tally = {}, {"evaluations": 0, "excluded": 0, "nfar off": 0.0, "capped": 0, "rounds": 0}
    for call in range(case.ncalls):
        Lmin = T.threshold(case, prob, call, nfound)
        before, offset = w.export(), rng.offset
        if case.mode == "rounds":
            rec, table = w.rounds_dev(Lmin, scale, case.kind, case.dirscale, rng, prob.tspec, prob.lspec, case.max_rounds)
            rows = [dict(nc=int(t[0]), nmovable=int(t[1]), nsuccess=int(t[2]), nfar=t[3], sumlog=t[4]) for t in table]
            want = S.rounds(before, ring, case.seed, offset, Lmin, scale, case.kind, case.dirscale, max_rounds=case.max_rounds, **args)
            assert rec["rounds"] == want["record"]["rounds"], (case.id, call, rec["rounds"], want["record"]["rounds"])
            tally["rounds"] += rec["rounds"]
            tally["capped"] += int(rec["rounds"] == abs(case.max_rounds) and not rec["found"])
        else:
            if case.mode == "user":
                rec = w.step_user(Lmin, scale, case.kind, case.dirscale, rng, model, True)
            else:       # kernel by kernel and graph replay, both ways round and each twice in a row
                rec = w.step_dev(Lmin, scale, case.kind, case.dirscale, rng, prob.tspec, prob.lspec, graph=call % 4 in (1, 2))
            rows = [rec]
        after = w.export()
        if case.mode != "rounds":
            override = after["currentv"] if case.kind in (2, 4) else None
            want = S.step(before, ring, case.seed, offset, Lmin, scale, case.kind, case.dirscale, v_override=override, **args)
        assert rng.offset == want["next_offset"], (case.id, call, rng.offset, want["next_offset"])
        _compare(case, prob, call, before, after, rec, rows, want, ratios, tally)
        if rec["found"]:
            nfound += 1
            scale = scale * 0.9 + 0.1 * (rec["right"] - rec["left"]) / 2
        ring = rec["ring"]
    assert tally["excluded"] <= 0.01 * tally["evaluations"], "%s: %d of %d walker-evaluations are undecided" % (
        case.id, tally["excluded"], tally["evaluations"])
    for name in sorted(ratios):
        print("%s: %s: largest deviation / bound = %.3g" % (case.id, name, ratios[name]))
    print("%s: %d evaluations, %d excluded, %d found, nfar off by at most %g" % (
        case.id, tally["evaluations"], tally["excluded"], nfound, tally["nfar off"]))
    return nfound, tally


@pytest.mark.parametrize("case", T.SINGLE, ids=[c.id for c in T.SINGLE])
def test_single_steps(case):
    """mlf_walkers_step_dev and mlf_walkers_step_graph, alternating: every call against the restatement"""
    nfound, tally = _drive(case)
    if case.schedule in ("rising", "jump"):
        assert nfound >= 10


@pytest.mark.parametrize("case", T.ROUNDS, ids=[c.id for c in T.ROUNDS])
def test_rounds(case):
    """mlf_walkers_rounds_dev: the number of rounds, the per-round statistics rows, the record and the state of every call"""
    nfound, tally = _drive(case)
    assert nfound >= 10 and tally["rounds"] > case.ncalls
    if case.id == "cap":
        assert tally["capped"] > 0


@pytest.mark.parametrize("case", T.USER, ids=[c.id for c in T.USER])
def test_user_model(case):
    """usermodels.gauss through mlf_walkers_step_user against the same restatement with the Gaussian reference"""
    nfound, tally = _drive(case)
    assert nfound >= 10
