"""The stateless step-function kernels (csrc/mlf_walk.hip: k_slice_update, k_line_intersection, k_evolve_*, k_step_back /
k_max_generation, k_within_unit_cube, k_row_dist2) past the sizes of the recorded vectors (test_stepfuncs_golden.py), against
``oracle.stepfuncs``, which those vectors pin bit for bit: the second point tile, the second worker tile and the carry of
k_slice_update's prefix sum (popsize > 1024), worker lists in the kernel's own round-robin order and in random order, rows of
1024 coordinates, more than one workgroup, and planted edge values.  Inputs come from the seeded generators below.

``impl`` = the HIP kernels (`-m gpu`), compared with the oracle bit for bit (NaN = NaN, -0.0 != 0.0; row_dist2 within its
derived bound of np.longdouble), or the oracle itself, compared with the plain restatements at the end of this module -- the
self-check of the generators and of the oracle at the new shapes, which runs everywhere together with the assertions that
every case holds what it was built to hold."""
import numpy as np
import pytest

from golden import inputs
from oracle import stepfuncs as O

import loglike_reference as LR


@pytest.fixture(params=["oracle", pytest.param("hip", marks=pytest.mark.gpu)])
def impl(request):
    if request.param == "oracle":
        return O
    import ultranest_amd.stepfuncs as mod
    return mod


def same_bits(a, b):
    """equal bit for bit; any NaN equals any NaN (x86 and the GPU give 0 * inf different sign bits)"""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a, b))
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan]))


def copies(case, *names):
    return [np.array(case[k]) for k in names]


# ------------------------------------------------------------------------------------------------ update_vectorised_slice_sampler
POPSIZES = (1, 63, 1023, 1024, 1025, 2049, 3000)
ORDERS = ("sorted", "round-robin", "permuted")
SLICE_OUT = ("tleft", "tright", "worker_running", "status", "allu", "allL", "allp", "discarded")


def busy_counts(popsize):
    """one unfinished point, a few, a third, every point"""
    return sorted({1, min(popsize, 5), max(1, popsize // 3), popsize})


def slice_case(seed, popsize, d, nparams, nbusy, order):
    """inputs.slice_update_inputs with the worker list in one of three orders, an eighth of the workers aimed at finished
    points (not in the round-robin order, which is the kernel's own and holds unfinished points only) and planted edges, each
    on the FIRST worker of a point of its own so that it meets the interval as generated:
        t == tleft, t == tright, t == 0 (no shrinking, all inside), proposed_L == threshold (not accepted, not discarded),
        two accepting workers of one point (t = +0.05, then -0.05: the second stays inside the shrunk interval)"""
    rs = np.random.RandomState(seed)
    status = np.ones(popsize, dtype=np.int64)
    busy = np.sort(rs.choice(popsize, size=nbusy, replace=False))
    status[busy] = 0
    if order == "round-robin":
        worker_running = busy[np.arange(popsize) % nbusy]
    else:
        worker_running = busy[rs.randint(nbusy, size=popsize)]
        done = np.flatnonzero(status == 1)
        if len(done):
            stray = rs.uniform(size=popsize) < 0.125
            worker_running[stray] = done[rs.randint(len(done), size=int(stray.sum()))]
        worker_running = np.sort(worker_running) if order == "sorted" else rs.permutation(worker_running)
    worker_running = worker_running.astype(np.int64)
    c = dict(worker_running=worker_running, status=status, threshold=0.2, planted={})
    c["tleft"], c["tright"] = -rs.uniform(0.2, 1.0, size=popsize), rs.uniform(0.2, 1.0, size=popsize)
    c["t"] = rs.uniform(-1.1, 1.1, size=popsize)
    c["proposed_L"] = rs.normal(size=popsize)
    c["proposed_u"], c["proposed_p"] = rs.uniform(size=(popsize, d)), rs.normal(size=(popsize, nparams))
    c["allu"], c["allL"], c["allp"] = rs.uniform(size=(popsize, d)), rs.normal(size=popsize), rs.normal(size=(popsize, nparams))
    # first worker of every point that has one, and the second one of the unfinished points
    order_of = np.argsort(worker_running, kind="stable")
    pts, start, count = np.unique(worker_running[order_of], return_index=True, return_counts=True)
    first = dict(zip(pts.tolist(), order_of[start].tolist()))
    twice = [int(p) for p, n in zip(pts, count) if n >= 2 and status[p] == 0]
    free = [int(p) for p in rs.permutation(pts) if status[p] == 0]
    if twice:
        p = twice[rs.randint(len(twice))]
        free.remove(p)
        l1, l2 = (int(l) for l in np.sort(order_of[start[pts == p][0]:][:2]))
        c["t"][[l1, l2]] = 0.05, -0.05
        c["proposed_L"][[l1, l2]] = 1.0, 2.0
        c["planted"]["twice"] = (p, l1, l2)
    for name in ("at_left", "at_right", "at_zero", "at_threshold"):
        if not free:
            break
        p = free.pop()
        l = first[p]
        if name == "at_left":
            c["t"][l] = c["tleft"][p]
        elif name == "at_right":
            c["t"][l] = c["tright"][p]
        elif name == "at_zero":
            c["t"][l] = 0.0
        else:
            c["t"][l], c["proposed_L"][l] = 0.01, c["threshold"]
        c["planted"][name] = (p, l)
    return c


def slice_call(mod, c, shrink):
    a = {k: np.array(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    return mod.update_vectorised_slice_sampler(a["t"], a["tleft"], a["tright"], a["proposed_L"], a["proposed_u"], a["proposed_p"],
                                               a["worker_running"], a["status"], c["threshold"], shrink, a["allu"], a["allL"],
                                               a["allp"], len(a["t"]))


def slice_next(c, out, seed):
    """the state one call left (its own round-robin worker list among it) with a fresh batch of evaluated workers"""
    rs = np.random.RandomState(seed)
    n, d, nparams = len(c["t"]), c["allu"].shape[1], c["allp"].shape[1]
    nxt = dict(zip(SLICE_OUT[:7], (np.array(a) for a in out[:7])), threshold=c["threshold"])
    nxt["t"] = rs.uniform(-0.6, 0.6, size=n)
    nxt["proposed_L"] = rs.normal(size=n)
    nxt["proposed_u"], nxt["proposed_p"] = rs.uniform(size=(n, d)), rs.normal(size=(n, nparams))
    return nxt


def slice_cases(popsize, d, nparams):
    for nbusy in busy_counts(popsize):
        for k, order in enumerate(ORDERS):
            yield nbusy, order, slice_case(7000 + 13 * popsize + 3 * nbusy + k, popsize, d, nparams, nbusy, order)


def check_slice(impl, popsize, d, nparams, shrink):
    ncalls = 0
    for nbusy, order, c in slice_cases(popsize, d, nparams):
        for call in range(2):
            want = slice_update_plain(c, shrink) if impl is O else slice_call(O, c, shrink)
            got = slice_call(impl, c, shrink)
            for name, g, w in zip(SLICE_OUT, got, want):
                assert same_bits(g, w) if name != "discarded" else g == w, (popsize, nbusy, order, call, name)
            if call == 0:
                c = slice_next(c, want, 9000 + popsize + nbusy)
            ncalls += 1
    return ncalls


@pytest.mark.parametrize("shrink", [1.0, 1.5])
@pytest.mark.parametrize("popsize", POPSIZES)
def test_update_vectorised_slice_sampler(impl, popsize, shrink):
    """all eight outputs, then a second call on the outputs of the first"""
    n = check_slice(impl, popsize, 3, 4, shrink)
    print("slice update popsize=%d shrink=%g: %d calls compared bit for bit" % (popsize, shrink, n))


@pytest.mark.parametrize("shrink", [1.0, 1.5])
def test_update_vectorised_slice_sampler_in_one_dimension(impl, shrink):
    check_slice(impl, 1025, 1, 1, shrink)


def test_slice_cases_hold_what_they_were_built_for():
    c = slice_case(1, 3000, 3, 4, 1000, "permuted")
    w, st = c["worker_running"], c["status"]
    assert (np.diff(w) < 0).any() and (st[w] == 1).any() and (st[w] == 0).any()
    assert set(c["planted"]) == {"twice", "at_left", "at_right", "at_zero", "at_threshold"}
    # both point tiles and both worker tiles beyond the first are reached, by workers that are accepted there
    busy = np.flatnonzero(st == 0)
    assert (busy < 1024).any() and ((busy >= 1024) & (busy < 2048)).any() and (busy >= 2048).any()
    out = dict(zip(SLICE_OUT, slice_call(O, c, 1.5)))
    taken = np.flatnonzero((st == 0) & (out["status"] == 1))
    assert (taken >= 2048).any() and (taken < 1024).any() and out["discarded"] > 0
    took = {int(p): int(np.flatnonzero(c["proposed_L"] == out["allL"][p])[0]) for p in taken}
    assert max(took.values()) >= 2048 and min(took.values()) < 1024
    # the prefix sum carries a total into its second and third chunk, and the list it deals out is not sorted
    left = np.flatnonzero(out["status"] == 0)
    assert (left < 1024).sum() > 0 and (left >= 2048).sum() > 0
    assert same_bits(out["worker_running"], left[np.arange(3000) % len(left)])
    p, l1, l2 = c["planted"]["twice"]
    assert l1 < l2 and out["allL"][p] == 1.0 and same_bits(out["allu"][p], c["proposed_u"][l1])
    assert 0 < out["tright"][p] <= 0.05 / 1.5 and 0 > out["tleft"][p] >= -0.05 / 1.5       # (later workers may shrink it further)
    p, l = c["planted"]["at_threshold"]
    assert out["allL"][p] != c["threshold"] and 0 < out["tright"][p] <= 0.01 / 1.5
    for name, side in (("at_left", "tleft"), ("at_right", "tright")):
        p, l = c["planted"][name]
        assert c["t"][l] == c[side][p] == out[side][p] or (w == p).sum() > 1
    # every point unfinished: as many points as workers; one point unfinished: its workers and the strays
    assert len(np.unique(slice_case(2, 1025, 3, 4, 1025, "round-robin")["worker_running"])) == 1025
    one = slice_case(3, 1025, 3, 4, 1, "sorted")
    assert (one["status"] == 0).sum() == 1 and (one["status"][one["worker_running"]] == 0).sum() > 800


# ------------------------------------------------------------------------------------------------ unitcube_line_intersection
LINE_KINDS = 8


def line_case(seed, n, d):
    """row i is of kind (i + seed) % 8:  0 plain;  1 zero and negative-zero components;  2 a single non-zero component;
    3 origin components on faces;  4 origin in a corner;  5 origin 0.5 under zero components (0 * inf = NaN, skipped);
    6 components of +-1e-300;  7 no direction at all under an origin of 0.5 (nothing but NaN: the result is NaN) -- not in a
    batch of one row, whose direction the wrapper refuses"""
    rs = np.random.RandomState(seed)
    o, v = rs.uniform(size=(n, d)), rs.normal(size=(n, d))
    kind = (np.arange(n) + seed) % LINE_KINDS if n > 1 else np.array([seed % (LINE_KINDS - 1)])
    for i, k in enumerate(kind):
        col = rs.randint(d)
        pick = rs.uniform(size=d) < 0.4
        if k == 1:
            v[i, pick] = np.where(rs.uniform(size=int(pick.sum())) < 0.5, 0.0, -0.0)
            v[i, col] = 0.7
        elif k == 2:
            v[i] = 0.0
            v[i, col] = -1.3
        elif k == 3:
            o[i, pick] = rs.randint(2, size=int(pick.sum()))
        elif k == 4:
            o[i] = rs.randint(2, size=d)
        elif k == 5:
            pick[col] = False
            v[i, pick], o[i, pick] = 0.0, 0.5
        elif k == 6:
            pick[col] = False
            v[i, pick] = np.where(rs.uniform(size=int(pick.sum())) < 0.5, 1e-300, -1e-300)
        elif k == 7:
            v[i], o[i] = 0.0, 0.5
    return o, v, kind


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("d", [1, 2, 128, 129, 1024])
def test_unitcube_line_intersection(impl, d, n):
    for seed in range(811, 811 + (LINE_KINDS - 1 if n == 1 else 1)):
        o, v, kind = line_case(seed, n, d)
        want = line_intersection_plain(o, v) if impl is O else O.unitcube_line_intersection(o, v)
        got = impl.unitcube_line_intersection(o, v)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        if n > 1:
            assert np.isnan(got[0][kind == 7]).all() and np.isnan(got[1][kind == 7]).all()
            assert np.isfinite(got[0][kind != 7]).all() and np.isfinite(got[1][kind != 7]).all()
    print("line intersection d=%d n=%d: %d rows compared bit for bit" % (d, n, n))


def test_line_cases_hold_what_they_were_built_for():
    o, v, kind = line_case(5, 257, 129)
    assert set(kind) == set(range(LINE_KINDS))
    assert ((v == 0) & np.signbit(v)).any() and ((v == 0) & ~np.signbit(v)).any() and (np.abs(v) == 1e-300).any()
    assert ((v != 0).sum(axis=1) == 1).any() and ((o == 0) | (o == 1)).all(axis=1).any()
    assert ((v == 0) & (o == 0.5)).any(axis=1)[kind == 5].all()
    lo, hi = O.unitcube_line_intersection(o, v)
    inner = kind == 0
    assert (lo[inner] < 0).all() and (hi[inner] > 0).all()


# ------------------------------------------------------------------------------------------------ evolve_update, evolve
WALKERS = (1, 255, 256, 257, 1025)


def update_case(seed, n, mode):
    """every pair of searching flags with hit and miss; Lnew == Lmin; currentt 0.0 and -0.0 (a bisecting walker puts either
    into current_right: -0.0 < 0 is false, and the sign must survive); mode: "mixed", "nobody" or "everybody" acceptable"""
    rs = np.random.RandomState(seed)
    c = dict(Lmin=-0.3)
    state = (np.arange(n) + seed) % 4            # 0 both, 1 right only, 2 bisecting, 3 left only
    c["searching_left"], c["searching_right"] = np.logical_or(state == 0, state == 3), np.logical_or(state == 0, state == 1)
    c["current_left"], c["current_right"] = -rs.uniform(0.01, 2.0, size=n), rs.uniform(0.01, 2.0, size=n)
    c["currentt"] = rs.uniform(-1, 1, size=n)
    zero = rs.uniform(size=n) < 0.2
    c["currentt"][zero] = np.where(rs.uniform(size=int(zero.sum())) < 0.5, 0.0, -0.0)
    c["acceptable"] = {"mixed": ((np.arange(n) + seed) // 4) % 2 == 0, "nobody": np.zeros(n, dtype=bool), "everybody": np.ones(n, dtype=bool)}[mode]
    L = rs.normal(size=n) if mode == "mixed" else c["Lmin"] + rs.uniform(0.1, 1.0, size=n)
    if mode == "mixed":
        L[((np.arange(n) + seed) // 8) % 3 == 0] = c["Lmin"]
    c["Lnew"] = L[c["acceptable"]]
    return c


def update_call(mod, c):
    s = dict(zip(("currentt", "current_left", "current_right", "searching_left", "searching_right"),
                 copies(c, "currentt", "current_left", "current_right", "searching_left", "searching_right")))
    search_right, bisecting = mod.evolve_prepare(s["searching_left"], s["searching_right"])
    success = np.zeros(len(s["currentt"]), dtype=bool)
    mod.evolve_update(c["acceptable"], c["Lnew"], c["Lmin"], search_right, bisecting, s["currentt"], s["current_left"],
                      s["current_right"], s["searching_left"], s["searching_right"], success)
    return [s["currentt"], s["current_left"], s["current_right"], s["searching_left"], s["searching_right"], success]


@pytest.mark.parametrize("mode", ["mixed", "nobody", "everybody"])
@pytest.mark.parametrize("n", WALKERS)
def test_evolve_update(impl, n, mode):
    for seed in range(821, 821 + (32 if n == 1 and mode == "mixed" else 1)):       # one walker: every combination in turn
        c = update_case(seed, n, mode)
        want = evolve_update_plain(c) if impl is O else update_call(O, c)
        for name, g, w in zip(("t", "left", "right", "sl", "sr", "success"), update_call(impl, c), want):
            assert same_bits(g, w), (n, mode, seed, name)


def test_update_cases_hold_what_they_were_built_for():
    c = update_case(1, 257, "mixed")
    full = np.full(257, np.nan)
    full[c["acceptable"]] = c["Lnew"]
    seen = {(bool(l), bool(r), bool(a), "eq" if L == c["Lmin"] else bool(L > c["Lmin"]))
            for l, r, a, L in zip(c["searching_left"], c["searching_right"], c["acceptable"], full)}
    for l in (False, True):
        for r in (False, True):
            assert {(l, r, True, True), (l, r, True, False), (l, r, True, "eq"), (l, r, False, False)} <= seen
    bis = ~(c["searching_left"] | c["searching_right"])
    t = c["currentt"][bis]
    assert ((t == 0) & np.signbit(t)).any() and ((t == 0) & ~np.signbit(t)).any()
    out = update_call(O, c)
    assert ((out[2] == 0) & np.signbit(out[2])).any()       # -0.0 arrived in current_right with its sign
    assert len(update_case(1, 257, "nobody")["Lnew"]) == 0 and update_call(O, update_case(1, 257, "everybody"))[5].any()


def evolve_call(mod, seed, n, d):
    s = inputs.walker_state(seed, n, d)
    s["currentt"][::5] = np.where(np.arange(len(s["currentt"][::5])) % 2 == 0, 0.0, -0.0)
    np.random.seed(seed)
    args = [s[key] for key in ("currentu", "currentL", "currentt", "currentv", "current_left", "current_right",
                               "searching_left", "searching_right")]
    (t, v, lo, hi, sl, sr), (success, unew, pnew, Lnew), nc = mod.evolve(inputs.walker_transform, inputs.walker_loglike, s["Lmin"], *args)
    return [t, v, lo, hi, sl, sr, success, unew, pnew, Lnew, args[0], np.int64(nc), np.float64(np.random.uniform())]


@pytest.mark.parametrize("d", [1, 129])
@pytest.mark.parametrize("n", WALKERS)
def test_evolve(impl, n, d):
    """state, accepted points, number of calls and the position of the numpy stream afterwards"""
    if impl is O:
        got, want = evolve_call(O, 830 + n, n, d), evolve_plain(830 + n, n, d)
    else:
        got, want = evolve_call(impl, 830 + n, n, d), evolve_call(O, 830 + n, n, d)
    names = ("t", "v", "left", "right", "sl", "sr", "success", "unew", "pnew", "Lnew", "currentu", "nc", "next_random")
    for name, g, w in zip(names, got, want):
        assert (g.size == 0 and w.size == 0 and g.shape[1:] == w.shape[1:]) or same_bits(g, w), (n, d, name)


# ------------------------------------------------------------------------------------------------ step_back
BACK_SIZES = ((1, 1), (255, 2), (257, 64), (1025, 7))


def back_case(seed, n, ngen, all_minus_one=False):
    """the states the sampler produces: allL[i] finite or infinite up to generation[i] and NaN behind it, so that no chain
    unwinds below generation 0 with entries left (where the kernel documents that it differs from numpy's negative indexing);
    entries equal to Lmin (not below it) and infinities of both signs among them"""
    rs = np.random.RandomState(seed)
    Lmin = 0.1
    generation = rs.randint(-1, ngen, size=n).astype(np.int64)
    if n > 1:
        generation[rs.randint(n)] = ngen - 1
    if all_minus_one:
        generation[:] = -1
    allL = np.full((n, ngen), np.nan)
    for i, g in enumerate(generation):
        row = rs.normal(size=g + 1) + 0.8
        special = rs.uniform(size=g + 1)
        row[special < 0.1] = Lmin
        row[(special >= 0.1) & (special < 0.14)] = np.inf
        row[(special >= 0.14) & (special < 0.18)] = -np.inf
        allL[i, :g + 1] = row
    currentt = rs.normal(size=n)
    currentt[rs.uniform(size=n) < 0.2] = np.nan
    return allL, generation, currentt, Lmin


def back_call(mod, case):
    allL, generation, currentt, Lmin = (np.array(a) for a in case)
    mod.step_back(float(Lmin), allL, generation, currentt)
    return allL, generation, currentt


@pytest.mark.parametrize("all_minus_one", [False, True])
@pytest.mark.parametrize("n,ngen", BACK_SIZES)
def test_step_back(impl, n, ngen, all_minus_one):
    for seed in range(841, 841 + (16 if n == 1 else 1)):
        case = back_case(seed, n, ngen, all_minus_one)
        want = step_back_plain(case) if impl is O else back_call(O, case)
        for name, g, w in zip(("allL", "generation", "t"), back_call(impl, case), want):
            assert same_bits(g, w), (n, ngen, seed, name)


def test_back_cases_hold_what_they_were_built_for():
    case = back_case(841, 257, 64)
    allL, generation, currentt, Lmin = case
    assert (allL == Lmin).any() and (allL == np.inf).any() and (allL == -np.inf).any() and generation.max() == 63
    assert all(np.isnan(allL[i, g + 1:]).all() and not np.isnan(allL[i, :g + 1]).any() for i, g in enumerate(generation))
    L2, g2, t2 = back_call(O, case)
    moved = g2 < generation
    assert moved.any() and (~moved).any() and (g2 >= -1).all() and (g2[moved] == -1).any() and np.isnan(t2[moved]).all()
    assert not (L2 < Lmin).any() and (L2 == Lmin).any()       # an entry at the threshold stays
    minus = back_case(841, 257, 64, True)
    assert (minus[1] == -1).all() and np.isnan(minus[0]).all()
    assert all(same_bits(a, b) for a, b in zip(back_call(O, minus), minus[:3]))


# ------------------------------------------------------------------------------------------------ within_unit_cube
CUBE_VALUES = (0.0, 1.0, np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0), -0.0, 1e-310, np.nan, -1e-300, np.nextafter(1.0, 2.0), 0.5)
CUBE_INSIDE = (False, False, True, True, False, True, False, False, False, True)


def cube_case(seed, n, d):
    """rows inside the cube; row i holds CUBE_VALUES[i % 10] in one column if i % 20 < 10"""
    rs = np.random.RandomState(seed)
    u = rs.uniform(0.01, 0.99, size=(n, d))
    want = np.ones(n, dtype=bool)
    for i in range(n):
        if i % 20 < 10:
            u[i, rs.randint(d)] = CUBE_VALUES[i % 10]
            want[i] = CUBE_INSIDE[i % 10]
    return u, want


@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("d", [1, 1024])
def test_within_unit_cube(impl, d, n):
    u, want = cube_case(851, n, d)
    assert np.array_equal(O.within_unit_cube(u), want) and np.array_equal(want, np.logical_and(u > 0, u < 1).all(axis=1))
    got = impl.within_unit_cube(u)
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    assert want.any() and not want.all() and 0 < 1e-310 < np.finfo(float).tiny


# ------------------------------------------------------------------------------------------------ row_dist2
def dist_case(seed, n, d):
    """row i: i % 3 == 0 two independent rows of the cube, 1 the same row twice (exactly 0), 2 rows 1e-9 apart around 0.5"""
    rs = np.random.RandomState(seed)
    a, b = rs.uniform(size=(n, d)), rs.uniform(size=(n, d))
    k = np.arange(n) % 3
    b[k == 1] = a[k == 1]
    a[k == 2] = 0.5 + 0.01 * rs.normal(size=(int((k == 2).sum()), d))
    b[k == 2] = a[k == 2] + 1e-9 * rs.normal(size=(int((k == 2).sum()), d))
    return a, b, k


def dist_reference(a, b):
    """sum_k (a_k - b_k)^2 in np.longdouble (64-bit mantissa: 2^-11 of the bound); exact rationals where there is none"""
    if LR.HAVE_LONGDOUBLE:
        diff = a.astype(LR.LD) - b.astype(LR.LD)
        return (diff * diff).sum(axis=1)
    from fractions import Fraction
    return np.array([sum((Fraction(x) - Fraction(y)) ** 2 for x, y in zip(ra, rb)) for ra, rb in zip(a.tolist(), b.tolist())], dtype=object)


@pytest.mark.parametrize("d", [1, 50, 129, 1024])
def test_row_dist2(impl, d):
    """|got - ref| <= (d + 2) 2^-53 ref.  Every term is non-negative, so every partial sum is at most the result: one
    rounding of the difference (relative 2^-53, which the square doubles), at most one of the square, and d - 1 of the
    sequential sum give (2 + 1 + d - 1) 2^-53 to first order; a fused multiply-add would take the square's away."""
    n = 257
    a, b, k = dist_case(861, n, d)
    got = impl.row_dist2(a, b)
    ref = dist_reference(a, b)
    assert got.shape == (n,) and (got[k == 1] == 0).all() and (got[k != 1] > 0).all()
    if LR.HAVE_LONGDOUBLE:
        err, size = np.abs(got.astype(LR.LD) - ref).astype(np.float64), ref.astype(np.float64)
    else:
        from fractions import Fraction
        err, size = (np.array([float(x) for x in col]) for col in ([abs(Fraction(float(g)) - r) for g, r in zip(got, ref)], ref))
    bound = size * ((d + 2) * 2.0 ** -53)
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    print("row_dist2 d=%d n=%d: largest error / bound = %.3f" % (d, n, worst))
    assert (err <= bound).all(), worst


# ------------------------------------------------------------------------------------------------ plain restatements
# The reference's functions (stepfuncs.pyx, popstepsampler.py) once more, in numpy and plain loops, written from their
# definitions and not from the oracle's C: what the oracle is held to at the shapes the recorded vectors do not reach.
def slice_update_plain(c, shrink):
    t, L, w, thr = c["t"], c["proposed_L"], c["worker_running"], c["threshold"]
    tleft, tright, status = np.array(c["tleft"]), np.array(c["tright"]), np.array(c["status"])
    allu, allL, allp = np.array(c["allu"]), np.array(c["allL"]), np.array(c["allp"])
    discarded = 0
    for l in range(len(t)):
        p = w[l]
        if t[l] > tright[p] or t[l] < tleft[p]:
            discarded += bool(L[l] > thr)
            continue
        if 0 < t[l] < tright[p]:
            tright[p] = t[l] / shrink
        if tleft[p] < t[l] < 0:
            tleft[p] = t[l] / shrink
        if L[l] > thr and status[p] == 0:
            status[p], allu[p], allL[p], allp[p] = 1, c["proposed_u"][l], L[l], c["proposed_p"][l]
    left = np.flatnonzero(status == 0)
    workers = left[np.arange(len(t)) % len(left)] if len(left) else np.array(w)
    return tleft, tright, workers.astype(np.int64), status, allu, allL, allp, discarded


def line_intersection_plain(o, v):
    with np.errstate(divide="ignore", invalid="ignore"):
        m = 1.0 / v
        nn, kk = m * (o - 0.5), np.abs(m) * 0.5
        return np.fmax.reduce(-nn - kk, axis=1), np.fmin.reduce(-nn + kk, axis=1)     # fmax / fmin skip NaN


def evolve_update_plain(c):
    t, left, right, sl, sr = copies(c, "currentt", "current_left", "current_right", "searching_left", "searching_right")
    hit = np.zeros(len(t), dtype=bool)
    hit[c["acceptable"]] = c["Lnew"] > c["Lmin"]
    search_right, bisecting = ~sl & sr, ~(sl | sr)
    left[hit & sl] *= 2
    right[hit & search_right] *= 2
    miss_left, miss_right = ~hit & sl, ~hit & search_right
    sl[miss_left] = False
    sr[miss_right] = False
    neg = bisecting & (t < 0)
    left[neg] = t[neg]
    right[bisecting & ~neg] = t[bisecting & ~neg]
    success = hit & bisecting
    t[success] = np.nan
    return [t, left, right, sl, sr, success]


def evolve_plain(seed, n, d):
    s = inputs.walker_state(seed, n, d)
    s["currentt"][::5] = np.where(np.arange(len(s["currentt"][::5])) % 2 == 0, 0.0, -0.0)
    np.random.seed(seed)
    u, t, v, left, right, sl, sr = (s[k] for k in ("currentu", "currentt", "currentv", "current_left", "current_right",
                                                   "searching_left", "searching_right"))
    bisecting = ~(sl | sr)
    draws = np.random.random_sample(int(bisecting.sum()))
    t[bisecting] = left[bisecting] + (right[bisecting] - left[bisecting]) * draws
    step = np.where(sl, left, np.where(sr, right, t))
    unew = u + v * step[:, None]
    acceptable = np.logical_and(unew > 0, unew < 1).all(axis=1)
    pnew = inputs.walker_transform(unew[acceptable]) if acceptable.any() else np.empty((0, 1))
    Lnew = inputs.walker_loglike(pnew) if acceptable.any() else np.empty(0)
    c = dict(currentt=t, current_left=left, current_right=right, searching_left=sl, searching_right=sr, acceptable=acceptable,
             Lnew=Lnew, Lmin=s["Lmin"])
    t, left, right, sl, sr, success = evolve_update_plain(c)
    took = success[acceptable]
    return [t, v, left, right, sl, sr, success, unew[success], pnew[took], Lnew[took], unew, np.int64(acceptable.sum()),
            np.float64(np.random.uniform())]


def step_back_plain(case):
    allL, generation, currentt, Lmin = (np.array(a) for a in case)
    width = generation.max() + 1
    if width <= 0:
        return allL, generation, currentt
    below = allL[:, :width] < Lmin
    while below.any():
        for i in np.flatnonzero(below.any(axis=1)):
            g = generation[i]
            assert g >= 0
            generation[i] = g - 1
            currentt[i] = np.nan
            allL[i, g] = np.nan
            below[i, g] = False
    return allL, generation, currentt
