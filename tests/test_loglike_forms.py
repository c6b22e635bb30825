"""Every form of the batch likelihoods (launch_loglike of csrc/mlf_misc.hip: k_loglike_rows<KIND, HW> for even d <= 128 on a
16-byte aligned batch, the LDS-staged k_loglike for odd d and misaligned batches, k_loglike_wide above 128) against the
high-precision references of loglike_reference.py, within 1e-12 * scale (see that module for the bound).

The CPU leg (no mark) holds two correct binary64 evaluations -- the C oracle and a numpy restatement of the pair layout with
its xor tree -- to 1e-13 * scale over the same matrix, and the two references to 1e-17 * scale of each other: the margin of
the device bound stays on record and is never measured on the kernel under test.
"""
import ctypes
import functools

import numpy as np
import pytest

import loglike_reference as R

gpu = pytest.mark.gpu

D_EVEN = (2, 4, 6, 8, 10, 16, 18, 32, 34, 50, 64, 66, 126, 128)
D_ODD = (1, 3, 5, 63, 65, 127)
D_WIDE = (129, 130, 200, 256, 257)
D_ALL = D_EVEN + D_ODD + D_WIDE
NS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4099)
NMAX = max(NS)

# the second trip of the grid-stride loop of k_loglike_rows: n = 32768 * RPW * 4 + 2 * RPW + 1, one case per HW
TRIPS = ((128, 131075), (64, 262149), (18, 524297), (10, 1048593), (6, 2097185), (2, 4194369))
TRIP_KIND = {128: "gauss", 64: "eggbox", 18: "eggbox2", 10: "rosenbrock", 6: "gauss", 2: "eggbox"}
TRIP_CASES = [(TRIP_KIND[d], d, n) for d, n in TRIPS] + [(k, 64, 262149) for k in R.KINDS if k != TRIP_KIND[64]]

FORM_D = (6, 50, 128, 7, 127, 200)          # rows (HW = 4, 32, 64), staged (short and longest), wide
HW_D = (2, 6, 10, 18, 34, 66)               # one d per HW


def ns_of(d):
    """batch lengths for dimensionality d: NS, and for the rows kernel the edges of the four loads in flight (4 RPW) and of
    one workgroup (16 RPW)"""
    ns = set(NS)
    if R.rows_form(d):
        rpw = R.rpw_of(d)
        ns.update((4 * rpw - 1, 4 * rpw, 4 * rpw + 1, 16 * rpw - 1, 16 * rpw + 1))
    return sorted(ns)


def test_the_matrix_is_the_one_the_kernels_need():
    """both ends of every HW class, RPW and the second-trip sizes follow from the launch arithmetic"""
    ends = {}
    for d in D_EVEN:
        ends.setdefault(R.hw_of(d), []).append(d)
    assert {hw: (min(v), max(v)) for hw, v in ends.items()} == {2: (2, 4), 4: (6, 8), 8: (10, 16), 16: (18, 32), 32: (34, 64),
                                                                 64: (66, 128)}
    assert sorted(R.hw_of(d) for d in HW_D) == [2, 4, 8, 16, 32, 64]
    for d, n in TRIPS:
        rpw = R.rpw_of(d)
        assert n == 32768 * rpw * 4 + 2 * rpw + 1
    assert sorted(R.hw_of(d) for d, _ in TRIPS) == [2, 4, 8, 16, 32, 64]


def _inputs(kind, d, which):
    """one batch of NMAX rows; every n of the matrix evaluates its first n rows (the kernels split a batch by n, so a row is
    handled by a different wave, lane and trip at every n)"""
    return R.make_inputs(kind, which, 1000 * d + 10 * R.KIND_ID[kind] + which, NMAX, d)


@functools.lru_cache(maxsize=4)
def _case(kind, d, which, with_mpmath=False):
    x, centers, sigma = _inputs(kind, d, which)
    return x, centers, sigma, R.Reference(kind, x, centers, sigma, marks=ns_of(d), with_mpmath=with_mpmath)


def _host(kind, x, centers, sigma):
    from ultranest_amd import likelihoods as lk
    if kind == "gauss":
        return lk.GaussLikelihood(centers, sigma, x.shape[1])(x)
    return {"eggbox": lk.eggbox_loglike, "eggbox2": lk.eggbox2_loglike, "rosenbrock": lk.rosenbrock_loglike}[kind](x)


def _oracle(orc, kind, x, centers, sigma):
    if kind == "gauss":
        return orc.loglike_gauss(x, centers, sigma)
    return {"eggbox": orc.loglike_eggbox, "eggbox2": orc.loglike_eggbox2, "rosenbrock": orc.loglike_rosenbrock}[kind](x)


# ------------------------------------------------------------------------------------------------ CPU leg
@pytest.mark.parametrize("d", D_ALL)
@pytest.mark.parametrize("kind", R.KINDS)
def test_binary64_evaluations_within_a_tenth_of_the_bound(kind, d, oracle):
    for which in (0, 1):
        x, centers, sigma, ref = _case(kind, d, which, True)
        worst, row = ref.excess(_oracle(oracle, kind, x, centers, sigma), rtol=1e-13)
        print("%s d=%d %s oracle: %.3g of 1e-13 scale at row %d" % (kind, d, R.INPUTS[kind][which][0], worst, row))
        assert worst <= 1, (kind, d, which, "oracle", worst, row)
        if R.rows_form(d):
            worst, row = ref.excess(R.pair_tree(kind, x, centers, sigma), rtol=1e-13)
            print("%s d=%d %s pair tree: %.3g of 1e-13 scale at row %d" % (kind, d, R.INPUTS[kind][which][0], worst, row))
            assert worst <= 1, (kind, d, which, "pair tree", worst, row)
        if R.HAVE_LONGDOUBLE and R.HAVE_MPMATH:
            assert all(n - 1 in ref.mp_rows for n in ns_of(d))      # the last row of every batch length
            assert ref.references_disagree_by() <= 1e-17, (kind, d, which, ref.references_disagree_by())
        elif not R.HAVE_LONGDOUBLE:
            assert len(ref.rows) >= 64


def _trip_reference(kind, d, n):
    x, centers, sigma = R.make_inputs(kind, 0, 7 * d + R.KIND_ID[kind], n, d)
    first_trip = 32768 * R.rpw_of(d) * 4          # rows [0, first_trip) belong to the first trip
    return x, centers, sigma, R.Reference(kind, x, centers, sigma, marks=(first_trip + 1,))


@pytest.mark.parametrize("kind,d,n", TRIP_CASES[:len(TRIPS)])
def test_second_trip_sizes_on_the_cpu(kind, d, n, oracle):
    x, centers, sigma, ref = _trip_reference(kind, d, n)
    first_trip = 32768 * R.rpw_of(d) * 4
    if R.HAVE_MPMATH:
        assert first_trip - 1 in ref.mp_rows and first_trip in ref.mp_rows and n - 1 in ref.mp_rows
    for name, got in (("oracle", _oracle(oracle, kind, x, centers, sigma)), ("pair tree", R.pair_tree(kind, x, centers, sigma))):
        worst, row = ref.excess(got, rtol=1e-13)
        assert worst <= 1, (kind, d, n, name, worst, row)
    if R.HAVE_LONGDOUBLE and R.HAVE_MPMATH:
        assert ref.references_disagree_by() <= 1e-17, (kind, d, n, ref.references_disagree_by())


def test_rosenbrock_of_one_coordinate_is_an_empty_sum():
    x = np.random.RandomState(1).uniform(-10, 10, size=(5, 1))
    for got in (R.plain_numpy("rosenbrock", x), R.ref_longdouble("rosenbrock", x)):
        assert np.array_equal(np.asarray(got, dtype=np.float64), np.zeros(5))


def test_loglike_dev_argument_errors_need_no_device():
    """d = 0, an unknown kind and null centres for the Gaussian are refused before anything touches a device"""
    from ultranest_amd import _lib
    L = _lib.lib()
    x, out, c = np.zeros(8), np.zeros(4), np.zeros(2)
    px, pout, pc = (ctypes.c_void_p(a.ctypes.data) for a in (x, out, c))
    bad = 1     # MLF_E_BADARG of include/mlfriends_hip.h
    assert L.mlf_loglike_dev(0, px, 0, 4, pc, 0.1, pout, None) == bad
    assert L.mlf_loglike_dev(1, px, 0, 4, None, 0.0, pout, None) == bad
    assert L.mlf_loglike_dev(4, px, 2, 4, pc, 0.1, pout, None) == bad
    assert L.mlf_loglike_dev(-1, px, 2, 4, pc, 0.1, pout, None) == bad
    assert L.mlf_loglike_dev(0, px, 2, 4, None, 0.1, pout, None) == bad
    assert L.mlf_loglike_dev(1, None, 2, 4, None, 0.0, pout, None) == bad
    assert L.mlf_loglike_dev(1, px, 2, 4, None, 0.0, None, None) == bad
    with pytest.raises(ValueError):
        _lib.check(L.mlf_loglike_dev(0, px, 2, 4, None, 0.1, pout, None))
    assert not out.any() and not x.any()
    # the host entries refuse the same before looking for a device
    assert L.mlf_loglike_eggbox(px, 0, 4, pout) == bad
    assert L.mlf_loglike_gauss(px, 0, 4, pc, 0.1, pout) == bad


# ------------------------------------------------------------------------------------------------ host entries
@gpu
@pytest.mark.parametrize("d", D_ALL)
@pytest.mark.parametrize("kind", R.KINDS)
def test_host_entry_against_the_reference(kind, d):
    for which in (0, 1):
        x, centers, sigma, ref = _case(kind, d, which)
        keep = x.copy()
        top = 0.0
        for n in ns_of(d):
            got = _host(kind, x[:n], centers, sigma)
            assert got.shape == (n,) and got.dtype == np.float64
            if kind == "rosenbrock" and d == 1:
                assert np.array_equal(got, np.zeros(n)), n      # the empty sum: -0.0 or 0.0, nothing else
                continue
            worst, row = ref.excess(got)
            top = max(top, worst)
            assert worst <= 1, (kind, d, R.INPUTS[kind][which][0], n, "row", row, "error / (1e-12 scale)", worst)
        assert np.array_equal(x, keep)
        print("%s d=%d %s: at most %.3g of 1e-12 scale" % (kind, d, R.INPUTS[kind][which][0], top))


@gpu
@pytest.mark.parametrize("kind,d,n", TRIP_CASES)
def test_second_grid_stride_trip(kind, d, n):
    """beyond 32768 waves x RPW x 4 rows the kernel comes round again: every row against the long double reference, the
    last row of the first trip, the first of the second and the last of the batch against mpmath as well"""
    x, centers, sigma, ref = _trip_reference(kind, d, n)
    got = _host(kind, x, centers, sigma)
    worst, row = ref.excess(got)
    print("%s d=%d n=%d: %.3g of 1e-12 scale at row %d" % (kind, d, n, worst, row))
    assert worst <= 1, (kind, d, n, "row", row, worst)
    if R.HAVE_MPMATH:
        first_trip = 32768 * R.rpw_of(d) * 4
        assert first_trip - 1 in ref.mp_rows and first_trip in ref.mp_rows
        s = R.scale(kind, x[ref.mp_rows], centers, sigma, [float(v) for v in ref.mp]) + R.ATOL[kind] / R.RTOL
        assert (R.mp_minus(ref.mp, got[ref.mp_rows]) <= R.RTOL * s).all(), (kind, d, n)


# ------------------------------------------------------------------------------------------------ device entry
_SENTINEL = 0x7FF8DEADBEEF1234      # a quiet NaN with a payload: not a value any kernel computes


class _Dev(object):
    """mlf_loglike_dev on torch tensors and a stream of its own"""

    def __init__(self):
        import torch
        from ultranest_amd import _lib
        self.torch, self.lib = torch, _lib
        self.dev = torch.device("cuda")
        self.stream = torch.cuda.Stream()

    def upload(self, a, lead=0):
        """a device copy of `a` that starts `lead` doubles into its allocation"""
        flat = self.torch.zeros(lead + a.size, dtype=self.torch.float64, device=self.dev)
        view = flat[lead:]
        view.copy_(self.torch.from_numpy(np.array(a, dtype=np.float64).reshape(-1)))
        return view

    def run(self, kind, tx, d, n, centers, sigma, guard=0):
        """-> (results, cells in front, cells behind) as int64 bit patterns"""
        torch = self.torch
        aux = self.upload(np.broadcast_to(np.asarray(centers, dtype=np.float64), (d,))) if kind == "gauss" else None
        out = torch.full((guard + n + guard,), _SENTINEL, dtype=torch.int64, device=self.dev).view(torch.float64)
        torch.cuda.synchronize()
        rc = self.lib.lib().mlf_loglike_dev(R.KIND_ID[kind], ctypes.c_void_p(tx.data_ptr()), d, n,
                                            ctypes.c_void_p(aux.data_ptr()) if aux is not None else None,
                                            float(sigma) if sigma is not None else 0.0,
                                            ctypes.c_void_p(out.data_ptr() + 8 * guard), ctypes.c_void_p(self.stream.cuda_stream))
        self.lib.check(rc)
        self.stream.synchronize()
        self.lib.check(self.lib.lib().mlf_synchronize())
        bits = out.view(torch.int64).cpu().numpy()
        return bits[guard:guard + n].view(np.float64), bits[:guard], bits[guard + n:]


@gpu
@pytest.mark.parametrize("d", FORM_D)
@pytest.mark.parametrize("kind", R.KINDS)
def test_device_entry_equals_the_host_entry_and_keeps_to_its_cells(kind, d):
    """aligned device batches: the host entry's bits; 128 sentinel cells in front of and behind the n results and the
    input batch are untouched"""
    dev = _Dev()
    x, centers, sigma = _inputs(kind, d, 0)
    for n in (1, 65, NMAX):
        tx = dev.upload(x[:n])
        assert tx.data_ptr() % 16 == 0
        before = tx.clone()
        got, front, back = dev.run(kind, tx, d, n, centers, sigma, guard=128)
        assert (front == _SENTINEL).all() and (back == _SENTINEL).all(), (kind, d, n, "a cell outside the results was written")
        assert dev.torch.equal(tx.view(dev.torch.int64), before.view(dev.torch.int64)), (kind, d, n, "the input was written")
        assert np.array_equal(got.view(np.int64), _host(kind, x[:n], centers, sigma).view(np.int64)), (kind, d, n)


@gpu
@pytest.mark.parametrize("d", (2, 6, 50, 128))
@pytest.mark.parametrize("kind", R.KINDS)
def test_misaligned_device_batch_takes_the_staged_form(kind, d):
    """a batch 8 bytes off a 16-byte boundary cannot be read as coordinate pairs: even d goes through k_loglike.  Within the
    bound, the same bits from two different misaligned starts, and the guard cells hold"""
    dev = _Dev()
    for which in (0, 1):
        x, centers, sigma, ref = _case(kind, d, which)
        for n in (1, 65, NMAX):
            results = []
            for lead in (1, 3):
                tx = dev.upload(x[:n], lead=lead)
                assert tx.data_ptr() % 16 == 8
                before = tx.clone()
                got, front, back = dev.run(kind, tx, d, n, centers, sigma, guard=128)
                assert (front == _SENTINEL).all() and (back == _SENTINEL).all(), (kind, d, n, lead)
                assert dev.torch.equal(tx.view(dev.torch.int64), before.view(dev.torch.int64)), (kind, d, n, lead)
                worst, row = ref.excess(got)
                assert worst <= 1, (kind, d, which, n, lead, "row", row, worst)
                results.append(got.view(np.int64))
            assert np.array_equal(results[0], results[1]), (kind, d, which, n)


# ------------------------------------------------------------------------------------------------ non-finite rows
@gpu
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("d", (6, 50, 128, 7, 200))
@pytest.mark.parametrize("kind", R.KINDS)
def test_non_finite_rows_stay_in_their_rows(kind, d, value):
    """one non-finite coordinate (first, middle, last) in rows 0, 1, 63, 64, 150, 299 of 300: those rows give what numpy
    gives for the formula, every other row keeps the bits of the all-finite batch (a shuffle that crossed a row boundary
    inside a wave would leak)"""
    x, centers, sigma = _inputs(kind, d, 0)
    x = x[:300]
    clean = _host(kind, x, centers, sigma)
    assert np.isfinite(clean).all()
    hit = np.array([0, 1, 63, 64, 150, 299])
    others = np.setdiff1d(np.arange(300), hit)
    for col in (0, d // 2, d - 1):
        bad = x.copy()
        bad[hit, col] = value
        got = _host(kind, bad, centers, sigma)
        want = R.plain_numpy(kind, bad, centers, sigma)
        assert not np.isfinite(want[hit]).any()
        assert np.array_equal(np.isnan(got[hit]), np.isnan(want[hit])), (kind, d, col, got[hit], want[hit])
        assert np.array_equal(np.isposinf(got[hit]), np.isposinf(want[hit])), (kind, d, col, got[hit], want[hit])
        assert np.array_equal(np.isneginf(got[hit]), np.isneginf(want[hit])), (kind, d, col, got[hit], want[hit])
        assert np.array_equal(got[hit], want[hit], equal_nan=True)
        assert np.array_equal(got[others].view(np.int64), clean[others].view(np.int64)), (kind, d, col)


# ------------------------------------------------------------------------------------------------ position independence
@gpu
@pytest.mark.parametrize("d", HW_D + (7, 200))
@pytest.mark.parametrize("kind", R.KINDS)
def test_a_row_gives_the_same_bits_wherever_it_stands(kind, d):
    """the same 64 rows at offsets 0, 1, 63, 64, 1000 of batches of 64, 65, 1064 and 5000 rows"""
    x, centers, sigma = _inputs(kind, d, 1)
    block, filler = x[:64], x[64:]
    want = _host(kind, block, centers, sigma).view(np.int64)
    rs = np.random.RandomState(d)
    for length in (64, 65, 1064, 5000):
        for offset in (0, 1, 63, 64, 1000):
            if offset + 64 > length:
                continue
            batch = filler[rs.randint(len(filler), size=length)]
            batch[offset:offset + 64] = block
            got = _host(kind, batch, centers, sigma)
            assert np.array_equal(got[offset:offset + 64].view(np.int64), want), (kind, d, length, offset)
