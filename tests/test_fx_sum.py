"""The exact fp64 SUM / AVG accumulator of the hash aggregate (query-engines_amd/csrc/qe_dev.hpp,
fx_*), built for the host (tests/native/fx_host.hip) and checked on the CPU against exact rational
sums (fractions.Fraction; float(Fraction) rounds correctly, ties to even).

The contract (BASELINE north_star): a group's fp64 SUM is within 1e-9 relative of the
exact sum. The accumulator gives more: the correctly rounded exact sum over the whole fp64 range
(math.fsum's value), bit-identical whatever order rows land in slots and slots merge (integer adds
are associative). These tests pin the arithmetic itself: row images, carries across words, the
running sum changing sign, wraps past 2^127, the full-range words E (inputs of 2^126 or more, bits
below 2^-128, subnormals, overflow to +-Inf), merges in word, RAW and CHUNK form, IEEE specials.
tests/test_fp64_sum_gpu.py runs the same cases on MI355X through every kernel path."""
import ctypes
import math
import pathlib
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import aggdata
from oracle.semantics import _fsum as fsum  # the contract: exact where math.fsum's partials overflow

NATIVE = pathlib.Path(__file__).resolve().parent / "native"
LIB = NATIVE / "_build" / "libqe_fx_host.so"


@pytest.fixture(scope="module")
def fx():
    subprocess.run(["make", "-s", "-C", str(NATIVE), "_build/libqe_fx_host.so"], check=True, capture_output=True)
    lib = ctypes.CDLL(str(LIB))
    lib.qe_fx_host_sum.restype = ctypes.c_double
    lib.qe_fx_host_sum.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_long, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_ulonglong)]
    lib.qe_fx_host_row_words.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_ulonglong)]
    lib.qe_fx_host_ext_result.restype = ctypes.c_double
    lib.qe_fx_host_ext_result.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
    for f in (lib.qe_fx_host_window_sum,):
        f.restype = ctypes.c_double
        f.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_long, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                      ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_ulonglong)]

    def run(xs, nslots=1, order=None):
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        order = list(range(nslots)) if order is None else list(order)
        o = (ctypes.c_int * nslots)(*order)
        err = ctypes.c_int()
        words = (ctypes.c_ulonglong * 39)()
        v = lib.qe_fx_host_sum(xs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(xs), nslots, o,
                               ctypes.byref(err), words)
        return v, bool(err.value), tuple(words)

    run.lib = lib
    return run


def exact(xs):
    """The correctly rounded exact sum (ties to even; IEEE overflow to +-Inf)."""
    q = sum((Fraction(float(x)) for x in xs), Fraction(0))
    try:
        return float(q)
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def same(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def test_wide_range_is_correctly_rounded(fx):
    rng = np.random.default_rng(1)
    for trial in range(40):
        n = int(rng.integers(1, 3000))
        xs = rng.normal(size=n) * np.exp2(rng.integers(-70, 100, n).astype(np.float64))
        v, err, w = fx(xs)
        assert not err
        assert same(v, exact(xs)), (trial, v, exact(xs))


def test_order_and_slots_do_not_matter(fx):
    rng = np.random.default_rng(2)
    xs = rng.normal(size=5000) * np.exp2(rng.integers(-60, 60, 5000).astype(np.float64))
    base = fx(xs)
    for nslots in (2, 7, 64):
        for _ in range(3):
            got = fx(rng.permutation(xs), nslots, rng.permutation(nslots))
            assert got[2] == base[2] and same(got[0], base[0])
    assert same(base[0], exact(xs))


def test_cancelling_pairs_keep_unit_terms(fx):
    """The verdict's adversarial group: +-2^60 pairs with unit terms between them. fp64 addition in
    arrival order loses the units (2^60's ulp is 256); the exact accumulator keeps every one."""
    rng = np.random.default_rng(3)
    units = 1000
    xs = np.concatenate([np.full(50, 2.0 ** 60), np.full(50, -(2.0 ** 60)), np.ones(units)])
    for _ in range(5):
        p = rng.permutation(xs)
        v, err, _ = fx(p, 8, rng.permutation(8))
        assert not err and v == units
    # the same with values around 1e-3 between +-1e15: exact 1e-9 relative holds only exactly
    xs = np.concatenate([np.full(20, 1e15), np.full(20, -1e15), rng.random(500) * 1e-3])
    v, err, _ = fx(rng.permutation(xs), 5)
    assert not err and same(v, exact(xs))


def test_sign_changes_and_carries(fx):
    # running sums that cross zero again and again, and carries across every word boundary
    xs = [1.0, -1.0] * 100 + [2.0 ** -64, -(2.0 ** -63), 2.0 ** -64] * 50
    xs += [2.0 ** 63, 2.0 ** 63, -(2.0 ** 64), 2.0 ** -128, -(2.0 ** -128), 2.0 ** 100, -(2.0 ** 100)]
    xs += [-0.5] * 7 + [0.25] * 9
    rng = np.random.default_rng(4)
    for _ in range(10):
        p = rng.permutation(np.array(xs))
        v, err, _ = fx(p, int(rng.integers(1, 9)))
        assert not err and same(v, exact(p))
    assert fx([-0.0, -0.0])[0] == 0.0


def test_wraps_beyond_2_127(fx):
    big = 2.0 ** 125 * 1.75
    xs = [big] * 10 + [-big] * 3
    v, err, w = fx(xs, 3)
    assert not err and same(v, exact(xs))
    assert (w[4] >> 8) != 0  # the words wrapped: the status carries the count
    xs = [big] * 10 + [-big] * 10 + [1.0]
    v, err, w = fx(np.random.default_rng(5).permutation(xs), 4)
    assert not err and v == 1.0
    assert (w[4] >> 8) == 0  # wraps cancelled


def test_ieee_specials(fx):
    inf = float("inf")
    assert math.isnan(fx([1.0, float("nan"), 2.0])[0])
    assert fx([1.0, inf, 2.0])[0] == inf
    assert fx([1.0, -inf])[0] == -inf
    v, err, _ = fx([inf, -inf, 1.0])
    assert math.isnan(v) and not err
    for big in ([2.0 ** 126, 1.0], [2.0 ** 125, 1.0], [-(2.0 ** 181) * 1.5, 3.0, 2.0 ** 140, -1e-20],
                [1e50, -1e50, 7.0], [2.0 ** 181, 2.0 ** 181, -(2.0 ** 170)], [2.0 ** 182, 1.0],
                [np.finfo(np.float64).max]):
        v, err, _ = fx(big, 2)  # 2^126 and up: the full-range words E, exact
        assert not err and same(v, exact(big)), big


def test_tiny_inputs(fx):
    # bits below 2^-128 go to E unrounded: every sum is the correctly rounded exact one
    for xs in ([1.0, 1.1e-25, 0.9e-25, 1.3e-25, 2.0], [1.1e-25, 0.9e-25, 1.3e-25], [3.7e-5, -3.7e-5],
               [1e-40, 2e-40, 5e-324], [2.0 ** -128, 2.0 ** -129, 2.0 ** -200]):
        v, err, _ = fx(xs, 2)
        assert not err and same(v, exact(xs)), xs
    assert fx([3.7e-5, -3.7e-5])[0] == 0.0


def test_full_range_matches_fsum(fx):
    """The verdict's full-range cases, bit for bit with math.fsum: groups of 1e-40 values, 1e300 with
    unit terms, subnormals, and an intermediate overflow that cancels."""
    rng = np.random.default_rng(9)
    cases = [[1e-40] * 1000, [1e300] + [1.0] * 1000 + [-1e300], [5e-324] * 777, [1e308, 1e308, -1e308],
             [1e308, -1e308, 1e308, 1e-300, -5e-324], [-1e-320, 3e-322, 2.2250738585072014e-308, -5e-324],
             [1e300, 1.0, -1e300, 2.0 ** -1000]]
    for xs in cases:
        for ns in (1, 3, 8):
            v, err, _ = fx(rng.permutation(np.array(xs)), ns, rng.permutation(ns))
            assert not err and same(v, fsum(xs)) and same(v, exact(xs)), (xs[:3], ns)
    # random exponents over the whole range, both signs, subnormals among them
    for trial in range(30):
        n = int(rng.integers(1, 400))
        e = rng.integers(-1074, 1020, n).astype(np.float64)
        xs = rng.choice([-1.0, 1.0], n) * np.ldexp(1.0 + rng.random(n), e.astype(np.int64))
        xs[rng.random(n) < 0.1] = 5e-324 * rng.integers(1, 2 ** 40, 1)[0]
        v, err, w = fx(xs, int(rng.integers(1, 9)))
        assert same(v, exact(xs)), trial
        assert same(v, fsum(xs)), trial


def test_overflow_and_underflow_edges(fx):
    mx = np.finfo(np.float64).max
    assert fx([mx, mx])[0] == math.inf and fx([-mx, -mx])[0] == -math.inf
    assert fx([mx, 2.0 ** 970])[0] == math.inf  # exactly half way to 2^1024: ties to even (up)
    assert fx([mx, 2.0 ** 969])[0] == mx  # below half way
    assert same(fx([mx, mx, -mx])[0], mx)
    tiny = 2.2250738585072014e-308  # smallest normal
    for xs in ([tiny, -5e-324], [5e-324] * 3, [tiny / 2, tiny / 2], [-5e-324], [tiny * 3, -tiny * 2.5]):
        v, _, _ = fx(xs, 2)
        assert same(v, exact(xs)) and same(v, fsum(xs)), xs


@pytest.mark.parametrize("name,xs", aggdata.BOUNDARY_CASES, ids=[c[0] for c in aggdata.BOUNDARY_CASES])
def test_rounding_boundaries(fx, name, xs):
    """The rounding-boundary groups of tests/test_fp64_sum_gpu.py on the host build: a device
    failure there is in the arithmetic header if the case fails here, outside it otherwise. Rows in
    one slot and spread over slots, through the plain accumulator and the LDS-window split."""
    want = fsum(xs)
    assert same(want, exact(xs))
    rng = np.random.default_rng(len(name))
    for ns in (1, 2, 5):
        v, err, _ = fx(rng.permutation(np.array(xs)), ns, rng.permutation(ns))
        assert not err and same(v, want), (name, ns, v, want)
        v, err, _, _ = window(fx, rng.permutation(np.array(xs)), ns)
        assert not err and same(v, want), (name, "window", ns, v, want)


def test_chunk_merges_equal_rows(fx):
    """Slots merged through CHUNK records (an exported group's E) and RAW rows give the very words
    of adding every row into one slot."""
    rng = np.random.default_rng(10)
    xs = np.ldexp(rng.random(300) + 0.5, rng.integers(-1074, 1000, 300))
    xs[::3] *= -1
    one = fx(xs, 1)
    each = fx(xs, 64, rng.permutation(64))
    assert one[2][5:] == each[2][5:] and one[2][:4] == each[2][:4]
    assert same(one[0], exact(xs))


def test_row_words_merge_like_rows(fx):
    """fx_row_words (one input as a whole partial: the global-table and record paths) merged with
    fx_add_words gives the same words as adding the rows into one slot."""
    rng = np.random.default_rng(6)
    xs = rng.normal(size=64) * np.exp2(rng.integers(-120, 120, 64).astype(np.float64))
    xs[::9] *= -1
    one = fx(xs, 1)
    each = fx(xs, 64, rng.permutation(64))
    assert one[2] == each[2]
    w = (ctypes.c_ulonglong * 5)()
    fx.lib.qe_fx_host_row_words(-1.0, w)
    assert tuple(w) == (0, 0, 2 ** 64 - 1, 2 ** 64 - 1, 0)  # -1.0 = -(2^128) units: sign extended


def window(fx, xs, nslots):
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    err, rare = ctypes.c_int(), ctypes.c_long()
    words = (ctypes.c_ulonglong * 39)()
    f = fx.lib.qe_fx_host_window_sum
    v = f(xs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(xs), nslots, ctypes.byref(err), ctypes.byref(rare),
          words)
    return v, bool(err.value), rare.value, tuple(words)


def test_lds_window_split(fx):
    """The specialised kernels keep a window per LDS slot — a 192-bit carry window (units 2^-96) —
    and send rows outside [2^-44, 2^62) to the global
    accumulator: the merged words equal those of adding every row to one full accumulator,
    whatever the split."""
    rng = np.random.default_rng(7)
    for trial in range(20):
        n = int(rng.integers(1, 4000))
        xs = rng.normal(size=n) * np.exp2(rng.integers(-50, 70, n).astype(np.float64))
        xs[rng.random(n) < 0.05] = 0.0
        xs[rng.random(n) < 0.02] = -0.0
        xs[rng.random(n) < 0.01] = 5e-324
        full = fx(xs)
        v, err, rare, w = window(fx, xs, int(rng.integers(1, 65)))
        assert w == full[2] and same(v, full[0]) and err == full[1], trial
        assert rare == int(np.sum((np.abs(xs) < 2.0 ** -44) & (xs != 0) | (np.abs(xs) >= 2.0 ** 62)))
    # window edges: the smallest and largest fast-path magnitudes, both signs, carries into u2
    edge = [2.0 ** -44, -(2.0 ** -44), np.nextafter(2.0 ** 62, 0), -np.nextafter(2.0 ** 62, 0), 2.0 ** 62,
            np.nextafter(2.0 ** -44, 0), 1.0, -1.0, 2.0 ** 20 + 2.0 ** -30]
    xs = np.array(edge * 50)
    for ns in (1, 3):
        v, err, rare, w = window(fx, rng.permutation(xs), ns)
        assert not err and same(v, exact(xs)) and rare == 100


def test_window_many_rows_and_signs(fx):
    """The carry window over long runs of one sign (carries and borrows through every word) and
    alternating magnitudes across the whole window folds exactly."""
    rng = np.random.default_rng(8)
    for trial in range(6):
        n = 20_000
        mag = np.exp2(rng.integers(-44, 62, n).astype(np.float64)) * (1 + rng.random(n))
        mag = np.minimum(mag, np.nextafter(2.0 ** 62, 0))
        sign = np.ones(n) if trial % 3 == 0 else (-np.ones(n) if trial % 3 == 1 else rng.choice([-1.0, 1.0], n))
        xs = mag * sign
        v, err, rare, w = window(fx, xs, 3)
        assert rare == 0 and not err and same(v, exact(xs)), trial
        assert w == fx(xs)[2]
