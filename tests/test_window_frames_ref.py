"""CPU tests of tests/windowframeref.py: its two statements of the framed window functions (a fresh
oracle accumulator per row over that row's frame, and the vectorised numpy form) agree on randomised
inputs, both reproduce the hand-derived vectors of tests/golden/window_frames_kat.json, and the
bounded frame with an unbounded end is the older frame of tests/windowref.py."""
import numpy as np
import pytest

import sortref as R
import windowframeref as F
import windowref as W

BOUNDED = (F.COUNT_STAR, F.COUNT, F.SUM, F.MIN, F.MAX, F.FIRST_VALUE, F.LAST_VALUE)


def test_kat_covers_what_it_should():
    kat = F.load_kat()
    assert len(kat) >= 12
    bounded = [f for v in kat for f in v[5] if f[1] == F.ROWS_BETWEEN and f[0] in BOUNDED]
    assert {f[0] for f in bounded} == set(BOUNDED)
    sign = lambda b: (b > 0) - (b < 0)  # noqa: E731
    patterns = {(sign(lo), sign(hi)) for _, _, _, _, lo, hi in bounded}
    assert patterns >= {(-1, -1), (-1, 0), (-1, 1), (0, 0), (0, 1), (1, 1), (1, -1)}
    assert any(lo == F.INT64_MIN for *_, lo, _ in bounded) and any(hi == F.INT64_MAX for *_, hi in bounded)
    assert any(v[1] for v in kat) and any(f[1] != F.ROWS_BETWEEN for v in kat for f in v[5])  # a partition key; an older frame
    assert any(c[2] is not None for v in kat for c in v[4])  # null inputs
    assert any(c[0] == R.TYPE_FLOAT64 and np.isnan(c[1]).any() for v in kat for c in v[4])
    assert any(c[0] == R.TYPE_FLOAT64 and np.signbit(c[1]).any() for v in kat for c in v[4])
    for fn in (F.FIRST_VALUE, F.LAST_VALUE):  # on a null row: a null result beside valid ones
        assert any(f[0] == fn and not ok.all() and ok.any() and v[4][f[2]][2] is not None
                   for v in kat for f, (_, ok) in zip(v[5], v[6]))
    assert any(f[0] == F.SUM and (vals < -(1 << 62)).any() for v in kat for f, (vals, _) in zip(v[5], v[6]))  # a wrapped sum
    assert any(f[0] == F.COUNT_STAR and (vals == 0).any() for v in kat for f, (vals, _) in zip(v[5], v[6]))  # an empty frame


def test_both_statements_reproduce_the_kat():
    for name, part, order, flags, inputs, fns, expected, rows in F.load_kat():
        assert F.same_results(F.fold(part, order, flags, inputs, fns, rows), expected), name
        assert F.same_results(F.vectorised(part, order, flags, inputs, fns, rows), expected), name


def _inputs(rng, n):
    x = rng.integers(-(1 << 63), (1 << 63) - 1, n) if rng.random() < 0.5 else rng.integers(-4, 5, n)
    f = rng.integers(-3, 4, n).astype(np.float64) * 0.5
    pick = rng.random(n)
    f[pick < 0.15] = np.nan
    f[(pick >= 0.15) & (pick < 0.25)] = -0.0
    f[(pick >= 0.25) & (pick < 0.3)] = np.inf
    small = rng.integers(0, 256, n).astype(np.uint8)
    return [(R.TYPE_INT64, x.astype(np.int64), rng.random(n) >= 0.25), (R.TYPE_FLOAT64, f, rng.random(n) >= 0.25),
            (R.TYPE_UINT8, small, None if rng.random() < 0.5 else rng.random(n) >= 0.5),
            (R.TYPE_INT32, rng.integers(-5, 5, n).astype(np.int32), rng.random(n) >= 0.1)]


def _bound(rng, n):
    choices = [F.INT64_MIN, -n - 1, *range(-5, 6), n + 1, F.INT64_MAX]
    return int(choices[rng.integers(len(choices))])


def _window(rng, n):
    part = [(R.TYPE_INT64, rng.integers(0, max(1, n // 8) + 1, n).astype(np.int64), None)] if rng.random() < 0.8 else []
    order = [(R.TYPE_INT32, rng.integers(0, 6, n).astype(np.int32), rng.random(n) >= 0.1)] if rng.random() < 0.8 else []
    return part, order, [int(rng.integers(0, 4))] * len(order)


@pytest.mark.parametrize("seed", range(30))
def test_fold_equals_vectorised_on_random_windows(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 301)) if seed else 300
    part, order, flags = _window(rng, n)
    inputs = _inputs(rng, n)
    fns = []
    for fn in BOUNDED:
        for inp in range(len(inputs)):
            if F.check(fn, F.ROWS_BETWEEN, inputs[inp][0], 0)[0] != F.OK or (fn == F.COUNT_STAR and inp):
                continue
            for _ in range(2):
                fns.append((fn, F.ROWS_BETWEEN, inp, 0, _bound(rng, n), _bound(rng, n)))
    fns += [(F.FIRST_VALUE, fr, 1, 0, 0, 0) for fr in (F.ROWS, F.RANGE, F.PARTITION)]
    fns += [(F.LAST_VALUE, fr, 0, 0, 0, 0) for fr in (F.ROWS, F.RANGE, F.PARTITION)]
    fns += [(F.RANK, F.ROWS_BETWEEN, 0, 0, 1, 1), (F.LEAD, F.ROWS_BETWEEN, 1, 2, -1, -1), (F.MIN, F.RANGE, 1, 0, 0, 0)]
    lit = F.fold(part, order, flags, inputs, fns, n)
    vec = F.vectorised(part, order, flags, inputs, fns, n)
    for k, f in enumerate(fns):
        assert F.same_results([lit[k]], [vec[k]]), (seed, n, f)


@pytest.mark.parametrize("seed", range(8))
def test_unbounded_ends_are_the_older_frames(seed):
    """(INT64_MIN, 0) is windowref's ROWS frame and (INT64_MIN, INT64_MAX) its PARTITION frame, for every
    aggregate; and the older ids pass through unchanged."""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 301))
    part, order, flags = _window(rng, n)
    inputs = _inputs(rng, n)
    aggs = [(F.COUNT_STAR, 0), (F.COUNT, 0), (F.COUNT, 1), (F.SUM, 0), (F.SUM, 3), (F.MIN, 0), (F.MIN, 1), (F.MAX, 1), (F.MAX, 2)]
    for frame, lo, hi in ((W.ROWS, F.INT64_MIN, 0), (W.PARTITION, F.INT64_MIN, F.INT64_MAX)):
        old = [(fn, frame, inp, 0) for fn, inp in aggs]
        want = W.vectorised(part, order, flags, inputs, old, n)
        new = [(fn, F.ROWS_BETWEEN, inp, 0, lo, hi) for fn, inp in aggs]
        assert F.same_results(F.vectorised(part, order, flags, inputs, new, n), want)
        assert F.same_results(F.fold(part, order, flags, inputs, new, n), want)
        assert F.same_results(F.vectorised(part, order, flags, inputs, [f + (7, -7) for f in old], n), want)
        assert F.same_results(F.fold(part, order, flags, inputs, [f + (7, -7) for f in old], n), want)


def test_the_plan_rules_widen_windowref():
    for fn in range(0, 14):
        for frame in range(-1, 5):
            for t in range(0, 9):
                for off in (-1, 0, 1):
                    st, out = F.check(fn, frame, t, off)
                    if fn <= W.LEAD and frame <= W.PARTITION:
                        assert (st, out) == W.check(fn, frame, t, off)
                    if frame == F.ROWS_BETWEEN:
                        assert F.check(fn, frame, t, off, has_bounds=False) == (F.INVALID_ARG, 0)
                        assert (st, out) == F.check(fn, F.ROWS, t, off)
    assert F.check(F.FIRST_VALUE, F.ROWS_BETWEEN, R.TYPE_FLOAT64, -5) == (F.OK, R.TYPE_FLOAT64)
    assert F.check(F.LAST_VALUE, F.RANGE, R.TYPE_UTF8, 0) == (F.UNSUPPORTED, 0)
    assert F.check(F.SUM, F.ROWS_BETWEEN, R.TYPE_FLOAT64, 0) == (F.UNSUPPORTED, 0)
    assert F.check(13, F.ROWS, R.TYPE_INT64, 0) == (F.INVALID_ARG, 0)
    n = 1000
    assert [F.clamp(b, n) for b in (F.INT64_MIN, -n - 1, -n, -3, 0, n, n + 1, F.INT64_MAX)] == [-n, -n, -n, -3, 0, n, n, n]
    # no bounded MIN / MAX: windowref's scans; a bounded MIN / MAX: one or two scans of its own
    old = [(W.SUM, W.ROWS, 1, 0), (W.COUNT, W.RANGE, 1, 0), (W.MIN, W.ROWS, 0, 0), (W.LAG, 0, 0, 1)]
    found, fwd, bwd = F.scans([f + (0, 0) for f in old] + [(F.SUM, F.ROWS_BETWEEN, 0, 0, -3, 3), (F.FIRST_VALUE, 3, 0, 0, -1, 1)], n)
    assert [k[:2] for k in found] == W.scans(old + [(W.SUM, 0, 0, 0)])[0] and all(k[2:] == (0, 0) for k in found)
    assert fwd == W.scans(old)[1] + [2, -1] and bwd == [-1] * 6
    mins = [(F.MIN, 3, 0, 0, lo, hi) for lo, hi in ((-3, 3), (0, 6), (-3, 2), (F.INT64_MIN, 2), (-2, F.INT64_MAX), (3, 1), (-n, n - 1),
                                                  (-n + 1, n - 1))]
    found, fwd, bwd = F.scans(mins + [(F.MIN, W.PARTITION, 0, 0, 0, 0)], n)
    assert found == [(2, 0, 0, 7), (2, 0, 1, 7), (2, 0, 0, 6), (2, 0, 1, 6), (2, 0, 0, 0), (2, 0, 1, 0)]
    assert fwd == [0, 0, 2, 4, -1, -1, 4, 4, 4] and bwd == [1, 1, 3, -1, 5, -1, -1, 5, -1]
    assert F.work_bytes(n, mins, 2048) == W.work_bytes(n, 6, len(mins), 2048)
