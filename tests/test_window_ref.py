"""CPU tests of tests/windowref.py: its two statements of the window functions (the literal
row-at-a-time fold and the vectorised numpy form) agree on randomised inputs, and both reproduce the
hand-derived vectors of tests/golden/window_kat.json."""
import numpy as np

import sortref as R
import windowref as W


def test_kat_covers_what_it_should():
    kat = W.load_kat()
    assert len(kat) >= 12
    fns = {f[0] for v in kat for f in v[5]}
    frames = {f[1] for v in kat for f in v[5]}
    assert fns == set(range(W.ROW_NUMBER, W.LEAD + 1)) and frames == {W.ROWS, W.RANGE, W.PARTITION}
    assert any(3 in v[3] for v in kat)  # a DESC NULLS FIRST order key
    assert any(k[2] is not None for v in kat for k in v[1])  # null partition keys
    assert any(not v[1] and not v[2] for v in kat)  # no key at all


def test_both_statements_reproduce_the_kat():
    for name, part, order, flags, inputs, fns, expected, rows in W.load_kat():
        lit = W.fold(part, order, flags, inputs, fns, rows)
        vec = W.vectorised(part, order, flags, inputs, fns, rows)
        assert W.same_results(lit, expected), name
        assert W.same_results(vec, expected), name


def _random_column(rng, t, n, null_p, special):
    if t == R.TYPE_FLOAT64:
        vals = rng.integers(-3, 4, n).astype(np.float64) * 0.5
        if special:
            pick = rng.random(n)
            vals[pick < 0.15] = np.nan
            vals[(pick >= 0.15) & (pick < 0.25)] = -0.0
            vals[(pick >= 0.25) & (pick < 0.3)] = np.inf
            vals[(pick >= 0.3) & (pick < 0.35)] = -np.inf
    elif t == R.TYPE_INT64:
        vals = rng.integers(-4, 5, n) if not special else rng.integers(-(1 << 63), (1 << 63) - 1, n)
    elif t == R.TYPE_UINT8:
        vals = rng.integers(0, 256 if special else 4, n).astype(np.uint8)
    else:
        vals = rng.integers(-3, 4, n).astype(np.int32)
    valid = rng.random(n) >= null_p if null_p else None
    return (t, vals, valid)


def test_statements_agree_on_random_inputs():
    rng = np.random.default_rng(20)
    fixed = [R.TYPE_INT64, R.TYPE_FLOAT64, R.TYPE_INT32, R.TYPE_DATE32, R.TYPE_UINT8]
    ran = 0
    for trial in range(60):
        n = int(rng.integers(1, 70))
        k, m = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        part = [_random_column(rng, fixed[int(rng.integers(0, 5))], n, 0.2 * (trial % 2), False) for _ in range(k)]
        order = [_random_column(rng, fixed[int(rng.integers(0, 5))], n, 0.2 * (trial % 3 == 0), False) for _ in range(m)]
        flags = [int(rng.integers(0, 4)) for _ in range(m)]
        inputs = [_random_column(rng, t, n, 0.3 * (trial % 2), True) for t in fixed]
        fns = [(W.ROW_NUMBER, 0, 0, 0), (W.RANK, 0, 0, 0), (W.DENSE_RANK, 0, 0, 0)]
        for frame in (W.ROWS, W.RANGE, W.PARTITION):
            fns += [(W.COUNT_STAR, frame, 0, 0), (W.COUNT, frame, 1, 0), (W.SUM, frame, 0, 0), (W.SUM, frame, 2, 0)]
            fns += [(f, frame, i, 0) for f in (W.MIN, W.MAX) for i in range(5)]
        fns += [(f, 0, i, off) for f in (W.LAG, W.LEAD) for i in range(5) for off in (0, 1, 2, n, 1 << 40)]
        assert W.same_results(W.fold(part, order, flags, inputs, fns, n), W.vectorised(part, order, flags, inputs, fns, n)), trial
        ran += len(fns)
    assert ran > 1000


def test_empty_input():
    col = (R.TYPE_INT64, np.zeros(0, dtype=np.int64), None)
    fns = [(W.ROW_NUMBER, 0, 0, 0), (W.SUM, W.ROWS, 0, 0)]
    for got in (W.fold([col], [], [], [col], fns), W.vectorised([col], [], [], [col], fns)):
        assert [len(v) for v, _ in got] == [0, 0]


def test_argument_rules():
    assert W.check(W.SUM, W.ROWS, R.TYPE_FLOAT64, 0) == (W.UNSUPPORTED, 0)
    assert W.check(W.SUM, W.ROWS, R.TYPE_INT32, 0) == (W.OK, R.TYPE_INT64)
    assert W.check(W.LAG, W.ROWS, R.TYPE_UTF8, 0) == (W.UNSUPPORTED, 0)
    assert W.check(W.LAG, W.ROWS, R.TYPE_INT64, -1) == (W.INVALID_ARG, 0)
    assert W.check(W.COUNT, W.RANGE, R.TYPE_UTF8, 0) == (W.OK, R.TYPE_INT64)
    assert W.check(11, W.ROWS, R.TYPE_INT64, 0)[0] == W.check(W.RANK, 3, 0, 0)[0] == W.INVALID_ARG
    found, of_fn = W.scans([(W.SUM, 0, 1, 0), (W.COUNT, 2, 1, 0), (W.RANK, 0, 0, 0), (W.MIN, 0, 1, 0), (W.MAX, 0, 1, 0), (W.SUM, 0, 0, 0)])
    assert found == [(1, 1), (2, 1), (3, 1), (1, 0)] and of_fn == [0, 0, -1, 1, 2, 3]
