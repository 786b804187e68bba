"""Window functions on the device: qe_window_boundaries + qe_window_eval (and WindowExec) against
tests/windowref.py. Every comparison is exact: validity, the bits of every valid value, and the
zeros of the null rows. The permutation comes from qe_sort_indices, as in the operator."""
import pathlib

import numpy as np
import pytest

import windowref as W
from kquery import native as N
from kquery.columnar import Context, DeviceColumn, Field, RecordBatch, Schema
from kquery.operators import WindowExec, sort_indices, window_boundaries, window_eval, window_layout
from test_sort import _Batches, _typed, to_device

pytestmark = pytest.mark.gpu
GOLD = pathlib.Path(__file__).resolve().parent / "golden"
VALUE_TYPES = [N.TYPE_INT64, N.TYPE_FLOAT64, N.TYPE_INT32, N.TYPE_DATE32, N.TYPE_UINT8]


@pytest.fixture(scope="module")
def layout(gpu_ctx):
    t, s = window_layout()
    assert 0 < t <= s
    return t, s


def device_order(ctx, part, order, flags, n):
    keys = [to_device(ctx, k) for k in list(part) + list(order)]
    if not keys:
        return keys, DeviceColumn.from_numpy(N.TYPE_INT32, np.arange(n, dtype=np.int32), ctx=ctx)
    return keys, sort_indices(keys, [0] * len(part) + list(flags))


def results(outs):
    return [(o.to_numpy().copy(), o.valid_mask()) for o in outs]


def run(ctx, part, order, flags, inputs, fns, n, dev_inputs=None):
    keys, perm = device_order(ctx, part, order, flags, n)
    ps = window_boundaries(keys[:len(part)], perm)
    gs = window_boundaries(keys, perm)
    outs = window_eval(perm, ps, gs, dev_inputs or [to_device(ctx, c) for c in inputs], fns)
    ctx.synchronize()
    return results(outs)


def check(ctx, part, order, flags, inputs, fns, n, dev_inputs=None, ref=W.vectorised, what=""):
    got = run(ctx, part, order, flags, inputs, fns, n, dev_inputs)
    want = ref(part, order, flags, inputs, fns, n)
    for k, ((gv, go), (wv, wo)) in enumerate(zip(got, want)):
        assert gv.dtype == wv.dtype and len(gv) == len(wv) == n, (what, k)
        bits = {8: np.uint64, 4: np.uint32, 1: np.uint8}[gv.dtype.itemsize]
        bad = np.nonzero((go != wo) | (gv.view(bits) != wv.view(bits)))[0]
        if len(bad):
            r = int(bad[0])
            raise AssertionError(f"{what} n={n} function {k} {fns[k]}: {len(bad)} rows differ, first row {r}: got "
                                 f"{gv[r]!r} valid={go[r]}, want {wv[r]!r} valid={wo[r]}")
    assert len(got) == len(fns)


# ---- known answers --------------------------------------------------------------------------------------
def test_known_answers(gpu_ctx):
    ran = 0
    for name, part, order, flags, inputs, fns, expected, rows in W.load_kat():
        got = run(gpu_ctx, part, order, flags, inputs, fns, rows)
        assert W.same_results(got, expected), name
        ran += 1
    assert ran >= 12


# ---- shapes ---------------------------------------------------------------------------------------------
def runs_of(layout_name, n, T, rng):
    """Partition id of every sorted position."""
    if layout_name == "one":
        return np.zeros(n, dtype=np.int64)
    if layout_name == "each":
        return np.arange(n, dtype=np.int64)
    if layout_name == "random":
        cuts = rng.random(n) < 0.02
        return np.cumsum(cuts).astype(np.int64)
    run_len = {"runs64": 64, "runsT": T, "runsT1": T + 1}[layout_name]
    return np.arange(n, dtype=np.int64) // run_len


def shaped_input(layout_name, n, T, seed):
    """Columns laid out in window order (partition id, peer groups of 100 positions that straddle
    wave and tile edges, an INT64 and a FLOAT64 input with nulls), then shuffled into a random row
    order: the device sort has to find the layout again."""
    rng = np.random.default_rng(seed)
    pid = runs_of(layout_name, n, T, rng) * 3 - 5
    pos = np.arange(n, dtype=np.int64)
    okey = (pos // 100).astype(np.int32)
    x = rng.integers(-(1 << 62), 1 << 62, n)
    f = rng.integers(-50, 50, n) * 0.25
    f[rng.random(n) < 0.05] = np.nan
    f[rng.random(n) < 0.05] = -0.0
    xv, fv = rng.random(n) >= 0.2, rng.random(n) >= 0.2
    sh = rng.permutation(n)
    part = [(N.TYPE_INT64, pid[sh], None)]
    order = [(N.TYPE_INT32, okey[sh], None)]
    return part, order, [0], [(N.TYPE_INT64, x[sh], xv[sh]), (N.TYPE_FLOAT64, f[sh], fv[sh])]


CALL_A = [(W.ROW_NUMBER, 0, 0, 0), (W.RANK, 0, 0, 0), (W.DENSE_RANK, 0, 0, 0), (W.COUNT_STAR, W.RANGE, 0, 0),
          (W.COUNT, W.ROWS, 0, 0), (W.SUM, W.PARTITION, 0, 0), (W.MIN, W.ROWS, 1, 0), (W.MAX, W.RANGE, 1, 0)]
CALL_B = [(W.LAG, 0, 0, 1), (W.LEAD, 0, 1, 1), (W.SUM, W.ROWS, 0, 0), (W.SUM, W.RANGE, 0, 0),
          (W.MIN, W.PARTITION, 1, 0), (W.MAX, W.ROWS, 0, 0), (W.COUNT_STAR, W.ROWS, 0, 0), (W.COUNT, W.PARTITION, 1, 0)]


@pytest.mark.parametrize("layout_name", ["one", "each", "runs64", "runsT", "runsT1", "random"])
def test_shapes(gpu_ctx, layout, layout_name):
    """Every function and every frame, in two calls of QE_MAX_AGGS functions. Sizes around the wave, the
    one-workgroup limit and the tile, and around the tile of the scans over the bitmap words (32 T rows)."""
    T, S = layout
    for n in (0, 1, 2, 63, 64, 65, S, S + 1, T - 1, T, T + 1, 3 * T + 17, 32 * T, 32 * T + 1, 64 * T + 77):
        part, order, flags, inputs = shaped_input(layout_name, n, T, n)
        dev = [to_device(gpu_ctx, c) for c in inputs]
        for fns in (CALL_A, CALL_B):
            check(gpu_ctx, part, order, flags, inputs, fns, n, dev, what=layout_name)


def test_each_function_alone(gpu_ctx, layout):
    T, S = layout
    for n in (S, 3 * T + 17):
        part, order, flags, inputs = shaped_input("random", n, T, 7)
        dev = [to_device(gpu_ctx, c) for c in inputs]
        for fn in CALL_A + CALL_B:
            check(gpu_ctx, part, order, flags, inputs, [fn], n, dev, what="alone")


def test_no_keys_and_partition_only(gpu_ctx, layout):
    T, S = layout
    for n in (65, S + 1, 3 * T + 17):
        part, order, flags, inputs = shaped_input("runs64", n, T, 3)
        check(gpu_ctx, [], [], [], inputs, CALL_A, n, what="no keys")
        check(gpu_ctx, part, [], [], inputs, CALL_B, n, what="partition only")
        check(gpu_ctx, [], order, [N.SORT_DESC], inputs, CALL_A, n, what="order only")


# ---- nulls and specials ---------------------------------------------------------------------------------
def test_leading_nulls_and_all_null_partition(gpu_ctx, layout):
    T, S = layout
    for n in (200, 3 * T + 17):
        rng = np.random.default_rng(n)
        pid = np.arange(n, dtype=np.int64) // 37
        within = np.arange(n) % 37
        valid = within >= 3  # the first three rows of every partition are null ...
        valid[pid == 2] = False  # ... and one partition is all null
        x = rng.integers(-1000, 1000, n)
        f = rng.integers(-1000, 1000, n) * 0.5
        sh = rng.permutation(n)
        part, order = [(N.TYPE_INT64, pid[sh], None)], [(N.TYPE_INT64, np.arange(n, dtype=np.int64)[sh], None)]
        inputs = [(N.TYPE_INT64, x[sh], valid[sh]), (N.TYPE_FLOAT64, f[sh], valid[sh])]
        fns = [(fn, fr, i, 0) for fr in (W.ROWS, W.PARTITION) for fn, i in ((W.SUM, 0), (W.MIN, 0), (W.MAX, 1), (W.COUNT, 1))]
        check(gpu_ctx, part, order, [0], inputs, fns, n, what="leading nulls")
        got = run(gpu_ctx, part, order, [0], inputs, fns[:3], n)
        for vals, ok in got:  # ROWS frames: null exactly up to the first value, never after
            assert np.array_equal(ok, valid[sh])
            assert not vals[~ok].any()


def test_fp64_min_max_specials(gpu_ctx, layout):
    T, S = layout
    nan, inf = np.nan, np.inf
    groups = [[nan, 1.0, 2.0], [1.0, nan, 0.5], [-0.0, 0.0], [0.0, -0.0], [inf, -inf, nan], [None, None, nan, 3.0], [-inf, inf],
              [None, 0.0, -0.0, nan], [None], [5.0]]
    for reps in (1, (3 * T + 17) // 29 + 1):
        vals, valid, pid = [], [], []
        for g in range(reps * len(groups)):
            for v in groups[g % len(groups)]:
                vals.append(0.0 if v is None else v)
                valid.append(v is not None)
                pid.append(g)
        n = len(vals)
        part = [(N.TYPE_INT64, np.array(pid, dtype=np.int64), None)]
        inputs = [(N.TYPE_FLOAT64, np.array(vals), np.array(valid))]
        fns = [(fn, fr, 0, 0) for fn in (W.MIN, W.MAX) for fr in (W.ROWS, W.RANGE, W.PARTITION)]
        check(gpu_ctx, part, [], [], inputs, fns, n, what="fp64 specials")  # no order key: input order inside a partition
        if reps == 1:
            check(gpu_ctx, part, [], [], inputs, fns, n, ref=W.fold, what="fp64 specials (fold)")
    # one long partition: a NaN seed sticks across every tile, a later NaN never shows
    n = 3 * T + 17
    later = np.arange(n, dtype=np.float64)
    later[T + 5] = nan
    seeded = later.copy()
    seeded[0] = nan
    for col in (later, seeded):
        check(gpu_ctx, [], [(N.TYPE_INT64, np.arange(n, dtype=np.int64), None)], [0], [(N.TYPE_FLOAT64, col, None)],
              [(W.MAX, W.ROWS, 0, 0), (W.MIN, W.ROWS, 0, 0)], n, what="long NaN")


def test_int64_sum_wraps(gpu_ctx, layout):
    T, S = layout
    for n in (10, 3 * T + 17):
        x = np.full(n, (1 << 62) + 12345, dtype=np.int64)
        x[1::3] = -(1 << 63)
        pid = (np.arange(n) // (T + 1)).astype(np.int64)
        fns = [(W.SUM, fr, 0, 0) for fr in (W.ROWS, W.RANGE, W.PARTITION)]
        check(gpu_ctx, [(N.TYPE_INT64, pid, None)], [], [], [(N.TYPE_INT64, x, None)], fns, n, what="wrap")
        if n == 10:
            check(gpu_ctx, [(N.TYPE_INT64, pid, None)], [], [], [(N.TYPE_INT64, x, None)], fns, n, ref=W.fold, what="wrap (fold)")


# ---- LAG / LEAD -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("t", VALUE_TYPES)
def test_lag_lead(gpu_ctx, layout, t, nullable):
    T, S = layout
    n = 3 * T + 17
    rng = np.random.default_rng(t)
    pid = np.zeros(n, dtype=np.int64)  # one partition of T + 40 rows, then random runs
    pid[T + 40:] = 1 + np.cumsum(rng.random(n - T - 40) < 0.01)
    longest = int(np.bincount(pid).max())
    assert longest >= T + 2
    vals = rng.normal(size=n) if t == N.TYPE_FLOAT64 else _typed(t, rng.integers(-(1 << 62), 1 << 62, n), True)
    sh = rng.permutation(n)
    part = [(N.TYPE_INT64, pid[sh], None)]
    order = [(N.TYPE_INT64, np.arange(n, dtype=np.int64)[sh], None)]
    inputs = [(t, np.asarray(vals)[sh], (rng.random(n) >= 0.3) if nullable else None)]
    dev = [to_device(gpu_ctx, c) for c in inputs]
    offsets = (0, 1, 63, 64, T, T + 1, longest + 1, 1 << 40)
    for fn in (W.LAG, W.LEAD):
        check(gpu_ctx, part, order, [0], inputs, [(fn, 0, 0, off) for off in offsets], n, dev, what="lag/lead")


# ---- boundaries alone -----------------------------------------------------------------------------------
def starts_of(ctx, cols, perm_col, n):
    out = window_boundaries(cols, perm_col)
    ctx.synchronize()
    raw = out.values.cpu().numpy()
    bits = np.unpackbits(raw, bitorder="little")
    words = (n + 31) // 32
    assert not bits[n:32 * words].any(), "bits at and past n of the last word must be 0"
    return bits[:n].astype(bool)


@pytest.mark.parametrize("t", [N.TYPE_INT64, N.TYPE_INT32, N.TYPE_DATE32, N.TYPE_UINT8, N.TYPE_BOOL, N.TYPE_FLOAT64, N.TYPE_UTF8])
def test_boundaries_each_key_type(gpu_ctx, layout, t):
    T, S = layout
    rng = np.random.default_rng(t)
    for n in (1, 2, 63, 64, 65, 3 * T + 17):
        u = rng.integers(0, 7, n)
        if t == N.TYPE_FLOAT64:
            table = np.array([0x7FF8000000000000, 0xFFF8000000000001, 0, 0x8000000000000000, 0x3FF0000000000000,
                              0x7FF0000000000000, 0xFFF0000000000000], dtype=np.uint64).view(np.float64)
            vals = table[u]
        else:
            vals = _typed(t, u, False)  # UTF8: "", "a", "ab", "abcdefgh", "abcdefghi", "a\0": equal prefixes, different lengths
        key = (t, vals, rng.random(n) >= 0.2)
        col = to_device(gpu_ctx, key)
        sorted_perm = sort_indices([col], [0])
        gpu_ctx.synchronize()
        for perm in (sorted_perm.to_numpy(), np.arange(n, dtype=np.int32), rng.permutation(n).astype(np.int32)):
            got = starts_of(gpu_ctx, [col], DeviceColumn.from_numpy(N.TYPE_INT32, perm, ctx=gpu_ctx), n)
            assert np.array_equal(got, W.starts([key], [0], perm)), (t, n)


def test_boundaries_no_key_and_second_key_only(gpu_ctx, layout):
    T, S = layout
    for n in (1, 64, 65, 3 * T + 17):
        perm = DeviceColumn.from_numpy(N.TYPE_INT32, np.arange(n, dtype=np.int32), ctx=gpu_ctx)
        got = starts_of(gpu_ctx, [], perm, n)
        assert got[0] and not got[1:].any()
        first = (N.TYPE_INT64, np.full(n, 7, dtype=np.int64), None)
        second = (N.TYPE_UTF8, [b"x" * (i // 5 % 3) for i in range(n)], None)
        cols = [to_device(gpu_ctx, first), to_device(gpu_ctx, second)]
        assert np.array_equal(starts_of(gpu_ctx, cols, perm, n), W.starts([first, second], [0, 0], np.arange(n)))
        assert np.array_equal(starts_of(gpu_ctx, cols[:1], perm, n), W.starts([first], [0], np.arange(n)))


def test_boundaries_around_one_bitmap_word(gpu_ctx):
    """A wave writes two 32-bit words: row counts that end just before, at and just after the first of
    them, and just after the second (a nullable key, so the validity bit is read too)."""
    rng = np.random.default_rng(33)
    for n in (31, 32, 33, 65):
        key = (N.TYPE_INT64, _typed(N.TYPE_INT64, rng.integers(0, 3, n), False), rng.random(n) >= 0.2)
        perm = np.arange(n, dtype=np.int32)
        got = starts_of(gpu_ctx, [to_device(gpu_ctx, key)], DeviceColumn.from_numpy(N.TYPE_INT32, perm, ctx=gpu_ctx), n)
        assert np.array_equal(got, W.starts([key], [0], perm)), n


# ---- refusals -------------------------------------------------------------------------------------------
def _filled(ctx, t, n, nullable):
    """An output column whose buffers hold a pattern no kernel writes."""
    c = DeviceColumn.empty(t, n, nullable, ctx=ctx)
    c.values.fill_(90)
    if nullable:
        c.validity.fill_(0xA5)
    return c


def _snapshot(c):
    return c.values.cpu().numpy().tobytes(), None if c.validity is None else c.validity.cpu().numpy().tobytes()


def test_refused_combinations_write_nothing(gpu_ctx):
    n = 100
    rng = np.random.default_rng(9)
    cols = {t: to_device(gpu_ctx, (t, _typed(t, rng.integers(0, 7, n), False) if t != N.TYPE_FLOAT64 else rng.normal(size=n),
                                   rng.random(n) >= 0.2)) for t in range(1, 8)}
    perm = DeviceColumn.from_numpy(N.TYPE_INT32, np.arange(n, dtype=np.int32), ctx=gpu_ctx)
    ps = window_boundaries([], perm)
    refused = 0
    for fn in range(0, 12):
        for frame in (-1, 0, 2, 3):
            for t in range(1, 8):
                for off in (-1, 0):
                    st, out_t = W.check(fn, frame, t, off)
                    if st == W.OK:
                        continue
                    out = _filled(gpu_ctx, t if t in N.FIXED_WIDTH else N.TYPE_INT64, n, True)
                    before = _snapshot(out)
                    with pytest.raises(N.QueryEngineError) as e:
                        window_eval(perm, ps, ps, [cols[t]], [(fn, frame, 0, off)], outs=[out])
                    gpu_ctx.synchronize()
                    assert e.value.status == st, (fn, frame, t, off)
                    assert _snapshot(out) == before
                    refused += 1
    assert refused > 100
    x = cols[N.TYPE_INT64]
    bad_calls = [
        dict(fns=[(W.SUM, 0, 0, 0)], outs=[_filled(gpu_ctx, N.TYPE_INT64, n, False)]),  # a nullable result without validity
        dict(fns=[(W.LAG, 0, 0, 1)], outs=[_filled(gpu_ctx, N.TYPE_INT64, n, False)]),
        dict(fns=[(W.RANK, 0, 0, 0)], outs=[_filled(gpu_ctx, N.TYPE_INT32, n, True)]),  # a wrong output type
        dict(fns=[(W.MIN, 0, 0, 0)], outs=[_filled(gpu_ctx, N.TYPE_FLOAT64, n, True)]),
        dict(fns=[(W.SUM, 0, 1, 0)], outs=[_filled(gpu_ctx, N.TYPE_INT64, n, True)]),  # an input index out of range
        dict(fns=[(W.SUM, 0, -1, 0)], outs=[_filled(gpu_ctx, N.TYPE_INT64, n, True)]),
        dict(fns=[(W.SUM, 0, 0, 0)], outs=[_filled(gpu_ctx, N.TYPE_INT64, n, True)],  # an order column of another length
             perm=DeviceColumn.from_numpy(N.TYPE_INT32, np.arange(n - 1, dtype=np.int32), ctx=gpu_ctx)),
        dict(fns=[(W.SUM, 0, 0, 0)], outs=[_filled(gpu_ctx, N.TYPE_INT64, n, True)],  # ... of another type
             perm=DeviceColumn.from_numpy(N.TYPE_INT64, np.arange(n, dtype=np.int64), ctx=gpu_ctx)),
    ]
    for call in bad_calls:
        before = _snapshot(call["outs"][0])
        with pytest.raises(N.IllegalArgumentException):
            window_eval(call.get("perm", perm), ps, ps, [x], call["fns"], outs=call["outs"])
        gpu_ctx.synchronize()
        assert _snapshot(call["outs"][0]) == before
    with pytest.raises(N.IllegalArgumentException):
        window_boundaries([x] * (N.MAX_KEYS + 1), perm)


def test_order_entry_out_of_range_fails_the_call(gpu_ctx, layout):
    """The bad entry is checked on the device and never used as an index: the call reports it, the
    inputs are untouched, and the next valid call on the same context is right."""
    T, S = layout
    for n in (100, 3 * T + 17):  # the one-workgroup path and the multi-workgroup one
        part, order, flags, inputs = shaped_input("random", n, T, 5)
        dev = [to_device(gpu_ctx, c) for c in inputs]
        keys, perm = device_order(gpu_ctx, part, order, flags, n)
        gpu_ctx.synchronize()
        for bad_value in (n, -1, 2**31 - 1):
            p = perm.to_numpy().copy()
            p[n // 2] = bad_value
            bad = DeviceColumn.from_numpy(N.TYPE_INT32, p, ctx=gpu_ctx)
            ps, gs = window_boundaries(keys[:1], bad), window_boundaries(keys, bad)
            before = [_snapshot(c) for c in dev]
            with pytest.raises(N.IllegalArgumentException, match="outside"):
                window_eval(bad, ps, gs, dev, CALL_A)
            gpu_ctx.synchronize()
            assert [_snapshot(c) for c in dev] == before
        check(gpu_ctx, part, order, flags, inputs, CALL_A, n, dev, what="after a refused call")


# ---- stream order, determinism --------------------------------------------------------------------------
def test_stream_order_two_calls_back_to_back(gpu_ctx, layout):
    T, S = layout
    n = 3 * T + 17
    part, order, flags, inputs = shaped_input("random", n, T, 11)
    dev = [to_device(gpu_ctx, c) for c in inputs]
    keys, perm = device_order(gpu_ctx, part, order, flags, n)
    ps, gs = window_boundaries(keys[:1], perm), window_boundaries(keys, perm)
    a = window_eval(perm, ps, gs, dev, CALL_A)  # queued behind the boundaries with no wait in between
    b = window_eval(perm, ps, gs, dev, CALL_B)
    gpu_ctx.synchronize()
    assert W.same_results(results(a), W.vectorised(part, order, flags, inputs, CALL_A, n))
    assert W.same_results(results(b), W.vectorised(part, order, flags, inputs, CALL_B, n))


def test_deterministic(gpu_ctx, layout):
    import torch

    T, S = layout
    n = 3 * T + 17
    part, order, flags, inputs = shaped_input("random", n, T, 13)

    def once(ctx):
        got = run(ctx, part, order, flags, inputs, CALL_A, n)
        return [(v.tobytes(), o.tobytes()) for v, o in got]

    runs = [once(gpu_ctx) for _ in range(3)]
    stream = torch.cuda.Stream(device=gpu_ctx.torch_device)
    with torch.cuda.stream(stream):  # the fourth run on a second context with its own stream
        other = Context(0, stream.cuda_stream)
        runs.append(once(other))
        other.synchronize()
    assert all(r == runs[0] for r in runs[1:])


# ---- WindowExec -----------------------------------------------------------------------------------------
def _batch_results(batch, first):
    return [(batch.field(i).to_numpy().copy(), batch.field(i).valid_mask()) for i in range(first, len(batch.fields))]


def test_windowexec_employee(gpu_ctx):
    """Rank the employees by salary within their state."""
    from kquery.csv_source import CsvDataSource
    from kquery.expressions import CastExpression, ColumnExpression, DenseRank, Rank, RowNumber, WindowMax
    from kquery.operators import ProjectionExec, ScanExec

    scan = ScanExec(CsvDataSource(str(GOLD / "employee.csv"), True, 1000, ctx=gpu_ctx), ["first_name", "state", "salary"])
    proj = ProjectionExec(scan, Schema([Field("first_name", N.TYPE_UTF8), Field("state", N.TYPE_UTF8), Field("salary", N.TYPE_FLOAT64)]),
                          [ColumnExpression(0), ColumnExpression(1), CastExpression(ColumnExpression(2), N.TYPE_FLOAT64)])
    schema = Schema(list(proj.schema().fields) + [Field("rank", N.TYPE_INT64), Field("row", N.TYPE_INT64), Field("dense", N.TYPE_INT64),
                                            Field("top", N.TYPE_FLOAT64)])
    fns = [Rank(), RowNumber(), DenseRank(), WindowMax(ColumnExpression(2), N.FRAME_PARTITION)]
    out = list(WindowExec(proj, [ColumnExpression(1)], [(ColumnExpression(2), False, False)], fns, schema).execute())
    assert len(out) == 1 and len(out[0].fields) == 7
    b = out[0]
    assert b.field(0).to_pylist() == ["Matte", "Other", "Pelle"]  # the input's rows in the input's order
    states = [s.encode() for s in b.field(1).to_pylist()]
    salary = np.array(b.field(2).to_pylist())
    want = W.fold([(N.TYPE_UTF8, states, None)], [(N.TYPE_FLOAT64, salary, None)], [N.SORT_DESC], [(N.TYPE_FLOAT64, salary, None)],
                  [(W.RANK, 0, 0, 0), (W.ROW_NUMBER, 0, 0, 0), (W.DENSE_RANK, 0, 0, 0), (W.MAX, W.PARTITION, 0, 0)])
    assert W.same_results(_batch_results(b, 3), want)
    assert b.field(3).to_pylist() == [1, 2, 1] and b.field(6).to_pylist() == [1337.0, 1337.0, 0.0]


def _window_plan(child, schema_in):
    from kquery.expressions import ColumnExpression, Lag, Lead, Rank, WindowCount, WindowMin, WindowSum

    fns = [Rank(), WindowSum(ColumnExpression(1), N.FRAME_ROWS), WindowMin(ColumnExpression(2)), Lag(ColumnExpression(1), 1),
           Lead(ColumnExpression(2), 2), WindowCount(None, N.FRAME_PARTITION), WindowCount(ColumnExpression(1), N.FRAME_ROWS)]
    schema = Schema(list(schema_in.fields) + [Field(f"w{i}", N.TYPE_FLOAT64 if i in (2, 4) else N.TYPE_INT64) for i in range(len(fns))])
    ref = [(W.RANK, 0, 0, 0), (W.SUM, W.ROWS, 0, 0), (W.MIN, W.RANGE, 1, 0), (W.LAG, 0, 0, 1), (W.LEAD, 0, 1, 2),
           (W.COUNT_STAR, W.PARTITION, 0, 0), (W.COUNT, W.ROWS, 0, 0)]
    return WindowExec(child, [ColumnExpression(0)], [(ColumnExpression(2), True, True)], fns, schema), ref


def test_windowexec_multi_batch_equals_single_batch(gpu_ctx):
    rng = np.random.default_rng(2)
    lens = [1001, 7, 0, 4096]
    n = sum(lens)
    k = rng.integers(-4, 4, n).astype(np.int64)
    x, xv = rng.integers(-100, 100, n), rng.random(n) >= 0.2
    f, fv = rng.integers(-5, 5, n) * 0.5, rng.random(n) >= 0.1
    schema = Schema([Field("k", N.TYPE_INT64), Field("x", N.TYPE_INT64), Field("f", N.TYPE_FLOAT64)])

    def batch(lo, hi):
        return RecordBatch(schema, [DeviceColumn.from_numpy(N.TYPE_INT64, k[lo:hi], ctx=gpu_ctx),
                                    DeviceColumn.from_numpy(N.TYPE_INT64, x[lo:hi], xv[lo:hi], ctx=gpu_ctx),
                                    DeviceColumn.from_numpy(N.TYPE_FLOAT64, f[lo:hi], fv[lo:hi], ctx=gpu_ctx)])

    cuts = np.concatenate([[0], np.cumsum(lens)])
    many, ref = _window_plan(_Batches(schema, [batch(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]), schema)
    single, _ = _window_plan(_Batches(schema, [batch(0, n)]), schema)
    out_many, out_single = list(many.execute()), list(single.execute())
    gpu_ctx.synchronize()
    assert len(out_many) == len(out_single) == 1 and out_many[0].rowCount() == n
    assert np.array_equal(out_many[0].field(0).to_numpy(), k)  # input columns unchanged, in input order
    want = W.vectorised([(N.TYPE_INT64, k, None)], [(N.TYPE_FLOAT64, f, fv)], [N.SORT_NULLS_FIRST],
                        [(N.TYPE_INT64, x, xv), (N.TYPE_FLOAT64, f, fv)], ref, n)
    assert W.same_results(_batch_results(out_many[0], 3), want)
    assert W.same_results(_batch_results(out_single[0], 3), want)


def test_windowexec_over_a_group_by_result(gpu_ctx):
    from kquery.expressions import ColumnExpression, CountStarExpression, Rank, SumExpression, WindowSum
    from kquery.operators import HashAggregateExec

    rng = np.random.default_rng(4)
    n = 5000
    region, store = rng.integers(0, 5, n).astype(np.int64), rng.integers(0, 40, n).astype(np.int64)
    amount = rng.integers(0, 1000, n).astype(np.int64)
    schema = Schema([Field("region", N.TYPE_INT64), Field("store", N.TYPE_INT64), Field("amount", N.TYPE_INT64)])
    src = _Batches(schema, [RecordBatch(schema, [DeviceColumn.from_numpy(N.TYPE_INT64, c, ctx=gpu_ctx) for c in (region, store, amount)])])
    agg_schema = Schema([Field("region", N.TYPE_INT64), Field("store", N.TYPE_INT64), Field("total", N.TYPE_INT64), Field("n", N.TYPE_INT64)])
    agg = HashAggregateExec(src, [ColumnExpression(0), ColumnExpression(1)], [SumExpression(ColumnExpression(2)), CountStarExpression()],
                            agg_schema)
    win_schema = Schema(list(agg_schema.fields) + [Field("rank", N.TYPE_INT64), Field("running", N.TYPE_INT64)])
    plan = WindowExec(agg, [ColumnExpression(0)], [(ColumnExpression(2), False, False)],
                      [Rank(), WindowSum(ColumnExpression(2), N.FRAME_ROWS)], win_schema)
    (b,) = list(plan.execute())
    gpu_ctx.synchronize()
    g_region, g_total = b.field(0).to_numpy(), b.field(2).to_numpy()
    totals = {}
    for r, s, a in zip(region, store, amount):
        totals[(int(r), int(s))] = totals.get((int(r), int(s)), 0) + int(a)
    assert {(int(r), int(s)): int(t) for r, s, t in zip(g_region, b.field(1).to_numpy(), g_total)} == totals
    want = W.vectorised([(N.TYPE_INT64, g_region, None)], [(N.TYPE_INT64, g_total, None)], [N.SORT_DESC],
                        [(N.TYPE_INT64, g_total, None)], [(W.RANK, 0, 0, 0), (W.SUM, W.ROWS, 0, 0)], len(g_total))
    assert W.same_results(_batch_results(b, 4), want)


def test_windowexec_empty_input_and_no_keys(gpu_ctx):
    from kquery.expressions import ColumnExpression, RowNumber, WindowCount, WindowSum

    schema = Schema([Field("x", N.TYPE_INT64)])
    out_schema = Schema(list(schema.fields) + [Field("row", N.TYPE_INT64), Field("sum", N.TYPE_INT64), Field("n", N.TYPE_INT64)])
    fns = [RowNumber(), WindowSum(ColumnExpression(0), N.FRAME_ROWS), WindowCount(None, N.FRAME_RANGE)]
    (empty,) = list(WindowExec(_Batches(schema, []), [], [], fns, out_schema).execute())
    assert empty.rowCount() == 0 and len(empty.fields) == 4
    x = np.arange(1, 301, dtype=np.int64)
    src = _Batches(schema, [RecordBatch(schema, [DeviceColumn.from_numpy(N.TYPE_INT64, x, ctx=gpu_ctx)])])
    (b,) = list(WindowExec(src, [], [], fns, out_schema).execute())  # no key: one partition of peers, in input order
    gpu_ctx.synchronize()
    assert np.array_equal(b.field(1).to_numpy(), x) and np.array_equal(b.field(2).to_numpy(), np.cumsum(x))
    assert np.array_equal(b.field(3).to_numpy(), np.full(300, 300))
    with pytest.raises(N.IllegalArgumentException):
        WindowExec(src, [ColumnExpression(0)] * 3, [(ColumnExpression(0), True, False)] * 2, fns, out_schema)
