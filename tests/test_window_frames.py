"""qe_window_eval_frames on the device (FIRST_VALUE / LAST_VALUE and the frame ROWS BETWEEN lo AND hi,
through WindowExec too) against tests/windowframeref.py. Every comparison is exact: validity, the bits
of every valid value, and the zeros of the null rows."""
import csv
import pathlib

import numpy as np
import pytest

import windowframeref as F
import windowref as W
from kquery import native as N
from kquery.columnar import Context, DeviceColumn, Field, RecordBatch, Schema
from kquery.operators import WindowExec, window_boundaries, window_eval, window_eval_frames, window_layout
from test_sort import _Batches, to_device
from test_window import _filled, _snapshot, device_order, results, shaped_input

pytestmark = pytest.mark.gpu
GOLD = pathlib.Path(__file__).resolve().parent / "golden"
B = F.ROWS_BETWEEN
LO, HI = F.INT64_MIN, F.INT64_MAX


@pytest.fixture(scope="module")
def layout(gpu_ctx):
    return window_layout()


class Window:
    """One window on the device: the sort and the two boundary calls run once for all of its calls."""

    def __init__(self, ctx, part, order, flags, inputs, n):
        self.ctx, self.args, self.n = ctx, (part, order, flags, inputs), n
        keys, self.perm = device_order(ctx, part, order, flags, n)
        self.ps = window_boundaries(keys[:len(part)], self.perm)
        self.gs = window_boundaries(keys, self.perm)
        self.dev = [to_device(ctx, c) for c in inputs]

    def run(self, fns, **kw):
        outs = window_eval_frames(self.perm, self.ps, self.gs, self.dev, fns, **kw)
        self.ctx.synchronize()
        return results(outs)

    def run_old(self, fns):
        outs = window_eval(self.perm, self.ps, self.gs, self.dev, fns)
        self.ctx.synchronize()
        return results(outs)

    def check(self, fns, what="", ref=F.vectorised):
        compare(self.run(fns), ref(*self.args, fns, self.n), fns, self.n, what)


def compare(got, want, fns, n, what=""):
    assert len(got) == len(want) == len(fns)
    for k, ((gv, go), (wv, wo)) in enumerate(zip(got, want)):
        assert gv.dtype == wv.dtype and len(gv) == len(wv) == n, (what, k)
        bits = {8: np.uint64, 4: np.uint32, 1: np.uint8}[gv.dtype.itemsize]
        bad = np.nonzero((go != wo) | (gv.view(bits) != wv.view(bits)))[0]
        if len(bad):
            r = int(bad[0])
            raise AssertionError(f"{what} n={n} function {k} {fns[k]}: {len(bad)} rows differ, first row {r}: got "
                                 f"{gv[r]!r} valid={go[r]}, want {wv[r]!r} valid={wo[r]}")


def bounds_of(n, T):
    return [(-2, -1), (-1, 1), (0, 0), (1, 3), (3, 1), (LO, -1), (2, HI), (-(T - 1), 0), (-T, 0), (-T, T + 1), (-n - 1, n + 1)]


def framed_call(q, lo, hi):
    """Every aggregate and FIRST / LAST under one pair of bounds, the INT64 input (0) and the FLOAT64
    input (1) swapping places with q."""
    a, b = q & 1, 1 - (q & 1)
    return [(F.COUNT_STAR, B, 0, 0, lo, hi), (F.COUNT, B, b, 0, lo, hi), (F.SUM, B, 0, 0, lo, hi), (F.MIN, B, a, 0, lo, hi),
            (F.MAX, B, b, 0, lo, hi), (F.MIN if q & 2 else F.MAX, B, 1, 0, lo, hi), (F.FIRST_VALUE, B, b, 0, lo, hi),
            (F.LAST_VALUE, B, a, 0, lo, hi)]


# ---- known answers --------------------------------------------------------------------------------------
def test_known_answers(gpu_ctx):
    ran = 0
    for name, part, order, flags, inputs, fns, expected, rows in F.load_kat():
        got = Window(gpu_ctx, part, order, flags, inputs, rows).run(fns)
        assert F.same_results(got, expected), name
        ran += 1
    assert ran >= 12


# ---- shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout_name", ["one", "each", "runs64", "runsT1", "random"])
def test_shapes(gpu_ctx, layout, layout_name):
    """Sizes around the wave, the one-workgroup limit (both paths run the same calls at S and S + 1) and
    the tile; bounds that put a block edge, a tile edge and a partition edge inside frames, widths of
    T and T + 1 positions among them."""
    T, S = layout
    for n in (0, 1, 2, 63, 64, 65, S, S + 1, T - 1, T, T + 1, 3 * T + 17):
        w = Window(gpu_ctx, *shaped_input(layout_name, n, T, n + 1), n)
        for q, (lo, hi) in enumerate(bounds_of(n, T)):
            w.check(framed_call(q, lo, hi), what=f"{layout_name} ({lo}, {hi})")


def test_shape_past_one_tile_of_the_word_scans(gpu_ctx, layout):
    T, S = layout
    n = 32 * T + 1
    w = Window(gpu_ctx, *shaped_input("random", n, T, 5), n)
    for q, (lo, hi) in enumerate(bounds_of(n, T)):
        w.check(framed_call(q, lo, hi), what=f"32T+1 ({lo}, {hi})")
    w = Window(gpu_ctx, *shaped_input("one", n, T, 6), n)
    for q, (lo, hi) in enumerate([(-T, T + 1), (-3 * T, -T), (-n - 1, n + 1), (-(n - 2), 0)]):
        w.check(framed_call(q, lo, hi), what=f"32T+1 one partition ({lo}, {hi})")


def test_first_last_under_the_older_frames_and_every_value_type(gpu_ctx, layout):
    T, S = layout
    for n in (S, 3 * T + 17):
        part, order, flags, inputs = shaped_input("random", n, T, 21)
        rng = np.random.default_rng(n)
        inputs = inputs + [(N.TYPE_INT32, rng.integers(-9, 9, n).astype(np.int32), rng.random(n) >= 0.3),
                           (N.TYPE_DATE32, rng.integers(0, 20000, n).astype(np.int32), None),
                           (N.TYPE_UINT8, rng.integers(0, 256, n).astype(np.uint8), rng.random(n) >= 0.3)]
        w = Window(gpu_ctx, part, order, flags, inputs, n)
        w.check([(fn, fr, 1, 0, 3, -3) for fn in (F.FIRST_VALUE, F.LAST_VALUE) for fr in (W.ROWS, W.RANGE, W.PARTITION)] +
                [(F.FIRST_VALUE, W.RANGE, 0, 0, 0, 0), (F.LAST_VALUE, W.RANGE, 0, 0, 0, 0)], what="older frames")
        for inp in (2, 3, 4):
            w.check([(F.FIRST_VALUE, B, inp, 0, -1, 1), (F.LAST_VALUE, B, inp, 0, -1, 1), (F.MIN, B, inp, 0, -3, 0),
                     (F.MAX, B, inp, 0, 0, T), (F.COUNT, B, inp, 0, -2, 2), (F.LAST_VALUE, W.ROWS, inp, 0, 0, 0)], what=f"input {inp}")
        w.check([(F.SUM, B, 2, 0, -T, 1)], what="int32 sum")


def test_small_case_against_the_fold(gpu_ctx):
    n = 200
    part, order, flags, inputs = shaped_input("random", n, 64, 3)
    w = Window(gpu_ctx, part, order, flags, inputs, n)
    for q, (lo, hi) in enumerate([(-2, -1), (-1, 1), (1, 3), (3, 1), (LO, -1), (2, HI), (-70, 0), (-n - 1, n + 1)]):
        w.check(framed_call(q, lo, hi), what="fold", ref=F.fold)


# ---- identities on the device ---------------------------------------------------------------------------
def test_unbounded_ends_equal_window_eval(gpu_ctx, layout):
    T, S = layout
    aggs = [(F.COUNT_STAR, 0), (F.COUNT, 1), (F.SUM, 0), (F.MIN, 0), (F.MIN, 1), (F.MAX, 0), (F.MAX, 1), (F.COUNT, 0)]
    for n in (S, 3 * T + 17):
        w = Window(gpu_ctx, *shaped_input("random", n, T, 8), n)
        for frame, lo, hi in ((W.ROWS, LO, 0), (W.PARTITION, LO, HI)):
            new = w.run([(fn, B, inp, 0, lo, hi) for fn, inp in aggs])
            old = w.run_old([(fn, frame, inp, 0) for fn, inp in aggs])
            assert F.same_results(new, old), (n, frame)
            assert F.same_results(w.run([(fn, frame, inp, 0, 1, -1) for fn, inp in aggs]), old), (n, frame)


def test_a_mixed_call_equals_one_function_per_call(gpu_ctx, layout):
    T, S = layout
    fns = [(F.SUM, W.RANGE, 0, 0, 0, 0), (F.MIN, B, 1, 0, -T, 0), (F.RANK, W.ROWS, 0, 0, 0, 0), (F.LAG, B, 1, 2, 5, -5),
           (F.MAX, W.ROWS, 1, 0, 0, 0), (F.SUM, B, 0, 0, -3, 3), (F.DENSE_RANK, B, 0, 0, LO, HI), (F.LAST_VALUE, B, 0, 0, 1, 70)]
    assert len(fns) == N.MAX_AGGS
    for n in (S, 3 * T + 17):
        w = Window(gpu_ctx, *shaped_input("random", n, T, 9), n)
        together = w.run(fns)
        alone = [w.run([f])[0] for f in fns]
        assert F.same_results(together, alone), n
        compare(together, F.vectorised(*w.args, fns, n), fns, n, "mixed")


def test_eight_bounded_min_max_of_eight_widths(gpu_ctx, layout):
    """Sixteen position scans in one call: the most a call can have."""
    T, S = layout
    for n in (S, 3 * T + 17):
        w = Window(gpu_ctx, *shaped_input("runsT1", n, T, 10), n)
        fns = [(F.MIN if k & 1 else F.MAX, B, k >> 2 & 1, 0, lo, hi)
               for k, (lo, hi) in enumerate([(-1, 0), (-1, 1), (0, 63), (-64, 0), (-T, -1), (-7, T - 7), (-T - 1, 1), (-T - 100, 100)])]
        assert len(F.scans(fns, n)[0]) == 2 * N.MAX_AGGS
        w.check(fns, what="eight widths")


# ---- refusals -------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gpu_ctx):
    n = 100
    rng = np.random.default_rng(9)
    cols = [to_device(gpu_ctx, c) for c in ((N.TYPE_INT64, rng.integers(-5, 5, n), rng.random(n) >= 0.2),
                                            (N.TYPE_FLOAT64, rng.normal(size=n), rng.random(n) >= 0.2),
                                            (N.TYPE_UTF8, [b"ab"[:i % 3] for i in range(n)], None))]
    perm = DeviceColumn.from_numpy(N.TYPE_INT32, np.arange(n, dtype=np.int32), ctx=gpu_ctx)
    ps = window_boundaries([], perm)
    calls = [
        (dict(fns=[(F.SUM, B, 0, 0, -1, 1)], pass_bounds=False), N.TYPE_INT64, F.INVALID_ARG),  # frame 3 without bounds
        (dict(fns=[(F.RANK, B, 0, 0, -1, 1)], pass_bounds=False), N.TYPE_INT64, F.INVALID_ARG),
        (dict(fns=[(13, B, 0, 0, -1, 1)]), N.TYPE_INT64, F.INVALID_ARG),
        (dict(fns=[(0, W.ROWS, 0, 0, 0, 0)]), N.TYPE_INT64, F.INVALID_ARG),
        (dict(fns=[(F.SUM, 4, 0, 0, -1, 1)]), N.TYPE_INT64, F.INVALID_ARG),
        (dict(fns=[(F.SUM, B, 1, 0, -1, 1)]), N.TYPE_INT64, F.UNSUPPORTED),  # SUM of FLOAT64
        (dict(fns=[(F.FIRST_VALUE, B, 2, 0, -1, 1)]), N.TYPE_INT64, F.UNSUPPORTED),  # FIRST_VALUE of UTF8
        (dict(fns=[(F.LAST_VALUE, W.ROWS, 2, 0, 0, 0)]), N.TYPE_INT64, F.UNSUPPORTED),
        (dict(fns=[(F.LAG, B, 0, -1, -1, 1)]), N.TYPE_INT64, F.INVALID_ARG),
        (dict(fns=[(F.FIRST_VALUE, B, 0, 0, -1, 1)], nullable=False), N.TYPE_INT64, F.INVALID_ARG),  # needs a validity buffer
        (dict(fns=[(F.LAST_VALUE, B, 1, 0, -1, 1)]), N.TYPE_INT64, F.INVALID_ARG),  # the output has the input's type
        (dict(fns=[(F.MIN, B, 3, 0, -1, 1)]), N.TYPE_INT64, F.INVALID_ARG),  # an input index out of range
        # a good function first: nothing of it is written either
        (dict(fns=[(F.MIN, B, 0, 0, -1, 1), (F.SUM, B, 1, 0, -1, 1)]), N.TYPE_INT64, F.UNSUPPORTED),
    ]
    for call, out_type, status in calls:
        fns = call["fns"]
        outs = [_filled(gpu_ctx, out_type, n, call.get("nullable", True)) for _ in fns]
        before = [_snapshot(o) for o in outs]
        with pytest.raises(N.QueryEngineError) as e:
            window_eval_frames(perm, ps, ps, cols, fns, outs=outs, pass_bounds=call.get("pass_bounds", True))
        gpu_ctx.synchronize()
        assert e.value.status == status, fns
        assert [_snapshot(o) for o in outs] == before, fns
    # the older frames need no bounds array
    got = window_eval_frames(perm, ps, ps, cols, [(F.FIRST_VALUE, W.PARTITION, 1, 0, 0, 0)], pass_bounds=False)
    gpu_ctx.synchronize()
    want = F.vectorised([], [], [], [(N.TYPE_FLOAT64, cols[1].to_numpy(), cols[1].valid_mask())], [(F.FIRST_VALUE, W.PARTITION, 0, 0, 0, 0)], n)
    assert F.same_results(results(got), want)


def test_order_entry_out_of_range_fails_the_call(gpu_ctx, layout):
    T, S = layout
    fns = framed_call(0, -T, 1)
    for n in (100, 3 * T + 17):
        w = Window(gpu_ctx, *shaped_input("random", n, T, 5), n)
        keys, _ = device_order(gpu_ctx, *w.args[:3], n)
        gpu_ctx.synchronize()
        for bad_value in (n, -1, 2**31 - 1):
            p = w.perm.to_numpy().copy()
            p[n // 2] = bad_value
            bad = DeviceColumn.from_numpy(N.TYPE_INT32, p, ctx=gpu_ctx)
            ps, gs = window_boundaries(keys[:1], bad), window_boundaries(keys, bad)
            before = [_snapshot(c) for c in w.dev]
            with pytest.raises(N.IllegalArgumentException, match="outside"):
                window_eval_frames(bad, ps, gs, w.dev, fns)
            gpu_ctx.synchronize()
            assert [_snapshot(c) for c in w.dev] == before
        w.check(fns, what="after a refused call")


# ---- determinism ----------------------------------------------------------------------------------------
def test_deterministic(gpu_ctx, layout):
    import torch

    T, S = layout
    n = 3 * T + 17
    args = shaped_input("random", n, T, 13)
    fns = framed_call(2, -T, 5)

    def once(ctx):
        return [(v.tobytes(), o.tobytes()) for v, o in Window(ctx, *args, n).run(fns)]

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


def _framed_plan(child, schema_in):
    """Over (k INT64, x INT64, f FLOAT64): PARTITION BY k ORDER BY f NULLS FIRST."""
    from kquery.expressions import ColumnExpression, FirstValue, LastValue, Rank, WindowCount, WindowMax, WindowMin, WindowSum

    x, f = ColumnExpression(1), ColumnExpression(2)
    fns = [WindowSum(x, bounds=(-2, 0)), WindowMax(f, bounds=(-1, 1)), FirstValue(f, bounds=(-1, 1)), LastValue(x, bounds=(0, 2)),
           Rank(), WindowCount(None, bounds=(N.UNBOUNDED_PRECEDING, -1)), WindowMin(f, N.FRAME_ROWS), FirstValue(x, N.FRAME_PARTITION)]
    types = [N.TYPE_INT64, N.TYPE_FLOAT64, N.TYPE_FLOAT64, N.TYPE_INT64, N.TYPE_INT64, N.TYPE_INT64, N.TYPE_FLOAT64, N.TYPE_INT64]
    assert [fn.output_type(N.TYPE_FLOAT64 if fn.expr is f else N.TYPE_INT64) for fn in fns] == types
    schema = Schema(list(schema_in.fields) + [Field(f"w{i}", t) for i, t in enumerate(types)])
    ref = [(F.SUM, B, 0, 0, -2, 0), (F.MAX, B, 1, 0, -1, 1), (F.FIRST_VALUE, B, 1, 0, -1, 1), (F.LAST_VALUE, B, 0, 0, 0, 2),
           (F.RANK, 0, 0, 0, 0, 0), (F.COUNT_STAR, B, 0, 0, LO, -1), (F.MIN, W.ROWS, 1, 0, 0, 0), (F.FIRST_VALUE, W.PARTITION, 0, 0, 0, 0)]
    return WindowExec(child, [ColumnExpression(0)], [(f, True, True)], fns, schema), ref


def test_windowexec_employee(gpu_ctx):
    """Per state by id: the salaries of the last three rows summed, the centred maximum, and the frame's
    first and last salary."""
    from kquery.expressions import ColumnExpression, FirstValue, LastValue, WindowMax, WindowSum

    with open(GOLD / "employee.csv", newline="", encoding="utf-8") as fh:
        rows = list(csv.DictReader(fh))
    ids = np.array([int(r["id"]) for r in rows], dtype=np.int64)
    states = [r["state"].encode() for r in rows]
    salary = np.array([int(r["salary"]) for r in rows], dtype=np.int64)
    pay = salary.astype(np.float64)
    schema = Schema([Field("id", N.TYPE_INT64), Field("state", N.TYPE_UTF8), Field("salary", N.TYPE_INT64), Field("pay", N.TYPE_FLOAT64)])
    cols = [(N.TYPE_INT64, ids, None), (N.TYPE_UTF8, states, None), (N.TYPE_INT64, salary, None), (N.TYPE_FLOAT64, pay, None)]
    src = _Batches(schema, [RecordBatch(schema, [to_device(gpu_ctx, c) for c in cols])])
    fns = [WindowSum(ColumnExpression(2), bounds=(-2, 0)), WindowMax(ColumnExpression(3), bounds=(-1, 1)),
           FirstValue(ColumnExpression(3), bounds=(-1, 1)), LastValue(ColumnExpression(2), bounds=(-1, 1))]
    out_schema = Schema(list(schema.fields) + [Field("sum3", N.TYPE_INT64), Field("top", N.TYPE_FLOAT64), Field("first", N.TYPE_FLOAT64),
                                               Field("last", N.TYPE_INT64)])
    (b,) = list(WindowExec(src, [ColumnExpression(1)], [(ColumnExpression(0), True, False)], fns, out_schema).execute())
    gpu_ctx.synchronize()
    assert b.field(0).to_pylist() == [1, 2, 3]
    want = F.fold([cols[1]], [cols[0]], [0], [cols[2], cols[3]],
                  [(F.SUM, B, 0, 0, -2, 0), (F.MAX, B, 1, 0, -1, 1), (F.FIRST_VALUE, B, 1, 0, -1, 1), (F.LAST_VALUE, B, 0, 0, -1, 1)])
    assert F.same_results(_batch_results(b, 4), want)
    assert b.field(4).to_pylist() == [1337, 2003, 0] and b.field(5).to_pylist() == [1337.0, 1337.0, 0.0]
    assert b.field(6).to_pylist() == [1337.0, 1337.0, 0.0] and b.field(7).to_pylist() == [666, 666, 0]


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
    many, ref = _framed_plan(_Batches(schema, [batch(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]), schema)
    single, _ = _framed_plan(_Batches(schema, [batch(0, n)]), schema)
    out_many, out_single = list(many.execute()), list(single.execute())
    gpu_ctx.synchronize()
    assert len(out_many) == len(out_single) == 1 and out_many[0].rowCount() == n
    assert np.array_equal(out_many[0].field(0).to_numpy(), k)
    want = F.vectorised([(N.TYPE_INT64, k, None)], [(N.TYPE_FLOAT64, f, fv)], [N.SORT_NULLS_FIRST],
                        [(N.TYPE_INT64, x, xv), (N.TYPE_FLOAT64, f, fv)], ref, n)
    assert F.same_results(_batch_results(out_many[0], 3), want)
    assert F.same_results(_batch_results(out_single[0], 3), want)


def test_windowexec_calls_the_entry_point_its_plan_needs(gpu_ctx, monkeypatch):
    """A plan without bounds and without FIRST / LAST still runs qe_window_eval; one with either runs
    qe_window_eval_frames."""
    from kquery import operators
    from kquery.expressions import ColumnExpression, FirstValue, Lag, Rank, WindowCount, WindowMin, WindowSum

    x = np.arange(1, 301, dtype=np.int64)
    schema = Schema([Field("x", N.TYPE_INT64)])
    src = _Batches(schema, [RecordBatch(schema, [DeviceColumn.from_numpy(N.TYPE_INT64, x, ctx=gpu_ctx)])])

    def refuse(*a, **kw):
        raise AssertionError("the wrong entry point")

    old = [Rank(), WindowSum(ColumnExpression(0), N.FRAME_ROWS), WindowMin(ColumnExpression(0)), Lag(ColumnExpression(0), 1),
           WindowCount(None, N.FRAME_PARTITION)]
    out_schema = Schema(list(schema.fields) + [Field(f"w{i}", N.TYPE_INT64) for i in range(len(old))])
    with monkeypatch.context() as m:
        m.setattr(operators, "window_eval_frames", refuse)
        (b,) = list(WindowExec(src, [], [], old, out_schema).execute())
        gpu_ctx.synchronize()
        assert np.array_equal(b.field(2).to_numpy(), np.cumsum(x))
    for new in (WindowSum(ColumnExpression(0), bounds=(-1, 0)), FirstValue(ColumnExpression(0), N.FRAME_ROWS)):
        plan = WindowExec(src, [], [], [Rank(), new], Schema(list(schema.fields) + [Field("r", N.TYPE_INT64), Field("w", N.TYPE_INT64)]))
        with monkeypatch.context() as m:
            m.setattr(operators, "window_eval", refuse)
            (b,) = list(plan.execute())
            gpu_ctx.synchronize()
        with monkeypatch.context() as m:
            m.setattr(operators, "window_eval_frames", refuse)
            with pytest.raises(AssertionError, match="wrong entry point"):
                list(plan.execute())
    assert np.array_equal(b.field(2).to_numpy(), np.ones(300, dtype=np.int64))  # FIRST_VALUE over [P, i]: the first row's x
