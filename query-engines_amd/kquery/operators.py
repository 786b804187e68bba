"""Physical operators (Main.kt:442-446, :564-660) over device-resident RecordBatches.

``ScanExec`` / ``ProjectionExec`` / ``HashAggregateExec`` keep the reference's names, arguments
and pull-based ``execute()`` sequence; ``SelectionExec`` is the north star's filter operator
(absent from the reference). ``fuse`` is the planner hook (the reference's selection
point is createPhysicalPlan, Main.kt:680-706): it rewrites HashAggregateExec over a
Selection/Projection/Scan chain into ``FusedHashAggregateExec`` — one HIP kernel pass over HBM.
"""
from __future__ import annotations

from typing import Iterator, List, Optional, Sequence

from . import native as N
from .aggregate import HashAggregateState, dictionary_keys, output_type
from .columnar import DeviceColumn, DeviceCount, Field, RecordBatch, Schema
from .expressions import (
    AggregateExpression,
    AndExpression,
    ArithmeticExpression,
    ColumnExpression,
    ComparisonExpression,
    Expression,
    LiteralDoubleExpression,
    LiteralLongExpression,
    ScalarColumn,
)


class PhysicalPlan:
    def schema(self) -> Schema:
        raise NotImplementedError

    def execute(self) -> Iterator[RecordBatch]:
        raise NotImplementedError

    def children(self) -> List["PhysicalPlan"]:
        raise NotImplementedError


class ScanExec(PhysicalPlan):
    """Main.kt:564-580."""

    def __init__(self, ds, projection: Sequence[str]):
        self.ds = ds
        self.projection = list(projection)

    def schema(self) -> Schema:
        return self.ds.schema().select(self.projection)

    def execute(self) -> Iterator[RecordBatch]:
        return self.ds.scan(self.projection)

    def children(self) -> List[PhysicalPlan]:
        return []

    def __repr__(self) -> str:
        return f"ScanExec: schema={self.schema()}, projection={self.projection}"


class ProjectionExec(PhysicalPlan):
    """Main.kt:582-603: per batch, evaluate every expression; row count and order unchanged."""

    def __init__(self, input: PhysicalPlan, schema: Schema, expr: Sequence[Expression]):  # noqa: A002
        self.input = input
        self._schema = schema
        self.expr = list(expr)

    def schema(self) -> Schema:
        return self._schema

    def execute(self) -> Iterator[RecordBatch]:
        for batch in self.input.execute():
            yield RecordBatch(self._schema, [e.evaluate(batch) for e in self.expr])

    def children(self) -> List[PhysicalPlan]:
        return [self.input]

    def __repr__(self) -> str:
        return f"ProjectionExec: {self.expr}"


class SelectionExec(PhysicalPlan):
    """Filter (build-defined): keeps rows whose predicate is true (null -> dropped), in order.
    K3b order-preserving compaction (qe_filter_apply)."""

    def __init__(self, input: PhysicalPlan, expr: Expression):  # noqa: A002
        self.input = input
        self.expr = expr

    def schema(self) -> Schema:
        return self.input.schema()

    def execute(self) -> Iterator[RecordBatch]:
        for batch in self.input.execute():
            mask = self.expr.evaluate(batch)
            if not isinstance(mask, DeviceColumn) or mask.type != N.TYPE_BOOL:
                raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "selection predicate must be BOOLEAN")
            yield filter_batch(batch, mask)

    def children(self) -> List[PhysicalPlan]:
        return [self.input]

    def __repr__(self) -> str:
        return f"SelectionExec: {self.expr}"


def _alloc_like(c: DeviceColumn, n: int, ctx) -> DeviceColumn:
    if c.type != N.TYPE_UTF8:
        return DeviceColumn.empty(c.type, n, c.nullable, ctx=ctx)
    import torch

    from .columnar import bitmap_bytes

    nbytes = int(c.offsets[c.length].item() - c.offsets[0].item()) if c.length else 0
    dev = ctx.torch_device
    return DeviceColumn(N.TYPE_UTF8, n, torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev),
                        torch.zeros(max(bitmap_bytes(n), 4), dtype=torch.uint8, device=dev) if c.nullable else None,
                        torch.empty(n + 1, dtype=torch.int32, device=dev), ctx)


# How SelectionExec compacts non-nullable int64 / fp64 columns: "select_project" (one pass of the
# select-project kernel with the mask as the selection, then a wait for its row count: C2 10M rows
# 0.130-0.133 ms per cmp -> compact -> arith chain) or "gather" (count, scan and gather with the
# count left in HBM and read back at the end, qe_filter_apply_async: 0.148 ms; the form every other
# fixed-width batch takes).
SELECTION_COMPACTION = "select_project"


_SELPROJ_SPECS = {}  # column count -> the compaction's select-project spec (read-only once built)


def _compact_selproj(batch: RecordBatch, cols, mask: DeviceColumn) -> Optional[RecordBatch]:
    """The compaction through the select-project kernel (qe_select_project_async with the mask
    column as the selection and the columns themselves as the outputs: one pass with a decoupled
    look-back instead of count, scan and gather), then its row count. None: the kernel cannot take
    the plan."""
    ctx = mask.ctx
    n = mask.length
    spec = _SELPROJ_SPECS.get(len(cols))
    if spec is None:  # (the spec depends only on the column count: built once)
        spec = N.QeSelectSpec()
        spec.mask_col = len(cols)
        spec.nterms = 0
        spec.nout = len(cols)
        for i in range(len(cols)):
            spec.outputs[i].ntokens = 1
            spec.outputs[i].tokens[0] = N.QeToken(N.TOK_COL, i, N.QeScalar())
        _SELPROJ_SPECS[len(cols)] = spec
    outs = [DeviceColumn.empty(c.type, n, False, ctx=ctx) for c in cols]
    cc = (N.QeColumn * (len(cols) + 1))(*([c.as_c() for c in cols] + [mask.as_c()]))
    oc = (N.QeColumn * len(outs))(*[o.as_c() for o in outs])
    pending = N.C.c_void_p()
    st = N.lib().qe_select_project_async(ctx.handle, cc, len(cols) + 1, N.C.byref(spec), oc, N.C.byref(pending))
    if st == N.QE_ERR_UNSUPPORTED:
        return None
    N.check(st)
    cnt = N.C.c_int64()
    N.check(N.lib().qe_select_pending_wait(pending, N.C.byref(cnt)))
    for o in outs:
        o.length = cnt.value
    return RecordBatch(batch.schema, outs)


def filter_batch(batch: RecordBatch, mask: DeviceColumn) -> RecordBatch:
    """SelectionExec's compaction. Fixed-width columns (at most 8) take the stream-ordered form
    (qe_filter_apply_async): outputs sized by the mask, the selected-row count left in HBM and read
    back only when a consumer needs a length (DeviceColumn.length), so cmp -> filter -> arith runs
    without a host round trip. UTF8 columns take qe_filter_apply (their byte sizes need the count)."""
    ctx = mask.ctx
    cols = batch.fields
    if (SELECTION_COMPACTION == "select_project" and 0 < len(cols) < N.MAX_COLS and len(cols) <= N.MAX_AGGS
            and all(isinstance(c, DeviceColumn) and c.type in (N.TYPE_INT64, N.TYPE_FLOAT64) and not c.nullable
                    for c in cols)):
        done = _compact_selproj(batch, cols, mask)
        if done is not None:
            return done
    if (0 < len(cols) <= N.MAX_COLS and all(isinstance(c, DeviceColumn) and c.type in N.FIXED_WIDTH for c in cols)):
        import torch

        n = mask.length
        outs = [DeviceColumn.empty(c.type, n, c.nullable, ctx=ctx) for c in cols]
        cnt = DeviceCount(torch.empty(1, dtype=torch.int64, device=ctx.torch_device), ctx)
        mc = mask.as_c()
        ins = (N.QeColumn * len(cols))(*[c.as_c() for c in cols])
        os_ = (N.QeColumn * len(cols))(*[o.as_c() for o in outs])
        N.check(N.lib().qe_filter_apply_async(ctx.handle, N.C.byref(mc), ins, len(cols), os_, cnt.ptr()))
        for o in outs:
            o.pending = cnt
        return RecordBatch(batch.schema, outs)
    cnt = N.C.c_int64()
    mc = mask.as_c()
    N.check(N.lib().qe_filter_count(ctx.handle, N.C.byref(mc), N.C.byref(cnt)))
    n = cnt.value
    cols = batch.fields
    for c in cols:
        if not isinstance(c, DeviceColumn):
            raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "selection input must be device columns")
    outs = [_alloc_like(c, n, ctx) for c in cols]
    done: list = [None] * len(cols)
    # qe_filter_apply gathers up to 8 columns per launch
    for s in range(0, len(cols), N.MAX_COLS):
        part = cols[s:s + N.MAX_COLS]
        ins = (N.QeColumn * len(part))(*[c.as_c() for c in part])
        os_ = (N.QeColumn * len(part))(*[o.as_c() for o in outs[s:s + N.MAX_COLS]])
        got = N.C.c_int64()
        N.check(N.lib().qe_filter_apply(ctx.handle, N.C.byref(mc), ins, len(part), os_, N.C.byref(got)))
        for k, o in enumerate(outs[s:s + N.MAX_COLS]):
            o.length = got.value
            done[s + k] = o
    return RecordBatch(batch.schema, done)


def sort_layout():
    """(rows per tile of the multi-workgroup sort passes, largest single-workgroup n)."""
    t, s = N.C.c_int32(), N.C.c_int32()
    N.check(N.lib().qe_sort_layout(N.C.byref(t), N.C.byref(s)))
    return t.value, s.value


def sort_indices(keys: Sequence[DeviceColumn], flags: Sequence[int], limit: Optional[int] = None) -> DeviceColumn:
    """qe_sort_indices: the INT32 row indices of the stable order of `keys` (the first key the most
    significant; flags: N.SORT_DESC | N.SORT_NULLS_FIRST per key), all of them or the first `limit`."""
    ctx = keys[0].ctx
    n = keys[0].length
    lim = -1 if limit is None else int(limit)
    out = DeviceColumn.empty(N.TYPE_INT32, n if lim < 0 else min(lim, n), False, ctx=ctx)
    kc = (N.QeColumn * len(keys))(*[k.as_c() for k in keys])
    fl = (N.C.c_int32 * len(keys))(*[int(f) for f in flags])
    oc = out.as_c()
    N.check(N.lib().qe_sort_indices(ctx.handle, kc, fl, len(keys), lim, N.C.byref(oc)))
    out.length = oc.length
    return out


def topk_indices(keys: Sequence[DeviceColumn], flags: Sequence[int], k: int, mode: int = N.TOPK_AUTO) -> DeviceColumn:
    """qe_topk_indices: the first min(k, n) row indices of the stable order of `keys` (sort_indices
    with limit=k, entry for entry). mode: N.TOPK_AUTO picks radix selection for a small k and the
    full sort otherwise; N.TOPK_SELECT / N.TOPK_SORT force one."""
    ctx = keys[0].ctx
    out = DeviceColumn.empty(N.TYPE_INT32, max(0, min(int(k), keys[0].length)), False, ctx=ctx)
    kc = (N.QeColumn * len(keys))(*[c.as_c() for c in keys])
    fl = (N.C.c_int32 * len(keys))(*[int(f) for f in flags])
    oc = out.as_c()
    N.check(N.lib().qe_topk_indices(ctx.handle, kc, fl, len(keys), int(k), int(mode), N.C.byref(oc)))
    out.length = oc.length
    return out


def topk_last_stats(ctx):
    """qe_topk_last_stats: (path taken: 0 sort / 1 selection, digit steps, candidates handed to the
    final sort, host read-backs) of the context's last topk_indices call."""
    st = (N.C.c_int64 * 4)()
    N.check(N.lib().qe_topk_last_stats(ctx.handle, st))
    return tuple(st)


def take(indices: DeviceColumn, cols: Sequence[DeviceColumn],
         utf8_bytes: Optional[Sequence[Optional[int]]] = None) -> List[DeviceColumn]:
    """qe_take: row indices[i] of every column, validity included. utf8_bytes[c]: the value bytes
    UTF8 output c needs (the sum of the taken lengths); None sizes it as the input's bytes, which
    is enough when no index repeats."""
    return _take(indices, cols, utf8_bytes, False)


def take_or_null(indices: DeviceColumn, cols: Sequence[DeviceColumn],
                 utf8_bytes: Optional[Sequence[Optional[int]]] = None) -> List[DeviceColumn]:
    """qe_take_or_null: as take, but index -1 means "no row" and gives a null row, so every output
    is nullable (the build side of a LEFT join)."""
    return _take(indices, cols, utf8_bytes, True)


def _take(indices: DeviceColumn, cols: Sequence[DeviceColumn], utf8_bytes, or_null: bool) -> List[DeviceColumn]:
    import torch

    from .columnar import bitmap_bytes

    ctx = indices.ctx
    m = indices.length
    dev = ctx.torch_device
    outs, caps = [], []
    for i, c in enumerate(cols):
        nullable = c.nullable or or_null
        if c.type != N.TYPE_UTF8:
            outs.append(DeviceColumn.empty(c.type, m, nullable, ctx=ctx))
            caps.append(0)
            continue
        cap = utf8_bytes[i] if utf8_bytes is not None and utf8_bytes[i] is not None else None
        if cap is None:
            cap = int(c.offsets[c.length].item() - c.offsets[0].item()) if c.length else 0
        outs.append(DeviceColumn(N.TYPE_UTF8, m, torch.empty(max(cap, 1), dtype=torch.uint8, device=dev),
                                 torch.zeros(max(bitmap_bytes(m), 4), dtype=torch.uint8, device=dev) if nullable else None,
                                 torch.empty(m + 1, dtype=torch.int32, device=dev), ctx))
        outs[-1].max_len = c.max_len
        caps.append(cap)
    ic = indices.as_c()
    fn = N.lib().qe_take_or_null if or_null else N.lib().qe_take
    for s in range(0, len(cols), N.MAX_COLS):  # qe_take gathers up to 8 columns per launch
        part = cols[s:s + N.MAX_COLS]
        ins = (N.QeColumn * len(part))(*[c.as_c() for c in part])
        os_ = (N.QeColumn * len(part))(*[o.as_c() for o in outs[s:s + N.MAX_COLS]])
        cp = (N.C.c_int64 * len(part))(*caps[s:s + N.MAX_COLS])
        N.check(fn(ctx.handle, N.C.byref(ic), ins, len(part), os_, cp))
    return outs


# ---------------------------------------------------------------------------------------------------
# Window functions (build-defined): run boundaries along a sort, scans, per-row evaluation
# ---------------------------------------------------------------------------------------------------
_WIN_NULLABLE = (N.WIN_SUM, N.WIN_MIN, N.WIN_MAX, N.WIN_LAG, N.WIN_LEAD, N.WIN_FIRST_VALUE, N.WIN_LAST_VALUE)
_WIN_INPUT_TYPE = (N.WIN_MIN, N.WIN_MAX, N.WIN_LAG, N.WIN_LEAD, N.WIN_FIRST_VALUE, N.WIN_LAST_VALUE)


def window_layout():
    """(positions per tile of the multi-workgroup scans, largest single-workgroup n)."""
    t, s = N.C.c_int32(), N.C.c_int32()
    N.check(N.lib().qe_window_layout(N.C.byref(t), N.C.byref(s)))
    return t.value, s.value


def window_boundaries(keys: Sequence[DeviceColumn], order: DeviceColumn) -> DeviceColumn:
    """qe_window_boundaries: the BOOL column whose bit i says that position i of the permutation
    `order` starts a run of rows equal on every key (no keys: only bit 0). Stream-ordered."""
    ctx = order.ctx
    out = DeviceColumn.empty(N.TYPE_BOOL, order.length, False, ctx=ctx)
    kc = (N.QeColumn * max(len(keys), 1))(*[k.as_c() for k in keys])
    oc, sc = order.as_c(), out.as_c()
    N.check(N.lib().qe_window_boundaries(ctx.handle, kc, len(keys), N.C.byref(oc), N.C.byref(sc)))
    return out


def window_eval(order: DeviceColumn, part_starts: DeviceColumn, peer_starts: DeviceColumn,
                inputs: Sequence[DeviceColumn], fns, outs: Optional[Sequence[DeviceColumn]] = None) -> List[DeviceColumn]:
    """qe_window_eval: fns is a sequence of (fn, frame, input index, offset); one output column per
    function at the input's row positions (`outs`: caller-provided outputs instead of fresh ones)."""
    ctx = order.ctx
    n = part_starts.length
    if outs is None:
        outs = []
        for fn, _, inp, _ in fns:
            t = inputs[inp].type if fn in _WIN_INPUT_TYPE and 0 <= inp < len(inputs) else N.TYPE_INT64
            outs.append(DeviceColumn.empty(t if t in N.FIXED_WIDTH else N.TYPE_INT64, n, fn in _WIN_NULLABLE, ctx=ctx))
    fc = (N.QeWindowFn * max(len(fns), 1))(*[N.QeWindowFn(int(fn), int(fr), int(inp), 0, int(off)) for fn, fr, inp, off in fns])
    ic = (N.QeColumn * max(len(inputs), 1))(*[c.as_c() for c in inputs])
    oc = (N.QeColumn * max(len(outs), 1))(*[o.as_c() for o in outs])
    rc, pc, gc = order.as_c(), part_starts.as_c(), peer_starts.as_c()
    N.check(N.lib().qe_window_eval(ctx.handle, N.C.byref(rc), N.C.byref(pc), N.C.byref(gc), ic, len(inputs), fc, len(fns), oc))
    return list(outs)


def window_eval_frames(order: DeviceColumn, part_starts: DeviceColumn, peer_starts: DeviceColumn,
                       inputs: Sequence[DeviceColumn], fns, outs: Optional[Sequence[DeviceColumn]] = None,
                       pass_bounds: bool = True) -> List[DeviceColumn]:
    """qe_window_eval_frames: fns is a sequence of (fn, frame, input index, offset, lo, hi), lo and hi
    the bounds of a FRAME_ROWS_BETWEEN frame (any int64; ignored under the other frames); otherwise as
    window_eval. pass_bounds=False passes a null bounds array."""
    ctx = order.ctx
    n = part_starts.length
    if outs is None:
        outs = []
        for fn, _, inp, _, _, _ in fns:
            t = inputs[inp].type if fn in _WIN_INPUT_TYPE and 0 <= inp < len(inputs) else N.TYPE_INT64
            outs.append(DeviceColumn.empty(t if t in N.FIXED_WIDTH else N.TYPE_INT64, n, fn in _WIN_NULLABLE, ctx=ctx))
    fc = (N.QeWindowFn * max(len(fns), 1))(*[N.QeWindowFn(int(fn), int(fr), int(inp), 0, int(off)) for fn, fr, inp, off, _, _ in fns])
    bc = (N.QeWindowBounds * max(len(fns), 1))(*[N.QeWindowBounds(int(lo), int(hi)) for _, _, _, _, lo, hi in fns])
    ic = (N.QeColumn * max(len(inputs), 1))(*[c.as_c() for c in inputs])
    oc = (N.QeColumn * max(len(outs), 1))(*[o.as_c() for o in outs])
    rc, pc, gc = order.as_c(), part_starts.as_c(), peer_starts.as_c()
    N.check(N.lib().qe_window_eval_frames(ctx.handle, N.C.byref(rc), N.C.byref(pc), N.C.byref(gc), ic, len(inputs), fc,
                                          bc if pass_bounds else None, len(fns), oc))
    return list(outs)


class WindowExec(PhysicalPlan):
    """fn(...) OVER (PARTITION BY ... ORDER BY ...) (build-defined). A pipeline breaker like
    SortExec: drains its input into one batch (concat_batches), evaluates the key and input
    expressions, sorts by (partition keys ascending, then order keys) to row indices
    (qe_sort_indices), finds the partition and peer boundaries along them (qe_window_boundaries,
    twice) and evaluates every function in one qe_window_eval (one qe_window_eval_frames when a
    function has bounds=(lo, hi) or is FirstValue / LastValue). partition_by: expressions; order_by:
    (Expression, ascending, nulls_first) triples; functions: WindowExpressions. Yields ONE batch in the
    INPUT's row order: the input's columns, then one column per function (`schema` names them). An
    empty input gives a 0-row batch; without keys the whole input is one partition of peers and no
    sort runs."""

    def __init__(self, input: PhysicalPlan, partition_by, order_by, functions, schema: Schema):  # noqa: A002
        if len(partition_by) + len(order_by) > N.MAX_KEYS:
            raise N.IllegalArgumentException(N.QE_ERR_INVALID_ARG,
                                             f"a window takes at most {N.MAX_KEYS} partition and order keys together")
        if len(functions) > N.MAX_AGGS:
            raise N.IllegalArgumentException(N.QE_ERR_INVALID_ARG, f"a window takes at most {N.MAX_AGGS} functions")
        self.input = input
        self.partition_by = list(partition_by)
        self.order_by = [(e, bool(asc), bool(nf)) for e, asc, nf in order_by]
        self.functions = list(functions)
        self._schema = schema

    def schema(self) -> Schema:
        return self._schema

    def children(self) -> List[PhysicalPlan]:
        return [self.input]

    def execute(self) -> Iterator[RecordBatch]:
        import torch

        from .columnar import Context, concat_batches

        schema = self._schema
        batches = [b for b in self.input.execute() if b.fields]
        for b in batches:
            for c in b.fields:
                if not isinstance(c, DeviceColumn):
                    raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "window input must be device columns")
        if not batches:
            ctx = Context.get(0)
            yield RecordBatch(schema, [
                DeviceColumn.from_strings([], ctx=ctx) if f.dataType == N.TYPE_UTF8
                else DeviceColumn.empty(f.dataType, 0, True, ctx=ctx) for f in schema.fields])
            return
        batch = concat_batches(batches)
        part = [e.evaluate(batch) for e in self.partition_by]
        okeys = [e.evaluate(batch) for e, _, _ in self.order_by]
        inputs: List[DeviceColumn] = []
        fns = []
        for f in self.functions:
            slot = 0
            if f.expr is not None:
                cv = f.expr.evaluate(batch)
                slot = next((i for i, c in enumerate(inputs) if c is cv), len(inputs))
                if slot == len(inputs):
                    inputs.append(cv)
            fns.append((f.fn, f.frame, slot, f.offset) + (f.bounds or (0, 0)))
        for c in part + okeys + inputs:
            if not isinstance(c, DeviceColumn):
                raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "a window key or input must evaluate to a column")
        if len(inputs) > N.MAX_COLS:
            raise N.IllegalArgumentException(N.QE_ERR_INVALID_ARG, f"a window takes at most {N.MAX_COLS} distinct inputs")
        ctx = batch.fields[0].ctx
        n = batch.fields[0].length
        keys = part + okeys
        if keys:
            flags = [0] * len(part) + [(0 if asc else N.SORT_DESC) | (N.SORT_NULLS_FIRST if nf else 0)
                                       for _, asc, nf in self.order_by]
            order = sort_indices(keys, flags)
        else:
            order = DeviceColumn(N.TYPE_INT32, n, torch.arange(max(n, 1), dtype=torch.int32, device=ctx.torch_device), ctx=ctx)
        part_starts = window_boundaries(part, order)
        peer_starts = window_boundaries(keys, order) if okeys else part_starts
        if any(f.frame == N.FRAME_ROWS_BETWEEN or f.fn in (N.WIN_FIRST_VALUE, N.WIN_LAST_VALUE) for f in self.functions):
            outs = window_eval_frames(order, part_starts, peer_starts, inputs, fns)
        else:  # a plan without the newer ids runs the call it always ran
            outs = window_eval(order, part_starts, peer_starts, inputs, [f[:4] for f in fns])
        yield RecordBatch(schema, list(batch.fields) + outs)

    def __repr__(self) -> str:
        return f"WindowExec: partition_by={self.partition_by}, order_by={self.order_by}, functions={self.functions}"


# ---------------------------------------------------------------------------------------------------
# Equi-join (build-defined): device hash build / probe -> row-index pairs
# ---------------------------------------------------------------------------------------------------
class JoinTable:
    """The device hash table of one build side (qe_join_build); close() releases it."""

    def __init__(self, ctx, handle, rows: int = 0):
        self.ctx = ctx
        self.handle = handle
        self.rows = rows  # the build side's rows, null keys included

    def close(self) -> None:
        if getattr(self, "handle", None) is not None:
            N.lib().qe_join_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def join_build(key: DeviceColumn) -> JoinTable:
    """qe_join_build over one key column (INT64, INT32, DATE32, UINT8, BOOL or FLOAT64; null keys
    are left out)."""
    h = N.C.c_void_p()
    kc = key.as_c()
    N.check(N.lib().qe_join_build(key.ctx.handle, N.C.byref(kc), N.C.byref(h)))
    return JoinTable(key.ctx, h, key.length)


def join_stats(table: JoinTable):
    """(non-null build rows, distinct keys, longest run of equal keys, slots)."""
    v = [N.C.c_int64() for _ in range(4)]
    N.check(N.lib().qe_join_stats(table.handle, *[N.C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def join_probe(table: JoinTable, key: DeviceColumn, kind: int = N.JOIN_INNER, capacity: Optional[int] = None):
    """qe_join_probe: the (probe row, build row) INT32 index columns of one probe batch, ordered by
    probe row, then build row; N.JOIN_LEFT pairs an unmatched row with -1. `kind | N.JOIN_TRACK`: the
    same pairs, and the build keys the batch matched are marked (join_build_rows). The first try sizes the
    outputs at `capacity` rows (default: the batch's rows, which a build side of unique keys never
    exceeds); a short one is carved again at the exact count the call reported: two tries at most."""
    ctx = key.ctx
    cap = key.length if capacity is None else int(capacity)
    kc = key.as_c()
    pairs = N.C.c_int64()
    for attempt in range(2):
        pi = DeviceColumn.empty(N.TYPE_INT32, cap, False, ctx=ctx)
        bi = DeviceColumn.empty(N.TYPE_INT32, cap, False, ctx=ctx)
        pc, bc = pi.as_c(), bi.as_c()
        st = N.lib().qe_join_probe(table.handle, N.C.byref(kc), int(kind), N.C.byref(pc), N.C.byref(bc), N.C.byref(pairs))
        if st == N.QE_ERR_CAPACITY and attempt == 0:
            cap = pairs.value
            continue
        N.check(st)
        pi.length = bi.length = pairs.value
        return pi, bi
    raise AssertionError("unreachable")


def join_probe_mask(table: JoinTable, key: DeviceColumn, anti: bool = False) -> DeviceColumn:
    """qe_join_probe_mask: BOOL mask of the probe rows that have a match (anti: that have none; a
    null key has none). Stream-ordered."""
    mask = DeviceColumn.empty(N.TYPE_BOOL, key.length, False, ctx=key.ctx)
    kc, mc = key.as_c(), mask.as_c()
    N.check(N.lib().qe_join_probe_mask(table.handle, N.C.byref(kc), 1 if anti else 0, N.C.byref(mc)))
    return mask


def join_mark(table: JoinTable, key: DeviceColumn) -> None:
    """qe_join_mark: marks the build keys that `key`'s non-null rows equal, as a tracked probe does,
    and writes nothing else. Stream-ordered."""
    kc = key.as_c()
    N.check(N.lib().qe_join_mark(table.handle, N.C.byref(kc)))


def join_build_rows(table: JoinTable, matched: bool) -> DeviceColumn:
    """qe_join_build_rows: the ascending INT32 indices of the build rows whose key is marked
    (matched) or is not (unmatched: the null-key rows are among these). Sized at the build side's
    rows, so one call always suffices."""
    idx = DeviceColumn.empty(N.TYPE_INT32, table.rows, False, ctx=table.ctx)
    ic = idx.as_c()
    rows = N.C.c_int64()
    N.check(N.lib().qe_join_build_rows(table.handle, 1 if matched else 0, N.C.byref(ic), N.C.byref(rows)))
    idx.length = rows.value
    return idx


def join_clear_marks(table: JoinTable) -> None:
    """qe_join_clear_marks: every mark clear again (the table can serve another left input)."""
    N.check(N.lib().qe_join_clear_marks(table.handle))


def _taken_bytes(indices: DeviceColumn, cols: Sequence[DeviceColumn]) -> List[Optional[int]]:
    """Per UTF8 column the value bytes a take by `indices` writes: the sum of the taken lengths
    (indices repeat in a join, so the input's byte count is no bound). -1 takes nothing."""
    import torch

    out: List[Optional[int]] = []
    idx = indices.values[: indices.length].to(torch.int64)
    hit = idx >= 0
    idx = idx.clamp(min=0)
    for c in cols:
        if c.type != N.TYPE_UTF8 or indices.length == 0 or c.length == 0:
            out.append(0 if c.type == N.TYPE_UTF8 else None)
            continue
        lens = (c.offsets[1: c.length + 1] - c.offsets[: c.length]).to(torch.int64)
        out.append(int((lens[idx] * hit).sum().item()))
    return out


def _and_validity(cols: Sequence[DeviceColumn]):
    """The AND of the columns' validity bitmaps (None: no column is nullable)."""
    v = None
    for c in cols:
        if c.validity is not None:
            v = c.validity.clone() if v is None else v & c.validity
    return v


class _JoinKeyEncoder:
    """Turns the key columns of either side into the one fixed-width key column qe_join_* takes. One
    fixed-width key passes through. A lone UTF8 key becomes wide INT64 dictionary codes; several keys
    become one INT32 key-tuple code (UTF8 members through INT32 string codes first) whose validity is
    the AND of the members': a null in any member matches nothing. The dictionaries, one per key
    position, are shared by both sides, so equal values get equal codes; values only the probe side
    has get fresh codes that match nothing."""

    def __init__(self, ctx, types: Sequence[int]):
        from .strdict import StringDictionary

        self.ctx = ctx
        self.types = list(types)
        self.lone_utf8 = len(self.types) == 1 and self.types[0] == N.TYPE_UTF8
        self.strings = {}
        self.tuples = None
        if self.lone_utf8:
            self.strings[0] = StringDictionary(ctx, wide=True)
        elif len(self.types) > 1:
            for k, t in enumerate(self.types):
                if t == N.TYPE_UTF8:
                    self.strings[k] = StringDictionary(ctx)
            self.tuples = StringDictionary(ctx)

    def encode(self, cols: Sequence[DeviceColumn]) -> DeviceColumn:
        for k, (c, t) in enumerate(zip(cols, self.types)):
            if not isinstance(c, DeviceColumn):
                raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "a join key must evaluate to a column")
            if len(self.types) > 1 and c.type != t:
                raise N.IllegalArgumentException(
                    N.QE_ERR_INVALID_ARG, f"join key {k}: types {c.type} and {t} differ (composite keys pair equal types)")
        n = cols[0].length
        if len(cols) == 1 and not self.lone_utf8:
            return cols[0]
        if self.lone_utf8:
            if cols[0].type != N.TYPE_UTF8:
                raise N.IllegalArgumentException(N.QE_ERR_INVALID_ARG, "a UTF8 join key pairs only with UTF8")
            if n == 0:
                return DeviceColumn.empty(N.TYPE_INT64, 0, False, ctx=self.ctx)
            return self.strings[0].encode(cols[0])
        if n == 0:
            return DeviceColumn.empty(N.TYPE_INT32, 0, False, ctx=self.ctx)
        members = [self.strings[k].encode(c) if k in self.strings else c for k, c in enumerate(cols)]
        codes = self.tuples.encode_tuple(members)
        return DeviceColumn(N.TYPE_INT32, n, codes.values, _and_validity(cols), None, self.ctx)

    def close(self) -> None:
        for d in list(self.strings.values()) + ([self.tuples] if self.tuples is not None else []):
            d.close()


def _null_columns(ctx, schema: Schema, n: int) -> List[DeviceColumn]:
    """n all-null rows of every field of `schema`: zero values, clear validity; a UTF8 column has
    n + 1 zero offsets and no bytes."""
    import torch

    from .columnar import bitmap_bytes

    dev = ctx.torch_device
    cols = []
    for f in schema.fields:
        if f.dataType == N.TYPE_UTF8:
            cols.append(DeviceColumn(N.TYPE_UTF8, n, torch.zeros(1, dtype=torch.uint8, device=dev),
                                     torch.zeros(max(bitmap_bytes(n), 4), dtype=torch.uint8, device=dev),
                                     torch.zeros(n + 1, dtype=torch.int32, device=dev), ctx))
            cols[-1].max_len = 0
        else:
            c = DeviceColumn.empty(f.dataType, n, True, ctx=ctx)
            c.values.zero_()
            cols.append(c)
    return cols


class HashJoinExec(PhysicalPlan):
    """Equi-join (build-defined; the reference's SQL has no JOIN). `on`: 1..MAX_KEYS pairs
    (left Expression, right Expression); kind: one of KINDS (inner, left, semi, anti) or of
    BUILD_SIDE_KINDS (right, full_outer, right_semi, right_anti). The RIGHT child is the build side of
    every kind: drained once into one batch (concat_batches) and hashed (qe_join_build). The LEFT child
    streams. A null key matches nothing.
    KINDS give one output batch per left batch, rows in probe order and, within a probe row, in build
    row order. Schema: inner / left: the left fields then the right fields (all null for an
    unmatched row of left); semi / anti: the left fields. An empty build side gives 0-row batches
    (inner, semi), all-null right columns (left) or every row (anti).
    BUILD_SIDE_KINDS need to know which build rows ever found a partner (the table's match marks), so
    they end with ONE more batch after the last left batch, yielded even when it has 0 rows: L left
    batches give L + 1 output batches (right, full_outer) or 1 (right_semi, right_anti).
      right       per left batch the inner pairs, then the unmatched build rows in build-row order with
                  every left column null. Schema: the left fields then the right fields.
      full_outer  the same with the left kind's pairs per batch ("full" is not a name of it).
      right_semi  nothing per left batch; at the end the matched build rows in build-row order.
      right_anti  likewise the unmatched build rows (a null-key build row is unmatched).
                  Schema of both: the right fields.
    A left child that yields no batch gives the final batch alone: every build row for right,
    full_outer and right_anti, none for right_semi. An empty build side gives a final batch of 0 rows."""

    KINDS = ("inner", "left", "semi", "anti")
    BUILD_SIDE_KINDS = ("right", "full_outer", "right_semi", "right_anti")

    def __init__(self, left: PhysicalPlan, right: PhysicalPlan, on, kind: str = "inner"):
        on = list(on)
        if not 1 <= len(on) <= N.MAX_KEYS:
            raise N.IllegalArgumentException(N.QE_ERR_INVALID_ARG, f"a join takes 1..{N.MAX_KEYS} key pairs")
        if kind not in self.KINDS + self.BUILD_SIDE_KINDS:
            raise N.IllegalArgumentException(N.QE_ERR_INVALID_ARG,
                                             f"join kind {kind!r} (one of {self.KINDS + self.BUILD_SIDE_KINDS})")
        self.left = left
        self.right = right
        self.on = [(le, re) for le, re in on]
        self.kind = kind

    def schema(self) -> Schema:
        if self.kind in ("semi", "anti"):
            return self.left.schema()
        if self.kind in ("right_semi", "right_anti"):
            return self.right.schema()
        return Schema(list(self.left.schema().fields) + list(self.right.schema().fields))

    def children(self) -> List[PhysicalPlan]:
        return [self.left, self.right]

    def _build_batch(self) -> RecordBatch:
        from .columnar import Context, concat_batches

        batches = [b for b in self.right.execute() if b.fields]
        for b in batches:
            for c in b.fields:
                if not isinstance(c, DeviceColumn):
                    raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "join input must be device columns")
        if batches:
            return concat_batches(batches)
        ctx = Context.get(0)
        schema = self.right.schema()
        return RecordBatch(schema, [
            DeviceColumn.from_strings([], ctx=ctx) if f.dataType == N.TYPE_UTF8
            else DeviceColumn.empty(f.dataType, 0, False, ctx=ctx) for f in schema.fields])

    def execute(self) -> Iterator[RecordBatch]:
        schema = self.schema()
        build = self._build_batch()
        build_keys = [re.evaluate(build) for _, re in self.on]
        for k in build_keys:
            if not isinstance(k, DeviceColumn):
                raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "a join key must evaluate to a column")
        enc = _JoinKeyEncoder(build_keys[0].ctx, [k.type for k in build_keys])
        table = None
        try:
            table = join_build(enc.encode(build_keys))
            for batch in self.left.execute():
                for c in batch.fields:
                    if not isinstance(c, DeviceColumn):
                        raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "join input must be device columns")
                key = enc.encode([le.evaluate(batch) for le, _ in self.on])
                if self.kind in ("semi", "anti"):
                    yield filter_batch(batch, join_probe_mask(table, key, anti=self.kind == "anti"))
                    continue
                if self.kind in ("right_semi", "right_anti"):
                    join_mark(table, key)
                    continue
                left = self.kind in ("left", "full_outer")
                track = N.JOIN_TRACK if self.kind in ("right", "full_outer") else 0
                pi, bi = join_probe(table, key, (N.JOIN_LEFT if left else N.JOIN_INNER) | track)
                lcols = take(pi, batch.fields, _taken_bytes(pi, batch.fields))
                rcols = (take_or_null if left else take)(bi, build.fields, _taken_bytes(bi, build.fields))
                yield RecordBatch(schema, lcols + rcols)
            if self.kind in self.BUILD_SIDE_KINDS:  # the one batch only the whole left input can settle
                rows = join_build_rows(table, matched=self.kind == "right_semi")
                rcols = take(rows, build.fields)  # (no index repeats: the input's bytes bound the output's)
                if self.kind in ("right_semi", "right_anti"):
                    yield RecordBatch(schema, rcols)
                else:
                    yield RecordBatch(schema, _null_columns(table.ctx, self.left.schema(), rows.length) + rcols)
        finally:
            if table is not None:
                table.close()
            enc.close()

    def __repr__(self) -> str:
        return f"HashJoinExec: kind={self.kind}, on={self.on}"


class SortExec(PhysicalPlan):
    """ORDER BY [LIMIT] (build-defined; the reference parses the clause and drops it,
    Main.kt:1129-1147). A pipeline breaker like HashAggregateExec: drains its input into one batch
    (concat_batches), evaluates the sort expressions, sorts to row indices (qe_sort_indices: stable,
    DESIGN §4) and gathers every column by them (qe_take). sort_exprs: (Expression, ascending,
    nulls_first) triples, the first the most significant. Yields ONE batch with the input's schema;
    an empty input gives a 0-row batch."""

    def __init__(self, input: PhysicalPlan, sort_exprs, limit: Optional[int] = None):  # noqa: A002
        if not sort_exprs or len(sort_exprs) > N.MAX_KEYS:
            raise N.IllegalArgumentException(N.QE_ERR_INVALID_ARG, f"ORDER BY takes 1..{N.MAX_KEYS} expressions")
        if limit is not None and limit < 0:
            raise N.IllegalArgumentException(N.QE_ERR_INVALID_ARG, "LIMIT must not be negative")
        self.input = input
        self.sort_exprs = [(e, bool(asc), bool(nf)) for e, asc, nf in sort_exprs]
        self.limit = limit

    def schema(self) -> Schema:
        return self.input.schema()

    def children(self) -> List[PhysicalPlan]:
        return [self.input]

    def execute(self) -> Iterator[RecordBatch]:
        from .columnar import Context, concat_batches

        schema = self.schema()
        batches = [b for b in self.input.execute() if b.fields]
        for b in batches:
            for c in b.fields:
                if not isinstance(c, DeviceColumn):
                    raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "sort input must be device columns")
        if not batches:
            ctx = Context.get(0)
            yield RecordBatch(schema, [
                DeviceColumn.from_strings([], ctx=ctx) if f.dataType == N.TYPE_UTF8
                else DeviceColumn.empty(f.dataType, 0, True, ctx=ctx) for f in schema.fields])
            return
        batch = concat_batches(batches)
        keys = [e.evaluate(batch) for e, _, _ in self.sort_exprs]
        for k in keys:
            if not isinstance(k, DeviceColumn):
                raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "a sort expression must evaluate to a column")
        flags = [(0 if asc else N.SORT_DESC) | (N.SORT_NULLS_FIRST if nf else 0) for _, asc, nf in self.sort_exprs]
        idx = sort_indices(keys, flags) if self.limit is None else topk_indices(keys, flags, self.limit)
        yield RecordBatch(schema, take(idx, batch.fields))

    def __repr__(self) -> str:
        return f"SortExec: {self.sort_exprs}, limit={self.limit}"


class HashAggregateExec(PhysicalPlan):
    """Main.kt:605-660: consumes every input batch, emits ONE batch of group columns then
    aggregate columns. Row-at-a-time HashMap + Accumulator objects are replaced by the device
    hash-aggregate (K4b). A global aggregate over empty input yields 0 rows (Main.kt:637)."""

    def __init__(self, input: PhysicalPlan, groupExpr: Sequence[Expression],  # noqa: A002,N803
                 aggregateExpr: Sequence[AggregateExpression], schema: Schema,  # noqa: N803
                 expected_groups: int = 1024):
        self.input = input
        self.groupExpr = list(groupExpr)
        self.aggregateExpr = list(aggregateExpr)
        self._schema = schema
        self.expected_groups = expected_groups
        self.state: Optional[HashAggregateState] = None

    def schema(self) -> Schema:
        return self._schema

    def children(self) -> List[PhysicalPlan]:
        return [self.input]

    def partial_state(self) -> Optional[HashAggregateState]:
        """Runs the aggregation and returns the device state (for the two-phase exchange)."""
        state = None
        for batch in self.input.execute():
            keys = [e.evaluate(batch) for e in self.groupExpr]
            inputs = [a.inputExpression().evaluate(batch) if a.inputExpression() is not None else None
                      for a in self.aggregateExpr]
            for c in keys + [i for i in inputs if i is not None]:
                if not isinstance(c, DeviceColumn):
                    raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "aggregate inputs must be device columns")
            present = keys + [i for i in inputs if i is not None]
            if not present and batch.fields:  # COUNT(*) alone: any column gives the row count
                present = [batch.field(0)]
                inputs = [present[0] if a.fn == N.AGG_COUNT_STAR else i for a, i in zip(self.aggregateExpr, inputs)]
            if not present:
                raise N.IllegalStateException(N.QE_ERR_UNSUPPORTED, "COUNT(*) over a batch without columns")
            if state is None:
                state = HashAggregateState(
                    present[0].ctx, [k.type for k in keys],
                    [(a.fn, (i.type if i is not None and a.fn != N.AGG_COUNT_STAR else N.TYPE_INT64))
                     for a, i in zip(self.aggregateExpr, inputs)],
                    self.expected_groups, async_update=True)
            state.update(keys, inputs)
        self.state = state
        return state

    def execute(self) -> Iterator[RecordBatch]:
        state = self.partial_state()
        yield finalize_batch(state, self._schema, self.groupExpr, self.aggregateExpr)

    def __repr__(self) -> str:
        return f"HashAggregateExec: groupExpr={self.groupExpr}, aggrExpr={self.aggregateExpr}"


def finalize_batch(state: Optional[HashAggregateState], schema: Schema, groupExpr, aggregateExpr) -> RecordBatch:  # noqa: N803
    if state is None:  # no input batch at all: empty output
        from .columnar import Context

        ctx = Context.get(0)
        cols = [DeviceColumn.empty(f.dataType if f.dataType in N.FIXED_WIDTH else N.TYPE_INT64, 0, True, ctx=ctx)
                for f in schema.fields]
        return RecordBatch(schema, cols)
    keys, aggs = state.finalize()
    return RecordBatch(schema, keys + aggs)


# ---------------------------------------------------------------------------------------------------
# Fusion: HashAggregateExec(Projection?(Selection?(Scan))) -> one kernel
# ---------------------------------------------------------------------------------------------------
class FusedHashAggregateExec(PhysicalPlan):
    """SelectionExec -> ProjectionExec -> HashAggregateExec in ONE pass over the scanned columns
    (qe_hashagg_update_fused). Same results as the unfused chain."""

    def __init__(self, scan: PhysicalPlan, slots: Sequence[int], spec: N.QeFusedSpec, key_types, aggs,
                 schema: Schema, groupExpr, aggregateExpr, expected_groups: int = 1024,  # noqa: N803
                 key_scan: Optional[Sequence[int]] = None):
        self.scan = scan
        self.key_scan = list(key_scan) if key_scan is not None else None  # dictionary keys: scan columns
        self.slots = list(slots)  # scan column index per slot
        self.spec = spec
        self.key_types = list(key_types)
        self.aggs = list(aggs)
        self._schema = schema
        self.groupExpr = groupExpr
        self.aggregateExpr = aggregateExpr
        self.expected_groups = expected_groups
        self.state: Optional[HashAggregateState] = None

    def schema(self) -> Schema:
        return self._schema

    def children(self) -> List[PhysicalPlan]:
        return [self.scan]

    def partial_state(self, state: Optional[HashAggregateState] = None) -> Optional[HashAggregateState]:
        for batch in self.scan.execute():
            cols = [batch.field(i) for i in self.slots]
            key_cols = [batch.field(i) for i in self.key_scan] if self.key_scan is not None else None
            if state is None:
                # stream-ordered updates: the host prepares batch i + 1 while batch i's kernel runs
                state = HashAggregateState((cols or key_cols)[0].ctx, self.key_types, self.aggs, self.expected_groups,
                                           async_update=True)
            state.update_fused(cols, self.spec, key_cols)
        self.state = state
        return state

    def execute(self) -> Iterator[RecordBatch]:
        yield finalize_batch(self.partial_state(), self._schema, self.groupExpr, self.aggregateExpr)

    def __repr__(self) -> str:
        return f"FusedHashAggregateExec: slots={self.slots}, aggrExpr={self.aggregateExpr}"


class FusedSelectProjectExec(PhysicalPlan):
    """SelectionExec -> ProjectionExec (or a bare SelectionExec) in ONE pass over the scanned
    columns (qe_select_project): order-preserving, same rows and values as the unfused chain.
    Falls back to the unfused operators when the kernel cannot take the plan."""

    def __init__(self, scan: PhysicalPlan, slots: Sequence[int], spec: N.QeSelectSpec, out_types: Sequence[int],
                 schema: Schema, unfused: PhysicalPlan):
        self.scan = scan
        self.slots = list(slots)
        self.spec = spec
        self.out_types = list(out_types)
        self._schema = schema
        self.unfused = unfused
        self.last_kernel_rows = 0

    def schema(self) -> Schema:
        return self._schema

    def children(self) -> List[PhysicalPlan]:
        return [self.scan]

    def launch_batch(self, batch: RecordBatch):
        """Queues the select-project of one batch (qe_select_project_async) and returns
        (outputs, pending), or None when the kernel cannot take the plan."""
        cols = [batch.field(i) for i in self.slots]
        ctx = cols[0].ctx
        n = cols[0].length
        outs = [DeviceColumn.empty(t, n, self._may_be_null(k, cols), ctx=ctx) for k, t in enumerate(self.out_types)]
        cc = (N.QeColumn * len(cols))(*[c.as_c() for c in cols])
        oc = (N.QeColumn * len(outs))(*[o.as_c() for o in outs])
        pending = N.C.c_void_p()
        st = N.lib().qe_select_project_async(ctx.handle, cc, len(cols), N.C.byref(self.spec), oc, N.C.byref(pending))
        if st == N.QE_ERR_UNSUPPORTED:
            return None
        N.check(st)
        return outs, pending, cols

    def finish_batch(self, launched) -> RecordBatch:
        """Waits for that batch's kernels only (not for what was queued behind them) and sets the
        output row count."""
        outs, pending, _cols = launched
        cnt = N.C.c_int64()
        N.check(N.lib().qe_select_pending_wait(pending, N.C.byref(cnt)))
        for o in outs:
            o.length = cnt.value
        return RecordBatch(self._schema, outs)

    def run_batch(self, batch: RecordBatch) -> Optional[RecordBatch]:
        launched = self.launch_batch(batch)
        return None if launched is None else self.finish_batch(launched)

    def _may_be_null(self, k: int, cols: Sequence[DeviceColumn]) -> bool:
        """Whether output k can hold a null, as compile_program decides it (qe_hashagg.hip): a
        referenced column with a validity bitmap, a null literal, or a division (int64 x / 0 ->
        null). Only such outputs get a validity bitmap: allocating and filling one for the C2
        output cost ~10 us of a ~73 us operator call (tools/selproj_op_overhead.py)."""
        pg = self.spec.outputs[k]
        for i in range(pg.ntokens):
            tk = pg.tokens[i]
            if tk.op == N.TOK_COL and cols[tk.arg].validity is not None:
                return True
            if (tk.op == N.TOK_LIT and tk.lit.is_null) or tk.op == N.TOK_DIV:
                return True
        return False

    def execute(self) -> Iterator[RecordBatch]:
        """Pipelined one batch ahead: batch i+1's kernels are queued before batch i's row count is
        read back, so the host wait for batch i overlaps batch i+1 on the device and the stream
        never drains between batches. Batches come out in input order (row order preserved)."""
        inflight = []  # launched, not yet waited on (at most two: this batch and the one ahead)
        try:
            for batch in self.scan.execute():
                launched = self.launch_batch(batch)
                if launched is not None:
                    inflight.append(launched)
                if len(inflight) > 1 or (launched is None and inflight):
                    yield self.finish_batch(inflight.pop(0))
                if launched is None:  # kernel specialisation unavailable: per-family operators
                    yield from _replay(self.unfused, batch)
            while inflight:
                yield self.finish_batch(inflight.pop(0))
        finally:
            # the consumer stopped early, or a scan / launch raised: every queued call is still
            # waited on once, which frees its pinned slot and event and runs its look-back stall
            # check (qe_select_pending_wait); an error here must not mask the one propagating
            for _outs, pending, _cols in inflight:
                N.lib().qe_select_pending_wait(pending, N.C.byref(N.C.c_int64()))

    def __repr__(self) -> str:
        return f"FusedSelectProjectExec: slots={self.slots}, outputs={self.out_types}"


class _OneBatch(PhysicalPlan):
    def __init__(self, batch: RecordBatch):
        self.batch = batch

    def execute(self) -> Iterator[RecordBatch]:
        yield self.batch


def _replay(plan: PhysicalPlan, batch: RecordBatch) -> Iterator[RecordBatch]:
    """Runs the unfused Projection/Selection chain of ``plan`` over one scanned batch."""
    if isinstance(plan, ProjectionExec):
        return ProjectionExec(_ReplayInput(plan.input, batch), plan.schema(), plan.expr).execute()
    if isinstance(plan, SelectionExec):
        return SelectionExec(_ReplayInput(plan.input, batch), plan.expr).execute()
    return iter([batch])


class _ReplayInput(PhysicalPlan):
    def __init__(self, plan: PhysicalPlan, batch: RecordBatch):
        self.plan = plan
        self.batch = batch

    def schema(self) -> Schema:
        return self.plan.schema()

    def execute(self) -> Iterator[RecordBatch]:
        return _replay(self.plan, self.batch)


class _NotFusable(Exception):
    pass


def _conjuncts(e: Expression) -> List[Expression]:
    if isinstance(e, AndExpression):
        return _conjuncts(e.l) + _conjuncts(e.r)
    return [e]


class _SlotMap:
    def __init__(self, scan_schema: Schema):
        self.schema = scan_schema
        self.slots: List[int] = []

    def slot(self, col_index: int) -> int:
        if col_index not in self.slots:
            if len(self.slots) >= N.MAX_COLS:
                raise _NotFusable("too many columns")
            self.slots.append(col_index)
        return self.slots.index(col_index)

    def type_of(self, col_index: int) -> int:
        return self.schema.fields[col_index].dataType


def _resolve(e: Expression, proj: Optional[List[Expression]]) -> Expression:
    """Substitute projection outputs (ColumnExpression over a ProjectionExec) by their definitions."""
    if proj is None:
        return e
    if isinstance(e, ColumnExpression):
        return proj[e.i]
    if isinstance(e, ArithmeticExpression):
        return type(e)(_resolve(e.l, proj), _resolve(e.r, proj))
    if isinstance(e, ComparisonExpression):
        return type(e)(_resolve(e.l, proj), _resolve(e.r, proj))
    return e


def _literal(e: Expression):
    if isinstance(e, LiteralLongExpression):
        return N.scalar(e.value, N.TYPE_INT64)
    if isinstance(e, LiteralDoubleExpression):
        return N.scalar(e.value, N.TYPE_FLOAT64)
    return None


def _program(e: Expression, sm: _SlotMap, out: list) -> bool:
    """Postfix tokens for an arithmetic tree; returns whether the result is fp64."""
    if isinstance(e, ColumnExpression):
        t = sm.type_of(e.i)
        if t not in N.FIXED_WIDTH:
            raise _NotFusable("non fixed-width input")
        out.append(N.QeToken(N.TOK_COL, sm.slot(e.i), N.QeScalar()))
        return t == N.TYPE_FLOAT64
    lit = _literal(e)
    if lit is not None:
        out.append(N.QeToken(N.TOK_LIT, 0, lit))
        return lit.type == N.TYPE_FLOAT64
    if isinstance(e, ArithmeticExpression):
        fl = _program(e.l, sm, out)
        fr = _program(e.r, sm, out)
        out.append(N.QeToken({N.OP_ADD: N.TOK_ADD, N.OP_SUB: N.TOK_SUB, N.OP_MUL: N.TOK_MUL,
                               N.OP_DIV: N.TOK_DIV}[e.op], 0, N.QeScalar()))
        return fl or fr
    raise _NotFusable(f"expression {e!r}")


def fuse(plan: PhysicalPlan) -> PhysicalPlan:
    """Rewrite HashAggregateExec over [ProjectionExec] over [SelectionExec] over ScanExec into a
    FusedHashAggregateExec when every expression is expressible in the fused kernel; otherwise
    return ``plan`` unchanged (the per-family operators then run)."""
    if isinstance(plan, (ProjectionExec, SelectionExec)):
        return _fuse_select_project(plan)
    if not isinstance(plan, HashAggregateExec):
        return plan
    try:
        node = plan.input
        proj = None
        if isinstance(node, ProjectionExec):
            proj = node.expr
            node = node.input
        pred = None
        if isinstance(node, SelectionExec):
            pred = node.expr
            node = node.input
        if not isinstance(node, ScanExec):
            raise _NotFusable("input is not a scan")
        sm = _SlotMap(node.schema())
        spec = N.QeFusedSpec()
        spec.mask_col = -1
        terms = _conjuncts(pred) if pred is not None else []
        if len(terms) > N.MAX_TERMS:
            raise _NotFusable("too many predicate terms")
        for i, t in enumerate(terms):
            if not isinstance(t, ComparisonExpression) or not isinstance(t.l, ColumnExpression):
                raise _NotFusable("predicate term")
            if sm.type_of(t.l.i) not in N.FIXED_WIDTH:
                raise _NotFusable("predicate on non fixed-width column")
            pt = spec.terms[i]
            pt.col = sm.slot(t.l.i)
            pt.op = t.op
            if isinstance(t.r, ColumnExpression):
                if sm.type_of(t.r.i) not in N.FIXED_WIDTH:
                    raise _NotFusable("predicate on non fixed-width column")
                pt.rhs_col = sm.slot(t.r.i)
            else:
                lit = _literal(t.r)
                if lit is None:
                    raise _NotFusable("predicate rhs")
                pt.rhs_col = -1
                pt.lit = lit
        spec.nterms = len(terms)
        key_types, key_scan = [], []
        for g in plan.groupExpr:
            g = _resolve(g, proj)
            if not isinstance(g, ColumnExpression):
                raise _NotFusable("group key must be a column")
            if sm.type_of(g.i) not in N.FIXED_WIDTH and sm.type_of(g.i) != N.TYPE_UTF8:
                raise _NotFusable("group key type")
            key_scan.append(g.i)
            key_types.append(sm.type_of(g.i))
        # UTF-8 keys / key sets wider than 63 bits: encoded to dictionary codes per batch, which
        # join the launch as extra slots (HashAggregateState.update_fused)
        ndict = dictionary_keys(key_types)
        if ndict is None:
            for k, i in enumerate(key_scan):
                spec.key_cols[k] = sm.slot(i)
        aggs = []
        for j, a in enumerate(plan.aggregateExpr):
            if a.fn == N.AGG_COUNT_STAR:
                aggs.append((a.fn, N.TYPE_INT64))
                continue
            toks: list = []
            is_f = _program(_resolve(a.inputExpression(), proj), sm, toks)
            if len(toks) > N.MAX_TOKENS:
                raise _NotFusable("expression too long")
            spec.inputs[j].ntokens = len(toks)
            for t, tok in enumerate(toks):
                spec.inputs[j].tokens[t] = tok
            aggs.append((a.fn, N.TYPE_FLOAT64 if is_f else N.TYPE_INT64))
        if ndict is not None and len(sm.slots) + ndict > N.MAX_COLS:
            raise _NotFusable("too many columns with the key codes")
        if not sm.slots and ndict is None:
            raise _NotFusable("no input columns")
        return FusedHashAggregateExec(node, sm.slots, spec, key_types, aggs, plan.schema(), plan.groupExpr,
                                      plan.aggregateExpr, plan.expected_groups,
                                      key_scan if ndict is not None else None)
    except _NotFusable:
        return plan


def _terms_into(pred: Optional[Expression], sm: "_SlotMap", terms, max_terms: int) -> int:
    conj = _conjuncts(pred) if pred is not None else []
    if len(conj) > max_terms:
        raise _NotFusable("too many predicate terms")
    for i, t in enumerate(conj):
        if not isinstance(t, ComparisonExpression) or not isinstance(t.l, ColumnExpression):
            raise _NotFusable("predicate term")
        if sm.type_of(t.l.i) not in N.FIXED_WIDTH:
            raise _NotFusable("predicate on non fixed-width column")
        pt = terms[i]
        pt.col = sm.slot(t.l.i)
        pt.op = t.op
        if isinstance(t.r, ColumnExpression):
            if sm.type_of(t.r.i) not in N.FIXED_WIDTH:
                raise _NotFusable("predicate on non fixed-width column")
            pt.rhs_col = sm.slot(t.r.i)
        else:
            lit = _literal(t.r)
            if lit is None:
                raise _NotFusable("predicate rhs")
            pt.rhs_col = -1
            pt.lit = lit
    return len(conj)


def _fuse_select_project(plan: PhysicalPlan) -> PhysicalPlan:
    """ProjectionExec(SelectionExec(ScanExec)), SelectionExec(ScanExec) or
    ProjectionExec(ScanExec) -> FusedSelectProjectExec; anything else unchanged."""
    try:
        node = plan
        proj = None
        if isinstance(node, ProjectionExec):
            proj = node.expr
            node = node.input
        pred = None
        if isinstance(node, SelectionExec):
            pred = node.expr
            node = node.input
        if not isinstance(node, ScanExec) or (proj is None and pred is None):
            raise _NotFusable("not a selection/projection over a scan")
        sm = _SlotMap(node.schema())
        spec = N.QeSelectSpec()
        spec.mask_col = -1
        spec.nterms = _terms_into(pred, sm, spec.terms, N.MAX_TERMS)
        exprs = proj if proj is not None else [ColumnExpression(i) for i in range(len(node.schema().fields))]
        if len(exprs) > N.MAX_AGGS:
            raise _NotFusable("too many outputs")
        out_types = []
        for k, e in enumerate(exprs):
            toks: list = []
            is_f = _program(e, sm, toks)
            if len(toks) > N.MAX_TOKENS:
                raise _NotFusable("expression too long")
            spec.outputs[k].ntokens = len(toks)
            for t, tok in enumerate(toks):
                spec.outputs[k].tokens[t] = tok
            if isinstance(e, ColumnExpression):
                if sm.type_of(e.i) == N.TYPE_BOOL:
                    raise _NotFusable("BOOL pass-through")
                out_types.append(sm.type_of(e.i))
            else:
                out_types.append(N.TYPE_FLOAT64 if is_f else N.TYPE_INT64)
        spec.nout = len(exprs)
        if not sm.slots:
            raise _NotFusable("no input columns")
        return FusedSelectProjectExec(node, sm.slots, spec, out_types, plan.schema(), plan)
    except _NotFusable:
        return plan


def aggregate_schema(input_schema: Schema, group_cols: Sequence[int], aggs: Sequence[AggregateExpression],
                     agg_input_types: Sequence[int]) -> Schema:
    """Output schema helper: group fields then one field per aggregate named by the function
    (the reference names every aggregate field after its function, Main.kt:91/:99)."""
    fields = [input_schema.fields[i] for i in group_cols]
    for a, t in zip(aggs, agg_input_types):
        fields.append(Field(a.name, output_type(a.fn, t)))
    return Schema(fields)
