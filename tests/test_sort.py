"""ORDER BY on the device: qe_sort_indices (stable multi-key radix sort to row indices), qe_take
(gather by row index), SortExec and concat_batches, against tests/sortref.py. Every check compares
the exact permutation or the exact columns: the sort is stable, so there is one right answer."""
import pathlib

import numpy as np
import pytest

import sortref as R
from kquery import native as N
from kquery.columnar import DeviceColumn, Field, RecordBatch, Schema, concat_batches
from kquery.operators import PhysicalPlan, SortExec, sort_indices, sort_layout, take
from oracle import gen

pytestmark = pytest.mark.gpu

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
BIG = 1_000_003
FIXED = [N.TYPE_INT64, N.TYPE_INT32, N.TYPE_DATE32, N.TYPE_UINT8, N.TYPE_BOOL, N.TYPE_FLOAT64]
ALL_FLAGS = [0, N.SORT_DESC, N.SORT_NULLS_FIRST, N.SORT_DESC | N.SORT_NULLS_FIRST]


# ---- columns ----------------------------------------------------------------------------------------
def _bitmap(ctx, bits):
    import torch

    from kquery.columnar import bitmap_bytes

    buf = np.zeros(max(bitmap_bytes(len(bits)), 4), dtype=np.uint8)
    packed = np.packbits(np.asarray(bits, dtype=bool), bitorder="little")
    buf[: len(packed)] = packed
    return torch.from_numpy(buf).to(ctx.torch_device)


def ucol(ctx, vals, valid=None, max_len=None):
    """UTF8 column from raw byte strings (any bytes: the sort orders bytes, not characters)."""
    import torch

    offs = np.zeros(len(vals) + 1, dtype=np.int32)
    if len(vals):
        offs[1:] = np.cumsum(np.fromiter((len(v) for v in vals), dtype=np.int64, count=len(vals)))
    data = np.frombuffer(b"".join(vals) or b"\0", dtype=np.uint8).copy()
    c = DeviceColumn(N.TYPE_UTF8, len(vals), torch.from_numpy(data).to(ctx.torch_device),
                     None if valid is None else _bitmap(ctx, valid), torch.from_numpy(offs).to(ctx.torch_device), ctx)
    c.max_len = max_len
    return c


def to_device(ctx, key, max_len=None):
    t, vals, valid = key
    if t == N.TYPE_UTF8:
        return ucol(ctx, vals, valid, max_len)
    return DeviceColumn.from_numpy(t, np.asarray(vals), valid, ctx=ctx)


def prefix(col: DeviceColumn, n: int) -> DeviceColumn:
    """The first n rows of a column, over the same buffers."""
    c = DeviceColumn(col.type, n, col.values, col.validity, col.offsets, col.ctx)
    c.max_len = col.max_len
    return c


def key_prefix(key, n):
    t, vals, valid = key
    return t, vals[:n], None if valid is None else valid[:n]


def gpu_order(ctx, cols, flags, limit=None):
    out = sort_indices(cols, flags, limit)
    ctx.synchronize()
    return out.to_numpy()


def check(ctx, keys, flags, limit=None, max_lens=None, cols=None):
    cols = cols or [to_device(ctx, k, ml) for k, ml in zip(keys, max_lens or [None] * len(keys))]
    got = gpu_order(ctx, cols, flags, limit)
    want = R.order(keys, flags, limit)
    assert got.dtype == np.int32 and got.shape == want.shape
    if not np.array_equal(got, want):
        bad = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"first difference at output row {bad} of {len(want)}: got {got[bad]}, want {want[bad]}")


# ---- generated keys, shared by the tests (a counter-based generator: row i does not depend on n) ----
def _typed(t, u, full):
    """Values of type t from int64 generator output u (mod 7 values, or full-range bits)."""
    if t == N.TYPE_INT64:
        return u if full else u - 3
    if t in (N.TYPE_INT32, N.TYPE_DATE32):
        return u.astype(np.int32) if full else (u - 3).astype(np.int32)
    if t == N.TYPE_UINT8:
        return u.astype(np.uint8)
    if t == N.TYPE_BOOL:
        return (u & 1).astype(bool)
    if t == N.TYPE_UTF8:
        if full:  # 0..16 hex digits of the value: shared prefixes, lengths across the 7/8-byte boundaries
            return [(b"%016x" % (int(x) & 0xFFFFFFFFFFFFFFFF))[: int(x) % 17] for x in u]
        return [(b"", b"a", b"ab", b"b", b"abcdefgh", b"abcdefghi", b"a\x00")[int(x)] for x in u]
    raise AssertionError(t)


_KEYS: dict = {}


def generated(ctx, t, dist, n):
    """(sortref key, device column) of n rows: dist 'dup' = value mod 7 with 10 % nulls, 'full' = the
    generator's full range (QE_GEN_RAW, or QE_GEN_UNIT53 for fp64) without nulls."""
    base = _KEYS.get((t, dist))
    if base is None:
        if dist == "dup":
            u, valid = gen.generate(gen.GEN_MOD, 7, 11, t, 0, BIG, 100)
            vals = (u - 3) * 0.5 if t == N.TYPE_FLOAT64 else _typed(t, u, False)
        else:
            valid = None
            if t == N.TYPE_FLOAT64:
                vals, _ = gen.generate(gen.GEN_UNIT53, 0, 12, t, 0, BIG)
            else:
                vals = _typed(t, gen.generate(gen.GEN_RAW, 0, 12, t, 0, BIG)[0], True)
        if t == N.TYPE_UTF8 and valid is not None:
            vals = [v if ok else b"" for v, ok in zip(vals, valid)]
        key = (t, vals, valid)
        base = _KEYS[(t, dist)] = (key, to_device(ctx, key))
    hit = _KEYS.get((t, dist, n))
    if hit is None:
        hit = _KEYS[(t, dist, n)] = (key_prefix(base[0], n), prefix(base[1], n))
    return hit


@pytest.fixture(scope="module")
def layout(gpu_ctx):
    t, s = sort_layout()
    assert 0 < s <= t
    return t, s


# ---- tests --------------------------------------------------------------------------------------------
def test_known_answers(gpu_ctx):
    for name, keys, flags, limit, expected, max_lens in R.load_kat():
        cols = [to_device(gpu_ctx, k, ml) for k, ml in zip(keys, max_lens)]
        got = gpu_order(gpu_ctx, cols, flags, limit)
        assert got.tolist() == expected.tolist(), name


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("t", FIXED + [N.TYPE_UTF8])
def test_shapes(gpu_ctx, layout, t, flags):
    T, S = layout
    for n in (0, 1, 2, 63, 64, 65, S, S + 1, T - 1, T, T + 1, 3 * T + 17, BIG):
        for dist in ("dup", "full"):
            key, col = generated(gpu_ctx, t, dist, n)
            check(gpu_ctx, [key], [flags], cols=[col])


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_fp64_specials(gpu_ctx, layout, flags):
    T, _ = layout
    n = T + 1
    special = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                        0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,
                        0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x3FF0000000000000,
                        0xBFF0000000000000], dtype=np.uint64).view(np.float64)
    rng = np.random.default_rng(5)
    vals = np.where(rng.random(n) < 0.6, special[rng.integers(len(special), size=n)], rng.normal(size=n))
    valid = rng.random(n) >= 0.05
    check(gpu_ctx, [(N.TYPE_FLOAT64, vals, valid)], [flags])


def test_skipped_passes(gpu_ctx, layout):
    """Constant digits cost no pass; the pair buffers' parity must still come out right."""
    T, _ = layout
    for n in (3 * T + 17, BIG):
        narrow, _ = gen.generate(gen.GEN_MOD, 1 << 20, 3, 0, 0, n)
        constant = np.full(n, 0x0102030405060708, dtype=np.int64)
        one_off = constant.copy()
        one_off[n // 2] = 0x0102030405FF0708
        for vals in (narrow, constant, one_off):
            for flags in (0, N.SORT_DESC):
                check(gpu_ctx, [(N.TYPE_INT64, vals, None)], [flags])
    odd = np.full(3 * T + 17, 7, dtype=np.int64)  # three varying digits -> an odd number of passes
    odd[5], odd[T + 9], odd[2 * T] = 0x010000, 0x0100, 0x01
    check(gpu_ctx, [(N.TYPE_INT64, odd, None)], [0])


def _multi_keys(rng, n, which):
    nul = lambda p: rng.random(n) >= p  # noqa: E731
    if which == "packed":  # UINT8, DATE32 desc, INT64
        return ([(N.TYPE_UINT8, rng.integers(0, 3, n).astype(np.uint8), nul(0.1)),
                 (N.TYPE_DATE32, rng.integers(18000, 18004, n).astype(np.int32), nul(0.1)),
                 (N.TYPE_INT64, rng.integers(-5, 5, n).astype(np.int64), None)], [0, N.SORT_DESC, 0])
    if which == "two_words":  # INT64, FLOAT64 desc nulls first
        return ([(N.TYPE_INT64, rng.integers(-2, 2, n).astype(np.int64) * (1 << 40), None),
                 (N.TYPE_FLOAT64, rng.integers(-3, 3, n) * 0.25, nul(0.2))],
                [0, N.SORT_DESC | N.SORT_NULLS_FIRST])
    words = [b"", b"a", b"ab", b"abcdefghij", b"abcdefgh", b"tripdata-2019", "Pärsson".encode()]
    s = [words[i] for i in rng.integers(len(words), size=n)]
    if which == "utf8_f64":
        return ([(N.TYPE_UTF8, s, nul(0.1)), (N.TYPE_FLOAT64, rng.integers(-3, 3, n) * 0.5, None)], [N.SORT_DESC, 0])
    return ([(N.TYPE_BOOL, rng.integers(0, 2, n).astype(bool), nul(0.1)),  # four keys
             (N.TYPE_INT32, rng.integers(-2, 2, n).astype(np.int32), None),
             (N.TYPE_UTF8, s, None),
             (N.TYPE_FLOAT64, rng.integers(0, 4, n) * 1.5, nul(0.3))],
            [N.SORT_NULLS_FIRST, N.SORT_DESC, 0, N.SORT_DESC | N.SORT_NULLS_FIRST])


@pytest.mark.parametrize("which", ["packed", "two_words", "utf8_f64", "four_keys"])
def test_multi_key(gpu_ctx, layout, which):
    T, S = layout
    for n in (S + 1, 3 * T + 17):
        keys, flags = _multi_keys(np.random.default_rng(n), n, which)
        for k in keys:  # null rows of a UTF8 reference key hold b""
            if k[0] == N.TYPE_UTF8 and k[2] is not None:
                k[1][:] = [v if ok else b"" for v, ok in zip(k[1], k[2])]
        check(gpu_ctx, keys, flags)


def _strings(rng, n, max_len):
    alphabet = [b"a", b"b", b"\x00", b"z", "é".encode(), "€".encode(), "\U0001F600".encode(), b"\xff"]
    stems = [b"", b"a", b"ab", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefghabcdefgh", b"abcdefghabcdefg\x00"]
    out = []
    for _ in range(n):
        s = stems[rng.integers(len(stems))] + b"".join(alphabet[i] for i in rng.integers(len(alphabet), size=rng.integers(0, 8)))
        out.append(s[: rng.integers(0, max_len + 1)])
    return out


@pytest.mark.parametrize("max_len,promise", [(7, True), (7, False), (40, False)])
def test_utf8(gpu_ctx, layout, max_len, promise):
    """Lengths 0..max_len: empty strings, shared prefixes, embedded 0x00, multi-byte characters,
    nulls. max_len 7 is the one-word path (with the column's bound, or found by the reduction);
    40 the chunked path, with lengths of exactly 7, 8, 9 and 16 among the stems."""
    T, S = layout
    for n in (S + 1, 3 * T + 17):
        rng = np.random.default_rng(n + max_len)
        vals = _strings(rng, n, max_len)
        for exact in (7, 8, 9, 16):
            if exact <= max_len:
                vals[exact] = b"abcdefghabcdefgh"[:exact]
        valid = rng.random(n) >= 0.1
        vals = [v if ok else b"" for v, ok in zip(vals, valid)]
        key = (N.TYPE_UTF8, vals, valid)
        col = ucol(gpu_ctx, vals, valid, max_len if promise else None)
        for flags in ALL_FLAGS:
            check(gpu_ctx, [key], [flags], cols=[col])


def test_utf8_bound_is_checked_on_the_device(gpu_ctx, layout):
    T, S = layout
    for n in (S, 3 * T + 17):
        vals = [b"ab"] * n
        vals[n - 1] = b"abcdefghij"
        with pytest.raises(N.IllegalArgumentException, match="max_len"):
            sort_indices([ucol(gpu_ctx, vals, None, 3)], [0])


def test_limit(gpu_ctx, layout):
    T, S = layout
    for n in (S + 1, 3 * T + 17):
        key, col = generated(gpu_ctx, N.TYPE_INT64, "dup", n)
        for limit in (0, 1, 10, n, n + 5, -1):
            got = sort_indices([col], [N.SORT_DESC], limit)
            gpu_ctx.synchronize()
            assert got.length == (n if limit < 0 else min(limit, n))
            assert np.array_equal(got.to_numpy(), R.order([key], [N.SORT_DESC], limit))


def test_argument_errors(gpu_ctx):
    a = DeviceColumn.from_numpy(N.TYPE_INT64, np.arange(10, dtype=np.int64), ctx=gpu_ctx)
    b = DeviceColumn.from_numpy(N.TYPE_INT64, np.arange(11, dtype=np.int64), ctx=gpu_ctx)
    with pytest.raises(N.IllegalArgumentException):
        sort_indices([a, b], [0, 0])
    with pytest.raises(N.IllegalArgumentException):
        sort_indices([a], [4])
    with pytest.raises(N.IllegalArgumentException):
        sort_indices([a] * 5, [0] * 5)
    bad = DeviceColumn.from_numpy(N.TYPE_INT64, np.arange(3, dtype=np.int64), ctx=gpu_ctx)  # indices must be INT32
    with pytest.raises(N.IllegalArgumentException):
        take(bad, [a])
    nullable = DeviceColumn.from_numpy(N.TYPE_INT32, np.arange(3, dtype=np.int32), np.ones(3, dtype=bool), ctx=gpu_ctx)
    with pytest.raises(N.IllegalArgumentException):
        take(nullable, [a])
    idx = DeviceColumn.from_numpy(N.TYPE_INT32, np.array([0, 0, 0], dtype=np.int32), ctx=gpu_ctx)
    with pytest.raises(N.CapacityError):  # repeated rows need more bytes than the caller said
        take(idx, [ucol(gpu_ctx, [b"abcdef", b"x"])], utf8_bytes=[7])


def _index_sets(rng, n, m):
    yield rng.integers(0, max(n, 1), size=m).astype(np.int32) if n else np.zeros(0, dtype=np.int32)  # repeats
    yield np.arange(n - 1, -1, -1, dtype=np.int32)  # reverse
    yield np.arange(n, dtype=np.int32)  # identity
    yield np.zeros(0, dtype=np.int32)  # empty


def test_take(gpu_ctx, layout):
    T, _ = layout
    for n, m in ((64, 63), (65, 130), (T, T + 1), (T + 1, T - 1), (100_003, 100_003)):
        rng = np.random.default_rng(n)
        valid = rng.random(n) >= 0.2
        data = {t: (_typed(t, rng.integers(-(1 << 62), 1 << 62, n), True), valid if i % 2 else None)
                for i, t in enumerate(FIXED[:5])}
        data[N.TYPE_FLOAT64] = (rng.normal(size=n), valid)
        strs = _strings(rng, n, 20)
        cols = [DeviceColumn.from_numpy(t, v, ok, ctx=gpu_ctx) for t, (v, ok) in data.items()]
        cols += [ucol(gpu_ctx, strs, valid), ucol(gpu_ctx, strs, None)]
        lens = np.array([len(s) for s in strs], dtype=np.int64)
        for idx in _index_sets(rng, n, m):
            need = int(lens[idx].sum())
            outs = take(DeviceColumn.from_numpy(N.TYPE_INT32, idx, ctx=gpu_ctx), cols,
                        utf8_bytes=[None] * len(data) + [need, need])
            gpu_ctx.synchronize()
            for o, (t, (v, ok)) in zip(outs, data.items()):
                assert o.length == len(idx) and o.type == t
                assert np.array_equal(o.to_numpy().view(np.uint8), np.asarray(v)[idx].view(np.uint8)), (n, t)
                assert (o.validity is None) == (ok is None)
                if ok is not None:
                    assert np.array_equal(o.valid_mask(), ok[idx])
                    pad = np.unpackbits(o.validity.cpu().numpy(), bitorder="little")[len(idx): (len(idx) + 31) // 32 * 32]
                    assert not pad.any()  # whole words are written: the padding bits are zero
            for o, ok in zip(outs[len(data):], (valid, None)):
                want = [strs[i] for i in idx]
                offs = o.offsets.cpu().numpy()[: len(idx) + 1]
                assert np.array_equal(offs, np.concatenate([[0], np.cumsum([len(s) for s in want])]).astype(np.int32))
                assert o.values.cpu().numpy().tobytes()[: offs[-1]] == b"".join(want)
                if ok is not None:
                    assert np.array_equal(o.valid_mask(), ok[idx])


def test_determinism(gpu_ctx):
    _, col = generated(gpu_ctx, N.TYPE_INT64, "dup", BIG)
    a = gpu_order(gpu_ctx, [col], [0])
    b = gpu_order(gpu_ctx, [col], [0])
    assert np.array_equal(a, b)


# ---- host mirror ---------------------------------------------------------------------------------------
class _Batches(PhysicalPlan):
    def __init__(self, schema, batches):
        self._schema, self.batches = schema, batches

    def schema(self):
        return self._schema

    def execute(self):
        return iter(self.batches)


def test_concat_batches(gpu_ctx):
    rng = np.random.default_rng(1)
    lens = [13, 0, 7, 100, 1]  # seams that are no multiples of 8, an empty batch in the middle
    schema = Schema([Field("i", N.TYPE_INT32), Field("b", N.TYPE_BOOL), Field("s", N.TYPE_UTF8), Field("f", N.TYPE_FLOAT64)])
    parts, batches = [], []
    for ln in lens:
        ok = rng.random(ln) >= 0.3
        i32 = rng.integers(-100, 100, ln).astype(np.int32)
        bl = rng.random(ln) < 0.5
        ss = [s if v else None for s, v in zip(["x" * int(k) + "é" for k in rng.integers(0, 5, ln)], ok)]
        f = rng.normal(size=ln)
        parts.append((i32, ok, bl, ss, f))
        batches.append(RecordBatch(schema, [DeviceColumn.from_numpy(N.TYPE_INT32, i32, ok, ctx=gpu_ctx),
                                            DeviceColumn.from_numpy(N.TYPE_BOOL, bl, ok, ctx=gpu_ctx),
                                            DeviceColumn.from_strings(ss, ctx=gpu_ctx),
                                            DeviceColumn.from_numpy(N.TYPE_FLOAT64, f, ctx=gpu_ctx)]))
    out = concat_batches(batches)
    ok = np.concatenate([p[1] for p in parts])
    assert out.rowCount() == sum(lens)
    assert out.field(0).to_pylist() == [int(v) if o else None for v, o in zip(np.concatenate([p[0] for p in parts]), ok)]
    assert out.field(1).to_pylist() == [bool(v) if o else None for v, o in zip(np.concatenate([p[2] for p in parts]), ok)]
    assert out.field(2).to_pylist() == [s for p in parts for s in p[3]]
    assert out.field(3).validity is None
    assert np.array_equal(out.field(3).to_numpy(), np.concatenate([p[4] for p in parts]))
    assert int(out.field(2).offsets[0].item()) == 0


def test_sortexec_employee(gpu_ctx):
    from kquery.csv_source import CsvDataSource
    from kquery.expressions import CastExpression, ColumnExpression, MaxExpression
    from kquery.operators import HashAggregateExec, ScanExec

    def query(ascending):
        agg = HashAggregateExec(ScanExec(CsvDataSource(str(GOLD / "employee.csv"), True, 1000, ctx=gpu_ctx), ["state", "salary"]),
                                [ColumnExpression(0)], [MaxExpression(CastExpression(ColumnExpression(1), N.TYPE_FLOAT64))],
                                Schema([Field("state", N.TYPE_UTF8), Field("max_amount", N.TYPE_FLOAT64)]))
        out = list(SortExec(agg, [(ColumnExpression(1), ascending, False)]).execute())
        assert len(out) == 1
        return list(zip(out[0].field(0).to_pylist(), out[0].field(1).to_pylist()))

    assert query(True) == [("Sthlm", 0.0), ("Uppsala", 1337.0)]
    assert query(False) == [("Uppsala", 1337.0), ("Sthlm", 0.0)]


def test_sortexec_multi_batch_equals_single_batch(gpu_ctx):
    from kquery.expressions import ColumnExpression

    rng = np.random.default_rng(2)
    lens = [1001, 7, 4096]
    n = sum(lens)
    k = rng.integers(-4, 4, n).astype(np.int64)
    kv = rng.random(n) >= 0.1
    pay = [None if rng.random() < 0.2 else f"row{i}-{'é' * (i % 3)}" for i in range(n)]
    schema = Schema([Field("k", N.TYPE_INT64), Field("payload", N.TYPE_UTF8)])

    def batch(lo, hi):
        return RecordBatch(schema, [DeviceColumn.from_numpy(N.TYPE_INT64, k[lo:hi], kv[lo:hi], ctx=gpu_ctx),
                                    DeviceColumn.from_strings(pay[lo:hi], ctx=gpu_ctx)])

    cuts = np.concatenate([[0], np.cumsum(lens)])
    exprs = [(ColumnExpression(0), False, True)]
    many = next(SortExec(_Batches(schema, [batch(a, b) for a, b in zip(cuts[:-1], cuts[1:])]), exprs).execute())
    one = next(SortExec(_Batches(schema, [batch(0, n)]), exprs).execute())
    perm = R.order([(N.TYPE_INT64, k, kv)], [N.SORT_DESC | N.SORT_NULLS_FIRST])
    want_k = [int(k[i]) if kv[i] else None for i in perm]
    want_p = [pay[i] for i in perm]
    for out in (many, one):
        assert out.field(0).to_pylist() == want_k
        assert out.field(1).to_pylist() == want_p
    empty = next(SortExec(_Batches(schema, []), exprs).execute())
    assert empty.rowCount() == 0 and len(empty.fields) == 2


def test_sortexec_limit_over_c4_aggregate(gpu_ctx):
    from kquery.aggregate import HashAggregateState
    from kquery.datasource import C4_COLUMNS, generate_column
    from kquery.expressions import ColumnExpression
    from kquery.workloads import C4_AGGS, c4_spec
    from oracle import semantics as S

    n = 200_003
    st = HashAggregateState(gpu_ctx, [N.TYPE_INT64], C4_AGGS, 1024)
    st.update_fused([generate_column(s, n, 0, 42, gpu_ctx) for s in C4_COLUMNS], c4_spec())
    keys, aggs = st.finalize()
    schema = Schema([Field("k", N.TYPE_INT64)] + [Field(f"a{j}", N.TYPE_INT64) for j in range(len(aggs))])
    plan = SortExec(_Batches(schema, [RecordBatch(schema, keys + aggs)]),
                    [(ColumnExpression(1), False, False), (ColumnExpression(0), True, False)], limit=5)
    out = next(plan.execute())
    got = list(zip(*[out.field(j).to_pylist() for j in range(1 + len(aggs))]))
    k, _ = gen.generate(gen.GEN_MOD, 1024, 42, 0, 0, n)
    a, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 1, 0, n)
    b, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 2, 0, n)
    ref = S.group_aggregate([k], [None], [a + b, None, a, b], [None] * 4,
                            [S.AGG_SUM, S.AGG_COUNT_STAR, S.AGG_MIN, S.AGG_MAX], a > (1 << 19))
    rows = sorted(((kk[0], *vals) for kk, vals in ref.items()), key=lambda r: (-r[1], r[0]))
    assert len(ref) == 1024 and got == [tuple(r) for r in rows[:5]]
