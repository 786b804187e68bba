"""ORDER BY ... LIMIT k on the device: qe_topk_indices (radix selection, then the stable sort of the
candidates) against tests/sortref.py and against qe_sort_indices on the same device columns. Every
check in selection mode asserts (a) the exact prefix of the stable order, (b) equality with the
truncated full sort, and (c), through qe_topk_last_stats, that the selection path ran and handed the
final sort at most max(small_max, 2 k) candidates: a silent fall-back to the full sort fails."""
import numpy as np
import pytest

import sortref as R
import topkref as TR
from kquery import native as N
from kquery.columnar import Context, DeviceColumn, Field, RecordBatch, Schema
from kquery.operators import SortExec, sort_indices, sort_layout, topk_indices, topk_last_stats
from oracle import gen
from test_sort import ALL_FLAGS, FIXED, _Batches, _multi_keys, _strings, _typed, key_prefix, prefix, to_device, ucol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def layout(gpu_ctx):
    t, s = sort_layout()
    assert 0 < s <= t
    return t, s


def check(ctx, S, keys, flags, k, cols=None, max_lens=None):
    """(a), (b), (c) for one input and k; returns the stats."""
    cols = cols or [to_device(ctx, key, ml) for key, ml in zip(keys, max_lens or [None] * len(keys))]
    n = cols[0].length
    got = topk_indices(cols, flags, k, N.TOPK_SELECT)
    ctx.synchronize()
    st = topk_last_stats(ctx)
    got = got.to_numpy()
    want = R.order(keys, flags, limit=k)
    assert got.dtype == np.int32 and got.shape == want.shape == (min(k, n),)
    if not np.array_equal(got, want):
        bad = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"n={n} k={k}: first difference at output row {bad}: got {got[bad]}, want {want[bad]}; stats {st}")
    srt = sort_indices(cols, flags, k)
    ctx.synchronize()
    assert np.array_equal(got, srt.to_numpy()), (n, k)
    if n > 0:
        assert st[0] == 1, f"n={n} k={k}: the call did not take the selection path: {st}"
        assert st[2] <= max(S, 2 * k) and st[2] >= min(k, n), (n, k, st)
        assert st[1] >= 0 and st[3] >= 0
    return st


# ---- generated keys (test_sort.py's generator and value rules, over the rows these shapes need) ----
_KEYS: dict = {}


def generated(ctx, t, dist, n, nmax):
    base = _KEYS.get((t, dist))
    if base is None:
        if dist == "dup":
            u, valid = gen.generate(gen.GEN_MOD, 7, 11, t, 0, nmax, 100)
            vals = (u - 3) * 0.5 if t == N.TYPE_FLOAT64 else _typed(t, u, False)
        else:
            valid = None
            if t == N.TYPE_FLOAT64:
                vals, _ = gen.generate(gen.GEN_UNIT53, 0, 12, t, 0, nmax)
            else:
                vals = _typed(t, gen.generate(gen.GEN_RAW, 0, 12, t, 0, nmax)[0], True)
        if t == N.TYPE_UTF8 and valid is not None:
            vals = [v if ok else b"" for v, ok in zip(vals, valid)]
        key = (t, vals, valid)
        base = _KEYS[(t, dist)] = (key, to_device(ctx, key))
    assert n <= base[1].length
    return key_prefix(base[0], n), prefix(base[1], n)


# ---- known answers ------------------------------------------------------------------------------------
def test_known_answers(gpu_ctx, layout):
    _, S = layout
    ran = 0
    for name, keys, flags, limit, expected, max_lens in R.load_kat():
        n = len(keys[0][1])
        cols = [to_device(gpu_ctx, k, ml) for k, ml in zip(keys, max_lens)]
        ks = [limit] if limit >= 0 else sorted({1, max(n - 1, 0)})
        for k in ks:
            got = topk_indices(cols, flags, k, N.TOPK_SELECT)
            gpu_ctx.synchronize()
            assert got.to_numpy().tolist() == expected.tolist()[:k], (name, k)
            check(gpu_ctx, S, keys, flags, k, cols=cols)
            ran += 1
    assert ran >= 10


# ---- shapes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("t", FIXED + [N.TYPE_UTF8])
def test_shapes(gpu_ctx, layout, t, flags):
    T, S = layout
    for n in (1, 63, 64, 65, S, S + 1, T - 1, T, T + 1, 2 * T + 1):
        for dist in ("dup", "full"):
            key, col = generated(gpu_ctx, t, dist, n, 2 * T + 1)
            for k in sorted({0, 1, 2, 63, 64, 65, n - 1, n, n + 5}):
                check(gpu_ctx, S, [key], [flags], k, cols=[col])


def test_k_far_beyond_n(gpu_ctx, layout):
    """k is any int64 >= 0, 2^63 - 1 ("no limit") included: the call works on min(k, n), and its working
    memory is sized for that."""
    T, S = layout
    rng = np.random.default_rng(59)
    for n in (S, S + 1, 2 * T + 1, 5 * T + 3):  # the last: more sort tiles than max(small_max, 2 k) would need for a small k
        key = (N.TYPE_INT64, rng.integers(-(1 << 62), 1 << 62, n), None)
        col = to_device(gpu_ctx, key)
        for k in (2**31, 2**62, 2**62 + 1, 2**63 - 1):
            for mode in (N.TOPK_SELECT, N.TOPK_AUTO, N.TOPK_SORT):
                got = topk_indices([col], [N.SORT_DESC], k, mode)
                gpu_ctx.synchronize()
                st = topk_last_stats(gpu_ctx)
                assert st[0] == int(mode == N.TOPK_SELECT) and st[2] == n
                assert np.array_equal(got.to_numpy(), R.order([key], [N.SORT_DESC]))


# ---- ties: stability decides ----------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, N.SORT_DESC])
def test_ties(gpu_ctx, layout, flags):
    T, S = layout
    n = 2 * T + 1
    same = (N.TYPE_INT64, np.full(n, -7, dtype=np.int64), None)
    for k in (1, 10, S, S + 1, n - 1):
        st = check(gpu_ctx, S, [same], [flags], k)
        if 2 * k < n and n > S:  # a constant key must not hand n rows to the final sort: the cut leaves k
            assert st[2] == k and st[1] == 0, st
    rng = np.random.default_rng(17)
    two = (rng.random(n) < 0.7).astype(np.int64) * 1000 + 5  # two values; the larger run is the 1005s
    first = 5 if not flags & N.SORT_DESC else 1005
    edge = int((two == first).sum())  # the run that sorts first ends here
    for k in (edge - 1, edge, edge + 1, edge // 2, (edge + n) // 2, 3, n - 2):
        check(gpu_ctx, S, [(N.TYPE_INT64, two, None)], [flags], k)


# ---- nulls --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_nullable_keys(gpu_ctx, layout, flags):
    T, S = layout
    n = 2 * T + 1
    rng = np.random.default_rng(23)
    vals = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    valid = rng.random(n) >= 0.3
    nn = int((~valid).sum())
    run_start = 0 if flags & N.SORT_NULLS_FIRST else n - nn  # the null run of the order
    for k in sorted({max(run_start, 1), run_start + 1, run_start + nn // 2, run_start + nn, 7, run_start + nn - 1}):
        check(gpu_ctx, S, [(N.TYPE_INT64, vals, valid)], [flags], min(k, n))
    none = np.zeros(n, dtype=bool)
    for k in (1, 100, n - 1):
        check(gpu_ctx, S, [(N.TYPE_INT64, vals, none)], [flags], k)
    f = rng.normal(size=n)
    check(gpu_ctx, S, [(N.TYPE_FLOAT64, f, valid)], [flags], nn // 2)


# ---- fp64 specials ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_fp64_specials(gpu_ctx, layout, flags):
    T, S = layout
    n = 2 * T + 1
    special = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                        0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,
                        0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x3FF0000000000000,
                        0xBFF0000000000000], dtype=np.uint64).view(np.float64)
    rng = np.random.default_rng(5)
    vals = np.where(rng.random(n) < 0.6, special[rng.integers(len(special), size=n)], rng.normal(size=n))
    valid = rng.random(n) >= 0.05
    key = (N.TYPE_FLOAT64, vals, valid)
    order = R.order([key], [flags])
    bits = vals.view(np.uint64)[order]
    ok = valid[order]
    # the cut between -0.0 and +0.0: the position where the zero runs meet in this order
    z = np.nonzero(ok[:-1] & ok[1:] & (np.minimum(bits[:-1], bits[1:]) == 0) & (np.maximum(bits[:-1], bits[1:]) == 1 << 63))[0]
    assert len(z) == 1
    cut = int(z[0]) + 1
    nan_first = int(np.nonzero(ok & np.isnan(vals[order]))[0][0])
    for k in sorted({cut - 1, cut, cut + 1, nan_first + 3, 1, 5, n - 3}):
        check(gpu_ctx, S, [key], [flags], k)


# ---- narrow ranges ------------------------------------------------------------------------------------------
def test_narrow_range_keys(gpu_ctx, layout):
    T, S = layout
    n = 2 * T + 1
    narrow, _ = gen.generate(gen.GEN_MOD, 1 << 20, 3, 0, 0, n)  # upper five digits constant
    for flags in (0, N.SORT_DESC):
        for k in (5, 700):  # threshold in the first bin of the first varying digit, and in a later one
            st = check(gpu_ctx, S, [(N.TYPE_INT64, narrow, None)], [flags], k)
            assert st[1] >= 1, st
    # digit 2 is the first that varies; nearly every row has it at 255 (ascending) / at 0 (descending)
    rng = np.random.default_rng(31)
    d2 = np.full(n, 255, dtype=np.int64)
    few = rng.choice(n, 50, replace=False)
    d2[few] = rng.integers(0, 255, 50)
    vals = (d2 << 16) | rng.integers(0, 1 << 16, n)
    for flags, k in ((0, 100), (0, 50), (0, 51), (N.SORT_DESC, 100), (N.SORT_DESC, n - 60)):
        st = check(gpu_ctx, S, [(N.TYPE_INT64, vals, None)], [flags], k)
        assert st[1] >= 1 or 2 * k >= n, st
    one_off = np.full(n, 0x0102030405060708, dtype=np.int64)
    one_off[n // 2] = 0x0102030405FF0708
    one_off[n // 3] = 0x0102030405000708
    for flags in (0, N.SORT_DESC):
        for k in (1, 2, 9):
            check(gpu_ctx, S, [(N.TYPE_INT64, one_off, None)], [flags], k)


# ---- keys of several words ------------------------------------------------------------------------------------
def test_selection_continues_into_the_second_word(gpu_ctx, layout):
    T, S = layout
    n = 2 * T + 1
    rng = np.random.default_rng(41)
    a = rng.integers(0, 3, n).astype(np.int64) * (1 << 33) - 5  # three values: runs of about n / 3 > small_max
    b = rng.normal(size=n)
    assert int((a == a.min()).sum()) > S and int((a == a.max()).sum()) > S
    for flags in ([0, 0], [N.SORT_DESC, N.SORT_DESC | N.SORT_NULLS_FIRST]):
        for k in (10, 300):
            st = check(gpu_ctx, S, [(N.TYPE_INT64, a, None), (N.TYPE_FLOAT64, b, None)], flags, k)
            assert st[1] >= 2 and st[3] >= 2, st  # a step in word 1, then steps in word 0


@pytest.mark.parametrize("which", ["packed", "two_words", "utf8_f64", "four_keys"])
def test_multi_key(gpu_ctx, layout, which):
    T, S = layout
    for n in (S + 1, 2 * T + 1):
        keys, flags = _multi_keys(np.random.default_rng(n), n, which)
        for key in keys:  # null rows of a UTF8 reference key hold b""
            if key[0] == N.TYPE_UTF8 and key[2] is not None:
                key[1][:] = [v if ok else b"" for v, ok in zip(key[1], key[2])]
        cols = [to_device(gpu_ctx, key) for key in keys]
        for k in (1, 17, S // 2, n - 1):
            check(gpu_ctx, S, keys, flags, k, cols=cols)


def test_long_utf8_with_a_shared_prefix(gpu_ctx, layout):
    T, S = layout
    n = T + 1
    rng = np.random.default_rng(43)
    stem = b"0123456789abcdef"  # the two leading chunk words tie on every row
    vals = [stem + bytes(rng.integers(97, 101, 24).astype(np.uint8)) for _ in range(n)]
    for i in rng.choice(n, 40, replace=False):
        vals[i] = vals[0]  # some whole-value ties
    for i in rng.choice(n, 40, replace=False):
        vals[i] = vals[i][: int(rng.integers(16, 40))]  # proper prefixes sort first
    valid = rng.random(n) >= 0.05
    vals = [v if ok else b"" for v, ok in zip(vals, valid)]
    col = ucol(gpu_ctx, vals, valid)
    for flags in ALL_FLAGS:
        for k in (1, 33, 500):
            st = check(gpu_ctx, S, [(N.TYPE_UTF8, vals, valid)], [flags], k, cols=[col])
            assert st[1] >= 1, st


def test_short_utf8_promise(gpu_ctx, layout):
    T, S = layout
    n = T + 1
    rng = np.random.default_rng(47)
    vals = _strings(rng, n, 7)
    valid = rng.random(n) >= 0.1
    vals = [v if ok else b"" for v, ok in zip(vals, valid)]
    col = ucol(gpu_ctx, vals, valid, 7)
    for flags in ALL_FLAGS:
        for k in (1, 64, 1000):
            check(gpu_ctx, S, [(N.TYPE_UTF8, vals, valid)], [flags], k, cols=[col])
    # the promise broken on the most significant key: every row's first word is encoded, so it is found
    for m in (S, T + 1):
        broken = [b"ab"] * m
        broken[m - 1] = b"abcdefghij"
        with pytest.raises(N.IllegalArgumentException, match="max_len"):
            topk_indices([ucol(gpu_ctx, broken, None, 3)], [0], 5, N.TOPK_SELECT)


# ---- the modes ------------------------------------------------------------------------------------------------
def test_auto_takes_the_path_the_rule_names(gpu_ctx, layout):
    _, S = layout
    _, div = TR.header_constants()
    n = 1 << 20
    vals = gen.generate(gen.GEN_RAW, 0, 12, N.TYPE_INT64, 0, n)[0]
    key = (N.TYPE_INT64, vals, None)
    col = to_device(gpu_ctx, key)
    full = R.order([key], [0])
    for k in (10, 1000):
        got = topk_indices([col], [0], k)  # AUTO
        gpu_ctx.synchronize()
        st = topk_last_stats(gpu_ctx)
        assert st[0] == int(TR.use_select(n, k, S, div)) == 1
        assert st[2] <= max(S, 2 * k)
        assert np.array_equal(got.to_numpy(), full[:k])
    for k, n_small in ((5, S), (S + 5, S + 5), (S + 1, S + 1)):  # AUTO sorts a single-workgroup input and k >= n
        c = prefix(col, n_small)
        got = topk_indices([c], [0], k)
        gpu_ctx.synchronize()
        assert topk_last_stats(gpu_ctx)[0] == int(TR.use_select(n_small, k, S, div)) == 0
        assert np.array_equal(got.to_numpy(), R.order([key_prefix(key, n_small)], [0], limit=k))


def test_the_three_modes_agree(gpu_ctx, layout):
    T, S = layout
    n = 2 * T + 1
    keys, flags = _multi_keys(np.random.default_rng(3), n, "two_words")
    cols = [to_device(gpu_ctx, key) for key in keys]
    for k in (0, 1, 100, n // 16, n // 2, n, n + 5):
        outs, paths = [], []
        for mode in (N.TOPK_AUTO, N.TOPK_SELECT, N.TOPK_SORT):
            o = topk_indices(cols, flags, k, mode)
            gpu_ctx.synchronize()
            outs.append(o.to_numpy().tobytes())
            paths.append(topk_last_stats(gpu_ctx)[0])
        assert outs[0] == outs[1] == outs[2] == R.order(keys, flags, limit=k).tobytes(), k
        assert paths[1] == 1 and paths[2] == 0


def test_two_calls_and_two_contexts_give_identical_bytes(gpu_ctx, layout):
    import torch

    T, S = layout
    n = 2 * T + 1
    rng = np.random.default_rng(53)
    vals = rng.integers(-3, 3, n).astype(np.int64)  # heavy ties: the order among equals is the point
    valid = rng.random(n) >= 0.1

    def run(ctx):
        col = DeviceColumn.from_numpy(N.TYPE_INT64, vals, valid, ctx=ctx)
        out = topk_indices([col], [N.SORT_DESC], 3000, N.TOPK_SELECT)
        ctx.synchronize()
        assert topk_last_stats(ctx)[0] == 1
        return out.to_numpy().tobytes()

    first = run(gpu_ctx)
    stream = torch.cuda.Stream(device=gpu_ctx.torch_device)
    with torch.cuda.stream(stream):  # the second call on a second context with its own stream
        other = Context(0, stream.cuda_stream)
        second = run(other)
        other.synchronize()
    assert first == second == R.order([(N.TYPE_INT64, vals, valid)], [N.SORT_DESC], limit=3000).tobytes()


def test_argument_errors(gpu_ctx):
    a = DeviceColumn.from_numpy(N.TYPE_INT64, np.arange(100, dtype=np.int64), ctx=gpu_ctx)
    kc = (N.QeColumn * 1)(a.as_c())
    fl = (N.C.c_int32 * 1)(0)

    def call(k, mode, out):
        oc = out.as_c()
        return N.lib().qe_topk_indices(gpu_ctx.handle, kc, fl, 1, k, mode, N.C.byref(oc))

    good = DeviceColumn.empty(N.TYPE_INT32, 10, False, ctx=gpu_ctx)
    assert call(10, N.TOPK_SELECT, good) == N.QE_OK
    assert call(-1, N.TOPK_SELECT, good) == N.QE_ERR_INVALID_ARG
    assert call(-1, N.TOPK_SORT, good) == N.QE_ERR_INVALID_ARG
    for mode in (3, -1, 99):
        assert call(10, mode, good) == N.QE_ERR_INVALID_ARG
    for mode in (N.TOPK_AUTO, N.TOPK_SELECT, N.TOPK_SORT):
        assert call(10, mode, DeviceColumn.empty(N.TYPE_INT32, 9, False, ctx=gpu_ctx)) == N.QE_ERR_CAPACITY
        assert call(10, mode, DeviceColumn.empty(N.TYPE_INT64, 10, False, ctx=gpu_ctx)) == N.QE_ERR_INVALID_ARG
    with pytest.raises(N.IllegalArgumentException):
        topk_indices([a], [0], -5)
    with pytest.raises(N.IllegalArgumentException):
        topk_indices([a], [4], 5)
    empty = DeviceColumn.from_numpy(N.TYPE_INT64, np.zeros(0, dtype=np.int64), ctx=gpu_ctx)
    for mode in (N.TOPK_AUTO, N.TOPK_SELECT, N.TOPK_SORT):  # k = 0 and n = 0 are legal and write nothing
        assert topk_indices([empty], [0], 5, mode).length == 0
        assert topk_indices([a], [0], 0, mode).length == 0


# ---- host mirror ------------------------------------------------------------------------------------------------
def test_sortexec_limit_equals_the_prefix_of_sortexec(gpu_ctx):
    from kquery.expressions import ColumnExpression

    rng = np.random.default_rng(2)
    lens = [1001, 7, 4096, 4900]
    n = sum(lens)
    k = rng.integers(-40, 40, n).astype(np.int64)
    kv = rng.random(n) >= 0.1
    pay = [None if rng.random() < 0.2 else f"row{i}-{'é' * (i % 3)}" for i in range(n)]
    schema = Schema([Field("k", N.TYPE_INT64), Field("payload", N.TYPE_UTF8)])

    def batches():
        cuts = np.concatenate([[0], np.cumsum(lens)])
        return _Batches(schema, [RecordBatch(schema, [DeviceColumn.from_numpy(N.TYPE_INT64, k[a:b], kv[a:b], ctx=gpu_ctx),
                                                       DeviceColumn.from_strings(pay[a:b], ctx=gpu_ctx)])
                                 for a, b in zip(cuts[:-1], cuts[1:])])

    exprs = [(ColumnExpression(0), False, True)]
    whole = next(SortExec(batches(), exprs).execute())
    wk, wp = whole.field(0).to_pylist(), whole.field(1).to_pylist()
    for limit in (0, 1, 25, 600, n, n + 3):
        out = next(SortExec(batches(), exprs, limit=limit).execute())
        assert out.rowCount() == min(limit, n)
        assert out.field(0).to_pylist() == wk[:limit] and out.field(1).to_pylist() == wp[:limit]
        if 0 < limit:
            st = topk_last_stats(gpu_ctx)
            assert st[0] == int(TR.use_select(n, limit, sort_layout()[1], TR.header_constants()[1]))


def test_sortexec_limit_over_a_group_by_result(gpu_ctx):
    from kquery.aggregate import HashAggregateState
    from kquery.datasource import C4_COLUMNS, generate_column
    from kquery.expressions import ColumnExpression
    from kquery.workloads import C4_AGGS, c4_spec

    n = 200_003
    st = HashAggregateState(gpu_ctx, [N.TYPE_INT64], C4_AGGS, 1024)
    st.update_fused([generate_column(s, n, 0, 42, gpu_ctx) for s in C4_COLUMNS], c4_spec())
    keys, aggs = st.finalize()
    schema = Schema([Field("k", N.TYPE_INT64)] + [Field(f"a{j}", N.TYPE_INT64) for j in range(len(aggs))])
    exprs = [(ColumnExpression(1), False, False), (ColumnExpression(0), True, False)]
    plan = lambda limit: SortExec(_Batches(schema, [RecordBatch(schema, keys + aggs)]), exprs, limit=limit)  # noqa: E731
    whole = next(plan(None).execute())
    rows = list(zip(*[whole.field(j).to_pylist() for j in range(1 + len(aggs))]))
    assert len(rows) == 1024
    for limit in (5, 64, 1024):
        out = next(plan(limit).execute())
        assert list(zip(*[out.field(j).to_pylist() for j in range(1 + len(aggs))])) == rows[:limit]
