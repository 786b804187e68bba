"""Equi-join on the device: qe_join_build / qe_join_probe / qe_join_probe_mask / qe_join_stats,
qe_take_or_null and HashJoinExec, against tests/joinref.py. The pair sequence is fixed (by probe row,
then by build row), so every check compares exact arrays: there is no tolerance anywhere."""
import numpy as np
import pytest

import joinref as R
from kquery import native as N
from kquery.columnar import Context, DeviceColumn, Field, RecordBatch, Schema
from kquery.operators import (HashJoinExec, PhysicalPlan, join_build, join_probe, join_probe_mask, join_stats, sort_layout,
                              take, take_or_null)

pytestmark = pytest.mark.gpu

KEY_TYPES = [N.TYPE_INT64, N.TYPE_INT32, N.TYPE_DATE32, N.TYPE_UINT8, N.TYPE_BOOL, N.TYPE_FLOAT64]
BUILD_ROWS = [0, 1, 63, 64, 65, 2049, 200_003]  # one wave, one workgroup, the multi-block scan, a ragged tail
PROBE_ROWS = [0, 1, 64, 4097, 1_000_003]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
KINDS = {"inner": N.JOIN_INNER, "left": N.JOIN_LEFT}


# ---- columns --------------------------------------------------------------------------------------
def dev(ctx, col) -> DeviceColumn:
    t, vals, valid = col
    return DeviceColumn.from_numpy(t, np.asarray(vals), valid, ctx=ctx)


def _nulls(rng, n, on):
    return (rng.random(n) >= 0.1) if on else None


def unique_values(t, n, rng):
    """(at most n distinct values of type t, further values that are none of them)."""
    if t == N.TYPE_BOOL:
        return np.array([True, False][: min(n, 2)], dtype=bool), np.array([True, False][min(n, 2):], dtype=bool)
    if t == N.TYPE_UINT8:
        p = rng.permutation(256).astype(np.uint8)
        k = min(n, 200)
        return p[:k], p[k:]
    if t == N.TYPE_FLOAT64:
        v = np.unique((rng.integers(-(1 << 40), 1 << 40, 2 * n + 16) * 0.25).astype(np.float64))
    elif t == N.TYPE_INT64:
        v = np.unique(rng.integers(0, 1 << 64, 2 * n + 16, dtype=np.uint64).view(np.int64))
    else:
        v = np.unique(rng.integers(-(1 << 31), 1 << 31, 2 * n + 16).astype(np.int32))
    v = rng.permutation(v)
    return v[:n], v[n:]


def probe_values(present, absent, m, rng):
    """m probe values, about half of them build keys (repeats included)."""
    pool = np.concatenate([present, absent]) if len(absent) else present
    if len(pool) == 0 or m == 0:
        return pool[:0]
    if len(present) == 0 or len(absent) == 0:
        return pool[rng.integers(0, len(pool), m)]
    pick = rng.random(m) < 0.5
    return np.where(pick, present[rng.integers(0, len(present), m)], absent[rng.integers(0, len(absent), m)])


def mod7_values(t, n, rng):
    u = rng.integers(0, 7, n)
    if t == N.TYPE_BOOL:
        return (u & 1).astype(bool)
    if t == N.TYPE_FLOAT64:
        return (u - 3) * 0.5
    if t == N.TYPE_UINT8:
        return u.astype(np.uint8)
    return (u - 3).astype(np.int64 if t == N.TYPE_INT64 else np.int32)


# ---- the device against the reference ------------------------------------------------------------------
def _same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{name}: first difference at {bad} of {len(want)}: got {got[bad]}, want {want[bad]}")


def check_probe(ctx, table, probe, want):
    dp = dev(ctx, probe)
    for kind, code in KINDS.items():
        pi, bi = join_probe(table, dp, code)
        ctx.synchronize()
        _same(f"{kind} probe rows", pi.to_numpy(), want[kind][0])
        _same(f"{kind} build rows", bi.to_numpy(), want[kind][1])
    for kind in ("semi", "anti"):
        mask = join_probe_mask(table, dp, anti=kind == "anti")
        ctx.synchronize()
        _same(kind, mask.to_numpy(), want[kind])
        n = dp.length
        if n % 32:  # whole words are written: the bits past the last row are clear
            words = mask.values.cpu().numpy().view(np.uint32)
            assert int(words[n // 32]) >> (n % 32) == 0


def check(ctx, build, probes, unique=None):
    """One build side against every probe side of `probes`, every kind, and the table's stats."""
    bw = R.key_words(build)
    table = join_build(dev(ctx, build))
    try:
        stats = join_stats(table)
        assert stats == R.stats(bw)
        if unique is not None:
            assert (stats[2] <= 1) == unique
        for probe in probes:
            assert R.compatible(build[0], probe[0])
            check_probe(ctx, table, probe, R.join_all(bw, R.key_words(probe)))
    finally:
        table.close()
    return stats


# ---- shapes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", BUILD_ROWS)
def test_every_shape_unique_int64_keys(gpu_ctx, nb):
    rng = np.random.default_rng(100 + nb)
    present, absent = unique_values(N.TYPE_INT64, nb, rng)
    # the largest probe side once per path of the build (empty, one workgroup, many): it costs the most
    sizes = [m for m in PROBE_ROWS if m < 1_000_003 or nb in (0, 65, 200_003)]
    probes = [(N.TYPE_INT64, probe_values(present, absent, m, rng), None) for m in sizes]
    stats = check(gpu_ctx, (N.TYPE_INT64, present, None), probes, unique=True)
    assert stats[0] == nb and stats[1] == nb and stats[2] == min(nb, 1)


@pytest.mark.parametrize("nulls", [False, True], ids=["nonull", "nulls"])
@pytest.mark.parametrize("t", KEY_TYPES)
def test_unique_build_keys_every_type(gpu_ctx, t, nulls):
    rng = np.random.default_rng(200 + t)
    present, absent = unique_values(t, 2049, rng)
    build = (t, present, _nulls(rng, len(present), nulls))
    probes = [(t, probe_values(present, absent, m, rng), _nulls(rng, m, nulls)) for m in (64, 4097)]
    stats = check(gpu_ctx, build, probes, unique=True)
    assert stats[0] > 0 and stats[2] == 1  # a primary-key build: no ordering work


@pytest.mark.parametrize("nulls", [False, True], ids=["nonull", "nulls"])
@pytest.mark.parametrize("t", KEY_TYPES)
def test_duplicate_build_keys_every_type(gpu_ctx, t, nulls):
    rng = np.random.default_rng(300 + t)
    build = (t, mod7_values(t, 2049, rng), _nulls(rng, 2049, nulls))
    probes = [(t, mod7_values(t, m, rng), _nulls(rng, m, nulls)) for m in (1, 300)]
    stats = check(gpu_ctx, build, probes, unique=False)
    assert stats[1] == (2 if t == N.TYPE_BOOL else 7)


@pytest.mark.parametrize("nulls", [False, True], ids=["nonull", "nulls"])
def test_int32_build_int64_probe(gpu_ctx, nulls):
    rng = np.random.default_rng(400)
    present, absent = unique_values(N.TYPE_INT32, 2049, rng)
    # INT64 probe values beyond the INT32 range whose low words are build keys must not match
    wide = present[:500].astype(np.int64) + (1 << 32)
    pv = np.concatenate([probe_values(present, absent, 3000, rng).astype(np.int64), wide])
    check(gpu_ctx, (N.TYPE_INT32, present, _nulls(rng, len(present), nulls)),
          [(N.TYPE_INT64, pv, _nulls(rng, len(pv), nulls))], unique=True)
    dup = (N.TYPE_INT32, mod7_values(N.TYPE_INT32, 2049, rng), _nulls(rng, 2049, nulls))
    check(gpu_ctx, dup, [(N.TYPE_INT64, mod7_values(N.TYPE_INT64, 300, rng), _nulls(rng, 300, nulls)),
                         (N.TYPE_DATE32, mod7_values(N.TYPE_DATE32, 300, rng), None)], unique=False)
    # and the other way round: an INT64 build side probed by INT32 and UINT8
    b64 = np.array([-1, 255, 0, 1 << 32, -(1 << 31), (1 << 31) - 1, 255], dtype=np.int64)
    check(gpu_ctx, (N.TYPE_INT64, b64, None),
          [(N.TYPE_INT32, np.array([-1, 255, 0, -(1 << 31), (1 << 31) - 1, 7], dtype=np.int32), None),
           (N.TYPE_UINT8, np.array([255, 0, 1], dtype=np.uint8), None),
           (N.TYPE_BOOL, np.array([True, False]), None)])


def test_skewed_duplicate_keys(gpu_ctx):
    """Key mod 7 plus one key holding 5,000 of the 20,000 build rows; 300 probe rows on it: 1.5M pairs."""
    rng = np.random.default_rng(500)
    bv = mod7_values(N.TYPE_INT64, 20_000, rng)
    bv[rng.permutation(20_000)[:5_000]] = 1000
    build = (N.TYPE_INT64, bv, None)
    heavy = (N.TYPE_INT64, np.full(300, 1000, dtype=np.int64), None)
    mixed = (N.TYPE_INT64, rng.choice(np.array([-3, 0, 3, 4, 1000, 1001], dtype=np.int64), 100), rng.random(100) >= 0.1)
    stats = check(gpu_ctx, build, [heavy, mixed], unique=False)
    assert stats == (20_000, 8, 5_000, R.slots(20_000))
    assert len(R.join_all(R.key_words(build), R.key_words(heavy))["inner"][0]) == 1_500_000


def test_big_duplicate_build_side(gpu_ctx):
    """Duplicates over many tiles of the ordering passes: 200,003 build rows, three rows per key on average."""
    rng = np.random.default_rng(600)
    bv = (rng.integers(0, 66_000, 200_003).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
    build = (N.TYPE_INT64, bv, rng.random(200_003) >= 0.1)
    pv = np.concatenate([bv[rng.integers(0, 200_003, 3000)], rng.integers(0, 1 << 62, 1097)])
    check(gpu_ctx, build, [(N.TYPE_INT64, pv, rng.random(4097) >= 0.1)], unique=False)


def test_duplicate_build_side_one_row_past_a_tile(gpu_ctx):
    """The ordering passes with a last tile of one row (T + 1 and 2 T + 1 build rows, three rows per key on
    average), over slot words whose bit count is no multiple of the 8-bit digit."""
    T, _ = sort_layout()
    for nb in (T + 1, 2 * T + 1):
        rng = np.random.default_rng(610 + nb)
        bv = (rng.integers(0, nb // 3, nb).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
        pv = np.concatenate([bv[rng.integers(0, nb, 500)], rng.integers(0, 1 << 62, 141)])
        stats = check(gpu_ctx, (N.TYPE_INT64, bv, rng.random(nb) >= 0.1), [(N.TYPE_INT64, pv, rng.random(641) >= 0.1)], unique=False)
        assert (stats[3] + 1).bit_length() % 8 != 0  # the passes sort by the bits of slots + 1


# ---- edge keys ---------------------------------------------------------------------------------------------
def test_edge_keys_catch_the_sentinel(gpu_ctx):
    edge = np.array([0, -1, I64_MIN, I64_MAX], dtype=np.int64)
    probe = np.array([I64_MAX, -1, 0, I64_MIN, 1, -2, I64_MIN + 1, I64_MAX - 1, -1, 0], dtype=np.int64)
    check(gpu_ctx, (N.TYPE_INT64, edge, None), [(N.TYPE_INT64, probe, None)], unique=True)
    # the same keys twice over, some null: -1 (every bit set) has its run like any other key
    b2 = np.concatenate([edge, edge[::-1], [5]])
    check(gpu_ctx, (N.TYPE_INT64, b2, np.array([1, 1, 1, 1, 1, 1, 0, 1, 1], dtype=bool)),
          [(N.TYPE_INT64, probe, np.array([1, 1, 1, 1, 1, 1, 1, 1, 0, 1], dtype=bool))], unique=False)
    # without the key -1 on the build side, a probe for it finds nothing
    check(gpu_ctx, (N.TYPE_INT64, np.array([0, I64_MIN, I64_MAX], dtype=np.int64), None), [(N.TYPE_INT64, probe, None)])
    # INT32 -1 sign-extends onto the same word
    check(gpu_ctx, (N.TYPE_INT32, np.array([-1, 0, 7], dtype=np.int32), None), [(N.TYPE_INT64, probe, None)])


def test_fp64_nans_and_zeros(gpu_ctx):
    bits = np.array([0x7FF8000000000000, 0xFFF8DEADBEEF0001, 0x0000000000000000, 0x8000000000000000,
                     0x3FF0000000000000, 0x7FF0000000000000], dtype=np.uint64)
    pbits = np.array([0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x8000000000000000, 0x0000000000000000,
                      0xFFF0000000000000, 0x3FF0000000000000, 0x7FF8000000000000, 0x0000000000000001], dtype=np.uint64)
    build = (N.TYPE_FLOAT64, bits.view(np.float64), None)
    probe = (N.TYPE_FLOAT64, pbits.view(np.float64), None)
    stats = check(gpu_ctx, build, [probe], unique=False)
    assert stats == (6, 5, 2, 64)  # the two NaNs are one key, the two zeros are two
    want = R.join_all(R.key_words(build), R.key_words(probe))["inner"]
    assert want[0].tolist() == [0, 0, 1, 1, 2, 3, 5, 6, 6] and want[1].tolist() == [0, 1, 0, 1, 3, 2, 4, 0, 1]


def test_type_pairs_that_do_not_join(gpu_ctx):
    ints = DeviceColumn.from_numpy(N.TYPE_INT64, np.arange(4), ctx=gpu_ctx)
    flts = DeviceColumn.from_numpy(N.TYPE_FLOAT64, np.arange(4) * 1.0, ctx=gpu_ctx)
    for b, p in ((ints, flts), (flts, ints)):
        table = join_build(b)
        try:
            with pytest.raises(N.IllegalArgumentException):
                join_probe(table, p)
            with pytest.raises(N.IllegalArgumentException):
                join_probe_mask(table, p)
        finally:
            table.close()
    with pytest.raises(N.IllegalArgumentException):
        join_build(DeviceColumn.from_strings(["a"], ctx=gpu_ctx))


# ---- capacity -----------------------------------------------------------------------------------------------
def test_capacity_carve_and_retry(gpu_ctx):
    import torch

    rng = np.random.default_rng(700)
    build = (N.TYPE_INT64, mod7_values(N.TYPE_INT64, 500, rng), None)
    probe = (N.TYPE_INT64, mod7_values(N.TYPE_INT64, 100, rng), None)
    want = R.join_all(R.key_words(build), R.key_words(probe))
    exact = len(want["inner"][0])
    assert exact > 100
    table = join_build(dev(gpu_ctx, build))
    try:
        dp = dev(gpu_ctx, probe)
        kc = dp.as_c()
        for cap in (0, 100, exact - 1):
            pi = DeviceColumn.empty(N.TYPE_INT32, exact, False, ctx=gpu_ctx)
            bi = DeviceColumn.empty(N.TYPE_INT32, exact, False, ctx=gpu_ctx)
            pi.values.fill_(0x5A5A5A5A)
            bi.values.fill_(0x3C3C3C3C)
            pi.length = bi.length = cap
            pc, bc = pi.as_c(), bi.as_c()
            pairs = N.C.c_int64(-1)
            st = N.lib().qe_join_probe(table.handle, N.C.byref(kc), N.JOIN_INNER, N.C.byref(pc), N.C.byref(bc), N.C.byref(pairs))
            gpu_ctx.synchronize()
            assert st == N.QE_ERR_CAPACITY and pairs.value == exact
            assert bool(torch.all(pi.values == 0x5A5A5A5A)) and bool(torch.all(bi.values == 0x3C3C3C3C))
        pi, bi = join_probe(table, dp, N.JOIN_INNER, capacity=exact)  # an exact capacity succeeds
        gpu_ctx.synchronize()
        _same("exact capacity", pi.to_numpy(), want["inner"][0])
        pi, bi = join_probe(table, dp, N.JOIN_INNER)  # the wrapper: a short first try, then the exact size
        gpu_ctx.synchronize()
        _same("retry probe rows", pi.to_numpy(), want["inner"][0])
        _same("retry build rows", bi.to_numpy(), want["inner"][1])
        pi, bi = join_probe(table, dp, N.JOIN_LEFT, capacity=1)
        gpu_ctx.synchronize()
        _same("left retry", bi.to_numpy(), want["left"][1])
    finally:
        table.close()


# ---- forged collisions -----------------------------------------------------------------------------------------
def test_forged_collisions_wrap_the_table_end(gpu_ctx):
    """1,000 distinct keys with one home slot three before the table's end: the probe chain is 1,000
    slots long and wraps. Probed with them and with 1,000 absent keys of the same home slot."""
    rng = np.random.default_rng(800)
    table = join_build(DeviceColumn.from_numpy(N.TYPE_INT64, np.arange(1000), ctx=gpu_ctx))
    try:
        nslots = join_stats(table)[3]
    finally:
        table.close()
    assert nslots == R.slots(1000) == 2048
    home = nslots - 3
    present = np.array([R.signed(w) for w in R.forge_keys(nslots, home, 1000)], dtype=np.int64)
    absent = np.array([R.signed(w) for w in R.forge_keys(nslots, home, 1000, first=1000)], dtype=np.int64)
    assert all(R.home_slot(int(k) & R.M64, nslots) == home for k in present[:10])
    pv = rng.permutation(np.concatenate([present, absent, present[:100]]))
    stats = check(gpu_ctx, (N.TYPE_INT64, rng.permutation(present), None), [(N.TYPE_INT64, pv, None)], unique=True)
    assert stats == (1000, 1000, 1, 2048)
    # duplicates of forged keys: runs must not depend on where in the chain a key landed
    dup = rng.permutation(np.concatenate([present[:300], present[:300], present[:50]]))
    check(gpu_ctx, (N.TYPE_INT64, dup, None), [(N.TYPE_INT64, pv, None)], unique=False)


# ---- qe_take_or_null --------------------------------------------------------------------------------------------
def _payload_columns(ctx, n, rng):
    ok = rng.random(n) >= 0.2
    strs = [None if rng.random() < 0.2 else "s%d-%s" % (i, "é" * (i % 4)) for i in range(n)]
    return [
        DeviceColumn.from_numpy(N.TYPE_INT64, rng.integers(-(1 << 62), 1 << 62, n), ok, ctx=ctx),
        DeviceColumn.from_numpy(N.TYPE_INT32, rng.integers(-100, 100, n).astype(np.int32), ctx=ctx),
        DeviceColumn.from_numpy(N.TYPE_UINT8, rng.integers(1, 255, n).astype(np.uint8), ctx=ctx),
        DeviceColumn.from_numpy(N.TYPE_BOOL, rng.random(n) < 0.5, ok, ctx=ctx),
        DeviceColumn.from_numpy(N.TYPE_BOOL, np.ones(n, dtype=bool), ctx=ctx),
        DeviceColumn.from_numpy(N.TYPE_FLOAT64, rng.normal(size=n), ctx=ctx),
        DeviceColumn.from_strings(strs, ctx=ctx),
        DeviceColumn.from_strings(["v%d" % i for i in range(n)], ctx=ctx),
    ]


def test_take_or_null(gpu_ctx):
    rng = np.random.default_rng(900)
    n = 37
    cols = _payload_columns(gpu_ctx, n, rng)
    rows = [c.to_pylist() for c in cols]
    idx = rng.integers(-1, n, 150).astype(np.int32)  # more than two waves, repeats, about four -1
    idx[[0, 63, 64, 149]] = -1
    di = DeviceColumn.from_numpy(N.TYPE_INT32, idx, ctx=gpu_ctx)
    nbytes = [sum(len(r[i].encode()) for i in idx if i >= 0 and r[i] is not None) if c.type == N.TYPE_UTF8 else None
              for c, r in zip(cols, rows)]
    outs = take_or_null(di, cols, nbytes)
    gpu_ctx.synchronize()
    for c, r, o in zip(cols, rows, outs):
        assert o.type == c.type and o.length == len(idx) and o.validity is not None
        assert o.to_pylist() == [None if i < 0 else r[i] for i in idx]
        if c.type != N.TYPE_UTF8:  # zero where a value is written
            assert not np.any(o.to_numpy()[idx < 0])
        else:
            offs = o.offsets.cpu().numpy()
            assert np.all((offs[1:] - offs[:-1])[idx < 0] == 0)
    # every index -1, and no index at all
    for m in (3, 0):
        outs = take_or_null(DeviceColumn.from_numpy(N.TYPE_INT32, np.full(m, -1, dtype=np.int32), ctx=gpu_ctx), cols,
                            [0 if c.type == N.TYPE_UTF8 else None for c in cols])
        gpu_ctx.synchronize()
        assert all(o.to_pylist() == [None] * m for o in outs)


def test_take_or_null_refusals(gpu_ctx):
    col = DeviceColumn.from_numpy(N.TYPE_INT64, np.arange(5), ctx=gpu_ctx)
    idx = DeviceColumn.from_numpy(N.TYPE_INT32, np.array([0, -1, 4], dtype=np.int32), ctx=gpu_ctx)
    out = DeviceColumn.empty(N.TYPE_INT64, 3, False, ctx=gpu_ctx)  # no validity buffer: refused
    ic, cc, oc = idx.as_c(), col.as_c(), out.as_c()
    st = N.lib().qe_take_or_null(gpu_ctx.handle, N.C.byref(ic), N.C.byref(cc), 1, N.C.byref(oc), None)
    assert st == N.QE_ERR_INVALID_ARG
    for bad in (5, -2):  # any other index outside [0, n) is still an error
        with pytest.raises(N.IllegalArgumentException):
            take_or_null(DeviceColumn.from_numpy(N.TYPE_INT32, np.array([0, bad], dtype=np.int32), ctx=gpu_ctx), [col])
    with pytest.raises(N.IllegalArgumentException):  # qe_take itself is unchanged: -1 is out of range
        take(idx, [col])
    assert take_or_null(idx, [col])[0].to_pylist() == [0, None, 4]


# ---- HashJoinExec ------------------------------------------------------------------------------------------------------
class _Batches(PhysicalPlan):
    def __init__(self, schema, batches):
        self._schema, self.batches = schema, batches

    def schema(self):
        return self._schema

    def execute(self):
        return iter(self.batches)


def _col(ctx, t, vals):
    """Device column from a list with None for nulls."""
    if t == N.TYPE_UTF8:
        return DeviceColumn.from_strings(vals, ctx=ctx)
    valid = np.array([v is not None for v in vals], dtype=bool)
    dt = {N.TYPE_INT64: np.int64, N.TYPE_FLOAT64: np.float64, N.TYPE_INT32: np.int32}[t]
    return DeviceColumn.from_numpy(t, np.array([v if v is not None else 0 for v in vals], dtype=dt),
                                   None if valid.all() else valid, ctx=ctx)


def _side(ctx, schema, table, cuts):
    """Batches [cuts[i], cuts[i + 1]) of a table given as one list per column."""
    return _Batches(schema, [RecordBatch(schema, [_col(ctx, f.dataType, c[a:b]) for f, c in zip(schema.fields, table)])
                             for a, b in zip(cuts[:-1], cuts[1:])])


def _words(keys):
    """Join key words of rows given as tuples of Python values: any null member -> None."""
    return [None if any(v is None for v in k) else k for k in keys]


def check_exec(ctx, lschema, ltab, lcuts, rschema, rtab, rcuts, on, lkeys, rkeys):
    """HashJoinExec of every kind, one output batch per left batch, column by column."""
    from kquery.expressions import ColumnExpression

    bw = _words(list(zip(*[rtab[j] for j in rkeys])))
    for kind in HashJoinExec.KINDS:
        plan = HashJoinExec(_side(ctx, lschema, ltab, lcuts), _side(ctx, rschema, rtab, rcuts),
                            [(ColumnExpression(a), ColumnExpression(b)) for a, b in on], kind)
        nl, nr = len(lschema.fields), len(rschema.fields)
        assert len(plan.schema().fields) == (nl if kind in ("semi", "anti") else nl + nr)
        outs = list(plan.execute())
        assert len(outs) == len(lcuts) - 1
        for out, a, b in zip(outs, lcuts[:-1], lcuts[1:]):
            pw = _words(list(zip(*[ltab[j][a:b] for j in lkeys])))
            want = R.join(bw, pw, kind)
            if kind in ("semi", "anti"):
                keep = np.flatnonzero(want)
                assert len(out.fields) == nl
                for j in range(nl):
                    assert out.field(j).to_pylist() == [ltab[j][a + i] for i in keep], (kind, j)
                continue
            pi, bi = want
            assert len(out.fields) == nl + nr
            for j in range(nl):
                assert out.field(j).to_pylist() == [ltab[j][a + i] for i in pi], (kind, j)
            for j in range(nr):
                assert out.field(nl + j).to_pylist() == [None if i < 0 else rtab[j][i] for i in bi], (kind, j)


def test_exec_two_probe_batches_with_utf8_payloads(gpu_ctx):
    rng = np.random.default_rng(1000)
    nl, nr = 1500, 400
    lschema = Schema([Field("k", N.TYPE_INT64), Field("lp", N.TYPE_UTF8)])
    rschema = Schema([Field("rk", N.TYPE_INT64), Field("rp", N.TYPE_UTF8), Field("rv", N.TYPE_FLOAT64)])
    ltab = [[None if rng.random() < 0.1 else int(v) for v in rng.integers(0, 150, nl)],
            [None if i % 11 == 0 else "left-%d-%s" % (i, "ü" * (i % 5)) for i in range(nl)]]
    # about four build rows per key: every matched left row repeats, and so do the right rows, so both
    # UTF8 payloads outgrow their input's byte count
    rtab = [[None if rng.random() < 0.1 else int(v) for v in rng.integers(0, 100, nr)],
            [None if i % 7 == 0 else "right-payload-%d" % i for i in range(nr)],
            [None if i % 5 == 0 else float(i) * 0.5 for i in range(nr)]]
    check_exec(gpu_ctx, lschema, ltab, [0, 1001, nl], rschema, rtab, [0, 100, 100, nr], [(0, 0)], [0], [0])


def test_exec_lone_utf8_key(gpu_ctx):
    rng = np.random.default_rng(1100)
    vocab = ["", "a", "abcdefg", "abcdefgh", "abcdefgX", "abcdefghi", "é" * 3 + "x", "é" * 4, "only-left", "only-right-long-value"]
    lschema = Schema([Field("name", N.TYPE_UTF8), Field("x", N.TYPE_INT64)])
    rschema = Schema([Field("name", N.TYPE_UTF8), Field("y", N.TYPE_INT32)])
    lv = [v for v in vocab if v != "only-right-long-value"]
    rv = [v for v in vocab if v != "only-left"]
    ltab = [[None if rng.random() < 0.1 else lv[int(i)] for i in rng.integers(0, len(lv), 300)], list(range(300))]
    rtab = [[None if rng.random() < 0.1 else rv[int(i)] for i in rng.integers(0, len(rv), 40)], list(range(40))]
    check_exec(gpu_ctx, lschema, ltab, [0, 130, 300], rschema, rtab, [0, 40], [(0, 0)], [0], [0])
    # every value at most 7 bytes: the keys are their own codes
    short = ["", "a", "abcdefg", "é" * 3 + "x"]
    ltab = [[short[int(i)] for i in rng.integers(0, 4, 100)], list(range(100))]
    rtab = [[short[int(i)] for i in rng.integers(0, 3, 10)], list(range(10))]
    check_exec(gpu_ctx, lschema, ltab, [0, 100], rschema, rtab, [0, 10], [(0, 0)], [0], [0])


def test_exec_two_keys_with_nulls_in_either_member(gpu_ctx):
    rng = np.random.default_rng(1200)
    lschema = Schema([Field("a", N.TYPE_INT64), Field("s", N.TYPE_UTF8), Field("x", N.TYPE_FLOAT64)])
    rschema = Schema([Field("s", N.TYPE_UTF8), Field("a", N.TYPE_INT64)])
    names = ["ab", "abcdefgh-long", "", "zz"]

    def rows(n):
        return ([None if rng.random() < 0.15 else int(v) for v in rng.integers(0, 4, n)],
                [None if rng.random() < 0.15 else names[int(v)] for v in rng.integers(0, 4, n)])

    la, ls = rows(500)
    ra, rs = rows(60)
    # rows whose keys are both null on both sides exist, and must not pair
    la[:2], ls[:2], ra[:2], rs[:2] = [None, 1], [None, None], [None, 1], [None, None]
    ltab = [la, ls, [float(i) for i in range(500)]]
    rtab = [rs, ra]
    check_exec(gpu_ctx, lschema, ltab, [0, 77, 500], rschema, rtab, [0, 60], [(0, 1), (1, 0)], [0, 1], [1, 0])


def test_exec_empty_build_side(gpu_ctx):
    lschema = Schema([Field("k", N.TYPE_INT64), Field("s", N.TYPE_UTF8)])
    rschema = Schema([Field("k", N.TYPE_INT64), Field("t", N.TYPE_UTF8), Field("b", N.TYPE_FLOAT64)])
    ltab = [[1, None, 3], ["x", "y", None]]
    rtab = [[], [], []]
    for rcuts in ([0], [0, 0]):  # no build batch at all, and one batch of no rows
        check_exec(gpu_ctx, lschema, ltab, [0, 3], rschema, rtab, rcuts, [(0, 0)], [0], [0])
    from kquery.expressions import ColumnExpression

    on = [(ColumnExpression(0), ColumnExpression(0))]
    out = {k: next(HashJoinExec(_side(gpu_ctx, lschema, ltab, [0, 3]), _side(gpu_ctx, rschema, rtab, [0]), on, k).execute())
           for k in HashJoinExec.KINDS}
    assert out["inner"].rowCount() == 0 and out["semi"].rowCount() == 0
    assert out["anti"].field(0).to_pylist() == [1, None, 3]
    assert [out["left"].field(j).to_pylist() for j in range(5)] == [[1, None, 3], ["x", "y", None]] + [[None] * 3] * 3
    with pytest.raises(N.IllegalArgumentException):
        HashJoinExec(_side(gpu_ctx, lschema, ltab, [0, 3]), _side(gpu_ctx, rschema, rtab, [0]), on, "full")
    with pytest.raises(N.IllegalArgumentException):
        HashJoinExec(_side(gpu_ctx, lschema, ltab, [0, 3]), _side(gpu_ctx, rschema, rtab, [0]), [], "inner")


def test_aggregate_over_inner_join(gpu_ctx):
    from kquery.expressions import ColumnExpression, CountStarExpression, SumExpression
    from kquery.operators import HashAggregateExec, fuse

    rng = np.random.default_rng(1300)
    nl, nr = 5000, 64
    lschema = Schema([Field("vendor", N.TYPE_INT64), Field("amount", N.TYPE_INT64)])
    rschema = Schema([Field("id", N.TYPE_INT64), Field("name", N.TYPE_UTF8)])
    ltab = [[int(v) for v in rng.integers(0, 80, nl)], [int(v) for v in rng.integers(-1000, 1000, nl)]]
    rtab = [list(range(nr)), ["vendor-%d" % (i % 9) for i in range(nr)]]  # several ids share a name
    join = HashJoinExec(_side(gpu_ctx, lschema, ltab, [0, 2000, nl]), _side(gpu_ctx, rschema, rtab, [0, nr]),
                        [(ColumnExpression(0), ColumnExpression(0))], "inner")
    agg = HashAggregateExec(join, [ColumnExpression(3)], [SumExpression(ColumnExpression(1)), CountStarExpression()],
                            Schema([Field("name", N.TYPE_UTF8), Field("sum", N.TYPE_INT64), Field("count", N.TYPE_INT64)]))
    assert fuse(agg) is agg and fuse(join) is join  # a join is left alone: the aggregate over it runs unfused
    out = next(fuse(agg).execute())
    got = {k: (s, c) for k, s, c in zip(*[out.field(j).to_pylist() for j in range(3)])}
    pi, bi = R.join(_words([(k,) for k in rtab[0]]), _words([(k,) for k in ltab[0]]), "inner")
    want: dict = {}
    for i, b in zip(pi, bi):  # the reference aggregate, computed on the joined rows
        s, c = want.get(rtab[1][b], (0, 0))
        want[rtab[1][b]] = (s + ltab[1][i], c + 1)
    assert len(want) == 9 and got == want


# ---- determinism and lifetime ------------------------------------------------------------------------------------------
def test_duplicate_key_join_is_bit_identical_from_run_to_run(gpu_ctx):
    import torch

    rng = np.random.default_rng(1400)
    bv = rng.integers(0, 500, 50_000).astype(np.int64)
    pv = rng.integers(0, 600, 4097).astype(np.int64)
    bvalid, pvalid = rng.random(50_000) >= 0.1, rng.random(4097) >= 0.1

    def run(ctx):
        table = join_build(DeviceColumn.from_numpy(N.TYPE_INT64, bv, bvalid, ctx=ctx))
        try:
            pi, bi = join_probe(table, DeviceColumn.from_numpy(N.TYPE_INT64, pv, pvalid, ctx=ctx), N.JOIN_LEFT)
            ctx.synchronize()
            return pi.to_numpy().tobytes(), bi.to_numpy().tobytes()
        finally:
            table.close()

    runs = [run(gpu_ctx) for _ in range(3)]
    stream = torch.cuda.Stream(device=gpu_ctx.torch_device)
    with torch.cuda.stream(stream):  # a second context with its own stream
        other = Context(0, stream.cuda_stream)
        runs.append(run(other))
        other.synchronize()
    assert all(r == runs[0] for r in runs[1:])
    want = R.join(R.key_words((N.TYPE_INT64, bv, bvalid)), R.key_words((N.TYPE_INT64, pv, pvalid)), "left")
    assert runs[0] == (want[0].tobytes(), want[1].tobytes())


def test_build_probe_destroy_then_build_again(gpu_ctx):
    """Three probe batches against one table, then another table of a different size on the same
    context: the allocator hands the first table's blocks out again."""
    rng = np.random.default_rng(1500)
    for nb, dup in ((2049, False), (65, True), (200_003, False), (1000, True)):
        if dup:
            build = (N.TYPE_INT64, mod7_values(N.TYPE_INT64, nb, rng), _nulls(rng, nb, True))
            probes = [(N.TYPE_INT64, mod7_values(N.TYPE_INT64, m, rng), None) for m in (64, 65, 1)]
        else:
            present, absent = unique_values(N.TYPE_INT64, nb, rng)
            build = (N.TYPE_INT64, present, None)
            probes = [(N.TYPE_INT64, probe_values(present, absent, m, rng), _nulls(rng, m, True)) for m in (4097, 64, 1)]
        check(gpu_ctx, build, probes, unique=not dup)
