"""The equi-join's build-side match marks on the device: QE_JOIN_TRACK, qe_join_mark,
qe_join_build_rows, qe_join_clear_marks and HashJoinExec's right, full_outer, right_semi and right_anti
kinds, against tests/joinref_outer.py. The row lists are ascending and fixed, so every check compares
exact arrays: there is no tolerance anywhere."""
import numpy as np
import pytest

import joinref as R
import joinref_outer as RO
from kquery import native as N
from kquery.columnar import DeviceColumn, Field, RecordBatch, Schema
from kquery.operators import (HashJoinExec, PhysicalPlan, join_build, join_build_rows, join_clear_marks, join_mark,
                              join_probe, join_probe_mask, join_stats)

pytestmark = pytest.mark.gpu

KEY_TYPES = [N.TYPE_INT64, N.TYPE_INT32, N.TYPE_DATE32, N.TYPE_UINT8, N.TYPE_BOOL, N.TYPE_FLOAT64]
BUILD_ROWS = [0, 1, 63, 64, 65, 2047, 2048, 2049, 200_003]  # the row compaction's tile is 2048 rows
PROBE_ROWS = [0, 1, 64, 4097]
COOP_MIN = 32  # QE_JOIN_COOP_MIN's default: from this run length on a wave writes a run together
TRACKED = {"inner": N.JOIN_INNER | N.JOIN_TRACK, "left": N.JOIN_LEFT | N.JOIN_TRACK}


# ---- columns --------------------------------------------------------------------------------------
def dev(ctx, col) -> DeviceColumn:
    t, vals, valid = col
    return DeviceColumn.from_numpy(t, np.asarray(vals), valid, ctx=ctx)


def i64(vals, valid=None):
    return (N.TYPE_INT64, np.asarray(vals, dtype=np.int64), valid)


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
    """m probe values, about half of them build keys, drawn from the first half of the build keys:
    a large probe side hits about half the build keys."""
    present = present[: (len(present) + 1) // 2]
    pool = np.concatenate([present, absent]) if len(absent) else present
    if len(pool) == 0 or m == 0:
        return pool[:0]
    if len(present) == 0 or len(absent) == 0:
        return pool[rng.integers(0, len(pool), m)]
    pick = rng.random(m) < 0.5
    return np.where(pick, present[rng.integers(0, len(present), m)], absent[rng.integers(0, len(absent), m)])


# ---- the device against the reference ------------------------------------------------------------------
def _same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{name}: first difference at {bad} of {len(want)}: got {got[bad]}, want {want[bad]}")


def lists(ctx, table):
    """(matched, unmatched) build rows of the table as it stands."""
    m, u = join_build_rows(table, True), join_build_rows(table, False)
    ctx.synchronize()
    return m.to_numpy(), u.to_numpy()


def check_lists(ctx, table, bw, sides, name=""):
    """The table's two lists against the reference's after tracked probes by `sides` (key words)."""
    got = lists(ctx, table)
    want = RO.both_lists(bw, sides)
    _same(f"{name} matched", got[0], want[0])
    _same(f"{name} unmatched", got[1], want[1])
    both = np.concatenate(got)
    assert len(both) == len(bw) and np.array_equal(np.sort(both), np.arange(len(bw)))  # a partition of [0, n)
    assert all(np.all(g[1:] > g[:-1]) for g in got)  # ascending
    return got


def track(ctx, table, probe, how="inner"):
    """Marks by one probe side: a tracked probe of either kind, or qe_join_mark."""
    dp = dev(ctx, probe)
    if how == "mark":
        join_mark(table, dp)
        return None
    return join_probe(table, dp, TRACKED[how])


# ---- shapes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", BUILD_ROWS)
def test_every_shape_unique_int64_keys(gpu_ctx, nb):
    rng = np.random.default_rng(100 + nb)
    present, absent = unique_values(N.TYPE_INT64, nb, rng)
    build = i64(present)
    bw = R.key_words(build)
    table = join_build(dev(gpu_ctx, build))
    try:
        check_lists(gpu_ctx, table, bw, [], "never tracked")  # every row unmatched, nothing allocated
        for m in PROBE_ROWS + ([nb] if nb > 4097 else []):  # (a large build side: marks in every tile)
            probe = i64(probe_values(present, absent, m, rng))
            join_clear_marks(table)
            track(gpu_ctx, table, probe, "inner" if m != 64 else "mark")
            got = check_lists(gpu_ctx, table, bw, [R.key_words(probe)], f"{m} probe rows")
            if m == 4097 and 63 <= nb <= 2049:  # about half the build keys are hit
                assert 0.3 * nb <= len(got[0]) <= 0.55 * nb
    finally:
        table.close()


# ---- types -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls", [False, True], ids=["nonull", "nulls"])
@pytest.mark.parametrize("t", KEY_TYPES)
def test_every_key_type(gpu_ctx, t, nulls):
    rng = np.random.default_rng(200 + t)
    present, absent = unique_values(t, 2049, rng)
    build = (t, present, _nulls(rng, len(present), nulls))
    probe = (t, probe_values(present, absent, 4097, rng), _nulls(rng, 4097, nulls))
    bw = R.key_words(build)
    table = join_build(dev(gpu_ctx, build))
    try:
        track(gpu_ctx, table, probe)
        matched, unmatched = check_lists(gpu_ctx, table, bw, [R.key_words(probe)])
        assert len(matched) > 0 or t == N.TYPE_BOOL  # (two build rows, either of which may be null)
        null_rows = [i for i, w in enumerate(bw) if w is None]
        assert set(null_rows) <= set(unmatched.tolist())  # a null-key build row is never matched
        if nulls and t not in (N.TYPE_BOOL,):
            assert null_rows
    finally:
        table.close()


# ---- duplicates ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["inner", "left", "mark"])
def test_duplicate_runs_of_one_to_seven_rows(gpu_ctx, how):
    rng = np.random.default_rng(300)
    keys = np.arange(300, dtype=np.int64) * 7919 - 1000
    bv = rng.permutation(np.repeat(keys, 1 + np.arange(300) % 7))  # key k holds 1 + k mod 7 rows
    build = i64(bv, rng.random(len(bv)) >= 0.1)
    probe = i64(np.concatenate([rng.permutation(keys)[:150], np.arange(50) * 7919 - 999]))
    bw = R.key_words(build)
    table = join_build(dev(gpu_ctx, build))
    try:
        assert join_stats(table)[2] == 7
        track(gpu_ctx, table, probe, how)
        check_lists(gpu_ctx, table, bw, [R.key_words(probe)])
    finally:
        table.close()


@pytest.mark.parametrize("how", ["inner", "left", "mark"])
def test_long_runs_hit_by_one_probe_row_each(gpu_ctx, how):
    """Runs at and around the length from which the wave writes a run together, each hit by exactly
    one probe row and by no other: a cooperative path that forgets to mark fails here."""
    rng = np.random.default_rng(310)
    runs = {9001: COOP_MIN - 1, 9002: COOP_MIN, 9003: 64, 9004: 100, 9005: COOP_MIN + 1, 9006: 70}
    bv = rng.permutation(np.concatenate([np.full(c, k, dtype=np.int64) for k, c in runs.items()]
                                        + [np.arange(500, dtype=np.int64)]))
    build = i64(bv)
    bw = R.key_words(build)
    table = join_build(dev(gpu_ctx, build))
    try:
        assert join_stats(table)[2] == 100
        # one probe row per probed run, far apart in the batch; 9005 and 9006 stay unprobed
        pv = rng.integers(100_000, 200_000, 700).astype(np.int64)
        pv[[5, 130, 400, 699]] = [9001, 9002, 9003, 9004]
        probe = i64(pv)
        track(gpu_ctx, table, probe, how)
        matched, unmatched = check_lists(gpu_ctx, table, bw, [R.key_words(probe)])
        assert len(matched) == (COOP_MIN - 1) + COOP_MIN + 64 + 100
        assert set(np.flatnonzero(bv == 9004).tolist()) <= set(matched.tolist())
        assert set(np.flatnonzero(bv == 9006).tolist()) <= set(unmatched.tolist())
    finally:
        table.close()


# ---- the side slot ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dup", [False, True], ids=["unique", "runs"])
@pytest.mark.parametrize("how", ["inner", "mark"])
def test_the_key_minus_one_lives_in_the_side_slot(gpu_ctx, how, dup):
    build = i64([-1, 5, -1, 7, 0] if dup else [5, -1, 7, 0])
    bw = R.key_words(build)
    assert (-1 & R.M64) in bw
    for probe, hit in ((i64([3, -1, 8]), True), (i64([3, 7, 8]), False),
                       ((N.TYPE_INT32, np.array([-1], dtype=np.int32), None), True)):
        table = join_build(dev(gpu_ctx, build))
        try:
            track(gpu_ctx, table, probe, how)
            matched, _ = check_lists(gpu_ctx, table, bw, [R.key_words(probe)])
            minus_one = [i for i, w in enumerate(bw) if w == R.M64]
            assert (set(minus_one) <= set(matched.tolist())) == hit
            assert hit or not set(minus_one) & set(matched.tolist())
        finally:
            table.close()


# ---- forged collisions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [32, 40])
def test_forged_collisions_mark_the_final_slot(gpu_ctx, nkeys):
    """Keys that share one home slot (32 fill half of a 64-slot table; 40 need the 128-slot one): a key's
    mark follows the slot it landed in, not its home slot."""
    rng = np.random.default_rng(400)
    nslots = R.slots(nkeys)
    assert nslots == (64 if nkeys == 32 else 128)
    home = nslots - 3  # the chain wraps the table's end
    keys = np.array([R.signed(w) for w in R.forge_keys(nslots, home, nkeys)], dtype=np.int64)
    absent = np.array([R.signed(w) for w in R.forge_keys(nslots, home, 10, first=nkeys)], dtype=np.int64)
    build = i64(rng.permutation(keys))
    bw = R.key_words(build)
    for how in ("inner", "mark"):
        table = join_build(dev(gpu_ctx, build))
        try:
            assert join_stats(table) == (nkeys, nkeys, 1, nslots)
            probe = i64(np.concatenate([keys[::2], absent]))  # every other key, and keys that are not there
            track(gpu_ctx, table, probe, how)
            matched, _ = check_lists(gpu_ctx, table, bw, [R.key_words(probe)])
            assert sorted(build[1][matched].tolist()) == sorted(keys[::2].tolist())  # exactly the probed keys
        finally:
            table.close()


# ---- accumulation ---------------------------------------------------------------------------------------------------
def test_marks_accumulate_and_are_idempotent(gpu_ctx):
    rng = np.random.default_rng(500)
    present, absent = unique_values(N.TYPE_INT64, 3000, rng)
    bv = np.concatenate([present, present[:500]])  # some keys twice
    build = i64(bv, rng.random(len(bv)) >= 0.05)
    bw = R.key_words(build)
    thirds = [i64(np.concatenate([present[a::3][:700], absent[:20]])) for a in range(3)]
    table = join_build(dev(gpu_ctx, build))
    try:
        sides = []
        for k, (probe, how) in enumerate(zip(thirds, ("inner", "mark", "left"))):
            track(gpu_ctx, table, probe, how)
            sides.append(R.key_words(probe))
            after = check_lists(gpu_ctx, table, bw, sides, f"batch {k}")
            track(gpu_ctx, table, probe, how)  # the same batch again changes nothing
            again = lists(gpu_ctx, table)
            assert all(np.array_equal(a, b) for a, b in zip(after, again))
        assert len(after[0]) > 2000
    finally:
        table.close()


# ---- the three ways to mark ---------------------------------------------------------------------------------------------
def test_mark_and_both_tracked_kinds_agree_and_pairs_are_unchanged(gpu_ctx):
    rng = np.random.default_rng(600)
    bv = rng.integers(0, 700, 2049).astype(np.int64)
    bv[:40] = 5000  # one run the wave writes together
    build = i64(bv, rng.random(2049) >= 0.1)
    probe = i64(np.concatenate([rng.integers(0, 1400, 995), [5000, 5000]]), rng.random(997) >= 0.1)
    bw, pw = R.key_words(build), R.key_words(probe)
    want = R.join_all(bw, pw)
    results = {}
    for how in ("inner", "left", "mark"):
        table = join_build(dev(gpu_ctx, build))
        try:
            if how != "mark":
                plain = join_probe(table, dev(gpu_ctx, probe), TRACKED[how] & ~N.JOIN_TRACK)
                gpu_ctx.synchronize()
                check_lists(gpu_ctx, table, bw, [], "untracked")
            tracked = track(gpu_ctx, table, probe, how)
            gpu_ctx.synchronize()
            if how != "mark":  # the tracked kind's pairs are the untracked kind's, bit for bit
                for name, a, b, w in zip(("probe rows", "build rows"), tracked, plain, want[how]):
                    _same(f"{how} {name}", a.to_numpy(), w)
                    assert a.to_numpy().tobytes() == b.to_numpy().tobytes()
            results[how] = check_lists(gpu_ctx, table, bw, [pw], how)
        finally:
            table.close()
    for how in ("left", "mark"):
        assert all(np.array_equal(a, b) for a, b in zip(results["inner"], results[how]))


# ---- what does not mark ------------------------------------------------------------------------------------------------------
def test_untracked_calls_leave_the_marks_and_clear_resets_them(gpu_ctx):
    rng = np.random.default_rng(700)
    present, absent = unique_values(N.TYPE_INT64, 2049, rng)
    build = i64(present)
    bw = R.key_words(build)
    first, other, third = (i64(present[a:a + 300]) for a in (0, 1000, 1700))
    table = join_build(dev(gpu_ctx, build))
    try:
        track(gpu_ctx, table, first)
        before = check_lists(gpu_ctx, table, bw, [R.key_words(first)])
        for kind in (N.JOIN_INNER, N.JOIN_LEFT):
            join_probe(table, dev(gpu_ctx, other), kind)
        for anti in (False, True):
            join_probe_mask(table, dev(gpu_ctx, other), anti=anti)
        after = lists(gpu_ctx, table)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        track(gpu_ctx, table, third, "left")
        check_lists(gpu_ctx, table, bw, [R.key_words(first), R.key_words(third)])
        join_clear_marks(table)
        matched, unmatched = check_lists(gpu_ctx, table, bw, [])
        assert len(matched) == 0 and np.array_equal(unmatched, np.arange(2049, dtype=np.int32))
        track(gpu_ctx, table, other, "mark")  # the cleared table serves another probe side
        check_lists(gpu_ctx, table, bw, [R.key_words(other)])
    finally:
        table.close()
    table = join_build(dev(gpu_ctx, build))  # clearing a table that was never tracked is no error
    try:
        join_clear_marks(table)
        check_lists(gpu_ctx, table, bw, [])
    finally:
        table.close()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def _probe_raw(ctx, table, dp, kind, cap):
    pi = DeviceColumn.empty(N.TYPE_INT32, max(cap, 1), False, ctx=ctx)
    bi = DeviceColumn.empty(N.TYPE_INT32, max(cap, 1), False, ctx=ctx)
    pi.length = bi.length = cap
    kc, pc, bc = dp.as_c(), pi.as_c(), bi.as_c()
    pairs = N.C.c_int64(-1)
    st = N.lib().qe_join_probe(table.handle, N.C.byref(kc), kind, N.C.byref(pc), N.C.byref(bc), N.C.byref(pairs))
    ctx.synchronize()
    return st, pairs.value


def test_a_failed_call_leaves_the_marks_alone(gpu_ctx):
    import torch

    rng = np.random.default_rng(800)
    bv = rng.integers(0, 7, 500).astype(np.int64)
    build = i64(bv)
    first, second = i64([0, 1]), i64(np.concatenate([rng.integers(3, 7, 100), [99]]))  # key 2 stays unmatched
    bw = R.key_words(build)
    exact = len(R.join_all(bw, R.key_words(second))["inner"][0])
    assert exact > 100
    for early in (False, True):  # a table whose marks exist already, and one the failing call would be the first to mark
        table = join_build(dev(gpu_ctx, build))
        try:
            sides = []
            if early:
                track(gpu_ctx, table, first)
                sides.append(R.key_words(first))
            before = check_lists(gpu_ctx, table, bw, sides)
            dp = dev(gpu_ctx, second)
            for kind, need in ((TRACKED["inner"], exact), (TRACKED["left"], exact + 1)):
                st, pairs = _probe_raw(gpu_ctx, table, dp, kind, need - 1)
                assert st == N.QE_ERR_CAPACITY and pairs == need
            for kind in (2, N.JOIN_TRACK | 2, 0x200, N.JOIN_TRACK | 0x200, -1):
                st, _ = _probe_raw(gpu_ctx, table, dp, kind, exact + 1)
                assert st == N.QE_ERR_INVALID_ARG, kind
            after = lists(gpu_ctx, table)
            assert all(np.array_equal(a, b) for a, b in zip(before, after))
            st, pairs = _probe_raw(gpu_ctx, table, dp, TRACKED["inner"], exact)  # the exact capacity succeeds, and marks
            assert st == N.QE_OK and pairs == exact
            matched, _ = check_lists(gpu_ctx, table, bw, sides + [R.key_words(second)])

            # qe_join_build_rows: one row short is refused with the exact count and nothing written
            for want_matched, rows in ((1, len(matched)), (0, 500 - len(matched))):
                assert rows > 1
                idx = DeviceColumn.empty(N.TYPE_INT32, 500, False, ctx=gpu_ctx)
                idx.values.fill_(0x5A5A5A5A)
                idx.length = rows - 1
                ic = idx.as_c()
                got = N.C.c_int64(-1)
                st = N.lib().qe_join_build_rows(table.handle, want_matched, N.C.byref(ic), N.C.byref(got))
                gpu_ctx.synchronize()
                assert st == N.QE_ERR_CAPACITY and got.value == rows
                assert bool(torch.all(idx.values == 0x5A5A5A5A))
                idx.length = rows  # the exact capacity succeeds
                ic = idx.as_c()
                st = N.lib().qe_join_build_rows(table.handle, want_matched, N.C.byref(ic), N.C.byref(got))
                gpu_ctx.synchronize()
                assert st == N.QE_OK and got.value == rows and ic.length == rows
                assert bool(torch.all(idx.values[rows:] == 0x5A5A5A5A))
        finally:
            table.close()


def test_type_pairs_that_do_not_join_are_refused_by_mark(gpu_ctx):
    ints = DeviceColumn.from_numpy(N.TYPE_INT64, np.arange(4), ctx=gpu_ctx)
    flts = DeviceColumn.from_numpy(N.TYPE_FLOAT64, np.arange(4) * 1.0, ctx=gpu_ctx)
    table = join_build(ints)
    try:
        with pytest.raises(N.IllegalArgumentException):
            join_mark(table, flts)
        with pytest.raises(N.IllegalArgumentException):
            join_probe(table, flts, TRACKED["inner"])
        join_mark(table, DeviceColumn.from_numpy(N.TYPE_INT64, np.zeros(0, dtype=np.int64), ctx=gpu_ctx))  # 0 rows: a no-op
        check_lists(gpu_ctx, table, R.key_words(i64(np.arange(4))), [])
    finally:
        table.close()


# ---- skew -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["inner", "mark"])
def test_a_hundred_thousand_probe_rows_on_one_key(gpu_ctx, how):
    rng = np.random.default_rng(900)
    present, _ = unique_values(N.TYPE_INT64, 2049, rng)
    build = i64(present)
    table = join_build(dev(gpu_ctx, build))
    try:
        track(gpu_ctx, table, i64(np.full(100_000, present[1234])), how)
        matched, unmatched = lists(gpu_ctx, table)
        assert matched.tolist() == [1234] and len(unmatched) == 2048 and 1234 not in unmatched
    finally:
        table.close()


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
def test_the_lists_are_bit_identical_from_run_to_run(gpu_ctx):
    rng = np.random.default_rng(1000)
    bv = rng.integers(0, 20_000, 50_000).astype(np.int64)
    bvalid = rng.random(50_000) >= 0.1
    probes = [i64(rng.integers(0, 40_000, m), rng.random(m) >= 0.1) for m in (4097, 1000, 64)]

    def run():
        out = []
        table = join_build(dev(gpu_ctx, i64(bv, bvalid)))
        try:
            for probe, how in zip(probes, ("inner", "mark", "left")):
                pairs = track(gpu_ctx, table, probe, how)
                m, u = lists(gpu_ctx, table)
                out += [m.tobytes(), u.tobytes()] + ([p.to_numpy().tobytes() for p in pairs] if pairs else [])
        finally:
            table.close()
        return out

    first, second = run(), run()
    assert first == second
    want = RO.both_lists(R.key_words(i64(bv, bvalid)), [R.key_words(p) for p in probes])
    assert first[-4] == want[0].tobytes() and first[-3] == want[1].tobytes()


# ---- HashJoinExec --------------------------------------------------------------------------------------------------------------------------------
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


def _keys(table, cols):
    """Per row the join key (a tuple), None when any member is null."""
    return [None if any(v is None for v in k) else k for k in zip(*[table[j] for j in cols])]


def _rows(batch):
    cols = [batch.field(j).to_pylist() for j in range(len(batch.fields))]
    return [tuple(r) for r in zip(*cols)]


def check_exec(ctx, lschema, ltab, lcuts, rschema, rtab, rcuts, on, lkeys, rkeys):
    """HashJoinExec of every build-side kind against the row-level reference, batch by batch; and the
    inner kind, which the new code must leave as it was."""
    from kquery.expressions import ColumnExpression

    nl, nr = len(lschema.fields), len(rschema.fields)
    lrows, rrows = list(zip(*ltab)) if ltab[0] else [], list(zip(*rtab)) if rtab[0] else []
    lk, rk = _keys(ltab, lkeys), _keys(rtab, rkeys)
    exprs = [(ColumnExpression(a), ColumnExpression(b)) for a, b in on]
    for kind in HashJoinExec.BUILD_SIDE_KINDS:
        plan = HashJoinExec(_side(ctx, lschema, ltab, lcuts), _side(ctx, rschema, rtab, rcuts), exprs, kind)
        width = nr if kind in ("right_semi", "right_anti") else nl + nr
        names = [f.name for f in plan.schema().fields]
        assert names == [f.name for f in (rschema.fields if width == nr else list(lschema.fields) + list(rschema.fields))]
        outs = list(plan.execute())
        want = RO.join_rows(kind, lrows, lk, rrows, rk, lcuts, nl, nr)
        # the batch count depends on the left batch count alone
        assert len(outs) == len(want) == (1 if width == nr else len(lcuts))
        for b, (out, w) in enumerate(zip(outs, want)):
            assert len(out.fields) == width and out.rowCount() == len(w), (kind, b)
            assert _rows(out) == w, (kind, b)
            if w and b == len(want) - 1 and width != nr:  # the final batch's left columns are all null
                assert all(out.field(j).to_pylist() == [None] * len(w) for j in range(nl))
                for j, f in enumerate(lschema.fields):
                    assert out.field(j).type == f.dataType
    plan = HashJoinExec(_side(ctx, lschema, ltab, lcuts), _side(ctx, rschema, rtab, rcuts), exprs, "inner")
    outs = list(plan.execute())
    assert len(outs) == len(lcuts) - 1
    for out, a, b in zip(outs, lcuts[:-1], lcuts[1:]):
        pi, bi = R.join(rk, lk[a:b], "inner")
        assert _rows(out) == [tuple(lrows[a + i]) + tuple(rrows[r]) for i, r in zip(pi, bi)]


def _int64_tables(rng, nl, nr):
    ltab = [[None if rng.random() < 0.1 else int(v) for v in rng.integers(0, 150, nl)],
            [None if i % 11 == 0 else "left-%d-%s" % (i, "ü" * (i % 5)) for i in range(nl)],
            [None if i % 4 == 0 else float(i) for i in range(nl)]]
    rtab = [[None if rng.random() < 0.1 else int(v) for v in rng.integers(50, 250, nr)],
            [None if i % 7 == 0 else "right-payload-%d" % i for i in range(nr)],
            [None if i % 5 == 0 else i * 3 for i in range(nr)]]
    return ltab, rtab


LS = Schema([Field("k", N.TYPE_INT64), Field("lp", N.TYPE_UTF8), Field("lv", N.TYPE_FLOAT64)])
RS = Schema([Field("rk", N.TYPE_INT64), Field("rp", N.TYPE_UTF8), Field("rv", N.TYPE_INT64)])


def test_exec_int64_key_three_left_batches_one_of_them_empty(gpu_ctx):
    ltab, rtab = _int64_tables(np.random.default_rng(1100), 700, 300)
    check_exec(gpu_ctx, LS, ltab, [0, 450, 450, 700], RS, rtab, [0, 100, 300], [(0, 0)], [0], [0])


def test_exec_left_side_of_no_batch_and_of_no_rows(gpu_ctx):
    _, rtab = _int64_tables(np.random.default_rng(1150), 1, 90)
    empty = [[], [], []]
    check_exec(gpu_ctx, LS, empty, [0], RS, rtab, [0, 90], [(0, 0)], [0], [0])  # no batch at all
    check_exec(gpu_ctx, LS, empty, [0, 0], RS, rtab, [0, 90], [(0, 0)], [0], [0])  # one batch of no rows


def test_exec_empty_right_side(gpu_ctx):
    ltab, _ = _int64_tables(np.random.default_rng(1180), 40, 1)
    for rcuts in ([0], [0, 0]):  # no build batch at all, and one batch of no rows
        check_exec(gpu_ctx, LS, ltab, [0, 15, 40], RS, [[], [], []], rcuts, [(0, 0)], [0], [0])


def test_exec_lone_utf8_key(gpu_ctx):
    rng = np.random.default_rng(1200)
    vocab = ["", "a", "abcdefg", "abcdefgh", "abcdefgX", "abcdefghi", "é" * 3 + "x", "é" * 4, "only-left", "only-right-long-value",
             "right-too"]
    lschema = Schema([Field("name", N.TYPE_UTF8), Field("x", N.TYPE_INT64)])
    rschema = Schema([Field("name", N.TYPE_UTF8), Field("y", N.TYPE_INT32), Field("s", N.TYPE_UTF8)])
    lv = [v for v in vocab if not v.startswith(("only-right", "right-too"))]
    rv = [v for v in vocab if v != "only-left"]
    ltab = [[None if rng.random() < 0.1 else lv[int(i)] for i in rng.integers(0, len(lv), 300)],
            [None if i % 9 == 0 else i for i in range(300)]]
    rtab = [[None if rng.random() < 0.1 else rv[int(i)] for i in rng.integers(0, len(rv), 60)], list(range(60)),
            [None if i % 6 == 0 else "s%d" % i for i in range(60)]]
    check_exec(gpu_ctx, lschema, ltab, [0, 130, 130, 300], rschema, rtab, [0, 60], [(0, 0)], [0], [0])
    # only the first few left rows: some right keys stay unmatched whatever the draw
    check_exec(gpu_ctx, lschema, [c[:5] for c in ltab], [0, 2, 5], rschema, rtab, [0, 25, 60], [(0, 0)], [0], [0])


def test_exec_composite_int32_utf8_key(gpu_ctx):
    rng = np.random.default_rng(1300)
    lschema = Schema([Field("a", N.TYPE_INT32), Field("s", N.TYPE_UTF8), Field("x", N.TYPE_FLOAT64)])
    rschema = Schema([Field("s", N.TYPE_UTF8), Field("a", N.TYPE_INT32), Field("p", N.TYPE_UTF8)])
    names = ["ab", "abcdefgh-long", "", "zz", "only-one-side"]

    def rows(n, k):
        return ([None if rng.random() < 0.15 else int(v) for v in rng.integers(0, 5, n)],
                [None if rng.random() < 0.15 else names[int(v)] for v in rng.integers(0, k, n)])

    la, ls = rows(400, 4)
    ra, rs = rows(80, 5)
    la[:2], ls[:2], ra[:2], rs[:2] = [None, 1], [None, None], [None, 1], [None, None]  # null members pair with nothing
    ltab = [la, ls, [None if i % 3 == 0 else float(i) for i in range(400)]]
    rtab = [rs, ra, [None if i % 4 == 0 else "p-%d" % i for i in range(80)]]
    check_exec(gpu_ctx, lschema, ltab, [0, 77, 77, 400], rschema, rtab, [0, 80], [(0, 1), (1, 0)], [0, 1], [1, 0])


def test_exec_kind_names(gpu_ctx):
    from kquery.expressions import ColumnExpression

    ltab, rtab = _int64_tables(np.random.default_rng(1400), 5, 5)
    sides = _side(gpu_ctx, LS, ltab, [0, 5]), _side(gpu_ctx, RS, rtab, [0, 5])
    on = [(ColumnExpression(0), ColumnExpression(0))]
    assert HashJoinExec.KINDS == ("inner", "left", "semi", "anti")  # the probe-side kinds are as they were
    assert HashJoinExec.BUILD_SIDE_KINDS == ("right", "full_outer", "right_semi", "right_anti")
    for kind in ("outer", "right_outer", "cross", ""):
        with pytest.raises(N.IllegalArgumentException):
            HashJoinExec(*sides, on, kind)
