"""Chunk turnover in the spilling pass and the chunked radix scatter, at the size where it happens.

The GROUP BY paths past the on-chip table write intermediate records into PART_CH = 2048-record
chunks that open streams claim from a device counter: one open chunk per wave and sub-bucket in the
spilling pass (qe_fused, qe_jit.hip), one per workgroup and bucket in the chunked scatter
(qe_pscatter). A stream whose chunk fills marks it full and claims the next; in the spilling pass a
step's records straddle both. The spilling pass runs 4096 waves on 256 CUs, so at the 400K to 2M rows
of the other spilling tests a wave spills ~65 records and claims once, into an empty stream: the
branch with 0 < room < tot, the "mark the old chunk full" store, sp_fill = tot - room and an
aggregation pass over a list that holds full chunks were reached by no correctness test. Here every
case runs 100M generated rows (nothing is uploaded; oracle/cpu_baseline.c qe_cpu_c4_mod regenerates
and aggregates the same rows on the CPU), so every stream turns over several times, and each case
first proves that from qe_hashagg_last_chunk_stats: full chunks >= 2 x the open ones.

Every group's SUM(a+b) / COUNT(*) / MIN(a) / MAX(b) must equal the C oracle's (pinned to
oracle/semantics.py by tests/test_oracle.py::test_cpu_baseline_chosen_value_ranges)."""
import ctypes as C
import os
import pathlib

import pytest

pytestmark = pytest.mark.gpu

from kquery import native as N  # noqa: E402
from kquery.aggregate import HashAggregateState  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parents[1]
SEED = 42
N_ROWS = 100_000_000


class _G(C.Structure):
    _fields_ = [(f, C.c_int64) for f in ("key", "sum", "count", "min", "max")]


def _oracle(row0, rows, threshold, nkeys, mod):
    """{key: (sum, count, min, max)} of rows [row0, row0 + rows) from qe_cpu_c4_mod."""
    lib = C.CDLL(str(ROOT / "oracle" / "build" / "libqe_oracle.so"))
    lib.qe_cpu_c4_mod.restype = C.c_double
    lib.qe_cpu_c4_mod.argtypes = [C.c_int64, C.c_int64, C.c_uint64, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                  C.c_int64, C.POINTER(_G), C.c_int64, C.POINTER(C.c_int64)]
    cap = nkeys + 16
    out = (_G * cap)()
    ng = C.c_int64()
    threads = min(16, len(os.sched_getaffinity(0)))
    assert lib.qe_cpu_c4_mod(row0, rows, SEED, threads, threshold, nkeys, mod, mod, out, cap, C.byref(ng)) >= 0
    assert ng.value <= cap
    return {int(g.key): (int(g.sum), int(g.count), int(g.min), int(g.max)) for g in out[: ng.value]}


# Rows: 100M, except where the measured statistics missed the turnover condition at 100M and the
# case runs 200M instead: spill-2sb-two-batches (its 60M-row batch: 16,384 chunks, 8,192 full: one
# full chunk per stream) and the two 65,536-group cases (512 workgroups x 64 buckets = 32,768
# streams of ~2.9K records: 65,536 chunks, 32,768 full).
SPILL_ENV = {"QE_LDS_COMPACT": "0", "QE_MP_SPILL": "1"}
COMPACT_1SB = (["multi-pass: 2 buckets (compact kept table)", "32-bit"], ["sub-buckets"])

# id: (expected groups, nkeys, env, value bits, threshold bits, batches (rows each),
#      per batch (note must contain, note must not contain), spilling)
CASES = {
    "spill-1sb": (6500, 6500, {}, 20, 16, [N_ROWS], [COMPACT_1SB], True),
    "spill-1sb-hi": (7500, 7500, {}, 20, 16, [N_ROWS], [COMPACT_1SB], True),
    "spill-2sb": (8192, 8192, {}, 20, 16, [N_ROWS], [(["in 2 sub-buckets"], [])], True),
    "spill-2sb-two-batches": (9500, 9500, {}, 20, 16, [120_000_000, 80_000_000],
                              [(["in 2 sub-buckets"], [])] * 2, True),
    "spill-regular-table": (4000, 4000, SPILL_ENV, 20, 16, [N_ROWS],
                            [(["multi-pass: 2 buckets, bucket 1 spilled"], [])], True),
    "spill-wide-records": (4000, 4000, SPILL_ENV, 40, 36, [1_000_000, N_ROWS - 1_000_000],
                           [(["re-read"], []), (["spilled as", "(column words)"], ["32-bit"])], True),
    "spill-more-groups": (7500, 20000, {}, 20, 16, [N_ROWS], [(["multi-pass: 2 buckets"], [])], True),
    "part-chunked-12k": (12000, 12000, {}, 20, 16, [N_ROWS],
                         [(["radix-partitioned", "chunked records", "32-bit"], [])], False),
    "part-chunked-64k": (65536, 65536, {}, 20, 16, [2 * N_ROWS], [(["chunked records"], [])], False),
    "part-chunked-64k-wide": (65536, 65536, {}, 40, 36, [2 * N_ROWS], [(["chunked records"], ["32-bit"])], False),
}
KNOBS = ("QE_LDS_COMPACT", "QE_MP_SPILL", "QE_PART_CHUNKED")  # unset unless the case sets them


def run_case(ctx, case, batches):
    """The case's batches through update_fused -> ({key: aggregates}, each batch's note, the larger
    batch's (row0, rows), each batch's chunk stats). The case's environment is the caller's to set."""
    from kquery.datasource import ColumnSpec, generate_column
    from kquery.workloads import C4_AGGS, c4_spec

    expected, nkeys, _, bits, thr_bits = CASES[case][:5]
    N.check(N.lib().qe_ctx_set_jit(ctx.handle, 1))  # (the generic kernel has no spilling pass)
    specs = [ColumnSpec("k", N.TYPE_INT64, N.GEN_MOD, nkeys, 0), ColumnSpec("a", N.TYPE_INT64, N.GEN_MOD, 1 << bits, 1),
             ColumnSpec("b", N.TYPE_INT64, N.GEN_MOD, 1 << bits, 2)]
    st = HashAggregateState(ctx, [N.TYPE_INT64], C4_AGGS, expected)
    big = max(range(len(batches)), key=lambda i: batches[i])  # the checked update: the larger batch
    row0, checked, notes, stats = 0, None, [], []
    for i, rows in enumerate(batches):
        cols = [generate_column(s, rows, row0, SEED, ctx) for s in specs]
        st.update_fused(cols, c4_spec(1 << thr_bits))
        notes.append(st.last_kernel_kind()[1])
        stats.append(st.last_chunk_stats())
        if i == big:
            checked = (row0, rows)
        del cols  # (released before the oracle takes its 2.4 GB on the host)
        row0 += rows
    kk, aa = st.finalize()
    kv = kk[0].to_numpy().tolist()
    av = [a.to_numpy().tolist() for a in aa]
    got = {kv[i]: tuple(a[i] for a in av) for i in range(kk[0].length)}
    st.close()
    return got, notes, checked, stats


@pytest.mark.parametrize("case", list(CASES))
def test_chunk_turnover_vs_oracle(gpu_ctx, monkeypatch, case):
    _, nkeys, env, bits, thr_bits, batches, notes_want, spilling = CASES[case]
    for kn in KNOBS:
        monkeypatch.delenv(kn, raising=False)
    for kn, v in env.items():
        monkeypatch.setenv(kn, v)
    got, notes, checked, stats = run_case(gpu_ctx, case, batches)
    print(f"{case}: rows {batches} stats(chunks, full, records) {stats} notes {notes}")
    for (must, must_not), note, bstats in zip(notes_want, notes, stats):
        assert all(m in note for m in must) and not any(m in note for m in must_not), notes
        if "re-read" in note:  # the misfitted records are not the update's: nothing to report
            assert bstats == (0, 0, 0), stats

    mod, thr = 1 << bits, 1 << thr_bits
    want = _oracle(0, sum(batches), thr, nkeys, mod)
    selected = sum(v[1] for v in (want if len(batches) == 1 else _oracle(*checked, thr, nkeys, mod)).values())
    # preconditions: the checked update turned its chunk streams over (on average every open stream
    # filled two chunks and went on), and the chunks hold the records they should
    chunks, full, records = stats[batches.index(checked[1])]
    assert chunks > 0, stats
    assert full >= 2 * (chunks - full), stats
    if spilling:
        assert 0 < records < selected, (stats, selected)
    else:
        assert records == selected, (stats, selected)

    assert len(got) == nkeys and got == want


def test_chunk_stats_zero_without_chunked_records(gpu_ctx, monkeypatch):
    """Updates that write no chunked records report zeros: the LDS table (1024 groups) and the
    counted radix scatter (20,000 groups at 1M rows: the open chunks would outnumber the rows)."""
    from kquery.datasource import ColumnSpec, generate_column
    from kquery.workloads import C4_AGGS, c4_spec

    for kn in KNOBS:
        monkeypatch.delenv(kn, raising=False)
    N.check(N.lib().qe_ctx_set_jit(gpu_ctx.handle, 1))
    for groups, start in ((1024, ""), (20_000, "radix-partitioned")):
        specs = [ColumnSpec("k", N.TYPE_INT64, N.GEN_MOD, groups, 0), ColumnSpec("a", N.TYPE_INT64, N.GEN_MOD, 1 << 20, 1),
                 ColumnSpec("b", N.TYPE_INT64, N.GEN_MOD, 1 << 20, 2)]
        cols = [generate_column(s, 1_000_003, 0, SEED, gpu_ctx) for s in specs]
        st = HashAggregateState(gpu_ctx, [N.TYPE_INT64], C4_AGGS, groups)
        st.update_fused(cols, c4_spec(1 << 16))
        note = st.last_kernel_kind()[1]
        assert note.startswith(start) and "chunked" not in note, note
        assert st.last_chunk_stats() == (0, 0, 0)
        assert st.num_groups() == groups
        st.close()
