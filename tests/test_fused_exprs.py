"""The predicate terms and aggregate programs of qe_hashagg_update_fused, through the C ABI, held to
the oracle-based reference of tests/fusedcases.py row by row: every plan of its enumeration runs
with the plan-specialised kernel and with the generic one, and the result is compared with
S.rows_equal(..., 0.0) value by value. There is no tolerance anywhere.

An observer plan groups by the row index, so each row's term outcome (the group exists or not) and
each program's value and validity (MIN and COUNT of a one-row group) come back as they were computed.
The expected groups of a state alone choose where the programs are evaluated: the regular LDS table
(whose overflow takes the global-table branch in the same launch), a 256-slot table that leaves most
rows to that branch, the two-bucket passes (spilled records or two passes) and the radix-partitioned
passes (records of values or of column words, chunked or counted). In jit mode the path is asserted
from the kernel note.

Refusals are plans the host compiler rejects before any launch (include/qe_hip.h lists the statuses).

Eight value-only slips were applied, one at a time, to a scratch copy of the library, and this file
(1,409 tests, all passing on the unmodified library) run against each. Tests that failed:
  1 binop4 drops yok from the validity: 65, generic only (21 same-type pair plans, 19 size cases, col op
    null literal 3, turnover 1, shared 4, grouped 4, value_records 1; on the 256-slot table 4; multi-pass 8)
  2 eval_fast ignores rhs_null: 10, generic only (col op null literal 3, turnover 1, and
    lit-i64-col_op_null_i64 on the 256-slot table 1, multi-pass 2, partitioned settings 3)
  3 T_I2F1 converts s0 in eval_program: 57, generic only (the 7 (int, f64) pair plans, 17 literal plans
    with an integer left side and an fp64 right side, deep 3, grouped 2, size 22, pair-i32-f64-nn on the
    further paths 6)
  4 agg_expr's T_DIV_I omits (b != 0) from ok: 78, jit only (all 25 integer pair plans, literal 12,
    size 19, grouped 3, value_records 1, 256-slot table 3, multi-pass 6, partitioned 9)
  5 compile_inputs skips the int -> fp64 promotion of a term's literal: 44, the same 22 in both kernels
    (an fp64 column against 7, -1, INT64_MIN under every op and INT64_MAX under the ordering ops)
  6 emit_col_loads zero-extends INT32: 168, jit only (column terms 40, literal terms 26, pair 22, literal
    programs 20, size 40, deep 3, convert 2, grouped 2, the 8-term plan 1, and the 8-term plan and
    pair-i32-f64-nn on the further paths 12)
  7 the glob branch evaluates a.col without its validity: 62, generic only (pair 21, col op lit 16,
    size 6, turnover 1, convert 1, value_records 1, 256-slot table 3, multi-pass 4, partitioned settings 9)
  8 the share test in compile_plan ignores the literal's value: 2, jit only (shared-lits-f64, shared-lits-i64).
    Dropping rhs_lit alone from that test changes nothing and fails nothing: the token comparison
    beside it covers the same literal, so the slip was applied to both.
Measured on an MI355X: the file 74 s with an empty QE_JIT_CACHE, 13 s warm; the slowest test 1.1 s
(test_partitioned[jit-chunked-pair-i64-i64-nn], three kernel compiles).
"""
import functools

import pytest

import exprcases as E
import fusedcases as F
import selprojcases as P
from oracle import semantics as S

pytestmark = pytest.mark.gpu

from kquery import native as N  # noqa: E402
from kquery.aggregate import HashAggregateState  # noqa: E402
from kquery.columnar import DeviceColumn  # noqa: E402

TYPES = {"i64": N.TYPE_INT64, "f64": N.TYPE_FLOAT64, "i32": N.TYPE_INT32, "u8": N.TYPE_UINT8, "date32": N.TYPE_DATE32,
         "bool": N.TYPE_BOOL}
# Expected groups that take an observer plan's 2,055 groups off the regular path. Two key-hash buckets:
# the first point of the grid 256, 512, 768, 1,024, 1,536, 2,048, 3,072, 4,096, 6,144, 8,192 at which the
# plan's note starts with "multi-pass: 2 buckets" under QE_LDS_COMPACT=0 (as test_hashagg_multipass
# sets it); the window is narrow: one grid point later every plan is radix-partitioned. Partitioned:
# the expected groups of test_partitioned_tiny_batches.
EG_MULTIPASS = {"pair-i64-i64-nn": 1024, "pair-i32-f64-nn": 512, "pair-u8-i64-nn": 1024, "eight_terms": 8192,
                "lit-i64-col_op_null_i64": 1024, "lit-i64-nan_f64_op_col": 512, "value_records": 4096}
EG_PARTITIONED = 100_000


@pytest.fixture(params=["jit", "generic"])
def fused_ctx(request, gpu_ctx):
    """Every case runs through both kernels: the hipRTC plan-specialised one and the generic
    interpreting one."""
    N.check(N.lib().qe_ctx_set_jit(gpu_ctx.handle, 1 if request.param == "jit" else 0))
    gpu_ctx.kernel_mode = request.param
    yield gpu_ctx
    N.check(N.lib().qe_ctx_set_jit(gpu_ctx.handle, 1))


def _scalar(lit):
    if lit is None:
        return N.QeScalar()
    return N.scalar(lit.value, N.TYPE_FLOAT64 if lit.is_f64 else N.TYPE_INT64)


def c_spec(case):
    """qe_fused_spec of a case; the key columns take the slots after the case's columns."""
    s = N.QeFusedSpec()
    s.mask_col = case.spec.mask_col
    s.nterms = len(case.spec.terms)
    for i, (col, op, rhs, lit) in enumerate(case.spec.terms):
        s.terms[i] = N.QePredTerm(col, op, rhs, 0, _scalar(lit))
    for k in range(len(case.keys)):
        s.key_cols[k] = len(case.cols) + k
    for j, prog in enumerate(case.spec.outputs):
        s.inputs[j].ntokens = len(prog)
        for i, (op, arg, lit) in enumerate(prog):
            s.inputs[j].tokens[i] = N.QeToken(op, arg, _scalar(lit))
    return s


def upload(ctx, case):
    return [DeviceColumn.from_numpy(TYPES[c.kind], c.values, c.valid, ctx=ctx) for c in case.cols + case.keys]


def new_state(ctx, case, expected_groups=None):
    return HashAggregateState(ctx, [TYPES[k.kind] for k in case.keys], [(fn, TYPES[kind]) for fn, kind in case.aggs],
                              case.expected_groups if expected_groups is None else expected_groups)


def result_of(st):
    keys, aggs = st.finalize()
    kv = [k.to_pylist() for k in keys]
    av = [a.to_pylist() for a in aggs]
    return {tuple(k[i] for k in kv): [a[i] for a in av] for i in range(keys[0].length)}


def run(ctx, case, expected_groups=None):
    """-> (result, (specialized, note), kernel signature) of one fused update on a fresh state."""
    st = new_state(ctx, case, expected_groups)
    st.update_fused(upload(ctx, case), c_spec(case))
    kind, sig = st.last_kernel_kind(), st.last_kernel_signature()
    return result_of(st), kind, sig


def assert_regular(ctx, kind):
    """The specialised kernel over the state's regular LDS table, or the generic kernel with an LDS
    table (not its global-only launch)."""
    spec, note = kind
    if ctx.kernel_mode == "jit":
        assert spec and note == "", kind
    else:
        assert not spec and note.startswith("jit disabled") and "generic kernel: 0 KiB" not in note, kind


def check_case(ctx, case_id):
    case = F.built(case_id)
    got, kind, _ = run(ctx, case)
    if len(case.keys[0].values):
        assert_regular(ctx, kind)
    else:
        assert kind == (False, "")  # no rows: nothing is launched
    assert F.results_differ(got, F.reference(case_id)) is None
    return got


# ---- programs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", F.case_ids("pair-"))
def test_pair_programs(fused_ctx, case_id):
    """MIN and COUNT of a + b, a - b, a * b, a / b for every ordered pair of operand kinds (and the
    four nullability combinations of five of them): same-type `col op col`, the mixed pairs whose
    promotion makes four tokens, 8-byte-only and narrow loads."""
    check_case(fused_ctx, case_id)


@pytest.mark.parametrize("case_id", F.case_ids("lit-"))
def test_literal_programs(fused_ctx, case_id):
    """`col op lit` and `lit op col` for every literal of exprcases.LITERALS: int against fp64, the
    int64 extremes, NaN, -0.0, +-Inf, and a null literal of each type (every value null, the result
    type that of a valid literal, the group still present)."""
    got = check_case(fused_ctx, case_id)
    case = F.built(case_id)
    if case.info["lit"].value is None:
        assert len(got) == F.N_ROWS and all(v == [None] * 4 + [0] * 4 for v in got.values())


@pytest.mark.parametrize("case_id", F.case_ids("deep-") + F.case_ids("convert-") + F.case_ids("shared-") +
                         F.case_ids("grouped-") + ["value_records"])
def test_deep_converted_and_shared_programs(fused_ctx, case_id):
    """Stack depth 2 and 4 and exactly QE_MAX_TOKENS typed tokens; MIN / AVG declared FLOAT64 over
    integer columns; SUM / AVG that may share an accumulator only when column, literal value and
    literal nullness all agree; the grouped forms of four pair plans."""
    check_case(fused_ctx, case_id)


@pytest.mark.parametrize("plan", ["program", "term"])
def test_literal_turnover(fused_ctx, plan):
    """One plan shape under the literal 7, then INT64_MIN, then the null literal, each on a fresh
    state and each against its own reference: the first two share a compiled kernel by design
    (literal values are runtime arguments), the third must not be served it (nullness is compiled in)."""
    sigs = []
    for lit in F.TURNOVER_LITS:
        case_id = f"turnover-{plan}-{F.lit_id(lit)}"
        got, kind, sig = run(fused_ctx, F.built(case_id))
        assert_regular(fused_ctx, kind)
        assert F.results_differ(got, F.reference(case_id)) is None, case_id
        sigs.append(sig)
    if fused_ctx.kernel_mode == "jit":
        assert sigs[0] == sigs[1] != sigs[2], sigs


# ---- predicate terms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", F.case_ids("cmp-") + F.case_ids("mixed-"))
def test_column_terms(fused_ctx, case_id):
    """`col CMP col`: every op for the same-kind pairs and four mixed ones, LT and GE for the other
    sixteen; full-range int64, and int64 against fp64 beyond 2^53 (compared as fp64)."""
    check_case(fused_ctx, case_id)


@pytest.mark.parametrize("case_id", F.case_ids("cmplit-"))
def test_literal_terms(fused_ctx, case_id):
    """`col CMP lit` for every literal: an int64 literal against an fp64 column (promoted on the
    host), an fp64 literal against integer columns, the int64 extremes against narrow columns, NaN,
    and null literals, which select nothing."""
    got = check_case(fused_ctx, case_id)
    if F.built(case_id).info["lit"].value is None:
        assert got == {}


def test_eight_terms_and_mask(fused_ctx):
    """QE_MAX_TERMS terms over all five kinds under a nullable BOOL mask whose null rows carry bit 1."""
    check_case(fused_ctx, "eight_terms")


# ---- sizes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", F.case_ids("size-"))
def test_sizes(fused_ctx, case_id):
    """One program plan and one term plan around a lane's row pairs (127..129), the wave step
    (255..257) and a 1,024-thread workgroup's step (4,095..4,097); no rows leave no group."""
    case = F.built(case_id)
    got = check_case(fused_ctx, case_id)
    if len(case.keys[0].values) == 0:
        assert got == {}


# ---- where the programs are evaluated ---------------------------------------------------------------
def test_reduced_set():
    assert set(EG_MULTIPASS) == set(F.REDUCED)


@pytest.mark.parametrize("case_id", F.REDUCED)
def test_global_table_rows(fused_ctx, case_id):
    """Expected groups 16: a 256-slot LDS table, so most of the 2,055 one-row groups live only in
    the global table and their rows take the per-row branch (eval_fast / eval_program per row)."""
    ref = F.reference(case_id)
    assert len(ref) - 256 >= len(ref) / 2
    got, kind, _ = run(fused_ctx, F.built(case_id), F.EG_GLOBAL)
    assert_regular(fused_ctx, kind)
    assert F.results_differ(got, ref) is None


@pytest.fixture(params=["spill", "twopass"])
def mp_mode(request, monkeypatch):
    """Both two-bucket updates: a fused pass that spills the second bucket's rows as records for a
    record-aggregation pass, and two fused passes (QE_MP_SPILL=0)."""
    monkeypatch.setenv("QE_MP_SPILL", "1" if request.param == "spill" else "0")
    monkeypatch.setenv("QE_LDS_COMPACT", "0")
    return request.param


@pytest.mark.parametrize("case_id", F.REDUCED)
def test_multipass(fused_ctx, mp_mode, case_id):
    got, (spec, note), _ = run(fused_ctx, F.built(case_id), EG_MULTIPASS[case_id])
    if fused_ctx.kernel_mode == "jit":
        assert spec and note.startswith("multi-pass: 2 bucket"), note
        assert ("spilled" in note) == (mp_mode == "spill"), note
    else:
        assert not spec
    assert F.results_differ(got, F.reference(case_id)) is None


@pytest.fixture(params=["auto", "chunked", "counted"])
def part_mode(request, monkeypatch):
    """Both record placements of the partitioned update (QE_PART_CHUNKED unset, 1 and 0)."""
    monkeypatch.delenv("QE_PART_CHUNKED", raising=False)
    if request.param != "auto":
        monkeypatch.setenv("QE_PART_CHUNKED", "1" if request.param == "chunked" else "0")
    return request.param


@pytest.mark.parametrize("case_id", F.REDUCED)
def test_partitioned(fused_ctx, part_mode, case_id):
    """The scatter pass evaluates the programs of a plan whose records hold values; a plan whose
    records hold column words has them evaluated again by the aggregation pass."""
    got, (spec, note), _ = run(fused_ctx, F.built(case_id), EG_PARTITIONED)
    if fused_ctx.kernel_mode == "jit":
        assert spec and note.startswith("radix-partitioned"), note
        if case_id == F.COLUMN_RECORDS:
            assert "(column words" in note, note
        if case_id == F.VALUE_RECORDS:
            assert "(value words" in note, note
    else:
        assert not spec
    assert F.results_differ(got, F.reference(case_id)) is None


# ---- refusals -----------------------------------------------------------------------------------------
def _refusal_base():
    """Slots 0 a INT64?, 1 b FLOAT64, 2 c INT32, 3 the observer key; 5 rows."""
    rng = E.rng_for("refusal")
    cols = [F.xcol("i64", E.column("i64", 5, rng), [True, True, False, True, True]), F.xcol("f64", E.column("f64", 5, rng)),
            F.xcol("i32", E.column("i32", 5, rng))]
    return cols


c = P._col
_ADD = (P.TOK_ADD, 0, None)
_TOO_LONG = functools.reduce(lambda prog, k: P._bin(P.TOK_ADD, prog, c(0)), range(5), P._bin(P.TOK_ADD, c(0), c(1)))
assert len(_TOO_LONG) == 13
REFUSALS = {  # name: (program of the one aggregate, its declared kind, terms, mask_col, nterms or None, status)
    "stack_depth_5": (c(0) * 5 + [_ADD] * 4, "i64", [], -1, None, N.QE_ERR_UNSUPPORTED),
    "stack_underflow": (c(0) + [_ADD], "i64", [], -1, None, N.QE_ERR_INVALID_ARG),
    "leaves_two_values": (c(0) + c(0), "i64", [], -1, None, N.QE_ERR_INVALID_ARG),
    "column_slot_past_the_end": (c(4), "i64", [], -1, None, N.QE_ERR_INVALID_ARG),
    "column_slot_negative": (c(-1), "i64", [], -1, None, N.QE_ERR_INVALID_ARG),
    "bad_token_op": (c(0) + c(0) + [(99, 0, None)], "i64", [], -1, None, N.QE_ERR_INVALID_ARG),
    "empty_program": ([], "i64", [], -1, None, N.QE_ERR_INVALID_ARG),
    "fp64_program_int64_aggregate": (P._bin(P.TOK_ADD, c(0), c(1)), "i64", [], -1, None, N.QE_ERR_INVALID_ARG),
    "too_long_after_promotion": (_TOO_LONG, "f64", [], -1, None, N.QE_ERR_UNSUPPORTED),
    "mask_not_bool": (c(0), "i64", [], 2, None, N.QE_ERR_INVALID_ARG),
    "mask_past_the_end": (c(0), "i64", [], 4, None, N.QE_ERR_INVALID_ARG),
    "nine_terms": (c(0), "i64", [], -1, 9, N.QE_ERR_UNSUPPORTED),
    "bad_comparison_op": (c(0), "i64", [(0, S.OP_ADD, -1, E.Lit(1, False))], -1, None, N.QE_ERR_INVALID_ARG),
    "term_column_past_the_end": (c(0), "i64", [(4, S.OP_LT, -1, E.Lit(1, False))], -1, None, N.QE_ERR_INVALID_ARG),
}


def _raw_update(st, dcols, spec):
    cc = (N.QeColumn * len(dcols))(*[d.as_c() for d in dcols])
    return N.lib().qe_hashagg_update_fused(st.handle, cc, len(dcols), N.C.byref(spec))


def _check_refused(ctx, good, bad_cols, bad_spec, status):
    """A valid update, then the refused one: its status, and the groups as the valid update left them."""
    st = new_state(ctx, good)
    st.update_fused(upload(ctx, good), c_spec(good))
    before = result_of(st)
    assert len(before) == 5
    assert _raw_update(st, bad_cols, bad_spec) == status, N.lib().qe_last_error()
    assert st.num_groups() == 5 and F.results_differ(result_of(st), before) is None


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(fused_ctx, name):
    """Plans the host compiler rejects before any launch: the documented status, and no group changes."""
    prog, kind, terms, mask_col, nterms, status = REFUSALS[name]
    cols = _refusal_base()
    aggs = [(S.AGG_MIN, kind), (S.AGG_COUNT_STAR, "i64")]
    good = F.Case(cols, P.Spec([], [c(1) if kind == "f64" else c(0), []], -1), F.observer_key(5), aggs, "observer", 16, {})
    bad = F.Case(cols, P.Spec(terms, [c(0), []], mask_col), good.keys, aggs, "observer", 16, {})
    spec = c_spec(bad)
    spec.inputs[0].ntokens = len(prog)  # (c_spec would not write an empty program over the good one)
    for i, (op, arg, lit) in enumerate(prog):
        spec.inputs[0].tokens[i] = N.QeToken(op, arg, _scalar(lit))
    if nterms is not None:
        spec.nterms = nterms
    _check_refused(fused_ctx, good, upload(fused_ctx, bad), spec, status)


@pytest.mark.parametrize("where", ["program", "term", "unused"])
def test_refuses_a_utf8_column(fused_ctx, where):
    """A UTF8 column among the fused columns (read by a program, by a term or by nothing) is not a
    fused input type: QE_ERR_UNSUPPORTED."""
    cols = _refusal_base()
    aggs = [(S.AGG_MIN, "i64"), (S.AGG_COUNT_STAR, "i64")]
    good = F.Case(cols, P.Spec([], [c(0), []], -1), F.observer_key(5), aggs, "observer", 16, {})
    dcols = upload(fused_ctx, good)
    dcols[2] = DeviceColumn.from_strings(["a", "bc", None, "", "def"], ctx=fused_ctx)
    terms = [(2, S.OP_EQ, -1, E.Lit(1, False))] if where == "term" else []
    bad = F.Case(cols, P.Spec(terms, [c(2) if where == "program" else c(0), []], -1), good.keys, aggs, "observer", 16, {})
    _check_refused(fused_ctx, good, dcols, c_spec(bad), N.QE_ERR_UNSUPPORTED)
