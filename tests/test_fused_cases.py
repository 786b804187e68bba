"""CPU checks of tests/fusedcases.py: the row loop and the vectorised reference agree on every plan
tests/test_fused_exprs.py runs (the same enumeration, the same seeds and sizes), and every data set
holds what its plans are there to show, asserted from the inputs alone."""
import math

import numpy as np
import pytest

import exprcases as E
import fusedcases as F
import selprojcases as P
from oracle import semantics as S

P53 = 1 << 53


@pytest.mark.parametrize("case_id", list(F.CASES))
def test_row_loop_equals_vectorised_reference(case_id):
    c = F.built(case_id)
    rows, ref = F.fused_rows(c.cols, c.spec, c.keys, c.aggs), F.reference(case_id)
    assert F.results_differ(rows, ref) is None
    n = len(c.keys[0].values)
    assert len(ref) == (int(F.selection_ref(c.cols, c.spec).sum()) if c.form == "observer" else min(n, 8))
    assert all(len(v) == len(c.aggs) for v in ref.values())


def test_references_on_hand_made_rows():
    """What both references must give, written out: INT64_MIN / -1 wraps, x / 0 is null, a null
    operand or literal makes the value null and leaves the group, a null or false term drops the row,
    int64 against fp64 is computed in fp64, a MIN declared FLOAT64 converts the integer."""
    a = P.Col("i64", [E.I64_MIN, 7, -7, 5, P53 + 1, 9, 1], [True, True, True, False, True, True, True])
    b = P.Col("i64", [-1, 0, 2, 1, 1, 1, 1], [True, True, True, True, True, False, True])
    f = P.Col("f64", [1.5, math.nan, -0.0, 2.0, 1.0, 1.0, 1.0])
    t = P.Col("i32", [0, 0, 0, 0, 0, 0, -1], [True, True, True, True, True, True, True])
    c = P._col
    progs = [P._bin(P.TOK_DIV, c(0), c(1)), P._bin(P.TOK_ADD, c(0), c(2)), P._bin(P.TOK_MUL, P._lit(E.Lit(None, True)), c(0)),
             c(0), P._bin(P.TOK_DIV, c(0), c(1)), []]
    aggs = [(S.AGG_MIN, "i64"), (S.AGG_MIN, "f64"), (S.AGG_MIN, "f64"), (S.AGG_MIN, "f64"), (S.AGG_COUNT, "i64"),
            (S.AGG_COUNT_STAR, "i64")]
    spec = P.Spec([(3, S.OP_GE, -1, E.Lit(0, False))], progs, -1)
    want = {(0,): [E.I64_MIN, float(E.I64_MIN) + 1.5, None, float(E.I64_MIN), 1, 1],
            (1,): [None, math.nan, None, 7.0, 0, 1],
            (2,): [-3, -7.0, None, -7.0, 1, 1],
            (3,): [None, None, None, None, 0, 1],
            (4,): [P53 + 1, float(P53) + 1.0, None, float(P53), 1, 1],
            (5,): [None, 10.0, None, 9.0, 0, 1]}  # row 6 fails the term
    keys = F.observer_key(7)
    for got in (F.fused_rows([a, b, f, t], spec, keys, aggs), F.fused_ref([a, b, f, t], spec, keys, aggs)):
        assert F.results_differ(got, want) is None
    # grouped: int64 SUM wraps, AVG converts each value and divides the exact sum once, MIN / MAX keep a NaN seed
    x = P.Col("i64", [E.I64_MAX, 1, P53 + 1, 1], [True, True, True, True])
    y = P.Col("f64", [math.nan, 1.0, 0.0, -0.0])
    k = [P.Col("u8", [0, 0, 1, 1], [True, True, True, True])]
    g = P.Spec([], [c(0), c(0), c(1), c(1)], -1)
    gaggs = [(S.AGG_SUM, "i64"), (S.AGG_AVG, "i64"), (S.AGG_MIN, "f64"), (S.AGG_MAX, "f64")]
    want = {(0,): [E.I64_MIN, (float(E.I64_MAX) + 1.0) / 2, math.nan, math.nan], (1,): [P53 + 2, (float(P53) + 1.0) / 2, 0.0, 0.0]}
    for got in (F.fused_rows([x, y], g, k, gaggs), F.fused_ref([x, y], g, k, gaggs)):
        assert F.results_differ(got, want) is None


# ---- the enumeration ----------------------------------------------------------------------------------
def test_enumeration_holds_what_the_gpu_file_is_to_run():
    ids = set(F.CASES)
    pairs = [(kl, kr) for kl in E.KINDS for kr in E.KINDS]
    assert all(f"pair-{kl}-{kr}-nn" in ids for kl, kr in pairs) and len(pairs) == 25
    for kl, kr in [("i64", "i64"), ("f64", "f64")] + E.SIZE_PAIRS:
        assert {f"pair-{kl}-{kr}-{x}" for x in ("nn", "nv", "vn", "vv")} <= ids
    assert len(F.case_ids("lit-")) == 2 * len(E.LITERALS) * 3 and len(E.LITERALS) == 13
    assert len(F.case_ids("cmplit-")) == 6 * len(E.LITERALS) * 4
    assert len(F.case_ids("cmp-")) == 6 * 9 + 2 * 16 and len(F.case_ids("mixed-")) == 12
    assert len(F.case_ids("size-")) == 2 * 4 * len(F.SIZES)
    for case_id in F.REDUCED:
        assert F.built(case_id).form == "observer"
    for case_id in F.CASES:
        c = F.built(case_id)
        assert len(c.aggs) <= F.MAX_AGGS and len(c.spec.terms) <= F.MAX_TERMS and len(c.cols) + len(c.keys) <= 8
        for (fn, kind), prog in zip(c.aggs, c.spec.outputs):
            assert (fn == S.AGG_COUNT_STAR) == (prog == [])
            if prog:
                assert F.stack_depth(prog) <= 4 and F.typed_tokens(c.cols, prog) <= F.MAX_TOKENS
                assert kind == "f64" or fn in (S.AGG_COUNT, S.AGG_AVG) or not F.is_f64_prog(c.cols, prog)


def test_program_shapes():
    """The shapes the host compiler tells apart: `col op col` of one type has three typed tokens,
    a mixed pair four (one promotion), a literal on the left never starts with a column; the deep
    programs reach stack depth 2 and 4 and exactly QE_MAX_TOKENS typed tokens."""
    for kl in E.KINDS:
        for kr in E.KINDS:
            c = F.built(f"pair-{kl}-{kr}-nn")
            want = 4 if (kl == "f64") != (kr == "f64") else 3
            assert all(F.typed_tokens(c.cols, p) == want for p in c.spec.outputs)
    for case_id in F.case_ids("lit-"):
        c = F.built(case_id)
        assert all((p[0][0] == P.TOK_LIT) == c.info["lit_left"] for p in c.spec.outputs)
    d2, d4, mx = (F.built(f"deep-{w}") for w in ("depth2", "depth4", "max_tokens"))
    assert {F.stack_depth(p) for p in d2.spec.outputs} == {2} and {F.stack_depth(p) for p in d4.spec.outputs} == {4}
    assert F.is_f64_prog(d2.cols, d2.spec.outputs[0]) and not F.is_f64_prog(d2.cols, d2.spec.outputs[1])
    assert F.typed_tokens(d4.cols, d4.spec.outputs[0]) == 10  # three promotions
    assert F.typed_tokens(mx.cols, mx.spec.outputs[0]) == F.MAX_TOKENS and len(mx.spec.outputs[0]) == 11
    assert len(F.EIGHT_TERMS) == F.MAX_TERMS


# ---- division ---------------------------------------------------------------------------------------
def _rows_with(a, av, b, bv, x, y):
    ok = (a == x) & (b == y)
    for v in (av, bv):
        if v is not None:
            ok = ok & v
    return np.flatnonzero(ok)


@pytest.mark.parametrize("case_id", F.case_ids("pair-") + F.case_ids("grouped-") + ["value_records"])
def test_pair_division_rows(case_id):
    """Valid rows with divisor 0 in every plan; in the integer plans each of exprcases.div_rows
    (INT64_MIN / -1 or the kinds' nearest equivalent, x / 0, a truncating quotient) in a full
    256-row step and in the partial last step."""
    c = F.built(case_id)
    (a, b), (kl, kr) = c.cols, c.info["kinds"]
    n = len(a.values)
    both = (np.ones(n, bool) if a.valid is None else a.valid) & (np.ones(n, bool) if b.valid is None else b.valid)
    assert (both & (b.values == 0)).sum() >= 3
    if "f64" in (kl, kr):
        return
    last = (n // F.STEP) * F.STEP
    assert n % F.STEP and last >= F.STEP
    rows = E.div_rows(kl, kr)
    assert ("min_by_minus_one" in rows) == (kl in E.SIGNED and kr in E.SIGNED) and rows["by_zero"][1] == 0
    for x, y in rows.values():
        at = _rows_with(a.values, a.valid, b.values, b.valid, x, y)
        assert (at < last).any() and (at >= last).any(), (x, y, at)
    if (kl, kr) == ("i64", "i64"):
        assert rows["min_by_minus_one"] == (E.I64_MIN, -1)


def test_size_cases_keep_the_division_rows():
    for kl, kr in F.SIZE_PAIRS:
        if "f64" in (kl, kr):
            continue
        for n in F.SIZES:
            c = F.built(f"size-program-{kl}-{kr}-{n}")
            assert len(c.cols[0].values) == n == len(c.keys[0].values)
            if n >= 16:  # (exprcases._plant: near the start, and from 16 rows on at the end too)
                for x, y in E.div_rows(kl, kr).values():
                    at = _rows_with(c.cols[0].values, c.cols[0].valid, c.cols[1].values, c.cols[1].valid, x, y)
                    assert len(at) >= 2 and at.max() >= n - 3


@pytest.mark.parametrize("kind", F.LIT_PROGRAM_KINDS)
def test_literal_program_column(kind):
    """The column of the literal plans: valid and null rows, valid zeros (lit / col divides by
    zero); the int64 one holds INT64_MIN (INT64_MIN / -1 with the literal -1, and -1 for
    INT64_MIN / col), and the literal list holds 0 (col / 0: every row null)."""
    a, av = F.lit_column(kind)
    assert 0.05 <= (~av).mean() <= 0.3 and (av & (a == 0)).sum() >= 10
    assert any(l.value == 0 and not l.is_f64 for l in E.LITERALS) and any(l.value == -1 for l in E.LITERALS)
    assert any(l.value == E.I64_MIN for l in E.LITERALS)
    if kind == "i64":
        assert (av & (a == E.I64_MIN)).any() and (av & (a == -1)).any() and (av & (a == P53 + 1)).any()
    if kind == "i32":
        assert (av & (a == E.I32_MIN)).any() and (av & (a == -1)).any()


@pytest.mark.parametrize("lit", [l for l in E.LITERALS if l.is_f64 and l.value is not None and math.isfinite(l.value) and l.value],
                         ids=repr)
def test_fp64_literal_plans_tell_promotion_from_truncation(lit):
    """An fp64 literal promotes an int64 column to fp64: on valid rows beyond 2^53 that differs, for
    some operation, from truncating the literal and computing in int64."""
    a, av = F.lit_column("i64")
    big = np.flatnonzero(av & (np.abs(a.astype(np.float64)) > float(P53)))
    assert len(big) >= 10
    differs = 0
    for i in big.tolist():
        x = int(a[i])
        for op in E.ARITH_OPS:
            p = E.row_arith(op, x, float(lit.value), True)
            t = E.row_arith(op, x, int(lit.value), False)
            differs += (t is None) or math.isnan(p) or p != t
    assert differs >= 10


# ---- comparisons ------------------------------------------------------------------------------------
def _states(case):
    """(true, false, null) shares of the case's single term over its rows."""
    (col, op, rhs, lit), = case.spec.terms
    a = case.cols[col]
    b = case.cols[rhs] if rhs >= 0 else None
    m, mv = S.cmp(op, a.values, a.valid, b.values if b else E.ref_operand(lit), b.valid if b else None)
    return E.state_shares(m, mv)


@pytest.mark.parametrize("case_id", F.case_ids("cmp-") + F.case_ids("size-term-"))
def test_column_comparison_data(case_id):
    c = F.built(case_id)
    a, b = c.cols
    n = len(a.values)
    if n >= 127:
        assert min(E.outcome_shares(a.values, a.valid, b.values, b.valid)) >= 0.2 - (0.08 if n < 1000 else 0)
        t, f, nl = _states(c)
        assert t >= 0.15 and f >= 0.15 and nl >= 0.15
    if c.info["kinds"] == ("i64", "i64") and n == F.N_ROWS:
        both = a.valid & b.valid
        assert (both & (a.values == E.I64_MIN) & (b.values == E.I64_MAX)).any()
        lt = S.cmp(S.OP_LT, a.values, None, b.values, None)[0]
        assert ((a.values.view(np.uint64) < b.values.view(np.uint64)) != lt)[both].sum() >= 0.2 * n
        assert ((a.values.astype(np.float64) < b.values.astype(np.float64)) != lt)[both].any()


@pytest.mark.parametrize("case_id", F.case_ids("mixed-"))
def test_mixed_precision_data(case_id):
    c = F.built(case_id)
    i, d = c.cols
    assert min(E.outcome_shares(i.values, None, d.values, None)) >= 0.2
    t, f, _ = _states(c)
    assert t >= 0.2 and f >= 0.2
    exact = np.array([(not math.isnan(y)) and x == int(y) for x, y in zip(i.values.tolist(), d.values.tolist())])
    eq = S.cmp(S.OP_EQ, i.values, None, d.values, None)[0]
    assert (eq & ~exact).sum() >= 0.05 * len(eq) and (np.abs(i.values[eq & ~exact].astype(np.float64)) >= float(P53)).all()


@pytest.mark.parametrize("case_id", F.case_ids("cmplit-"))
def test_literal_comparison_data(case_id):
    c = F.built(case_id)
    kind, lit = c.info["kind"], c.info["lit"]
    t, f, nl = _states(c)
    assert abs(t + f + nl - 1.0) < 1e-9
    if lit.value is None:
        assert nl == 1.0  # a null literal selects nothing
    elif E.literal_admits_all(kind, lit):
        assert min(E.outcome_shares(c.cols[0].values, c.cols[0].valid, E.ref_operand(lit), None)) >= 0.2
        assert t >= 0.15 and f >= 0.15 and nl >= 0.05
    else:
        assert 0.05 <= nl <= 0.3  # (what such a literal gives on the valid rows is the row loop's, above)
        if not math.isnan(lit.value):
            assert max(E.outcome_shares(c.cols[0].values, c.cols[0].valid, E.ref_operand(lit), None)) >= 0.2
    if isinstance(lit.value, float) and math.isnan(lit.value):
        assert (t > 0) == (c.info["op"] == S.OP_NE)


def test_eight_term_plan():
    c = F.built("eight_terms")
    n = F.N_ROWS
    sel = F.selection_ref(c.cols, c.spec)
    assert 0.1 <= sel.mean() <= 0.6
    assert {x.kind for x in c.cols} == {"i64", "f64", "i32", "date32", "u8", "bool"}
    mask = c.cols[c.spec.mask_col]
    assert mask.valid is not None and mask.values[~mask.valid].all() and (~mask.valid).sum() >= 0.05 * n
    mask_ok = S.select_mask(mask.values, mask.valid)
    passes = []
    for term in c.spec.terms:
        one = P.Spec([term], [], -1)
        passes.append(F.selection_ref(c.cols, one))
    passes = np.array(passes)
    for k in range(len(passes)):  # every term, and the mask, alone decides some row
        others = np.delete(passes, k, axis=0).all(axis=0) & mask_ok
        assert (others & ~passes[k]).sum() >= 5, k
    assert (passes.all(axis=0) & ~mask_ok & ~mask.valid).sum() >= 5  # null mask rows, bit 1, every term true
    assert (passes.all(axis=0) & ~mask_ok & mask.valid).sum() >= 5
    # null rows of a whose value passes both of a's terms, every other term and the mask true
    a = c.cols[0]
    with_a = [k for k, t in enumerate(c.spec.terms) if 0 in (t[0], t[2])]
    assert with_a == [0, 5] and a.valid is not None
    all_valid = list(c.cols)
    all_valid[0] = P.Col("i64", a.values)
    ignoring = F.selection_ref(all_valid, c.spec) & ~a.valid
    assert ignoring.sum() >= 5 and not (ignoring & sel).any()


def test_global_table_run_leaves_the_lds_table():
    """A 256-slot LDS table (expected groups 16) cannot hold more than 256 of an observer plan's
    groups: at least half of every reduced plan's selected rows take the global-table branch."""
    for case_id in F.REDUCED:
        ref = F.reference(case_id)
        assert len(ref) - 256 >= len(ref) / 2, (case_id, len(ref))


def test_grouped_inputs_are_tame():
    for case_id in F.case_ids("shared-") + F.case_ids("grouped-") + ["convert-grouped"]:
        c = F.built(case_id)
        assert c.form == "grouped" and c.expected_groups == F.EG_GROUPED
        key = c.keys[0]
        assert key.valid is not None and 0.03 <= (~key.valid).mean() <= 0.2 and set(key.values.tolist()) == set(range(7))
        for col in c.cols:
            if col.kind == "f64":
                k = np.arange(len(col.values)) % 7
                assert not np.isnan(col.values[k != 5]).any() and np.isfinite(col.values[k < 5]).all()
        ref = F.reference(case_id)
        assert len(ref) == 8
        for j, (fn, kind) in enumerate(c.aggs):
            if fn in (S.AGG_SUM, S.AGG_AVG) and c.info.get("which") != "null":
                vals = [v[j] for v in ref.values()]
                assert sum(v is not None and math.isfinite(v) for v in vals) >= 5, (case_id, j, vals)
