"""Inputs and references for the fused GROUP BY step's predicate terms and aggregate programs
(tests/test_fused_cases.py on the CPU, tests/test_fused_exprs.py on the GPU). Nothing here needs a
GPU or the library.

The data comes from the builders of tests/exprcases.py (column, arith_pair, cmp_pair, ...), a plan
is the Col / Spec / token form of tests/selprojcases.py: Spec.outputs[j] is the postfix program of
aggregate j (empty for COUNT(*)); a literal, in a term or a token, is an exprcases.Lit (so a null
literal keeps its type).

Two forms of key make a plan's results readable:
  observer  an INT64 key equal to the row index. Every group has exactly one row, so the group
            exists iff the row passed the mask and every term, MIN(program) is the program's value
            bit for bit (null iff the program is null) and COUNT(program) is 0 or 1. Nothing is
            summed and no order rule applies: no aggregate can mask a wrong value.
  grouped   a nullable UINT8 key row % 7 (eight groups with the null one), for SUM and AVG of the
            same program: the same-slot lanes of the LDS accumulate and the shared accumulator.
Both references return {key tuple: [aggregate values, None = null]}; an absent row is an absent key.
fused_rows is a literal row loop over Python values (exprcases.row_arith / row_cmp, its own
accumulators); fused_ref is vectorised on oracle.semantics (cmp, arith, select_mask,
group_aggregate). They share no code.

enumerate_cases() lists every plan the GPU file runs, by id; both test files take their cases from
it, so the CPU file checks exactly what the GPU file runs.
"""
import dataclasses
import functools
import math
from fractions import Fraction
from typing import Any, Dict, List, Tuple

import numpy as np

import exprcases as E
import selprojcases as P
from oracle import semantics as S

N_ROWS = E.MATRIX_N  # 2,055: eight whole 256-row wave steps and a 7-row tail
STEP = 256
MAX_TERMS, MAX_TOKENS, MAX_AGGS = 8, 16, 8
SP_KIND = {"i64": "i64", "f64": "f64", "i32": "i32", "d32": "date32", "u8": "u8"}
ARITH = {P.TOK_ADD: S.OP_ADD, P.TOK_SUB: S.OP_SUB, P.TOK_MUL: S.OP_MUL, P.TOK_DIV: S.OP_DIV}
ARITH_TOKS = (P.TOK_ADD, P.TOK_SUB, P.TOK_MUL, P.TOK_DIV)
OP_NAME = {S.OP_EQ: "eq", S.OP_NE: "ne", S.OP_LT: "lt", S.OP_LE: "le", S.OP_GT: "gt", S.OP_GE: "ge"}
# a lane holds rows 2 lane + {0, 1} and 128 + 2 lane + {0, 1} of a step; the loads' `full` flag
# changes at a multiple of 256; 4,096 rows are one step of a 1,024-thread workgroup
SIZES = [0, 1, 2, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097]
SIZE_PAIRS = E.SIZE_PAIRS + [("i64", "f64")]  # (i64, f64): every column 8 bytes wide (the all8 loads)
FULL_OP_PAIRS = [(k, k) for k in E.KINDS] + [("i64", "f64"), ("f64", "i64"), ("i32", "u8"), ("u8", "i32")]
LIT_PROGRAM_KINDS = ("i64", "i32", "f64")
LIT_TERM_KINDS = ("i64", "i32", "u8", "f64")
TURNOVER_LITS = [E.Lit(7, False), E.Lit(E.I64_MIN, False), E.Lit(None, False)]

# Expected groups of a state. They alone choose the path. The regular path needs the LDS table of
# both kernels to hold them (the generic kernel's budget is 80 KiB): COUNT(*) alone takes 12 bytes a
# slot, so every observer group fits; eight aggregates take ~76 (int64) to ~204 (fp64 MIN with its
# row-order words) bytes a slot, so the table holds a part of the 2,055 groups and the other rows
# take the global-table branch in the same launch.
EG_TERMS, EG_INT, EG_F64, EG_GROUPED, EG_GLOBAL = N_ROWS, 800, 200, 16, 16


@dataclasses.dataclass
class Case:
    cols: List[P.Col]
    spec: P.Spec            # terms, outputs = the aggregates' programs, mask_col
    keys: List[P.Col]
    aggs: List[Tuple[int, str]]  # (S.AGG_*, declared input kind "i64" / "f64")
    form: str               # "observer" / "grouped"
    expected_groups: int
    info: Dict[str, Any]


def xcol(kind, values, valid=None):
    return P.Col(SP_KIND[kind], values, valid)


def observer_key(n):
    return [P.Col("i64", np.arange(n, dtype=np.int64))]


def grouped_key(n):
    rng = E.rng_for("fusedkey", n)
    return [P.Col("u8", (np.arange(n) % 7).astype(np.uint8), E.validity(n, rng, 0.1))]


def keys_of(form, n):
    return observer_key(n) if form == "observer" else grouped_key(n)


def is_f64_prog(cols, prog):
    return any((t == P.TOK_COL and cols[a].kind == "f64") or (t == P.TOK_LIT and v.is_f64) for t, a, v in prog)


def typed_tokens(cols, prog):
    """How many tokens the program has once every int operand of an fp64 operation is promoted."""
    st, n = [], 0
    for t, a, v in prog:
        n += 1
        if t == P.TOK_COL:
            st.append(cols[a].kind == "f64")
        elif t == P.TOK_LIT:
            st.append(v.is_f64)
        else:
            y, x = st.pop(), st.pop()
            n += (x != y)
            st.append(x or y)
    return n


def stack_depth(prog):
    d = m = 0
    for t, _, _ in prog:
        d += 1 if t in (P.TOK_COL, P.TOK_LIT) else -1
        m = max(m, d)
    return m


# ---- references -----------------------------------------------------------------------------------
def _exact_sum(vals):
    if any(math.isnan(v) for v in vals):
        return math.nan
    pos, neg = math.inf in vals, -math.inf in vals
    if pos or neg:
        return math.nan if pos and neg else (math.inf if pos else -math.inf)
    q = sum((Fraction(v) for v in vals), Fraction(0))
    try:
        return float(q)  # correctly rounded, ties to even; an exact zero is +0.0
    except OverflowError:
        return math.inf if q > 0 else -math.inf


class _Acc:
    """One aggregate of one group, literally: nulls skipped; the first non-null value seeds MIN /
    MAX and only a strictly smaller / greater one replaces it; int64 SUM wraps, fp64 SUM is the
    correctly rounded exact sum; AVG is that sum over the count, in one division."""

    def __init__(self, fn):
        self.fn, self.rows, self.vals = fn, 0, []

    def add(self, v):
        self.rows += 1
        if v is not None:
            self.vals.append(v)

    def result(self):
        fn, vals = self.fn, self.vals
        if fn == S.AGG_COUNT_STAR:
            return self.rows
        if fn == S.AGG_COUNT:
            return len(vals)
        if not vals:
            return None
        if fn in (S.AGG_MIN, S.AGG_MAX):
            m = vals[0]
            for v in vals[1:]:
                if (v < m) if fn == S.AGG_MIN else (v > m):
                    m = v
            return m
        if fn == S.AGG_AVG:
            return _exact_sum(vals) / len(vals)
        if isinstance(vals[0], float):
            return _exact_sum(vals)
        s = sum(vals) & ((1 << 64) - 1)
        return s - (1 << 64) if s >= 1 << 63 else s


def _lit_value(lit):
    return None if lit.value is None else (float(lit.value) if lit.is_f64 else int(lit.value))


def fused_rows(cols, spec, keys, aggs):
    """Row at a time over Python values, None = null."""
    n = len(keys[0].values)
    vals = [E.rows_of(c.values, c.valid, n) for c in cols]
    isf = [c.kind == "f64" for c in cols]
    kvals = [E.rows_of(k.values, k.valid, n) for k in keys]
    groups: Dict[tuple, list] = {}
    for i in range(n):
        if spec.mask_col >= 0 and vals[spec.mask_col][i] is not True:
            continue  # false or null
        keep = True
        for col, op, rhs, lit in spec.terms:
            if rhs >= 0:
                y, yf = vals[rhs][i], isf[rhs]
            else:
                y, yf = _lit_value(lit), lit.is_f64
            if E.row_cmp(op, vals[col][i], y, isf[col] or yf) is not True:
                keep = False  # false or null
                break
        if not keep:
            continue
        key = tuple(kv[i] for kv in kvals)
        accs = groups.get(key)
        if accs is None:
            accs = groups[key] = [_Acc(fn) for fn, _ in aggs]
        for j, (fn, kind) in enumerate(aggs):
            if fn == S.AGG_COUNT_STAR:
                accs[j].add(None)
                continue
            st = []
            for t, a, lit in spec.outputs[j]:
                if t == P.TOK_COL:
                    st.append((vals[a][i], isf[a]))
                elif t == P.TOK_LIT:
                    st.append((_lit_value(lit), lit.is_f64))
                else:
                    (y, yf), (x, xf) = st.pop(), st.pop()
                    st.append((E.row_arith(ARITH[t], x, y, xf or yf), xf or yf))
            (v, f), = st
            if v is not None and not f and fn != S.AGG_COUNT and (kind == "f64" or fn == S.AGG_AVG):
                v = float(v)  # the widened integer, converted (round to nearest even)
            accs[j].add(v)
    return {k: [a.result() for a in accs] for k, accs in groups.items()}


def selection_ref(cols, spec):
    n = len(cols[0].values)
    sel = np.ones(n, dtype=bool)
    if spec.mask_col >= 0:
        sel &= S.select_mask(cols[spec.mask_col].values, cols[spec.mask_col].valid)
    for col, op, rhs, lit in spec.terms:
        r = cols[rhs] if rhs >= 0 else None
        m, mv = S.cmp(op, cols[col].values, cols[col].valid, r.values if r else E.ref_operand(lit), r.valid if r else None)
        sel &= S.select_mask(m, mv)
    return sel


def program_ref(cols, prog):
    """(values, valid or None) of a program over all rows, on oracle.semantics."""
    st = []
    for t, a, lit in prog:
        if t == P.TOK_COL:
            st.append((cols[a].values, cols[a].valid))
        elif t == P.TOK_LIT:
            st.append((E.ref_operand(lit), None))
        else:
            (y, yv), (x, xv) = st.pop(), st.pop()
            st.append(S.arith(ARITH[t], x, xv, y, yv))
    (v, vv), = st
    return v, vv


def fused_ref(cols, spec, keys, aggs):
    """The same, vectorised: S.cmp per term, S.select_mask, S.arith per operation, S.group_aggregate."""
    sel = selection_ref(cols, spec)
    inputs, valids = [], []
    for (fn, kind), prog in zip(aggs, spec.outputs):
        if fn == S.AGG_COUNT_STAR:
            inputs.append(None)
            valids.append(None)
            continue
        v, vv = program_ref(cols, prog)
        v = np.asarray(v)
        if v.dtype != np.float64:
            v = v.astype(np.int64)  # narrow columns widen by value
            if fn != S.AGG_COUNT and (kind == "f64" or fn == S.AGG_AVG):
                v = v.astype(np.float64)
        inputs.append(v)
        valids.append(vv)
    return S.group_aggregate([k.values for k in keys], [k.valid for k in keys], inputs, valids, [f for f, _ in aggs], sel)


def canon_result(d):
    """{canonical key: values} of either reference's (or the library's) result."""
    return {tuple(S.canon(x) for x in k): v for k, v in d.items()}


def results_differ(got, want):
    """None when two results agree bit for bit (S.rows_equal, no tolerance), else the first difference."""
    got, want = canon_result(got), canon_result(want)
    if len(got) != len(want):
        extra, missing = sorted(set(got) - set(want), key=repr)[:5], sorted(set(want) - set(got), key=repr)[:5]
        return f"{len(got)} groups, expected {len(want)}; unexpected {extra}, missing {missing}"
    for k, w in want.items():
        if k not in got:
            return f"group {k} missing"
        for j, (a, b) in enumerate(zip(got[k], w)):
            if not S.rows_equal(a, b, 0.0) or isinstance(a, float) != isinstance(b, float):
                return f"group {k} aggregate {j}: {a!r}, expected {b!r}"
    return None


# ---- plans ------------------------------------------------------------------------------------------
def _min_count(cols, progs):
    """MIN of each program, then COUNT of each."""
    kinds = ["f64" if is_f64_prog(cols, p) else "i64" for p in progs]
    return [(S.AGG_MIN, k) for k in kinds] + [(S.AGG_COUNT, k) for k in kinds], progs + progs


def _eg(aggs):
    if all(fn == S.AGG_COUNT_STAR for fn, _ in aggs):
        return EG_TERMS
    return EG_F64 if any(k == "f64" for _, k in aggs) else EG_INT


def _case(cols, terms, progs, aggs, form, mask_col=-1, **info):
    n = len(cols[0].values)
    return Case(cols, P.Spec(terms, progs, mask_col), keys_of(form, n), aggs, form,
                EG_GROUPED if form == "grouped" else _eg(aggs), info)


def pair_program_case(kl, kr, nulls, n=N_ROWS):
    """MIN and COUNT of a + b, a - b, a * b, a / b: eight aggregates, the most a state takes."""
    a, av, b, bv = E.arith_pair(kl, kr, n)
    cols = [xcol(kl, a, av if nulls[0] else None), xcol(kr, b, bv if nulls[1] else None)]
    aggs, progs = _min_count(cols, [P._bin(t, P._col(0), P._col(1)) for t in ARITH_TOKS])
    return _case(cols, [], progs, aggs, "observer", family="pair", kinds=(kl, kr), division=True)


@functools.lru_cache(maxsize=None)
def lit_column(kind, n=N_ROWS):
    rng = E.rng_for("fusedlit", kind, n)
    return E.column(kind, n, rng), E.validity(n, rng)


def lit_program_case(kind, lit, lit_left):
    a, av = lit_column(kind)
    cols = [xcol(kind, a, av)]
    x, y = (P._lit(lit), P._col(0)) if lit_left else (P._col(0), P._lit(lit))
    aggs, progs = _min_count(cols, [P._bin(t, x, y) for t in ARITH_TOKS])
    return _case(cols, [], progs, aggs, "observer", family="lit", kind=kind, lit=lit, lit_left=lit_left, division=True)


DEEP_KINDS = ("i64", "f64", "i32", "u8", "d32")


def deep_case(which):
    """depth2: ((a + b) * c) - d; depth4: a b c d + + +; max_tokens: i f + i * i - i / i +, whose five
    promotions bring its 11 tokens to QE_MAX_TOKENS typed ones. Slots: 0 i64, 1 f64, 2 i32, 3 u8, 4 d32."""
    rng = E.rng_for("fuseddeep", which)
    cols = [xcol(k, E.column(k, N_ROWS, rng), E.validity(N_ROWS, rng, 0.08)) for k in DEEP_KINDS]
    c = P._col
    if which == "depth2":
        progs = [P._bin(P.TOK_SUB, P._bin(P.TOK_MUL, P._bin(P.TOK_ADD, c(2), c(0)), c(1)), c(3)),
                 P._bin(P.TOK_SUB, P._bin(P.TOK_MUL, P._bin(P.TOK_ADD, c(2), c(0)), c(3)), c(4))]
    elif which == "depth4":
        add3 = [(P.TOK_ADD, 0, None)] * 3
        progs = [c(0) + c(2) + c(1) + c(3) + add3, c(4) + c(3) + c(2) + c(0) + add3]
    else:
        prog = P._bin(P.TOK_ADD, c(0), c(1))
        for t, k in ((P.TOK_MUL, 2), (P.TOK_SUB, 3), (P.TOK_DIV, 4), (P.TOK_ADD, 0)):
            prog = P._bin(t, prog, c(k))
        progs = [prog]
    aggs, progs = _min_count(cols, progs)
    return _case(cols, [], progs, aggs, "observer", family="deep", which=which)


def convert_case(form):
    """MIN and AVG declared FLOAT64 over bare INT64 / INT32 / UINT8 columns: the value is the
    conversion of the widened integer (2^53 + 1 and INT64_MIN are among the int64 edges)."""
    rng = E.rng_for("fusedcvt", form)
    kinds = ("i64", "i32", "u8")
    cols = [xcol(k, E.column(k, N_ROWS, rng), E.validity(N_ROWS, rng)) for k in kinds]
    aggs, progs = [], []
    for s in range(3):
        aggs += [(S.AGG_MIN, "f64"), (S.AGG_AVG, "i64")]
        progs += [P._col(s), P._col(s)]
    aggs += [(S.AGG_COUNT, "i64")]  # (seven aggregates: an eighth fp64 one leaves the generic kernel no LDS table)
    progs += [P._col(0)]
    return _case(cols, [], progs, aggs, form, family="convert")


def turnover_case(plan, lit):
    """The same plan shape under three literals: a value, another value (the same compiled kernel)
    and the null literal of the same type (which must not be served that kernel)."""
    a, av = lit_column("i64")
    cols = [xcol("i64", a, av)]
    if plan == "term":
        return _case(cols, [(0, S.OP_GE, -1, lit)], [[]], [(S.AGG_COUNT_STAR, "i64")], "observer", family="turnover")
    aggs, progs = _min_count(cols, [P._bin(P.TOK_ADD, P._col(0), P._lit(lit)), P._bin(P.TOK_SUB, P._lit(lit), P._col(0))])
    return _case(cols, [], progs, aggs, "observer", family="turnover")


def _tame(values, key):
    """fp64 inputs of a grouped plan: NaN only in group 5, +Inf only in group 6, so that the other
    groups' SUM and AVG are finite."""
    if values.dtype != np.float64:
        return values
    v = values.copy()
    v[np.isnan(v) & (key != 5)] = 0.5
    v[(v == np.inf) & (key != 6)] = 3e5
    v[v == -np.inf] = -3e5
    return v


def shared_case(which, kind):
    """Aggregates that may or may not share an accumulator: cols SUM(a+b), AVG(a+b), SUM(a+c);
    lits SUM(a+1), SUM(a+2) and their AVGs; null SUM(a+null), SUM(a+0)."""
    rng = E.rng_for("fusedshare", which, kind)
    key = np.arange(N_ROWS) % 7
    cols = [xcol(kind, _tame(E.column(kind, N_ROWS, rng), key), E.validity(N_ROWS, rng)) for _ in range(3)]
    f = kind == "f64"
    L = lambda v: P._lit(E.Lit(None if v is None else (float(v) if f else v), f))
    add = lambda x, y: P._bin(P.TOK_ADD, x, y)
    c = P._col
    if which == "cols":
        fns = [S.AGG_SUM, S.AGG_AVG, S.AGG_SUM, S.AGG_AVG]
        progs = [add(c(0), c(1)), add(c(0), c(1)), add(c(0), c(2)), add(c(0), c(2))]
    elif which == "lits":
        fns = [S.AGG_SUM, S.AGG_SUM, S.AGG_AVG, S.AGG_AVG]
        progs = [add(c(0), L(1)), add(c(0), L(2)), add(c(0), L(1)), add(c(0), L(2))]
    else:
        fns = [S.AGG_SUM, S.AGG_SUM, S.AGG_AVG, S.AGG_AVG]
        progs = [add(c(0), L(None)), add(c(0), L(0)), add(c(0), L(0)), add(c(0), L(None))]
    aggs = [(fn, kind) for fn in fns] + [(S.AGG_COUNT_STAR, "i64")]
    return _case(cols, [], progs + [[]], aggs, "grouped", family="shared", which=which, kind=kind)


def grouped_pair_case(kl, kr):
    """The grouped form of a pair plan: SUM, AVG, MIN, COUNT of a + b, SUM and AVG of a * b, MAX and
    COUNT of a / b."""
    a, av, b, bv = E.arith_pair(kl, kr, N_ROWS)
    key = np.arange(N_ROWS) % 7
    cols = [xcol(kl, _tame(a, key), av), xcol(kr, _tame(b, key), bv)]
    f = "f64" if "f64" in (kl, kr) else "i64"
    op = lambda t: P._bin(t, P._col(0), P._col(1))
    fns = [S.AGG_SUM, S.AGG_AVG, S.AGG_MIN, S.AGG_COUNT, S.AGG_SUM, S.AGG_AVG, S.AGG_MAX, S.AGG_COUNT]
    progs = [op(P.TOK_ADD)] * 4 + [op(P.TOK_MUL)] * 2 + [op(P.TOK_DIV)] * 2
    return _case(cols, [], progs, [(fn, f) for fn in fns], "grouped", family="grouped_pair", kinds=(kl, kr), division=True)


def _count_star():
    return [[]], [(S.AGG_COUNT_STAR, "i64")]


def cmp_cols_case(kl, kr, op, n=N_ROWS):
    a, av, b, bv = E.cmp_pair(kl, kr, n)
    progs, aggs = _count_star()
    return _case([xcol(kl, a, av), xcol(kr, b, bv)], [(0, op, 1, None)], progs, aggs, "observer",
                 family="cmp_cols", kinds=(kl, kr), op=op)


def mixed_precision_case(int_left, op):
    """int64 against fp64 beyond 2^53 (no nulls): the comparison is made in fp64."""
    i, d = E.mixed_precision_pairs(N_ROWS)
    cols = [xcol("i64", i), xcol("f64", d)]
    progs, aggs = _count_star()
    term = (0, op, 1, None) if int_left else (1, op, 0, None)
    return _case(cols, [term], progs, aggs, "observer", family="mixed_precision", int_left=int_left, op=op)


def cmp_lit_case(kind, lit, op):
    a, av = E.column_around(kind, lit, N_ROWS)
    progs, aggs = _count_star()
    return _case([xcol(kind, a, av)], [(0, op, -1, lit)], progs, aggs, "observer", family="cmp_lit", kind=kind, lit=lit, op=op)


EIGHT_TERMS = [  # over slots 0 a i64?, 1 b f64?, 2 c i32, 3 d date32?, 4 e u8, mask 5 (? = nullable)
    (0, S.OP_LT, -1, E.Lit(900, False)), (1, S.OP_NE, -1, E.Lit(33.5, True)), (2, S.OP_GE, -1, E.Lit(-50, False)),
    (3, S.OP_NE, -1, E.Lit(7, False)), (4, S.OP_LE, -1, E.Lit(230, False)), (0, S.OP_GT, 2, None),
    (4, S.OP_NE, 3, None), (1, S.OP_LE, 2, None)]


def eight_terms_case():
    """QE_MAX_TERMS terms over all five kinds and a nullable BOOL mask. c is drawn first, a a little
    above it and b a little below (each on the wrong side on a tenth of the rows, b NaN on a few), so
    that every term fails alone on some rows. The null rows of the mask carry bit 1, and the null
    rows of a carry values that mostly pass a's terms (ignoring a validity would select them)."""
    n = N_ROWS
    rng = E.rng_for("fused8", n)
    c = rng.integers(-100, 1000, n).astype(np.int32)
    c[rng.random(n) < 0.02] = E.I32_MIN
    a = c.astype(np.int64) + np.where(rng.random(n) < 0.1, -rng.integers(0, 4, n), rng.integers(1, 31, n))
    b = c.astype(np.float64) - np.where(rng.random(n) < 0.1, -0.5 - rng.integers(0, 4, n), rng.integers(0, 31, n) + 0.25)
    b[rng.random(n) < 0.03] = np.nan
    b[rng.random(n) < 0.06] = 33.5
    e = rng.integers(0, 256, n).astype(np.uint8)
    d = rng.integers(0, 21, n).astype(np.int32)
    same = rng.random(n) < 0.08
    d[same] = e[same]
    m = rng.random(n) < 0.8
    mv = E.validity(n, rng, 0.1)
    m[~mv] = True
    cols = [xcol("i64", a, E.validity(n, rng, 0.1)), xcol("f64", b, E.validity(n, rng, 0.1)), xcol("i32", c),
            xcol("d32", d, E.validity(n, rng, 0.1)), xcol("u8", e), P.Col("bool", m, mv)]
    progs, aggs = _count_star()
    return _case(cols, list(EIGHT_TERMS), progs, aggs, "observer", mask_col=5, family="eight_terms")


def value_records_case():
    """One aggregate over two columns: a partitioned record holds the program's value (two words
    against the columns' three), evaluated by the scatter pass."""
    a, av, b, bv = E.arith_pair("u8", "i64", N_ROWS)
    cols = [xcol("u8", a, av), xcol("i64", b, bv)]
    return _case(cols, [], [P._bin(P.TOK_DIV, P._col(0), P._col(1))], [(S.AGG_MIN, "i64")], "observer",
                 family="value_records", kinds=("u8", "i64"), division=True)


# ---- the enumeration ----------------------------------------------------------------------------------
def lit_id(lit):
    return ("null" if lit.value is None else repr(lit.value)) + ("_f64" if lit.is_f64 else "_i64")


def _nulls_id(nulls):
    return "".join("n" if x else "v" for x in nulls)  # n: nullable side, v: no validity


def enumerate_cases() -> Dict[str, tuple]:
    """{case id: (builder, arguments)} of every plan tests/test_fused_exprs.py runs, in order."""
    out: Dict[str, tuple] = {}
    for kl in E.KINDS:
        for kr in E.KINDS:
            out[f"pair-{kl}-{kr}-nn"] = (pair_program_case, (kl, kr, (True, True)))
    for kl, kr in [("i64", "i64"), ("f64", "f64")] + E.SIZE_PAIRS:
        for nulls in E.NULL_COMBOS[1:]:
            out[f"pair-{kl}-{kr}-{_nulls_id(nulls)}"] = (pair_program_case, (kl, kr, nulls))
    for kind in LIT_PROGRAM_KINDS:
        for lit in E.LITERALS:
            out[f"lit-{kind}-col_op_{lit_id(lit)}"] = (lit_program_case, (kind, lit, False))
            out[f"lit-{kind}-{lit_id(lit)}_op_col"] = (lit_program_case, (kind, lit, True))
    for which in ("depth2", "depth4", "max_tokens"):
        out[f"deep-{which}"] = (deep_case, (which,))
    for form in ("observer", "grouped"):
        out[f"convert-{form}"] = (convert_case, (form,))
    for plan in ("program", "term"):
        for lit in TURNOVER_LITS:
            out[f"turnover-{plan}-{lit_id(lit)}"] = (turnover_case, (plan, lit))
    for which in ("cols", "lits", "null"):
        for kind in ("f64", "i64"):
            out[f"shared-{which}-{kind}"] = (shared_case, (which, kind))
    for kl, kr in SIZE_PAIRS + [("i64", "i64"), ("f64", "f64")]:
        out[f"grouped-{kl}-{kr}"] = (grouped_pair_case, (kl, kr))
    for kl in E.KINDS:
        for kr in E.KINDS:
            for op in (E.CMP_OPS if (kl, kr) in FULL_OP_PAIRS else [S.OP_LT, S.OP_GE]):
                out[f"cmp-{kl}-{kr}-{OP_NAME[op]}"] = (cmp_cols_case, (kl, kr, op))
    for int_left in (True, False):
        for op in E.CMP_OPS:
            out[f"mixed-{'i64_f64' if int_left else 'f64_i64'}-{OP_NAME[op]}"] = (mixed_precision_case, (int_left, op))
    for kind in LIT_TERM_KINDS:
        for lit in E.LITERALS:
            for op in E.CMP_OPS:
                out[f"cmplit-{kind}-{OP_NAME[op]}-{lit_id(lit)}"] = (cmp_lit_case, (kind, lit, op))
    out["eight_terms"] = (eight_terms_case, ())
    out["value_records"] = (value_records_case, ())
    for kl, kr in SIZE_PAIRS:
        for n in SIZES:
            out[f"size-program-{kl}-{kr}-{n}"] = (pair_program_case, (kl, kr, (True, True), n))
            out[f"size-term-{kl}-{kr}-{n}"] = (cmp_cols_case, (kl, kr, S.OP_LT, n))
    return out


CASES = enumerate_cases()
# the plans that also run where the programs are evaluated elsewhere: the global-table branch, the
# multi-pass spill and the radix-partitioned passes
REDUCED = ["pair-i64-i64-nn", "pair-i32-f64-nn", "pair-u8-i64-nn", "eight_terms",
           "lit-i64-col_op_null_i64", "lit-i64-nan_f64_op_col", "value_records"]
COLUMN_RECORDS, VALUE_RECORDS = "pair-i64-i64-nn", "value_records"
assert set(REDUCED) <= set(CASES)


def case_ids(prefix):
    return [k for k in CASES if k.startswith(prefix)]


@functools.lru_cache(maxsize=400)
def built(case_id) -> Case:
    """The case (never modified by a test)."""
    fn, args = CASES[case_id]
    return fn(*args)


@functools.lru_cache(maxsize=400)
def reference(case_id):
    """fused_ref of the case, computed once for the kernel modes and paths that run it."""
    c = built(case_id)
    return fused_ref(c.cols, c.spec, c.keys, c.aggs)
