"""Inputs and references for the fused select-project tests (tests/test_selproj_cases.py on the
CPU, tests/test_selproj_shapes.py on the GPU). Nothing here needs a GPU or the library.

A case is built backwards: a selection builder makes the boolean vector `sel` first, placed
relative to a tile size T (and a workgroup size `block`: inside a tile, thread t of stripe r holds
row base + r * block + t, wave = t // 64, lane = t % 64); a plan shape S1..S8 then derives its
predicate columns from it, so that the plan selects exactly `sel` whatever its literals are.

Two references compute what a plan yields: select_project_rows, a literal row-at-a-time loop, and
select_project_ref, vectorised on oracle.semantics. Both return, per output, the values and the
validity of the selected rows in input order.
"""
import functools

import numpy as np

from oracle import semantics as S

# token codes of an output program (include/qe_hip.h QE_TOK_*)
TOK_COL, TOK_LIT, TOK_ADD, TOK_SUB, TOK_MUL, TOK_DIV = 1, 2, 3, 4, 5, 6
_ARITH = {TOK_ADD: S.OP_ADD, TOK_SUB: S.OP_SUB, TOK_MUL: S.OP_MUL, TOK_DIV: S.OP_DIV}

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
_DTYPE = {"i64": np.int64, "f64": np.float64, "i32": np.int32, "u8": np.uint8, "date32": np.int32, "bool": np.bool_}

TILE_SIZES = (1024, 2048, 4096, 8192, 12288, 16384)  # every tile / group size the generator may report
BLOCKS = (256, 1024)


class Col:
    """A host column: kind (i64 / f64 / i32 / u8 / date32 / bool), values, validity (bool) or None."""

    def __init__(self, kind, values, valid=None):
        self.kind = kind
        self.values = np.ascontiguousarray(values, dtype=_DTYPE[kind])
        self.valid = None if valid is None else np.ascontiguousarray(valid, dtype=bool)


class Spec:
    """mask_col (-1: none), terms [(col, op, rhs_col or -1, literal)], outputs [[(tok, arg, literal)]]."""

    def __init__(self, terms, outputs, mask_col=-1):
        self.mask_col, self.terms, self.outputs = mask_col, list(terms), [list(p) for p in outputs]


# ---- selection builders ---------------------------------------------------------------------------
def _tiles(n, T):
    return (n + T - 1) // T


def _local(n, T, block):
    """Per row: tile, stripe, wave and lane under the stripe map."""
    row = np.arange(n, dtype=np.int64)
    loc = row % T
    t = loc % block
    return row // T, loc // block, t // 64, t % 64


def sel_none(n, T, block=256, seed=0):
    return np.zeros(n, dtype=bool)


def sel_all(n, T, block=256, seed=0):
    return np.ones(n, dtype=bool)


def first_only(n, T, block=256, seed=0):
    s = np.zeros(n, dtype=bool)
    s[:1] = True
    return s


def last_only(n, T, block=256, seed=0):
    s = np.zeros(n, dtype=bool)
    s[n - 1:] = True
    return s


def tail_tile_only(n, T, block=256, seed=0):
    """Every row of the partial last tile (nothing when n is a multiple of T)."""
    s = np.zeros(n, dtype=bool)
    s[(n // T) * T:] = True
    return s


def one_per_tile(pos):
    """Exactly one row per tile, at local position 0 ("first"), the tile's last row ("last") or a
    seeded random one ("rand"): 32 consecutive tiles share one output validity word."""
    def build(n, T, block=256, seed=0):
        nt = _tiles(n, T)
        base = np.arange(nt, dtype=np.int64) * T
        rows = np.minimum(T, n - base)
        off = {"first": np.zeros(nt, dtype=np.int64), "last": rows - 1,
               "rand": np.random.default_rng(seed).integers(0, rows)}[pos]
        s = np.zeros(n, dtype=bool)
        s[base + off] = True
        return s
    return build


def alternate_tiles(n, T, block=256, seed=0):
    """Tiles alternately full (even) and empty (odd)."""
    return (np.arange(n, dtype=np.int64) // T) % 2 == 0


def count_sequence(seq):
    """Tile i selects seq[i % len(seq)] of its rows (at most what it has), spread by seed."""
    seq = np.asarray(seq, dtype=np.int64)

    def build(n, T, block=256, seed=0):
        tile = np.arange(n, dtype=np.int64) // T
        key = np.random.default_rng(seed).random(n)
        order = np.lexsort((key, tile))
        rank = np.arange(n, dtype=np.int64) - tile * T  # (sorted by tile: position inside the tile)
        s = np.zeros(n, dtype=bool)
        s[order] = rank < seq[tile % len(seq)]
        return s
    return build


def full_with_one_short(j):
    """Every tile full, except that tile j leaves one (seeded) row out: the [T] sequence with a
    single tile of T - 1."""
    def build(n, T, block=256, seed=0):
        nt = _tiles(n, T)
        seq = np.full(nt, T, dtype=np.int64)
        seq[j % nt] = min(T, n - (j % nt) * T) - 1
        return count_sequence(seq)(n, T, block, seed)
    return build


def one_wave(w):
    """Inside each tile only wave w (negative: from the last) of every stripe selects."""
    def build(n, T, block=256, seed=0):
        _, _, wave, _ = _local(n, T, block)
        return wave == (w % (block // 64))
    return build


def one_stripe(r):
    """Inside each tile only stripe r (negative: from the last) selects."""
    def build(n, T, block=256, seed=0):
        _, stripe, _, _ = _local(n, T, block)
        return stripe == (r % (T // block))
    return build


def alternate_groups(G):
    """Inside each tile, groups of G rows alternately full and empty, starting full in even tiles
    and empty in odd ones (the resident pass stores a tile group by group)."""
    def build(n, T, block=256, seed=0):
        row = np.arange(n, dtype=np.int64)
        return (row // T + (row % T) // G) % 2 == 0
    return build


def lane0_only(n, T, block=256, seed=0):
    return _local(n, T, block)[3] == 0


def lane63_only(n, T, block=256, seed=0):
    return _local(n, T, block)[3] == 63


def uniform(p):
    def build(n, T, block=256, seed=0):
        return np.random.default_rng(seed).random(n) < p
    return build


SEQ_MIXED = (1, 31, 32, 33, 0, 63)
BUILDERS = {
    "none": sel_none, "all": sel_all, "first_only": first_only, "last_only": last_only,
    "tail_tile_only": tail_tile_only,
    "one_per_tile_first": one_per_tile("first"), "one_per_tile_last": one_per_tile("last"),
    "one_per_tile_rand": one_per_tile("rand"),
    "alternate_tiles": alternate_tiles,
    "seq_31": count_sequence([31]), "seq_33": count_sequence([33]), "seq_mixed": count_sequence(SEQ_MIXED),
    "seq_123": count_sequence([1, 2, 3]), "seq_full_short": full_with_one_short(3),
    "one_wave_0": one_wave(0), "one_wave_last": one_wave(-1),
    "one_stripe_0": one_stripe(0), "one_stripe_last": one_stripe(-1),
    "lane0_only": lane0_only, "lane63_only": lane63_only,
    "uniform_01": uniform(0.01), "uniform_50": uniform(0.5), "uniform_99": uniform(0.99),
}


def tile_counts(sel, T):
    """Selected rows per tile."""
    n = len(sel)
    pad = np.zeros(_tiles(n, T) * T, dtype=np.int64)
    pad[:n] = sel
    return pad.reshape(-1, T).sum(axis=1)


def tile_bases(sel, T):
    """Output row at which each tile's rows start (exclusive prefix of the counts)."""
    c = tile_counts(sel, T)
    return np.cumsum(c) - c


# ---- plan shapes ----------------------------------------------------------------------------------
def _col(k):
    return [(TOK_COL, k, None)]


def _bin(op, x, y):
    return x + y + [(op, 0, None)]


def _lit(v):
    return [(TOK_LIT, 0, v)]


def _pred_i64(rng, sel, lit):
    """int64 values with (a > lit) == sel."""
    n = len(sel)
    d = rng.integers(0, 1 << 20, n)
    return np.where(sel, lit + 1 + d, lit - d).astype(np.int64)


def _nulls(rng, n, share=0.1):
    return rng.random(n) >= share


def shape_names():
    return ["S1", "S2", "S3", "S4", "S5", "S6", "S6v", "S7", "S8"]


def make_case(shape, sel, seed=0, T=4096, block=256):
    """(cols, spec) of plan shape `shape` ("S6v": S6 whose mask has validity) selecting exactly
    `sel`. T / block place S7's special values in whole stripes and in the tail."""
    sel = np.asarray(sel, dtype=bool)
    n = len(sel)
    rng = np.random.default_rng([seed, n, len(shape), ord(shape[1])])
    lit = int(rng.integers(-(1 << 40), 1 << 40))
    gt = lambda c: [(c, S.OP_GT, -1, lit)]
    full = lambda: rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64, endpoint=True)
    if shape in ("S1", "S2", "S3", "S5", "S8"):
        a = Col("i64", _pred_i64(rng, sel, lit))
        b = Col("i64", full(), _nulls(rng, n) if shape in ("S3", "S5") else None)
        ab = _bin(TOK_ADD, _col(0), _col(1))
        if shape == "S8":
            # a quarter of the unselected rows are null with a value that passes a > lit
            null = ~sel & (rng.random(n) < 0.25)
            a = Col("i64", np.where(null, lit + 1 + rng.integers(0, 1 << 20, n), a.values), ~null)
        outs = {"S1": [ab], "S8": [ab], "S2": [ab, _col(1)], "S3": [ab, _col(1)],
                "S5": [_col(0), _col(1), ab, _bin(TOK_SUB, _col(0), _col(1)), _bin(TOK_MUL, _col(1), _lit(3))]}[shape]
        return [a, b], Spec(gt(0), outs)
    if shape == "S4":
        def under(vals, valid, lo, hi):
            return np.where(valid, vals, np.where(rng.random(n) < 0.5, lo, hi))
        cv, dv, ev = _nulls(rng, n, 0.2), _nulls(rng, n, 0.2), _nulls(rng, n, 0.2)
        c = Col("i32", under(rng.integers(I32_MIN, I32_MAX, n, endpoint=True), cv, I32_MIN, -1), cv)
        d = Col("u8", under(rng.integers(0, 256, n), dv, 128, 255), dv)
        e = Col("date32", under(rng.integers(I32_MIN, I32_MAX, n, endpoint=True), ev, I32_MIN, -1), ev)
        return [Col("i64", _pred_i64(rng, sel, lit)), c, d, e], Spec(gt(0), [_col(1), _col(2), _col(3)])
    if shape in ("S6", "S6v"):
        y = rng.normal(size=n)
        y[rng.random(n) < 0.05] = np.nan
        y[rng.random(n) < 0.05] = -0.0
        x = Col("i64", full())
        if shape == "S6":
            m = Col("bool", sel)
        else:  # null mask rows carry value bit 1: ignoring the validity would select them
            null = ~sel & (rng.random(n) < 0.25)
            m = Col("bool", sel | null, ~null)
        return [x, Col("f64", y), m], Spec([], [_col(0), _col(1)], mask_col=2)
    if shape == "S7":
        return _make_s7(rng, sel, T, block)
    raise ValueError(shape)


S7_SPECIAL_Q = (np.nan, 0.0, -0.0, np.inf, -np.inf)


def _make_s7(rng, sel, T, block):
    """(i32 p, f64 q, i64 b): p >= plit AND q < qlit AND p < b. Each unselected row fails a random
    non-empty subset of the terms. Stripes 1, 3, 5 (mod 7) of the row range hold p = -1, INT32_MAX
    and (on their rows failing the first term) INT32_MIN throughout, and the partial last tile
    cycles through the three; q is NaN, +-0.0 or +-Inf on a fifth of the rows."""
    n = len(sel)
    plit = int(rng.integers(-1000, -1))  # -1 and INT32_MAX pass p >= plit, INT32_MIN fails
    qlit = float(rng.choice([0.0, 0.5]))
    row = np.arange(n, dtype=np.int64)
    stripe = row // block
    tail = row >= (n // T) * T
    kind = np.where(tail, row % 3, np.where(stripe % 7 == 1, 0, np.where(stripe % 7 == 3, 1,
                                                                        np.where(stripe % 7 == 5, 2, -1))))
    fail = np.where(sel, 0, rng.integers(1, 8, n))  # bit k: term k fails
    # whole stripes of -1 / INT32_MAX: their unselected rows fail through q or b, not through p
    keep1 = (kind == 0) | (kind == 1)
    fail = np.where(~sel & keep1 & (fail & 1 == 1), np.where(fail >> 1 == 0, 2, fail & 6), fail)
    # INT32_MIN stripes: every unselected row there fails through p (at least)
    fail = np.where(~sel & (kind == 2), fail | 1, fail)
    f1, f2, f3 = (fail & 1) != 0, (fail & 2) != 0, (fail & 4) != 0
    p = np.where(f1, rng.integers(I32_MIN, plit, n), rng.integers(plit, I32_MAX, n, endpoint=True)).astype(np.int64)
    p = np.where(~f1 & (kind == 0), -1, p)
    p = np.where(~f1 & (kind == 1), I32_MAX, p)
    p = np.where(f1 & (kind == 2), I32_MIN, p)
    d = rng.integers(1, 1 << 33, n)
    b = np.where(f3, p - (d - 1), p + d).astype(np.int64)  # p < b fails / passes
    mag = np.abs(rng.normal(size=n)) + 1e-3
    q = np.where(f2, qlit + mag, qlit - mag)
    special = rng.random(n) < 0.2
    sq = np.asarray(S7_SPECIAL_Q)
    with np.errstate(invalid="ignore"):
        passing, failing = sq[sq < qlit], sq[~(sq < qlit)]
    q = np.where(special & f2, rng.choice(failing, n), q)
    q = np.where(special & ~f2, rng.choice(passing, n), q)
    cols = [Col("i32", p), Col("f64", q), Col("i64", b)]
    spec = Spec([(0, S.OP_GE, -1, plit), (1, S.OP_LT, -1, qlit), (0, S.OP_LT, 2, None)],
                [_bin(TOK_ADD, _col(0), _col(2)), _col(1)])
    return cols, spec


def output_kinds(cols, spec):
    """Per output: (kind, nullable): a lone column keeps its kind and nullability; other programs
    give f64 if any operand is, else i64, and can be null if a column read can or they divide."""
    res = []
    for prog in spec.outputs:
        if len(prog) == 1 and prog[0][0] == TOK_COL:
            c = cols[prog[0][1]]
            res.append((c.kind, c.valid is not None))
            continue
        is_f = any((t == TOK_COL and cols[a].kind == "f64") or (t == TOK_LIT and isinstance(v, float)) for t, a, v in prog)
        nullable = any((t == TOK_COL and cols[a].valid is not None) or t == TOK_DIV for t, a, v in prog)
        res.append(("f64" if is_f else "i64", nullable))
    return res


# ---- references -----------------------------------------------------------------------------------
def _wrap(x):
    return ((x + (1 << 63)) % (1 << 64)) - (1 << 63)


def _cmp_row(op, x, y):
    return {S.OP_EQ: x == y, S.OP_NE: x != y, S.OP_LT: x < y, S.OP_LE: x <= y, S.OP_GT: x > y, S.OP_GE: x >= y}[op]


def _py(c, i):
    return float(c.values[i]) if c.kind == "f64" else int(c.values[i])


def select_project_rows(cols, spec):
    """Row at a time: a row is kept when the mask (if any) and every term are true, a null operand
    making the term null and the row dropped; each output program runs on a stack of (value, valid)
    with int64 wrap-around, fp64 promotion, and integer x / 0 -> null."""
    n = len(cols[0].values)
    kinds = output_kinds(cols, spec)
    vals = [[] for _ in spec.outputs]
    oks = [[] for _ in spec.outputs]
    ok = lambda c, i: c.valid is None or bool(c.valid[i])
    for i in range(n):
        keep = True
        if spec.mask_col >= 0:
            m = cols[spec.mask_col]
            keep = ok(m, i) and bool(m.values[i])
        for col, op, rhs, lit in spec.terms:
            if not keep:
                break
            if not ok(cols[col], i) or (rhs >= 0 and not ok(cols[rhs], i)):
                keep = False  # null -> dropped
                break
            x = _py(cols[col], i)
            y = _py(cols[rhs], i) if rhs >= 0 else lit
            if isinstance(x, float) or isinstance(y, float):
                x, y = float(x), float(y)
            keep = bool(_cmp_row(op, x, y))
        if not keep:
            continue
        for k, prog in enumerate(spec.outputs):
            st = []
            for t, a, v in prog:
                if t == TOK_COL:
                    st.append((_py(cols[a], i), ok(cols[a], i)))
                elif t == TOK_LIT:
                    st.append((v, True))
                else:
                    (y, yo), (x, xo) = st.pop(), st.pop()
                    if isinstance(x, float) or isinstance(y, float):
                        with np.errstate(all="ignore"):
                            x, y = np.float64(x), np.float64(y)
                            r = float({TOK_ADD: x + y, TOK_SUB: x - y, TOK_MUL: x * y}[t] if t != TOK_DIV else x / y)
                        st.append((r, xo and yo))
                    elif t == TOK_DIV:
                        if y == 0:
                            st.append((0, False))  # x / 0 -> null
                        else:
                            q = abs(x) // abs(y)
                            st.append((_wrap(q if (x < 0) == (y < 0) else -q), xo and yo))
                    else:
                        st.append((_wrap({TOK_ADD: x + y, TOK_SUB: x - y, TOK_MUL: x * y}[t]), xo and yo))
            vals[k].append(st[0][0])
            oks[k].append(st[0][1])
    return [(np.array(vals[k], dtype=_DTYPE[kinds[k][0]]), np.array(oks[k], dtype=bool)) for k in range(len(vals))]


def select_project_ref(cols, spec):
    """The same on oracle.semantics: cmp per term, select_mask, filter_columns, arith."""
    n = len(cols[0].values)
    kinds = output_kinds(cols, spec)
    sel = np.ones(n, dtype=bool)
    if spec.mask_col >= 0:
        sel &= S.select_mask(cols[spec.mask_col].values, cols[spec.mask_col].valid)
    for col, op, rhs, lit in spec.terms:
        r = cols[rhs] if rhs >= 0 else None
        m, mv = S.cmp(op, cols[col].values, cols[col].valid, r.values if r else lit, r.valid if r else None)
        sel &= S.select_mask(m, mv)
    fv = S.filter_columns(sel, None, [c.values for c in cols])
    fo = S.filter_columns(sel, None, [np.ones(n, dtype=bool) if c.valid is None else c.valid for c in cols])
    res = []
    for k, prog in enumerate(spec.outputs):
        st = []
        for t, a, v in prog:
            if t == TOK_COL:
                st.append((fv[a], fo[a]))
            elif t == TOK_LIT:
                st.append((v, None))
            else:
                (y, yo), (x, xo) = st.pop(), st.pop()
                st.append(S.arith(_ARITH[t], x, xo, y, yo))
        val, valid = st[0]
        res.append((np.asarray(val).astype(_DTYPE[kinds[k][0]]), np.asarray(valid, dtype=bool)))
    return res


def selection_of(cols, spec):
    """The boolean selection a plan makes (vectorised)."""
    n = len(cols[0].values)
    sel = np.ones(n, dtype=bool)
    if spec.mask_col >= 0:
        sel &= S.select_mask(cols[spec.mask_col].values, cols[spec.mask_col].valid)
    for col, op, rhs, lit in spec.terms:
        r = cols[rhs] if rhs >= 0 else None
        m, mv = S.cmp(op, cols[col].values, cols[col].valid, r.values if r else lit, r.valid if r else None)
        sel &= S.select_mask(m, mv)
    return sel


@functools.lru_cache(maxsize=8)
def cached_case(shape, builder, n, T, block, seed=0):
    """(sel, cols, spec, reference) of one case; shared by the tests that run it under several
    schemes, and never modified."""
    sel = BUILDERS[builder](n, T, block, seed)
    cols, spec = make_case(shape, sel, seed, T, block)
    return sel, cols, spec, select_project_ref(cols, spec)
