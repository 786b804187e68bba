"""Inputs and plain references for the unfused expression and selection kernels (K1 arithmetic,
K2 comparison, K3a boolean logic, K3b compaction): tests/test_expr_cases.py asserts on the CPU what
each data set must hold, tests/test_expr_ops.py runs the kernels on them.

Kinds name the five operand types of `load8`: "i64", "f64", "i32", "d32" (DATE32, int32 storage)
and "u8". A literal is a `Lit`; a null one has value None and keeps its type. Every builder is
seeded from its arguments (crc32, not hash()), so both test files see the same arrays.

The row_* functions are the row-at-a-time references: one Python value per row, None = null. They
restate include/qe_hip.h directly and share no code with oracle/semantics.py, which they check."""
from __future__ import annotations

import dataclasses
import itertools
import math
import zlib
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import semantics as S

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
KINDS = ("i64", "f64", "i32", "d32", "u8")
NP_DTYPE = {"i64": np.int64, "f64": np.float64, "i32": np.int32, "d32": np.int32, "u8": np.uint8}
RANGE = {"i64": (I64_MIN, I64_MAX), "i32": (I32_MIN, I32_MAX), "d32": (I32_MIN, I32_MAX), "u8": (0, 255),
         "f64": (-(1 << 31), 1 << 31)}  # fp64: the integers used where a pair needs equal values
SIGNED = ("i64", "i32", "d32")
# One thread takes 8 rows, one block 2,048: every path of load8 / store8 (vector, scalar tail, none)
# in the first and in a second block.
SIZES = [0, 1, 7, 8, 9, 2047, 2048, 2049, 2055]
MATRIX_N = 2055
SIZE_PAIRS = [("i32", "i32"), ("u8", "i64"), ("i32", "f64")]
ARITH_OPS = [S.OP_ADD, S.OP_SUB, S.OP_MUL, S.OP_DIV]
CMP_OPS = [S.OP_EQ, S.OP_NE, S.OP_LT, S.OP_LE, S.OP_GT, S.OP_GE]
BOOL_OPS = [S.OP_AND, S.OP_OR, S.OP_NOT, S.OP_IS_NULL, S.OP_IS_NOT_NULL]
NULL_COMBOS = [(True, True), (True, False), (False, True), (False, False)]

# Values a missing sign extension, a wrong zero extension or an unsigned compare would change.
EDGES = {
    "i64": [I64_MIN, -1, 0, I64_MAX, 1, -7, 7, 2, -2, I32_MIN, I32_MAX + 1, (1 << 53) + 1],
    "i32": [I32_MIN, -1, 0, I32_MAX, 1, -7, 7, 2, -2],
    "u8": [0, 127, 128, 255, 1, 7, 2],
    "f64": [math.nan, -0.0, 0.0, math.inf, -math.inf, 1.5, -7.0, 7.0, 2.0, -2.0, -1.0, 2.0 ** 53, 5e-324],
}
EDGES["d32"] = EDGES["i32"]
TAIL_EDGE = {"i64": I64_MIN, "i32": I32_MIN, "d32": -1, "u8": 255, "f64": -0.0}


def rng_for(*parts) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(repr(parts).encode()))


@dataclasses.dataclass(frozen=True)
class Lit:
    value: Any  # int, float or None (null)
    is_f64: bool

    def __repr__(self) -> str:
        return f"{'null' if self.value is None else self.value!r}:{'f64' if self.is_f64 else 'i64'}"


LITERALS = [Lit(7, False), Lit(-1, False), Lit(0, False), Lit(I64_MAX, False), Lit(I64_MIN, False),
            Lit(100.0, True), Lit(1.5, True), Lit(math.nan, True), Lit(-0.0, True), Lit(math.inf, True),
            Lit(-math.inf, True), Lit(None, False), Lit(None, True)]


def ref_operand(x):
    """The oracle's form of an operand: arrays as they are, literals as int / float / NullLiteral."""
    if isinstance(x, Lit):
        if x.value is None:
            return S.NULL_F64 if x.is_f64 else S.NULL_I64
        return float(x.value) if x.is_f64 else int(x.value)
    return x


# ---- columns ---------------------------------------------------------------------------------------
def validity(n: int, rng, null_rate: float = 0.15) -> np.ndarray:
    return rng.random(n) >= null_rate


def column(kind: str, n: int, rng) -> np.ndarray:
    """Full-range random values with the kind's edge values on every third row (each edge in
    vector groups and, at the sizes used, in the scalar tail) and TAIL_EDGE in the last row."""
    dt = NP_DTYPE[kind]
    if kind == "f64":
        v = rng.normal(size=n) * 1000.0
        whole = rng.random(n) < 0.3
        v[whole] = np.round(v[whole])
    else:
        lo, hi = RANGE[kind]
        v = rng.integers(lo, hi, n, dtype=dt, endpoint=True)
    e = np.array(EDGES[kind], dtype=dt)
    rows = np.nonzero(np.arange(n) % 3 == 1)[0]
    v[rows] = e[(rows // 3) % len(e)]
    if n:
        v[n - 1] = TAIL_EDGE[kind]
    return v.astype(dt)


def _plant(a, av, b, bv, rows):
    """Writes (x, y) pairs as valid rows near the start (a vector group when n >= 8) and, from 16
    rows on, again at the end (the tail group)."""
    n = len(a)
    if n < len(rows):
        return
    for k, (x, y) in enumerate(rows):
        spots = [k + (1 if n > len(rows) else 0)] + ([n - 1 - k] if n >= 16 else [])
        for i in spots:
            a[i], b[i] = x, y
            av[i] = bv[i] = True


def div_rows(kl: str, kr: str) -> Dict[str, Tuple[int, int]]:
    """The integer DIV rows a pair of kinds can hold: x / 0 always; MIN / -1 when both sides are
    signed; a quotient that truncates toward zero, negative when either side is signed."""
    rows = {"by_zero": (7, 0)}
    if kl in SIGNED and kr in SIGNED:
        rows["min_by_minus_one"] = (RANGE[kl][0], -1)
    if kl in SIGNED:
        rows["truncating"] = (-7, 2)
    elif kr in SIGNED:
        rows["truncating"] = (7, -2)
    else:
        rows["truncating"] = (7, 2)
    return rows


def arith_pair(kl: str, kr: str, n: int):
    """(a, av, b, bv) for K1. Integer pairs carry div_rows()."""
    rng = rng_for("arith", kl, kr, n)
    a, b = column(kl, n, rng), column(kr, n, rng)
    av, bv = validity(n, rng), validity(n, rng)
    if "f64" not in (kl, kr):
        _plant(a, av, b, bv, list(div_rows(kl, kr).values()))
    return a, av, b, bv


def int64_cmp_pair(n: int):
    """Full-range int64: b == a on a quarter, a +- 1 on a quarter, the opposite sign on a quarter,
    random on the rest; (INT64_MIN, INT64_MAX) in both orders."""
    rng = rng_for("cmp64", n)
    a = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    b = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    cls = rng.integers(0, 4, n)
    b[cls == 0] = a[cls == 0]
    near = cls == 1
    a[near] = np.clip(a[near], I64_MIN + 1, I64_MAX - 1)
    b[near] = a[near] + rng.choice(np.array([-1, 1], dtype=np.int64), int(near.sum()))
    b[cls == 2] = ~a[cls == 2]
    av, bv = validity(n, rng), validity(n, rng)
    _plant(a, av, b, bv, [(I64_MIN, I64_MAX), (I64_MAX, I64_MIN)])
    return a, av, b, bv


def cmp_pair(kl: str, kr: str, n: int):
    """(a, av, b, bv) for K2: on 30 % of the rows b == a, on 25 % each b == a + 1 and b == a - 1
    (values both kinds hold exactly), the rest independent with the kinds' edges."""
    if kl == kr == "i64":
        return int64_cmp_pair(n)
    rng = rng_for("cmp", kl, kr, n)
    lo = max(RANGE[kl][0], RANGE[kr][0]) + 1
    hi = min(RANGE[kl][1], RANGE[kr][1]) - 1
    v = rng.integers(lo, hi, n, dtype=np.int64, endpoint=True)
    v[rng.random(n) < 0.5] //= (1 << 20) if hi > (1 << 24) else 1  # some small magnitudes too
    v = np.clip(v, lo, hi)
    cls = rng.integers(0, 20, n)
    d = np.where(cls < 6, 0, np.where(cls < 11, 1, -1))
    a = v.astype(NP_DTYPE[kl])
    b = (v + d).astype(NP_DTYPE[kr])
    free = cls >= 16
    a[free] = column(kl, n, rng)[free]
    b[free] = column(kr, n, rng)[free]
    av, bv = validity(n, rng), validity(n, rng)
    if kl == kr == "f64":
        _plant(a, av, b, bv, [(0.0, -0.0), (math.nan, math.nan), (math.inf, math.inf), (math.nan, 1.0)])
    return a, av, b, bv


def literal_admits_all(kind: str, lit: Lit) -> bool:
    """Whether a column of `kind` can be below, equal to and above the literal."""
    if lit.value is None or not math.isfinite(lit.value):
        return False
    if kind != "f64" and float(lit.value) != math.floor(lit.value):
        return False
    lo, hi = (I64_MIN, I64_MAX) if kind == "f64" else RANGE[kind]
    return lo + 1 <= lit.value <= hi - 1


def column_around(kind: str, lit: Lit, n: int):
    """(a, av): 30 % of the rows equal to the literal, 25 % each just below and just above it (or
    around 1 where the kind cannot hold the literal), the rest column()."""
    rng = rng_for("around", kind, repr(lit), n)
    a = column(kind, n, rng)
    if literal_admits_all(kind, lit):
        if kind == "f64":
            c = float(lit.value)
            trio = [np.nextafter(c, -math.inf), c, np.nextafter(c, math.inf)]
        else:
            trio = [int(lit.value) - 1, int(lit.value), int(lit.value) + 1]
    else:
        trio = [0, 1, 2]
    cls = rng.integers(0, 20, n)
    dt = NP_DTYPE[kind]
    a[cls < 6] = dt(trio[1])
    a[(cls >= 6) & (cls < 11)] = dt(trio[0])
    a[(cls >= 11) & (cls < 16)] = dt(trio[2])
    return a, validity(n, rng)


def mixed_precision_pairs(n: int):
    """int64 against fp64 around 2^53 and 2^63, where the conversion to fp64 rounds: the header
    pins "compares as fp64", so 2^53 + 1 equals float(2^53). Returns (ints, doubles), the pair list
    repeated to n rows (39 pairs: no multiple of 8, so the pairs move through the lanes)."""
    p53 = 1 << 53
    near = [float(p53), float(p53 + 2), float(p53 - 1)]
    pairs = []
    for k in range(-2, 3):
        pairs += [(p53 + k, d) for d in near]
        pairs += [(-p53 - k, -d) for d in near]
    pairs += [(I64_MAX, 2.0 ** 63), (I64_MIN, -(2.0 ** 63)), (I64_MAX, -(2.0 ** 63)), (I64_MIN, 2.0 ** 63)]
    pairs += [(p53, math.nan), (-p53, math.nan), (I64_MAX, math.nan), (I64_MIN, math.nan), (0, math.nan)]
    ints = np.resize(np.array([p[0] for p in pairs], dtype=np.int64), n)
    dbls = np.resize(np.array([p[1] for p in pairs], dtype=np.float64), n)
    return ints, dbls


def outcome_shares(a, av, b, bv) -> Tuple[float, float, float]:
    """Shares of <, = and > among the valid rows, by the oracle."""
    _, v = S.cmp(S.OP_EQ, a, av, b, bv)
    nv = max(int(v.sum()), 1)
    return tuple(float(S.cmp(op, a, av, b, bv)[0].sum()) / nv for op in (S.OP_LT, S.OP_EQ, S.OP_GT))


# ---- row-at-a-time references -------------------------------------------------------------------------
def rows_of(x, valid, n: int) -> List[Any]:
    """One Python value per row: int (widened by value), float, or None for a null row."""
    if isinstance(x, Lit):
        return [x.value if x.value is None else (float(x.value) if x.is_f64 else int(x.value))] * n
    vals = x.tolist()
    return [v if (valid is None or valid[i]) else None for i, v in enumerate(vals)]


def is_f64(x) -> bool:
    return x.is_f64 if isinstance(x, Lit) else x.dtype == np.float64


def _wrap64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def row_arith(op: int, x, y, f64: bool):
    if x is None or y is None:
        return None
    if f64:
        fx, fy = np.float64(x), np.float64(y)  # (an integer converts rounding to nearest even)
        with np.errstate(all="ignore"):
            return float({S.OP_ADD: fx + fy, S.OP_SUB: fx - fy, S.OP_MUL: fx * fy, S.OP_DIV: fx / fy}[op])
    if op == S.OP_ADD:
        return _wrap64(x + y)
    if op == S.OP_SUB:
        return _wrap64(x - y)
    if op == S.OP_MUL:
        return _wrap64(x * y)
    if y == 0:
        return None
    q = abs(x) // abs(y)  # truncation toward zero
    return _wrap64(q if (x < 0) == (y < 0) else -q)


def row_cmp(op: int, x, y, f64: bool):
    if x is None or y is None:
        return None
    if f64:
        x, y = float(np.float64(x)), float(np.float64(y))
    return {S.OP_EQ: x == y, S.OP_NE: x != y, S.OP_LT: x < y, S.OP_LE: x <= y, S.OP_GT: x > y,
            S.OP_GE: x >= y}[op]


def row_cmp_utf8(op: int, x: Optional[bytes], lit: Optional[bytes]):
    if x is None or lit is None:
        return None
    return (x == lit) if op == S.OP_EQ else (x != lit)


def row_bool(op: int, x, y=None):
    """SQL three-valued logic on True / False / None."""
    if op == S.OP_NOT:
        return None if x is None else not x
    if op == S.OP_IS_NULL:
        return x is None
    if op == S.OP_IS_NOT_NULL:
        return x is not None
    if op == S.OP_AND:
        if x is False or y is False:
            return False
        return None if (x is None or y is None) else True
    if x is True or y is True:
        return True
    return None if (x is None or y is None) else False


def rows_result(rows: Sequence[Any], dtype) -> Tuple[np.ndarray, np.ndarray]:
    """(values, valid) arrays of a row-loop result; null rows hold 0."""
    valid = np.array([r is not None for r in rows], dtype=bool)
    vals = np.array([0 if r is None else r for r in rows], dtype=dtype) if len(rows) else np.zeros(0, dtype=dtype)
    return vals, valid


def same_f64(a: np.ndarray, b: np.ndarray) -> bool:
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


# ---- UTF-8 ----------------------------------------------------------------------------------------
UTF8_SIZES = [1, 8, 9, 2049]
UTF8_LITERALS = {"empty": b"", "ca": b"CA", "long40": b"0123456789abcdefghijABCDEFGHIJ!#%&/()=?+",
                 "multibyte": "Pärsson".encode()}
assert len(UTF8_LITERALS["long40"]) == 40 and len(UTF8_LITERALS["multibyte"]) == 8


def utf8_classes(lit: bytes) -> Dict[str, List[Optional[bytes]]]:
    """The value classes around a literal (a cut inside a code point is a prefix too: the kernel
    compares bytes)."""
    c: Dict[str, List[Optional[bytes]]] = {"null": [None], "empty": [b""], "lit": [lit], "plus": [lit + b"x"]}
    if len(lit) > 1:
        c["prefix"] = [lit[:k] for k in range(1, len(lit))]
    if lit:
        c["changed"] = [lit[:-1] + bytes([lit[-1] ^ 1])]
    return c


def utf8_values(lit: bytes, n: int) -> List[Optional[bytes]]:
    """Round-robin over the classes (so every group of 8 rows, one validity byte, mixes nulls,
    equal and unequal values), the prefixes taken in turn; from 9 rows on, the rows of a tail group
    end in nulls. One row: the literal itself."""
    classes = utf8_classes(lit)
    names = list(classes)
    out: List[Optional[bytes]] = []
    for i in range(n):
        vals = classes[names[i % len(names)]]
        out.append(vals[(i // len(names)) % len(vals)])
    if n == 1:
        out[0] = lit
    if n >= 9 and n % 8:
        out[n - 1] = None
        if n % 8 >= 2:
            out[n - 2] = None
    return out


def utf8_class_of(v: Optional[bytes], lit: bytes) -> str:
    for name, vals in utf8_classes(lit).items():
        if name != "empty" and v in vals:
            return name
    return "empty" if v == b"" else "other"


def utf8_arrays(values: Sequence[Optional[bytes]], null_bytes: bytes = b""):
    """(offsets int32[n + 1], bytes uint8, valid bool[n]); a null row spans `null_bytes`."""
    enc = [null_bytes if v is None else v for v in values]
    offs = np.zeros(len(enc) + 1, dtype=np.int32)
    if enc:
        offs[1:] = np.cumsum([len(e) for e in enc])
    data = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy()
    return offs, data, np.array([v is not None for v in values], dtype=bool)


def utf8_from_pool(pool: Sequence[bytes], idx: np.ndarray):
    """(offsets, bytes) of the column pool[idx[i]], built without a Python loop over the rows."""
    width = max(max(len(p) for p in pool), 1)
    mat = np.zeros((len(pool), width), dtype=np.uint8)
    for k, p in enumerate(pool):
        mat[k, :len(p)] = np.frombuffer(p, dtype=np.uint8)
    lens = np.array([len(p) for p in pool], dtype=np.int64)[idx]
    offs = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    assert offs[-1] < 1 << 31
    keep = np.arange(width)[None, :] < lens[:, None]
    data = mat[idx][keep]
    if data.size == 0:
        data = np.zeros(1, dtype=np.uint8)
    return offs.astype(np.int32), data


# ---- K3a ------------------------------------------------------------------------------------------
BOOL_SIZES = [1, 8, 9, 2049]


def bool_pair(n: int, left_nullable: bool, right_nullable: bool):
    """(a, av, b, bv): every combination of the operands' states (true / false, and null where the
    side is nullable) in each run of len(combinations) rows, permuted; av / bv None for a side
    without validity. The value bit under a null is random: the kernel must not read it."""
    rng = rng_for("bool", n, left_nullable, right_nullable)
    sa = [True, False] + ([None] if left_nullable else [])
    sb = [True, False] + ([None] if right_nullable else [])
    combos = list(itertools.product(sa, sb))
    rows = []
    while len(rows) < n:
        rows += [combos[i] for i in rng.permutation(len(combos))]
    rows = rows[:n]
    junk = rng.random((2, n)) < 0.5
    a = np.array([junk[0][i] if r[0] is None else r[0] for i, r in enumerate(rows)], dtype=bool)
    b = np.array([junk[1][i] if r[1] is None else r[1] for i, r in enumerate(rows)], dtype=bool)
    av = np.array([r[0] is not None for r in rows], dtype=bool) if left_nullable else None
    bv = np.array([r[1] is not None for r in rows], dtype=bool) if right_nullable else None
    return a, av, b, bv


def state_shares(r: np.ndarray, v: np.ndarray) -> Tuple[float, float, float]:
    n = max(len(r), 1)
    return float((r & v).sum()) / n, float((~r & v).sum()) / n, float((~v).sum()) / n


# ---- K3b ------------------------------------------------------------------------------------------
TILE = 8192
# (counts per tile, rows after the last whole tile, selected rows among those): the cases of
# flush_valid_bits, whose words are 32 output rows
TILE_VECTORS = {
    "aligned": ((32, 64, 5), 5, 0),            # tiles start on word boundaries
    "inside_word": ((31, 1, 40), 5, 0),        # a tile wholly inside a word it shares on both sides
    "empty_middle": ((33, 0, 5), 5, 0),        # an empty tile between two that share a word
    "all": ((8192, 8192, 5), 5, 0),            # everything selected in whole tiles: plain stores only
    "ones": ((1, 1, 1), 5, 0),
    "none": ((0, 0, 0), 5, 0),                 # total 0
    "boundary_then_tail": ((45, 19, 0), 5, 5),  # ends on a word boundary, then a partial tile
    "light_after_heavy": ((8191,), 40, 40),    # a short tile's bits in the last word of a full one
}


def mask_with_tile_counts(counts: Sequence[int], tail: int, seed=0, tail_selected: int = 0, nullable: bool = False):
    """(mask, mask_valid or None) of len(counts) * TILE + tail rows: tile t selects exactly
    counts[t] rows (the partial tile tail_selected), spread by a seeded permutation. With
    `nullable`, the unselected rows are false, null-over-true or null-over-false in equal parts."""
    rng = rng_for("mask", tuple(counts), tail, seed, tail_selected)
    n = len(counts) * TILE + tail
    sel = np.zeros(n, dtype=bool)
    for t, c in enumerate(list(counts) + [tail_selected]):
        rows = TILE if t < len(counts) else tail
        assert 0 <= c <= rows
        sel[t * TILE + rng.permutation(rows)[:c]] = True
    if not nullable:
        return sel, None
    kind = rng.integers(0, 3, n)
    valid = sel | (kind == 0)
    mask = sel | (~valid & (kind == 1))
    return mask, valid


def tile_counts(mask, mask_valid, ntiles: int) -> List[int]:
    sel = S.select_mask(mask, mask_valid)
    return [int(sel[t * TILE:(t + 1) * TILE].sum()) for t in range(ntiles + 1)]


def gathered_validity(sel: np.ndarray, phase: int, seed=0) -> np.ndarray:
    """Validity of a gathered column: about half set, and in OUTPUT order a run of 40 equal bits
    centred on every tile's first selected row (ones or zeros by the parity of tile + phase), so
    the words two tiles share hold a known pattern on both sides of the seam."""
    rng = rng_for("gv", len(sel), int(sel.sum()), phase, seed)
    n = len(sel)
    total = int(sel.sum())
    out = rng.random(total) < 0.5
    starts = np.cumsum([0] + [int(sel[t:t + TILE].sum()) for t in range(0, n, TILE)])
    for i, p in enumerate(starts[:-1].tolist() + [total]):
        out[max(p - 20, 0):min(p + 20, total)] = (i + phase) % 2 == 0
    valid = rng.random(n) < 0.5
    valid[sel] = out
    return valid


FIXED_FILTER_COLUMNS = [  # (name, kind, nullable): 8 columns, the most one call takes
    ("i64n", "i64", True), ("f64n", "f64", True), ("i32n", "i32", True), ("d32n", "d32", True), ("u8n", "u8", True),
    ("i64", "i64", False), ("i32", "i32", False), ("u8", "u8", False)]
UTF8_POOL = [b"", b"x" * 40, b"a", "Pärsson".encode(), b"Uppsala", b"CA", b"0123456789" * 4, b"\xf0\x9f\x99\x82"]


def filter_inputs(sel: np.ndarray, seed=0):
    """{name: (kind, values, valid or None)} for FIXED_FILTER_COLUMNS, and three UTF-8 columns
    {name: (offsets, bytes, valid or None, per-row pool index)} (two nullable, one not) over
    UTF8_POOL: empty strings, 40-byte strings, and null rows that still span their bytes."""
    n = len(sel)
    fixed = {}
    for phase, (name, kind, nullable) in enumerate(FIXED_FILTER_COLUMNS):
        rng = rng_for("fcol", name, n, seed)
        fixed[name] = (kind, column(kind, n, rng), gathered_validity(sel, phase, seed) if nullable else None)
    utf8 = {}
    for phase, (name, nullable) in enumerate([("s0n", True), ("s1n", True), ("s2", False)]):
        rng = rng_for("scol", name, n, seed)
        idx = rng.integers(0, len(UTF8_POOL), n)
        offs, data = utf8_from_pool(UTF8_POOL, idx)
        utf8[name] = (offs, data, gathered_validity(sel, phase + 1, seed) if nullable else None, idx)
    return fixed, utf8


# ---- the composed predicate ((a > k) AND NOT (s = 'CA')) OR (c IS NULL) --------------------------------
PREDICATE_N = 16_389
PREDICATE_K = 1000


def predicate_batch():
    """a: nullable INT32 around k; s: UTF-8 with nulls, 'CA' on a third of the rows and its
    neighbours 'C' / 'CAX' / ''; c: nullable FLOAT64; two payload columns."""
    n = PREDICATE_N
    rng = rng_for("predicate", n)
    a, av = column_around("i32", Lit(PREDICATE_K, False), n)
    pool = [b"CA", b"C", b"CAX", b"", b"NY", b"ca"]
    sidx = rng.integers(0, len(pool), n)
    sidx[rng.random(n) < 0.25] = 0
    s = [pool[i] for i in sidx]
    snull = rng.random(n) < 0.15
    s = [None if z else v for v, z in zip(s, snull)]
    c = column("f64", n, rng)
    cv = rng.random(n) >= 0.3
    pay_i = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    pay_s = [pool[i] + str(j % 97).encode() for j, i in enumerate(rng.integers(0, len(pool), n))]
    return dict(a=a, av=av, s=s, c=c, cv=cv, pay_i=pay_i, pay_s=pay_s)


def predicate_rows(b) -> np.ndarray:
    """Row at a time, three-valued: the rows SelectionExec keeps (predicate true; null drops)."""
    keep = np.zeros(len(b["a"]), dtype=bool)
    for i in range(len(keep)):
        a = int(b["a"][i]) if b["av"][i] else None
        s = b["s"][i]
        c_is_null = not b["cv"][i]
        gt = row_cmp(S.OP_GT, a, PREDICATE_K, False)
        eq = row_cmp_utf8(S.OP_EQ, s, b"CA")
        p = row_bool(S.OP_OR, row_bool(S.OP_AND, gt, row_bool(S.OP_NOT, eq)), c_is_null)
        keep[i] = p is True
    return keep
