"""CPU reference of the window functions (qe_window_boundaries / qe_window_eval), test
infrastructure only. oracle/ has no window semantics, so they are restated here, twice:

  * fold(): the literal statement. The rows are walked in the order of sortref.order over (partition
    keys ascending, then order keys), cut into partitions and peer groups with sortref.compare, and
    every aggregate is the row-at-a-time fold of oracle/semantics.py's accumulator classes over the
    partition's rows in window order: the value after row e is the frame [partition start, e].
  * vectorised(): numpy over whole columns. Boundaries from sortref.key_columns' encodings, indices
    from running maxima / minima, SUM / COUNT from wrapping prefix sums, MIN / MAX from a running
    arg-extreme of value ranks.

A column is (type_id, values, valid) as in sortref: values a numpy array (or a list of bytes for
UTF8), valid a bool array or None. A function is (fn, frame, input index, offset). A result is
(values, valid): values in the output type with 0 at null rows, valid a bool array.

Also the argument rules of qe_window_plan.hpp (check, scans, work_bytes) and the known-answer
vectors of tests/golden/window_kat.json.
"""
import json
import pathlib

import numpy as np

import sortref as R
from oracle import semantics as S

(ROW_NUMBER, RANK, DENSE_RANK, COUNT_STAR, COUNT, SUM, MIN, MAX, LAG, LEAD) = range(1, 11)
ROWS, RANGE, PARTITION = 0, 1, 2
FN_NAMES = {"row_number": ROW_NUMBER, "rank": RANK, "dense_rank": DENSE_RANK, "count_star": COUNT_STAR, "count": COUNT,
            "sum": SUM, "min": MIN, "max": MAX, "lag": LAG, "lead": LEAD}
FRAME_NAMES = {"rows": ROWS, "range": RANGE, "partition": PARTITION}
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -2
MAX_AGGS = 8
VALUE_TYPES = (R.TYPE_INT64, R.TYPE_FLOAT64, R.TYPE_INT32, R.TYPE_DATE32, R.TYPE_UINT8)
ALL_TYPES = VALUE_TYPES + (R.TYPE_BOOL, R.TYPE_UTF8)
CANON_NAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
KAT = pathlib.Path(__file__).resolve().parent / "golden" / "window_kat.json"


# ---- argument rules (qe_window_plan.hpp) ------------------------------------------------------------
def takes_input(fn):
    return fn in (COUNT, SUM, MIN, MAX, LAG, LEAD)


def nullable(fn):
    return fn in (SUM, MIN, MAX, LAG, LEAD)


def check(fn, frame, in_type, offset):
    """(status, output type) of one function; the type is 0 when it is refused."""
    if fn not in range(ROW_NUMBER, LEAD + 1) or frame not in (ROWS, RANGE, PARTITION):
        return INVALID_ARG, 0
    if fn in (LAG, LEAD) and offset < 0:
        return INVALID_ARG, 0
    if not takes_input(fn):
        return OK, R.TYPE_INT64
    if in_type not in ALL_TYPES:
        return INVALID_ARG, 0
    if fn == COUNT:
        return OK, R.TYPE_INT64
    if fn == SUM:
        return (OK, R.TYPE_INT64) if in_type in (R.TYPE_INT64, R.TYPE_INT32) else (UNSUPPORTED, 0)
    return (OK, in_type) if in_type in VALUE_TYPES else (UNSUPPORTED, 0)


def scans(fns):
    """The distinct (scan kind, input) pairs in order of first use (1 SUM and COUNT(x), 2 MIN, 3 MAX),
    and each function's index into them (-1: none)."""
    kind_of = {COUNT: 1, SUM: 1, MIN: 2, MAX: 3}
    found, of_fn = [], []
    for fn, _, inp, _ in fns:
        if fn not in kind_of:
            of_fn.append(-1)
            continue
        pair = (kind_of[fn], inp)
        if pair not in found:
            found.append(pair)
        of_fn.append(found.index(pair))
    return found, of_fn


def _a256(x):
    return (x + 255) // 256 * 256


def work_bytes(n, nscans, nfns, tile_rows):
    """Working memory of one qe_window_eval: the flag's head, the inverse permutation, five word
    arrays, (values, counts / flags) per scan, the tile aggregates and carries of every scan, and
    the staging records (per position: every function's value and one word of validity bits)."""
    words, tiles = (n + 31) // 32, (n + tile_rows - 1) // tile_rows
    return (256 + _a256(4 * n) + 5 * _a256(4 * words) + nscans * (_a256(8 * n) + _a256(4 * n))
            + 2 * _a256((5 + nscans) * (tiles + 1) * 16) + _a256(8 * n * (nfns + 1)))


# ---- shared helpers ---------------------------------------------------------------------------------
def _n_rows(part, order, inputs, n):
    for cols in (part, order, inputs):
        for _, values, _ in cols:
            return len(values)
    return n


def window_order(part, order, flags, n):
    keys = list(part) + list(order)
    if not keys:
        return np.arange(n, dtype=np.int32)
    return R.order(keys, [0] * len(part) + list(flags))


def _out_dtype(fn, in_type):
    return R.NP_DTYPE[in_type] if fn in (MIN, MAX, LAG, LEAD) else np.int64


def _cell(col, r):
    t, values, valid = col
    if valid is not None and not valid[r]:
        return None
    if t == R.TYPE_UTF8:
        return bytes(values[r])
    return float(values[r]) if t == R.TYPE_FLOAT64 else int(values[r]) if t != R.TYPE_BOOL else bool(values[r])


def _put(out, ok, r, fn, value):
    if value is None:
        return
    ok[r] = True
    if out.dtype == np.float64:
        out[r] = CANON_NAN if value != value else value
    else:
        out[r] = value


# ---- the literal statement --------------------------------------------------------------------------
def fold(part, order, flags, inputs, fns, n=0):
    n = _n_rows(part, order, inputs, n)
    perm = window_order(part, order, flags, n)
    results = []
    for fn, _, inp, _ in fns:
        results.append((np.zeros(n, dtype=_out_dtype(fn, inputs[inp][0] if takes_input(fn) else 0)), np.zeros(n, dtype=bool)))

    def same(cols, fl, a, b):
        return all(R.compare(c[0], _cell(c, a), _cell(c, b), f) == 0 for c, f in zip(cols, fl))

    start = 0
    while start < n:
        end = start + 1
        while end < n and same(part, [0] * len(part), perm[end - 1], perm[end]):
            end += 1
        rows = [int(r) for r in perm[start:end]]
        L = len(rows)
        peer_first, peer_last, dense = [0] * L, [0] * L, [0] * L
        g0, ordinal = 0, 1
        for j in range(1, L + 1):
            if j == L or not same(order, flags, rows[j - 1], rows[j]):
                for q in range(g0, j):
                    peer_first[q], peer_last[q], dense[q] = g0, j - 1, ordinal
                g0, ordinal = j, ordinal + 1
        for k, (fn, frame, inp, off) in enumerate(fns):
            out, ok = results[k]
            ends = [j if frame == ROWS else peer_last[j] if frame == RANGE else L - 1 for j in range(L)]
            if fn in (ROW_NUMBER, RANK, DENSE_RANK, COUNT_STAR):
                for j, r in enumerate(rows):
                    _put(out, ok, r, fn, {ROW_NUMBER: j + 1, RANK: peer_first[j] + 1, DENSE_RANK: dense[j],
                                          COUNT_STAR: ends[j] + 1}[fn])
            elif fn in (LAG, LEAD):
                for j, r in enumerate(rows):
                    q = j - off if fn == LAG else j + off
                    if 0 <= q < L:
                        _put(out, ok, r, fn, _cell(inputs[inp], rows[q]))
            else:
                acc = {COUNT: lambda: S.CountAccumulator(False), SUM: lambda: S.SumAccumulator(False),
                       MIN: S.MinAccumulator, MAX: S.MaxAccumulator}[fn]()
                after = []  # after[e]: the fold over the partition's rows 0 .. e
                for r in rows:
                    acc.accumulate(_cell(inputs[inp], r))
                    after.append(acc.finalValue())
                for j, r in enumerate(rows):
                    _put(out, ok, r, fn, after[ends[j]])
        start = end
    return results


# ---- the vectorised statement -----------------------------------------------------------------------
def starts(keys, flags, perm):
    """Bit i: position i of perm starts a run of rows equal on every key."""
    n = len(perm)
    out = np.zeros(n, dtype=bool)
    if n:
        out[0] = True
    for (t, values, valid), f in zip(keys, flags):
        for col in R.key_columns(t, values, valid, f):
            c = col[perm]
            out[1:] |= c[1:] != c[:-1]
    return out


def vectorised(part, order, flags, inputs, fns, n=0):
    n = _n_rows(part, order, inputs, n)
    perm = window_order(part, order, flags, n)
    idx = np.arange(n, dtype=np.int64)
    ps = starts(part, [0] * len(part), perm)
    gs = starts(list(part) + list(order), [0] * len(part) + list(flags), perm)
    if n == 0:
        return [(np.zeros(0, dtype=_out_dtype(fn, inputs[inp][0] if takes_input(fn) else 0)), np.zeros(0, dtype=bool))
                for fn, _, inp, _ in fns]
    P = np.maximum.accumulate(np.where(ps, idx, 0))
    G = np.maximum.accumulate(np.where(gs, idx, 0))
    nxt = np.append(np.where(ps, idx, n)[1:], n)  # the next partition start after i
    Pe = np.minimum.accumulate(nxt[::-1])[::-1] - 1
    nxt = np.append(np.where(gs, idx, n)[1:], n)
    Ge = np.minimum.accumulate(nxt[::-1])[::-1] - 1
    cg = np.cumsum(gs)
    seg = np.cumsum(ps) - 1
    results = []
    for fn, frame, inp, off in fns:
        e = idx if frame == ROWS else Ge if frame == RANGE else Pe
        ok = np.ones(n, dtype=bool)
        if takes_input(fn):
            t, values, valid = inputs[inp]
            v = (np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool))[perm]
            cnt = np.concatenate([[0], np.cumsum(v)])
            have = cnt[e + 1] - cnt[P]
        if fn == ROW_NUMBER:
            val = idx - P + 1
        elif fn == RANK:
            val = G - P + 1
        elif fn == DENSE_RANK:
            val = cg - cg[P] + 1
        elif fn == COUNT_STAR:
            val = e - P + 1
        elif fn == COUNT:
            val = have
        elif fn == SUM:
            x = np.where(v, np.asarray(values)[perm].astype(np.int64), 0).view(np.uint64)
            run = np.concatenate([[np.uint64(0)], np.cumsum(x, dtype=np.uint64)])
            val = (run[e + 1] - run[P]).view(np.int64)
            ok = have > 0
        elif fn in (MIN, MAX):
            x = np.asarray(values)[perm]
            nan = v & (x != x) if t == R.TYPE_FLOAT64 else np.zeros(n, dtype=bool)
            num = v & ~nan
            # the partition's first non-null position at or before i (-1: none yet): is it a NaN?
            first = v & (cnt[1:] - cnt[P] == 1)
            seed = np.maximum.accumulate(np.where(first, idx, -1))
            seed_nan = (seed >= P) & nan[np.maximum(seed, 0)]
            # running arg-extreme of (rank of the value, position): equal values (-0.0 == +0.0) share a
            # rank, and the earliest position wins; partitions are kept apart by an offset per partition
            _, rank = np.unique(np.where(num, x, x[num][0] if num.any() else 0), return_inverse=True)
            rank = rank.astype(np.int64).reshape(n)
            span = (int(rank.max()) + 2) * n
            if fn == MIN:
                y = np.where(num, rank * n + idx, span - 1) - seg * span
                best = np.minimum.accumulate(y) + seg * span
                pos = best % n
            else:
                y = np.where(num, rank * n + (n - 1 - idx), -1) + seg * span
                best = np.maximum.accumulate(y) - seg * span
                pos = n - 1 - best % n
            ok = have > 0
            val = np.where(seed_nan[e], CANON_NAN, x[pos[e]]) if t == R.TYPE_FLOAT64 else x[pos[e]]
        else:
            inside = (off <= idx - P) if fn == LAG else (off <= Pe - idx)
            q = np.where(inside, idx - off if fn == LAG else idx + off, 0)
            ok = inside & v[q]
            val = np.asarray(values)[perm][q]
        out = np.zeros(n, dtype=_out_dtype(fn, inputs[inp][0] if takes_input(fn) else 0))
        okr = np.zeros(n, dtype=bool)
        out[perm] = np.where(ok, val, 0).astype(out.dtype)
        okr[perm] = ok
        results.append((out, okr))
    return results


def same_results(a, b):
    """Exact: equal validity, and equal bits at the valid rows and the zeros at the null ones."""
    if len(a) != len(b):
        return False
    for (va, oa), (vb, ob) in zip(a, b):
        if va.dtype != vb.dtype or not np.array_equal(oa, ob):
            return False
        bits = {8: np.uint64, 4: np.uint32, 1: np.uint8}[va.dtype.itemsize]
        if not np.array_equal(va.view(bits), vb.view(bits)):
            return False
    return True


# ---- known-answer vectors ---------------------------------------------------------------------------
def _column(k):
    t = R.TYPE_NAMES[k["type"]]
    raw = k["values"]
    valid = np.array([x is not None for x in raw], dtype=bool)
    if t == R.TYPE_UTF8:
        vals = [bytes.fromhex(x) if x is not None else b"" for x in raw]
    elif t == R.TYPE_FLOAT64:
        vals = np.array([int(x, 16) if x is not None else 0 for x in raw], dtype=np.uint64).view(np.float64)
    else:
        vals = np.array([x if x is not None else 0 for x in raw], dtype=R.NP_DTYPE[t])
    return (t, vals, None if valid.all() else valid)


def load_kat():
    """tests/golden/window_kat.json -> [(name, partition keys, order keys, flags, inputs, fns, expected)];
    float64 values are hex bit patterns, utf8 values hex byte strings, null is null."""
    out = []
    for v in json.loads(KAT.read_text())["vectors"]:
        part = [_column(k) for k in v.get("partition", [])]
        order = [_column(k) for k in v.get("order", [])]
        flags = [k.get("flags", 0) for k in v.get("order", [])]
        inputs = [_column(k) for k in v.get("inputs", [])]
        fns = [(FN_NAMES[f["fn"]], FRAME_NAMES[f.get("frame", "range")], f.get("input", 0), f.get("offset", 0)) for f in v["fns"]]
        expected = []
        for (fn, _, inp, _), raw in zip(fns, v["expected"]):
            dt = _out_dtype(fn, inputs[inp][0] if takes_input(fn) else 0)
            ok = np.array([x is not None for x in raw], dtype=bool)
            if dt == np.float64:
                vals = np.array([int(x, 16) if x is not None else 0 for x in raw], dtype=np.uint64).view(np.float64)
            else:
                vals = np.array([x if x is not None else 0 for x in raw], dtype=dt)
            expected.append((vals, ok))
        out.append((v["name"], part, order, flags, inputs, fns, expected, v["rows"]))
    return out
