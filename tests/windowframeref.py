"""CPU reference of qe_window_eval_frames: the window functions of tests/windowref.py
plus FIRST_VALUE / LAST_VALUE and the frame ROWS BETWEEN lo AND hi, test infrastructure only.

A function is (fn, frame, input index, offset, lo, hi); lo and hi are read for ROWS_BETWEEN only. For
position i of a partition that occupies positions [P, Pe] the frame is [s, e]: [P, frame end] under
the three older frames, [max(P, i + lo), min(Pe, i + hi)] under ROWS_BETWEEN (Python integers: exact),
empty when s > e. The semantics are stated twice, as in windowref:

  * fold(): per row, a FRESH oracle accumulator (oracle/semantics.py) folded over that row's frame in
    window order; FIRST / LAST are the cell at s / e. O(n x frame width): a few hundred rows.
  * vectorised(): numpy over whole columns. SUM / COUNT from wrapping prefix sums at s and e, MIN / MAX
    from a sparse table (range arg-extreme of value ranks, the earliest position on ties) and the
    frame's first non-null position for the NaN seed.

The ranks and LAG / LEAD ignore the frame; both statements hand them to windowref.

Also the argument rules that qe_window_plan.hpp adds for the call (check, clamp, scans, work_bytes)
and the known-answer vectors of tests/golden/window_frames_kat.json.
"""
import json
import pathlib

import numpy as np

import sortref as R
import windowref as W
from oracle import semantics as S

(ROW_NUMBER, RANK, DENSE_RANK, COUNT_STAR, COUNT, SUM, MIN, MAX, LAG, LEAD, FIRST_VALUE, LAST_VALUE) = range(1, 13)
ROWS, RANGE, PARTITION, ROWS_BETWEEN = 0, 1, 2, 3
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
UNBOUNDED_PRECEDING, UNBOUNDED_FOLLOWING = INT64_MIN, INT64_MAX
FN_NAMES = dict(W.FN_NAMES, first_value=FIRST_VALUE, last_value=LAST_VALUE)
FRAME_NAMES = dict(W.FRAME_NAMES, rows_between=ROWS_BETWEEN)
OK, INVALID_ARG, UNSUPPORTED = W.OK, W.INVALID_ARG, W.UNSUPPORTED
KAT = pathlib.Path(__file__).resolve().parent / "golden" / "window_frames_kat.json"
AGGREGATES = (COUNT_STAR, COUNT, SUM, MIN, MAX)


# ---- argument rules (qe_window_plan.hpp: window_frames_*) -------------------------------------------
def takes_input(fn):
    return fn in range(COUNT, LAST_VALUE + 1)


def nullable(fn):
    return fn in range(SUM, LAST_VALUE + 1)


def check(fn, frame, in_type, offset, has_bounds=True):
    """(status, output type) of one function of qe_window_eval_frames. The bounds' values never refuse."""
    if fn not in range(ROW_NUMBER, LAST_VALUE + 1) or frame not in (ROWS, RANGE, PARTITION, ROWS_BETWEEN):
        return INVALID_ARG, 0
    if frame == ROWS_BETWEEN and not has_bounds:
        return INVALID_ARG, 0
    if fn in (FIRST_VALUE, LAST_VALUE):
        if in_type not in W.ALL_TYPES:
            return INVALID_ARG, 0
        return (OK, in_type) if in_type in W.VALUE_TYPES else (UNSUPPORTED, 0)
    return W.check(fn, ROWS if frame == ROWS_BETWEEN else frame, in_type, offset)


def clamp(b, n):
    """A bound clamped to [-n, n]: no frame of a partition of at most n rows changes."""
    return max(-n, min(n, b))


def scans(fns, n):
    """The distinct scans (kind, input, backward, block length) of a call over n rows in order of first
    use, and per function the index of its forward and of its backward scan (-1: none)."""
    kind_of = {COUNT: 1, SUM: 1, MIN: 2, MAX: 3}
    found, fwd, bwd = [], [], []

    def slot(key):
        if key not in found:
            found.append(key)
        return found.index(key)

    for fn, frame, inp, _, lo, hi in fns:
        f = b = -1
        if fn in kind_of:
            kind = kind_of[fn]
            lo, hi = clamp(lo, n), clamp(hi, n)
            if kind == 1 or frame != ROWS_BETWEEN:
                f = slot((kind, inp, 0, 0))
            elif lo > hi:
                pass  # every frame is empty
            elif lo == -n:
                f = slot((kind, inp, 0, 0))
            elif hi == n:
                b = slot((kind, inp, 1, 0))
            else:
                width = hi - lo + 1
                block = 0 if width >= n else width
                f, b = slot((kind, inp, 0, block)), slot((kind, inp, 1, block))
        fwd.append(f)
        bwd.append(b)
    return found, fwd, bwd


def work_bytes(n, fns, tile_rows):
    return W.work_bytes(n, len(scans(fns, n)[0]), len(fns), tile_rows)


# ---- shared -----------------------------------------------------------------------------------------
def _old(f):
    return (f[0], f[1] if f[1] != ROWS_BETWEEN else ROWS, f[2], f[3])


def _out_dtype(fn, in_type):
    return R.NP_DTYPE[in_type] if fn in (MIN, MAX, LAG, LEAD, FIRST_VALUE, LAST_VALUE) else np.int64


def _empty_result(fn, inputs, inp, n):
    return np.zeros(n, dtype=_out_dtype(fn, inputs[inp][0] if takes_input(fn) else 0)), np.zeros(n, dtype=bool)


# ---- the literal statement --------------------------------------------------------------------------
def fold(part, order, flags, inputs, fns, n=0):
    n = W._n_rows(part, order, inputs, n)
    perm = W.window_order(part, order, flags, n)
    results = [None] * len(fns)
    framed = [k for k, f in enumerate(fns) if f[0] in AGGREGATES or f[0] in (FIRST_VALUE, LAST_VALUE)]
    rest = [k for k in range(len(fns)) if k not in framed]
    for k, r in zip(rest, W.fold(part, order, flags, inputs, [_old(fns[k]) for k in rest], n)):
        results[k] = r
    for k in framed:
        results[k] = _empty_result(fns[k][0], inputs, fns[k][2], n)

    def same(cols, fl, a, b):
        return all(R.compare(c[0], W._cell(c, a), W._cell(c, b), f) == 0 for c, f in zip(cols, fl))

    start = 0
    while start < n:
        end = start + 1
        while end < n and same(part, [0] * len(part), perm[end - 1], perm[end]):
            end += 1
        rows = [int(r) for r in perm[start:end]]
        m = len(rows)
        peer_last = [0] * m
        g0 = 0
        for j in range(1, m + 1):
            if j == m or not same(order, flags, rows[j - 1], rows[j]):
                for q in range(g0, j):
                    peer_last[q] = j - 1
                g0 = j
        for k in framed:
            fn, frame, inp, _, lo, hi = fns[k]
            out, ok = results[k]
            for j, r in enumerate(rows):
                if frame == ROWS_BETWEEN:
                    s, e = max(0, j + lo), min(m - 1, j + hi)
                else:
                    s, e = 0, j if frame == ROWS else peer_last[j] if frame == RANGE else m - 1
                members = rows[s:e + 1] if s <= e else []
                if fn in (FIRST_VALUE, LAST_VALUE):
                    value = W._cell(inputs[inp], members[0 if fn == FIRST_VALUE else -1]) if members else None
                else:
                    acc = {COUNT_STAR: lambda: S.CountAccumulator(True), COUNT: lambda: S.CountAccumulator(False),
                           SUM: lambda: S.SumAccumulator(False), MIN: S.MinAccumulator, MAX: S.MaxAccumulator}[fn]()
                    for q in members:
                        acc.accumulate(0 if fn == COUNT_STAR else W._cell(inputs[inp], q))
                    value = acc.finalValue()
                W._put(out, ok, r, fn, value)
        start = end
    return results


# ---- the vectorised statement -----------------------------------------------------------------------
def _range_extreme(key, s, e, smallest):
    """Per query the extreme of key[s .. e] (s <= e), by a sparse table of power-of-two spans."""
    pick = np.minimum if smallest else np.maximum
    table = [key]
    while 2 << (len(table) - 1) <= len(key):
        half = 1 << (len(table) - 1)
        table.append(pick(table[-1][:-half], table[-1][half:]))
    span = e - s + 1
    level = np.zeros(len(s), dtype=np.int64)
    for k in range(1, len(table)):
        level[span >= (1 << k)] = k
    out = np.empty(len(s), dtype=key.dtype)
    for k, t in enumerate(table):
        sel = level == k
        out[sel] = pick(t[s[sel]], t[e[sel] - (1 << k) + 1])
    return out


def vectorised(part, order, flags, inputs, fns, n=0):
    n = W._n_rows(part, order, inputs, n)
    results = [None] * len(fns)
    framed = [k for k, f in enumerate(fns) if f[0] in AGGREGATES or f[0] in (FIRST_VALUE, LAST_VALUE)]
    rest = [k for k in range(len(fns)) if k not in framed]
    for k, r in zip(rest, W.vectorised(part, order, flags, inputs, [_old(fns[k]) for k in rest], n)):
        results[k] = r
    if n == 0:
        for k in framed:
            results[k] = _empty_result(fns[k][0], inputs, fns[k][2], 0)
        return results
    perm = W.window_order(part, order, flags, n)
    idx = np.arange(n, dtype=np.int64)
    ps = W.starts(part, [0] * len(part), perm)
    gs = W.starts(list(part) + list(order), [0] * len(part) + list(flags), perm)
    P = np.maximum.accumulate(np.where(ps, idx, 0))
    nxt = np.append(np.where(ps, idx, n)[1:], n)
    Pe = np.minimum.accumulate(nxt[::-1])[::-1] - 1
    nxt = np.append(np.where(gs, idx, n)[1:], n)
    Ge = np.minimum.accumulate(nxt[::-1])[::-1] - 1
    for k in framed:
        fn, frame, inp, _, lo, hi = fns[k]
        if frame == ROWS_BETWEEN:
            s, e = np.maximum(P, idx + clamp(lo, n)), np.minimum(Pe, idx + clamp(hi, n))
        else:
            s, e = P, idx if frame == ROWS else Ge if frame == RANGE else Pe
        there = s <= e
        s, e = np.where(there, s, 0), np.where(there, e, 0)  # an empty frame reads position 0 and drops it
        ok = np.ones(n, dtype=bool)
        if fn == COUNT_STAR:
            val = np.where(there, e - s + 1, 0)
        else:
            t, values, valid = inputs[inp]
            v = (np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool))[perm]
            cnt = np.concatenate([[0], np.cumsum(v)])
            have = np.where(there, cnt[e + 1] - cnt[s], 0)
            x = None if t == R.TYPE_UTF8 else np.asarray(values)[perm]
        if fn == COUNT:
            val = have
        elif fn == SUM:
            y = np.where(v, x.astype(np.int64), 0).view(np.uint64)
            run = np.concatenate([[np.uint64(0)], np.cumsum(y, dtype=np.uint64)])
            val = (run[e + 1] - run[s]).view(np.int64)
            ok = have > 0
        elif fn in (MIN, MAX):
            nan = v & (x != x) if t == R.TYPE_FLOAT64 else np.zeros(n, dtype=bool)
            num = v & ~nan
            # the first non-null position at or after s seeds the fold
            first = np.minimum.accumulate(np.where(v, idx, n)[::-1])[::-1]
            ok = have > 0
            seed_nan = ok & nan[np.minimum(first[s], n - 1)]
            # arg-extreme of (rank of the value, position): equal values (-0.0 == +0.0) share a rank and
            # the earliest position wins
            _, rank = np.unique(np.where(num, x, x[num][0] if num.any() else 0), return_inverse=True)
            rank = rank.astype(np.int64).reshape(n)
            if fn == MIN:
                best = _range_extreme(np.where(num, rank * n + idx, (int(rank.max()) + 1) * n), s, e, True)
                pos = np.minimum(best % n, n - 1)
            else:
                best = _range_extreme(np.where(num, rank * n + (n - 1 - idx), -1), s, e, False)
                pos = n - 1 - np.maximum(best, 0) % n
            val = np.where(seed_nan, W.CANON_NAN, x[pos]) if t == R.TYPE_FLOAT64 else x[pos]
        elif fn in (FIRST_VALUE, LAST_VALUE):
            q = s if fn == FIRST_VALUE else e
            ok = there & v[q]
            val = x[q]
        out, okr = _empty_result(fn, inputs, inp, n)
        out[perm] = np.where(ok, val, 0).astype(out.dtype)
        okr[perm] = ok
        results[k] = (out, okr)
    return results


same_results = W.same_results


# ---- known-answer vectors ---------------------------------------------------------------------------
def load_kat():
    """tests/golden/window_frames_kat.json -> [(name, partition keys, order keys, flags, inputs, fns,
    expected, rows)], in windowref.load_kat's encoding; a function may carry "lo" and "hi"."""
    out = []
    for v in json.loads(KAT.read_text())["vectors"]:
        part = [W._column(k) for k in v.get("partition", [])]
        order = [W._column(k) for k in v.get("order", [])]
        flags = [k.get("flags", 0) for k in v.get("order", [])]
        inputs = [W._column(k) for k in v.get("inputs", [])]
        fns = [(FN_NAMES[f["fn"]], FRAME_NAMES[f.get("frame", "rows_between")], f.get("input", 0), f.get("offset", 0),
                f.get("lo", 0), f.get("hi", 0)) for f in v["fns"]]
        expected = []
        for (fn, _, inp, _, _, _), raw in zip(fns, v["expected"]):
            dt = _out_dtype(fn, inputs[inp][0] if takes_input(fn) else 0)
            ok = np.array([x is not None for x in raw], dtype=bool)
            if dt == np.float64:
                vals = np.array([int(x, 16) if x is not None else 0 for x in raw], dtype=np.uint64).view(np.float64)
            else:
                vals = np.array([x if x is not None else 0 for x in raw], dtype=dt)
            expected.append((vals, ok))
        out.append((v["name"], part, order, flags, inputs, fns, expected, v["rows"]))
    return out
