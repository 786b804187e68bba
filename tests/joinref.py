"""CPU restatement of the equi-join (include/qe_hip.h "equi-JOIN"): the semantics the
device hash join is held to, written independently of query-engines_amd/csrc/qe_join_plan.hpp.

A key column is ``(type, values, valid)``: numpy values (bool array for BOOL), ``valid`` a bool
sequence or None. Every non-null row has one 64-bit key word; rows join iff their words are equal:

  INT64           the value's two's-complement bits
  INT32 / DATE32  sign-extended to 64 bits
  UINT8 / BOOL    zero-extended
  FLOAT64         the IEEE bits, every NaN the one pattern 0x7FF8000000000000 (Double.equals: all NaNs
                  one key, -0.0 and +0.0 apart); FLOAT64 pairs only with FLOAT64

A null key matches nothing on either side. Pairs come ordered by probe row, then by build row.
"""
from __future__ import annotations

import json
import pathlib

import numpy as np

M64 = (1 << 64) - 1
CANON_NAN = 0x7FF8000000000000
TYPE_INT64, TYPE_FLOAT64, TYPE_BOOL, TYPE_UTF8, TYPE_INT32, TYPE_UINT8, TYPE_DATE32 = 1, 2, 3, 4, 5, 6, 7
KEY_TYPES = (TYPE_INT64, TYPE_INT32, TYPE_DATE32, TYPE_UINT8, TYPE_BOOL, TYPE_FLOAT64)
KAT = pathlib.Path(__file__).resolve().parent / "golden" / "join_kat.json"


def key_word(t: int, v) -> int:
    """The key word of one non-null value (a Python / numpy scalar; FLOAT64 as a float)."""
    if t == TYPE_INT64:
        return int(v) & M64
    if t in (TYPE_INT32, TYPE_DATE32):
        v = int(v)
        assert -(1 << 31) <= v < (1 << 31)
        return v & M64  # Python's & on a negative int sign-extends
    if t == TYPE_UINT8:
        v = int(v)
        assert 0 <= v < 256
        return v
    if t == TYPE_BOOL:
        return 1 if v else 0
    if t == TYPE_FLOAT64:
        bits = int(np.array([v], dtype=np.float64).view(np.uint64)[0])
        return CANON_NAN if (bits & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000 else bits
    raise ValueError(f"type {t} is no join key")


def compatible(build_type: int, probe_type: int) -> bool:
    return (build_type in KEY_TYPES and probe_type in KEY_TYPES
            and (build_type == TYPE_FLOAT64) == (probe_type == TYPE_FLOAT64))


def key_words(col) -> list:
    """Per row the key word, None for a null row."""
    t, vals, valid = col
    if t == TYPE_FLOAT64:  # bits straight from the array: a NaN's payload must not pass through a Python float
        bits = np.ascontiguousarray(vals, dtype=np.float64).view(np.uint64)
        nan = (bits & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)
        words = np.where(nan, np.uint64(CANON_NAN), bits).tolist()
    elif t == TYPE_INT64:
        words = np.ascontiguousarray(vals, dtype=np.int64).view(np.uint64).tolist()
    elif t in (TYPE_INT32, TYPE_DATE32):
        words = np.ascontiguousarray(vals, dtype=np.int32).astype(np.int64).view(np.uint64).tolist()
    elif t == TYPE_UINT8:
        words = np.ascontiguousarray(vals, dtype=np.uint8).astype(np.uint64).tolist()
    elif t == TYPE_BOOL:
        words = np.asarray(vals, dtype=bool).astype(np.uint64).tolist()
    else:
        raise ValueError(f"type {t} is no join key")
    if valid is not None:
        words = [w if ok else None for w, ok in zip(words, valid)]
    return words


def build_table(words) -> dict:
    """key word -> build rows, ascending."""
    d: dict = {}
    for r, w in enumerate(words):
        if w is not None:
            d.setdefault(w, []).append(r)
    return d


def stats(words):
    """(non-null build rows, distinct keys, longest run, slots)."""
    d = build_table(words)
    rows = sum(len(v) for v in d.values())
    return rows, len(d), max((len(v) for v in d.values()), default=0), slots(rows)


def join(build_words, probe_words, kind: str):
    """inner / left: (probe_idx, build_idx) int32 arrays in the fixed order, -1 for left's unmatched
    rows. semi / anti: the bool mask of kept probe rows."""
    d = build_table(build_words)
    if kind in ("semi", "anti"):
        hit = np.array([w is not None and w in d for w in probe_words], dtype=bool)
        return ~hit if kind == "anti" else hit
    assert kind in ("inner", "left")
    pi, bi = [], []
    for i, w in enumerate(probe_words):
        rows = d.get(w) if w is not None else None
        if rows:
            pi.extend([i] * len(rows))
            bi.extend(rows)
        elif kind == "left":
            pi.append(i)
            bi.append(-1)
    return np.array(pi, dtype=np.int32), np.array(bi, dtype=np.int32)


def join_all(build_words, probe_words) -> dict:
    """Every kind's answer over one pair of sides ({kind: join(...)}), the table built once."""
    d = build_table(build_words)
    none: list = []
    runs = [d.get(w, none) if w is not None else none for w in probe_words]
    counts = np.fromiter((len(r) for r in runs), dtype=np.int64, count=len(runs))
    hit = counts > 0
    rows = np.arange(len(runs), dtype=np.int32)
    inner_b = np.fromiter((b for r in runs for b in r), dtype=np.int32, count=int(counts.sum()))
    inner = (np.repeat(rows, counts), inner_b)
    left_counts = np.maximum(counts, 1)
    left_b = np.full(int(left_counts.sum()), -1, dtype=np.int32)
    # a matched row's run fills its slice; an unmatched row's one slot keeps the -1
    left_b[np.repeat(hit, left_counts)] = inner_b
    return {"inner": inner, "left": (np.repeat(rows, left_counts), left_b), "semi": hit, "anti": ~hit}


# ---- the table's shape (include/qe_hip.h states it; the collision test forges keys from it) --------
def fmix64(k: int) -> int:
    k &= M64
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    k ^= k >> 33
    return k


def fmix64_inverse(h: int) -> int:
    """x with fmix64(x) == h: x ^= x >> 33 is its own inverse, the multipliers are inverted mod 2^64."""
    h &= M64
    h ^= h >> 33
    h = (h * 0x9CB4B2F8129337DB) & M64
    h ^= h >> 33
    h = (h * 0x4F74430C22A54005) & M64
    h ^= h >> 33
    return h


def slots(rows: int) -> int:
    s = 64
    while s < 2 * rows:
        s *= 2
    return s


def home_slot(word: int, nslots: int) -> int:
    return fmix64(word) & (nslots - 1)


def forge_keys(nslots: int, slot: int, count: int, first: int = 0) -> list:
    """`count` distinct key words whose home slot is `slot`, the `first`-th onwards of a fixed series."""
    out = [fmix64_inverse(((first + j) * nslots + slot) & M64) for j in range(count)]
    assert len(set(out)) == count and all(home_slot(w, nslots) == slot for w in out)
    return out


def signed(w: int) -> int:
    return w - (1 << 64) if w >= 1 << 63 else w


def load_kat():
    """[(name, build column, probe column, {kind: expected})] of tests/golden/join_kat.json."""
    out = []
    for v in json.loads(KAT.read_text())["vectors"]:
        cols = []
        for side in ("build", "probe"):
            t = v[side]["type"]
            raw = v[side]["values"]
            valid = [x is not None for x in raw]
            if t == TYPE_FLOAT64:  # fp64 values are given as bit patterns (hex strings)
                vals = np.array([int(x, 16) if x is not None else 0 for x in raw], dtype=np.uint64).view(np.float64)
            elif t == TYPE_BOOL:
                vals = np.array([bool(x) for x in raw], dtype=bool)
            else:
                dt = {TYPE_INT64: np.int64, TYPE_INT32: np.int32, TYPE_DATE32: np.int32, TYPE_UINT8: np.uint8}[t]
                vals = np.array([x if x is not None else 0 for x in raw], dtype=dt)
            cols.append((t, vals, None if all(valid) else valid))
        out.append((v["name"], cols[0], cols[1], v["expect"]))
    return out
