"""CPU reference of ORDER BY (qe_sort_indices / qe_take), test infrastructure only.

Two independent statements of the order:
  * compare(): a pairwise comparator written from the semantics (Double.compare, byte order, null
    placement independent of DESC);
  * order(): the stable permutation. Fixed-width keys are encoded to order-preserving unsigned
    words with numpy and sorted with np.lexsort (stable); UTF8 keys are ranked by a stable Python
    sorted() over their bytes.
A key is (type_id, values, valid): values a numpy array (fixed width, bool) or a list of bytes
(UTF8); valid a bool array or None.
"""
import json
import pathlib
import struct

import numpy as np

TYPE_INT64, TYPE_FLOAT64, TYPE_BOOL, TYPE_UTF8, TYPE_INT32, TYPE_UINT8, TYPE_DATE32 = 1, 2, 3, 4, 5, 6, 7
DESC, NULLS_FIRST = 1, 2
TYPE_NAMES = {"int64": TYPE_INT64, "float64": TYPE_FLOAT64, "bool": TYPE_BOOL, "utf8": TYPE_UTF8,
              "int32": TYPE_INT32, "uint8": TYPE_UINT8, "date32": TYPE_DATE32}
NP_DTYPE = {TYPE_INT64: np.int64, TYPE_FLOAT64: np.float64, TYPE_INT32: np.int32, TYPE_DATE32: np.int32,
            TYPE_UINT8: np.uint8, TYPE_BOOL: np.bool_}
KAT = pathlib.Path(__file__).resolve().parent / "golden" / "sort_kat.json"


# ---- pairwise comparator ------------------------------------------------------------------------
def _cmp(a, b):
    return (a > b) - (a < b)


def _double_compare(x: float, y: float) -> int:
    """java.lang.Double.compare: numeric order, -0.0 < +0.0, every NaN equal and above +Inf."""
    xn, yn = x != x, y != y
    if xn or yn:
        return _cmp(xn, yn)
    if x != y:
        return -1 if x < y else 1
    sx, sy = struct.pack(">d", x)[0] >> 7, struct.pack(">d", y)[0] >> 7  # equal values: the signs of zero
    return _cmp(sy, sx)


def compare(type_id: int, a, b, flags: int) -> int:
    """Order of two key values (None = null): negative when a sorts first, 0 when they tie."""
    if a is None or b is None:
        if a is None and b is None:
            return 0
        first = -1 if flags & NULLS_FIRST else 1
        return first if a is None else -first
    if type_id == TYPE_FLOAT64:
        c = _double_compare(float(a), float(b))
    elif type_id == TYPE_UTF8:
        c = _cmp(bytes(a), bytes(b))  # unsigned byte-lexicographic, a proper prefix first
    else:
        c = _cmp(int(a), int(b))
    return -c if flags & DESC else c


# ---- stable permutation ---------------------------------------------------------------------------
def encode_fixed(type_id: int, values: np.ndarray) -> np.ndarray:
    """Ascending order-preserving uint64 of every value."""
    if type_id == TYPE_FLOAT64:
        bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64).copy()
        bits[(bits & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)] = np.uint64(0x7FF8000000000000)
        neg = (bits >> np.uint64(63)) == 1
        return np.where(neg, ~bits, bits | np.uint64(1 << 63))
    if type_id == TYPE_BOOL:
        return np.asarray(values, dtype=bool).astype(np.uint64)
    if type_id == TYPE_UINT8:
        return np.asarray(values, dtype=np.uint8).astype(np.uint64)
    v = np.asarray(values).astype(np.int64)
    return v.view(np.uint64) ^ np.uint64(1 << 63)


_RANKS: dict = {}  # id(values) -> (values, ranks): one ranking per shared test column


def _utf8_ranks(values, valid) -> np.ndarray:
    hit = _RANKS.get(id(values))
    if hit is not None and hit[0] is values:
        return hit[1]
    distinct = sorted({bytes(v) for v in values})  # Python's bytes order: unsigned, a prefix first
    rank = {b: i for i, b in enumerate(distinct)}
    ranks = np.array([rank[bytes(v)] for v in values], dtype=np.uint64)
    _RANKS[id(values)] = (values, ranks)
    return ranks


def key_columns(type_id: int, values, valid, flags: int):
    """(null column, value column): sorting by them in that order, ascending, is the key's order."""
    n = len(values)
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    enc = _utf8_ranks(values, ok) if type_id == TYPE_UTF8 else encode_fixed(type_id, values)
    if flags & DESC:
        enc = ~enc
    enc = np.where(ok, enc, np.uint64(0))
    nulls = ok.astype(np.uint8) if flags & NULLS_FIRST else (~ok).astype(np.uint8)
    return nulls, enc


def order(keys, flags, limit=None) -> np.ndarray:
    """The stable ORDER BY permutation (int32 row indices); limit None or < 0: all rows."""
    cols = []
    for (t, values, valid), f in zip(keys, flags):
        cols.extend(key_columns(t, values, valid, f))
    n = len(keys[0][1])
    perm = np.lexsort(cols[::-1]).astype(np.int32) if n else np.zeros(0, dtype=np.int32)
    return perm if limit is None or limit < 0 else perm[:limit]


# ---- known-answer vectors -------------------------------------------------------------------------
def load_kat():
    """tests/golden/sort_kat.json -> [(name, keys, flags, limit, expected, max_lens)]. float64
    values are hex bit patterns (NaN payloads survive), utf8 values hex byte strings."""
    out = []
    for v in json.loads(KAT.read_text())["vectors"]:
        keys, flags, max_lens = [], [], []
        for k in v["keys"]:
            t = TYPE_NAMES[k["type"]]
            raw = k["values"]
            valid = np.array([x is not None for x in raw], dtype=bool)
            if t == TYPE_UTF8:
                vals = [bytes.fromhex(x) if x is not None else b"" for x in raw]
            elif t == TYPE_FLOAT64:
                vals = np.array([int(x, 16) if x is not None else 0 for x in raw], dtype=np.uint64).view(np.float64)
            else:
                vals = np.array([x if x is not None else 0 for x in raw], dtype=NP_DTYPE[t])
            keys.append((t, vals, None if valid.all() else valid))
            flags.append(k["flags"])
            max_lens.append(k.get("max_len"))
        out.append((v["name"], keys, flags, v.get("limit", -1), np.array(v["expected"], dtype=np.int32), max_lens))
    return out
