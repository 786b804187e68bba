"""CPU tests of the ORDER BY semantics: the order-preserving key encoders of qe_sort_key.hpp,
compiled for the host with g++, against tests/sortref.py's comparator on every pair of edge values;
and sortref against the hand-derived vectors of tests/golden/sort_kat.json."""
import itertools
import pathlib
import struct
import subprocess

import numpy as np

import sortref as R

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _f64(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


I64 = [-(1 << 63), -(1 << 63) + 1, -1, 0, 1, (1 << 63) - 1, 1 << 32, -(1 << 32)]
I32 = [-(1 << 31), -1, 0, 1, (1 << 31) - 1]
U8 = [0, 1, 127, 128, 255]
F64_BITS = [
    0x0000000000000000, 0x8000000000000000,  # +-0
    0x7FF0000000000000, 0xFFF0000000000000,  # +-Inf
    0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF,  # +-subnormals
    0x0010000000000000, 0x8010000000000000,  # +-smallest normal
    0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
    0xFFFFFFFFFFFFFFFF, 0x7FF8DEADBEEF0001,  # NaNs: quiet, signalling, both signs, payloads
    0x3FF0000000000000, 0x3FEFFFFFFFFFFFFF, 0x3FF0000000000001, 0xBFF0000000000000,  # 1.0, its neighbours, -1.0
    0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,  # +-largest finite
]


def _cases():
    """(type, [(python value or None, raw bits)])."""
    yield R.TYPE_INT64, [(v, v & ((1 << 64) - 1)) for v in I64]
    yield R.TYPE_INT32, [(v, v & 0xFFFFFFFF) for v in I32]
    yield R.TYPE_DATE32, [(v, v & 0xFFFFFFFF) for v in I32]
    yield R.TYPE_UINT8, [(v, v) for v in U8]
    yield R.TYPE_BOOL, [(0, 0), (1, 1)]
    yield R.TYPE_FLOAT64, [(_f64(b), b) for b in F64_BITS]


def _driver(tmp_path):
    exe = tmp_path / "sort_key_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "query-engines_amd" / "csrc"), str(ROOT / "tests" / "native" / "sort_key_host.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_encoded_keys_agree_with_the_comparator_on_every_pair(tmp_path):
    exe = _driver(tmp_path)
    lines, meta = [], []
    for t, vals in _cases():
        for flags in range(4):
            rows = vals + [(None, 0), (None, 0)]  # two nulls: they tie
            for v, raw in rows:
                lines.append(f"{t} {flags} {0 if v is None else 1} {raw:x}")
                meta.append((t, flags, v))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    got = out.strip().split("\n")
    assert got[-1] == "place c000000000000000 00000000000000ab 0000000000000000"
    enc = [(int(a), int(b, 16)) for a, b in (ln.split() for ln in got[:-1])]
    assert len(enc) == len(meta)
    checked = 0
    for (t, flags), grp in itertools.groupby(zip(meta, enc), key=lambda me: me[0][:2]):
        grp = list(grp)
        for ((_, _, a), ea), ((_, _, b), eb) in itertools.product(grp, grp):
            want = R.compare(t, a, b, flags)
            have = (ea > eb) - (ea < eb)
            assert (want > 0) - (want < 0) == have, (t, flags, a, b, ea, eb)
            checked += 1
        for (_, _, v), (_, field) in grp:  # the value field stays inside the type's bits
            assert field < 1 << {R.TYPE_INT64: 64, R.TYPE_FLOAT64: 64, R.TYPE_BOOL: 1, R.TYPE_UINT8: 8}.get(t, 32)
    assert checked > 3000


def test_sortref_reproduces_every_known_answer():
    kat = R.load_kat()
    assert len(kat) >= 12
    for name, keys, flags, limit, expected, _ in kat:
        got = R.order(keys, flags, limit)
        assert got.dtype == np.int32 and got.tolist() == expected.tolist(), name
        # and the comparator agrees that the answer is ordered, with ties in input order
        full = R.order(keys, flags)
        for a, b in zip(full[:-1], full[1:]):
            c = 0
            for (t, vals, valid), f in zip(keys, flags):
                va = None if valid is not None and not valid[a] else vals[a]
                vb = None if valid is not None and not valid[b] else vals[b]
                c = R.compare(t, va, vb, f)
                if c:
                    break
            assert c < 0 or (c == 0 and a < b), (name, int(a), int(b))
