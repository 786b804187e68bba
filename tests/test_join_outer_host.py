"""CPU tests of the equi-join's match-mark rules: the probe-kind decoding, the bitmap size and a slot's
word and bit of qe_join_plan.hpp, compiled for the host with g++ (once more with the address and
undefined-behaviour sanitizers, as a stand-alone program), against tests/joinref_outer.py; and
joinref_outer against vectors derived by hand below."""
import pathlib
import subprocess

import numpy as np
import pytest

import joinref as R
import joinref_outer as RO

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("joinmarks") / f"join_marks_host_{request.param}"
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "query-engines_amd" / "csrc"), str(ROOT / "tests" / "native" / "join_marks_host.cpp"),
                    "-o", str(exe)], check=True)

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True)
        assert out.stderr == "", out.stderr  # a sanitizer report
        got = out.stdout.strip().split("\n")
        assert got[-1] == "const 0 1 256"
        assert len(got) == len(lines) + 1
        return got[:-1]

    return run


def test_probe_kind_decoding_of_every_value(driver):
    kinds = list(range(0x200))
    got = [tuple(int(x) for x in g.split()) for g in driver([f"k {k}" for k in kinds])]
    accepted = [k for k, g in zip(kinds, got) if g[2]]
    assert accepted == [0, 1, 0x100, 0x101]  # INNER, LEFT, and each with the TRACK bit: nothing else
    for k, (base, track, ok) in zip(kinds, got):
        rbase, rtrack, rok = RO.probe_kind(k)
        assert ok == int(rok), k
        if ok:  # a refused kind has no meaning to compare
            assert (base, track) == (rbase, int(rtrack)), k
    assert RO.probe_kind(0x200) == (0x200, False, False) and RO.probe_kind(2)[2] is False
    assert RO.probe_kind(0x102)[2] is False


def test_bitmap_size(driver):
    slots = [64, 128, 1 << 20]
    got = [int(x) for x in driver([f"m {s}" for s in slots])]
    assert got == [RO.mark_words(s) for s in slots]
    assert got == [3, 5, (1 << 15) + 1]  # slots + 1 bits: the side slot opens one more word


def test_word_and_bit_of_a_slot(driver):
    for nslots in (64, 128, 1 << 20):
        slots = [0, 31, 32, nslots - 1, nslots]  # the last is the side slot
        got = [(int(a), int(b, 16)) for a, b in (g.split() for g in driver([f"p {s}" for s in slots]))]
        assert got == [RO.mark_position(s) for s in slots]
        assert got[:3] == [(0, 1), (0, 1 << 31), (1, 1)]
        assert got[3] == (nslots // 32 - 1, 1 << 31) and got[4] == (nslots // 32, 1)
        assert all(w < RO.mark_words(nslots) for w, _ in got)  # the side slot's word is inside the bitmap


# ---- joinref_outer against vectors derived by hand ------------------------------------------------------------
def _i64(vals, valid=None):
    return R.key_words((R.TYPE_INT64, np.array(vals, dtype=np.int64), valid))


def _lists(build, sides):
    m, u = RO.both_lists(build, sides)
    assert m.dtype == np.int32 and u.dtype == np.int32
    assert sorted(m.tolist() + u.tolist()) == list(range(len(build)))  # the lists partition the build rows
    return m.tolist(), u.tolist()


def test_hand_vectors():
    # a null build key is never matched, even when its stored value is probed
    build = _i64([5, 5, 7, 5], [True, False, True, True])
    assert _lists(build, [_i64([5])]) == ([0, 3], [1, 2])
    assert _lists(build, []) == ([], [0, 1, 2, 3])
    # a null probe key marks nothing (its stored value 1 is a build key)
    assert _lists(_i64([1, 2, 3]), [_i64([1, 2], [False, True])]) == ([1], [0, 2])
    # a duplicate run is matched as a whole, by one probe row or by many
    assert _lists(_i64([4, 4, 9, 4]), [_i64([4])]) == ([0, 1, 3], [2])
    assert _lists(_i64([4, 4, 9, 4]), [_i64([4, 4, 4, 8])]) == ([0, 1, 3], [2])
    # the key -1 (every bit set), probed as INT32 -1, and left alone
    probe32 = R.key_words((R.TYPE_INT32, np.array([-1], dtype=np.int32), None))
    assert _lists(_i64([-1, 0, -1]), [probe32]) == ([0, 2], [1])
    assert _lists(_i64([-1, 0, -1]), [_i64([0])]) == ([1], [0, 2])
    # every NaN payload is one key; the two zeros are two
    bits = np.array([0x7FF8000000000000, 0xFFF8DEADBEEF0001, 0x0000000000000000, 0x8000000000000000], dtype=np.uint64)
    fb = R.key_words((R.TYPE_FLOAT64, bits.view(np.float64), None))

    def fp(b):
        return R.key_words((R.TYPE_FLOAT64, np.array([b], dtype=np.uint64).view(np.float64), None))

    assert _lists(fb, [fp(0x7FF0000000000001)]) == ([0, 1], [2, 3])
    assert _lists(fb, [fp(0x8000000000000000)]) == ([3], [0, 1, 2])
    # marks accumulate over probe sides and setting one twice changes nothing
    build = _i64([1, 2, 3, 1])
    assert _lists(build, [_i64([3])]) == ([2], [0, 1, 3])
    assert _lists(build, [_i64([3]), _i64([1, 9])]) == ([0, 2, 3], [1])
    assert _lists(build, [_i64([3]), _i64([1, 9]), _i64([3])]) == ([0, 2, 3], [1])
    assert RO.marks_after(build, [_i64([3]), _i64([9])]) == {3}


def test_row_level_joins_by_hand():
    lrows = [(1, "a"), (None, "b"), (2, "c"), (9, "d")]
    rrows = [(2, "x"), (None, "y"), (1, "z"), (2, "w"), (7, "v")]
    lkeys = [None if r[0] is None else (r[0],) for r in lrows]
    rkeys = [None if r[0] is None else (r[0],) for r in rrows]
    args = (lrows, lkeys, rrows, rkeys, [0, 2, 2, 4], 2, 2)
    tail = [(None, None, None, "y"), (None, None, 7, "v")]
    assert RO.join_rows("right", *args) == [[(1, "a", 1, "z")], [], [(2, "c", 2, "x"), (2, "c", 2, "w")], tail]
    assert RO.join_rows("full_outer", *args) == [[(1, "a", 1, "z"), (None, "b", None, None)], [],
                                                 [(2, "c", 2, "x"), (2, "c", 2, "w"), (9, "d", None, None)], tail]
    assert RO.join_rows("right_semi", *args) == [[(2, "x"), (1, "z"), (2, "w")]]
    assert RO.join_rows("right_anti", *args) == [[(None, "y"), (7, "v")]]
    # a left side of no batch at all: the final batch alone
    none = (lrows[:0], lkeys[:0], rrows, rkeys, [0], 2, 2)
    assert RO.join_rows("right", *none) == [[(None, None) + r for r in rrows]]
    assert RO.join_rows("right_semi", *none) == [[]] and RO.join_rows("right_anti", *none) == [list(rrows)]
