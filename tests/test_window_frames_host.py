"""CPU tests of the host rules qe_window_plan.hpp adds for qe_window_eval_frames: the accept / refuse
table, the clamp of a frame's bounds, the scans a call's functions share and the working-memory size,
compiled for the host with g++ (once more with the address and undefined-behaviour sanitizers, as a
stand-alone program), against tests/windowframeref.py."""
import pathlib
import subprocess

import numpy as np
import pytest

import windowframeref as F
import windowref as W

ROOT = pathlib.Path(__file__).resolve().parents[1]
EXTREMES = (F.INT64_MIN, F.INT64_MIN + 1, -1, 0, 1, F.INT64_MAX - 1, F.INT64_MAX)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("windowframes") / f"window_frames_host_{request.param}"
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "query-engines_amd" / "csrc"), str(ROOT / "tests" / "native" / "window_frames_host.cpp"),
                    "-o", str(exe)], check=True)

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True)
        assert out.stderr == "", out.stderr  # a sanitizer report
        got = out.stdout.strip().split("\n")
        assert got[-1].startswith("const ") and len(got) == len(lines) + 1
        return got[:-1]

    run.constants = lambda: tuple(int(x) for x in subprocess.run(
        [str(exe)], input="", check=True, capture_output=True, text=True).stdout.split()[1:])
    return run


def _fn_words(fns):
    return f"{len(fns)} " + " ".join(f"{fn} {fr} {inp} {lo} {hi}" for fn, fr, inp, _, lo, hi in fns)


def test_accept_refuse_table(driver):
    """fn 0 .. 13 x frame -1 .. 4 x every type (and 0, 8) x offsets on both sides of 0 x with and without
    a bounds array x bounds at the ends of int64: the bounds' values never change the answer."""
    pairs = [(EXTREMES[i], EXTREMES[-1 - i]) for i in range(len(EXTREMES))]
    cases = [(fn, frame, t, off, has, *pairs[(fn + frame + t) % len(pairs)]) for fn in range(0, 14) for frame in range(-1, 5)
             for t in range(0, 9) for off in (-(2**63), -1, 0, 2**63 - 1) for has in (0, 1)]
    cases += [(fn, 3, 1, 0, 1, lo, hi) for fn in (F.SUM, F.MIN, F.FIRST_VALUE) for lo in EXTREMES for hi in EXTREMES]
    got = [tuple(int(x) for x in line.split()) for line in driver(["c " + " ".join(str(x) for x in c) for c in cases])]
    want = []
    for fn, fr, t, off, has, lo, hi in cases:
        st, out = F.check(fn, fr, t, off, bool(has))
        known = fn in range(F.ROW_NUMBER, F.LAST_VALUE + 1)
        want.append((st, out, int(known and F.takes_input(fn)), int(known and F.nullable(fn)), F.clamp(lo, 2**31 - 1),
                     F.clamp(hi, 2**31 - 1)))
    assert got == want
    ok = {(fn, fr, t) for (fn, fr, t, off, has, _, _), g in zip(cases, got) if g[0] == F.OK}
    assert {t for fn, fr, t in ok if fn == F.FIRST_VALUE} == {1, 2, 5, 6, 7} == {t for fn, fr, t in ok if fn == F.LAST_VALUE}
    assert {fr for fn, fr, t in ok if fn == F.LAST_VALUE} == {0, 1, 2, 3} == {fr for fn, fr, t in ok if fn == F.RANK}
    assert (F.SUM, 3, 1) in ok and (F.SUM, 3, 5) in ok and (F.SUM, 3, 2) not in ok  # FLOAT64 SUM stays unsupported
    assert not any(fn in (0, 13) or fr in (-1, 4) for fn, fr, t in ok)
    for (fn, fr, t, off, has, _, _), g in zip(cases, got):
        if fr == 3 and not has:
            assert g[0] == F.INVALID_ARG
        if fn <= W.LEAD and fr <= W.PARTITION:  # the ids qe_window_eval knows: its answer
            assert g[:2] == W.check(fn, fr, t, off)
    assert {g[0] for g in got} == {F.OK, F.INVALID_ARG, F.UNSUPPORTED}


def test_clamp(driver):
    ns = (0, 1, 2, 1000, 2**31 - 1)
    bs = sorted({*EXTREMES, *(s * (n + d) for n in ns for d in (-1, 0, 1) for s in (-1, 1))})
    cases = [(b, n) for n in ns for b in bs]
    got = [int(x) for x in driver([f"k {b} {n}" for b, n in cases])]
    assert got == [F.clamp(b, n) for b, n in cases]
    for (b, n), g in zip(cases, got):
        assert -n <= g <= n and (g == b or abs(b) > n)


def _random_call(rng, n):
    fns = []
    for _ in range(int(rng.integers(1, W.MAX_AGGS + 1))):
        fn = int(rng.integers(1, 13))
        frame = int(rng.integers(0, 4))
        choices = [F.INT64_MIN, -n - 1, -n, -n + 1, *range(-3, 4), n - 1, n, n + 1, F.INT64_MAX]
        fns.append((fn, frame, int(rng.integers(0, 2)), 0, int(choices[rng.integers(len(choices))]),
                    int(choices[rng.integers(len(choices))])))
    return fns


def test_shared_scans(driver):
    rng = np.random.default_rng(5)
    b = F.ROWS_BETWEEN
    calls = [(100, []), (100, [(F.ROW_NUMBER, b, 0, 0, -1, 1), (F.FIRST_VALUE, b, 0, 0, -1, 1), (F.COUNT_STAR, b, 0, 0, -1, 1)]),
             # a bounded SUM / COUNT shares the running pair; bounded MIN / MAX of one width share their two scans
             (100, [(F.SUM, b, 1, 0, -2, 0), (F.COUNT, W.ROWS, 1, 0, 0, 0), (F.MIN, b, 1, 0, -2, 0), (F.MIN, b, 1, 0, 0, 2),
                    (F.MAX, b, 1, 0, -2, 0), (F.MIN, b, 0, 0, -2, 0), (F.MIN, b, 1, 0, -3, 0)]),
             # an unbounded start shares the older frames' scan; an unbounded end needs one backward scan
             (100, [(F.MIN, W.ROWS, 0, 0, 0, 0), (F.MIN, b, 0, 0, F.INT64_MIN, 0), (F.MIN, b, 0, 0, -100, 5),
                    (F.MIN, b, 0, 0, 0, F.INT64_MAX), (F.MIN, b, 0, 0, -5, 100), (F.MIN, b, 0, 0, -99, 99), (F.MIN, b, 0, 0, 2, 1)]),
             (1000, [(F.MAX, b, 0, 0, -w, 0) for w in range(1, 9)]),  # the most scans a call can have
             (1, [(F.MAX, b, 0, 0, 0, 0)]), (0, [(F.MAX, b, 0, 0, -1, 1)])]
    for _ in range(60):
        n = int(rng.choice([1, 2, 5, 100, 2**31 - 1]))
        calls.append((n, _random_call(rng, n)))
    most = 0
    for line, (n, call) in zip(driver([f"s {n} " + _fn_words(call) for n, call in calls]), calls):
        v = [int(x) for x in line.split()]
        found, fwd, bwd = F.scans(call, n)
        assert v[0] == len(found) <= 2 * len(call)
        assert [tuple(v[1 + 4 * j:5 + 4 * j]) for j in range(v[0])] == found
        assert v[1 + 4 * v[0]:1 + 4 * v[0] + len(call)] == fwd and v[1 + 4 * v[0] + len(call):] == bwd
        most = max(most, v[0])
    assert most == 2 * W.MAX_AGGS
    found, fwd, bwd = F.scans(calls[2][1], 100)
    assert len(found) == 9 and fwd[:2] == [0, 0] and (fwd[2], bwd[2]) == (fwd[3], bwd[3]) and fwd[6] != fwd[2]
    found, fwd, bwd = F.scans(calls[3][1], 100)
    assert found == [(2, 0, 0, 0), (2, 0, 1, 0)] and fwd == [0, 0, 0, -1, -1, 0, -1] and bwd == [-1, -1, -1, 1, 1, 1, -1]


def test_working_memory_size(driver):
    tile, small, max_aggs = driver.constants()
    assert 0 < tile <= small and max_aggs == W.MAX_AGGS
    rng = np.random.default_rng(6)
    ns = sorted({1, 2, 63, 64, 65, small, small + 1, tile - 1, tile, tile + 1, 3 * tile + 17, 32 * tile + 1, 10**8, 2**31 - 1})
    cases = [(n, _random_call(rng, n)) for n in ns for _ in range(6)]
    cases += [(n, [(F.MAX, F.ROWS_BETWEEN, 0, 0, -w, 0) for w in range(1, 9)]) for n in ns]
    got = [tuple(int(x) for x in line.split()) for line in driver([f"b {n} " + _fn_words(call) for n, call in cases])]
    unbounded = 0
    for (n, call), (frames_bytes, eval_bytes) in zip(cases, got):
        assert frames_bytes == F.work_bytes(n, call, tile)
        bounded = any(fn in (F.MIN, F.MAX) and fr == F.ROWS_BETWEEN for fn, fr, *_ in call)
        if not bounded:  # no bounded MIN / MAX: what qe_window_eval allocates for the same functions
            assert frames_bytes == eval_bytes == W.work_bytes(n, len(W.scans([f[:4] for f in call])[0]), len(call), tile)
            unbounded += 1
        assert frames_bytes % 256 == 0 and frames_bytes >= 4 * n + len(F.scans(call, n)[0]) * 12 * n + 8 * n * (len(call) + 1)
    assert unbounded >= 10
