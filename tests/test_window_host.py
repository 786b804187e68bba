"""CPU tests of the window functions' host rules: the accept / refuse table (function x input type x
frame x offset), the output types, the scans a call's functions share and the working-memory size
of qe_window_plan.hpp, compiled for the host with g++ (once more with the address and
undefined-behaviour sanitizers, as a stand-alone program), against tests/windowref.py."""
import pathlib
import subprocess

import numpy as np
import pytest

import windowref as W

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("windowplan") / f"window_plan_host_{request.param}"
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "query-engines_amd" / "csrc"), str(ROOT / "tests" / "native" / "window_plan_host.cpp"),
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


def test_accept_refuse_table(driver):
    """Every function (and one id on each side of the range) x every type (and 0, 8) x every frame (and
    -1, 3) x offsets on both sides of 0 and at the ends of int64."""
    cases = [(fn, frame, t, off) for fn in range(0, 12) for frame in (-1, 0, 1, 2, 3) for t in range(0, 9)
             for off in (-(2**63), -1, 0, 1, 2**40, 2**63 - 1)]
    got = [tuple(int(x) for x in line.split()) for line in driver([f"c {fn} {fr} {t} {off}" for fn, fr, t, off in cases])]
    want = []
    for fn, fr, t, off in cases:
        st, out = W.check(fn, fr, t, off)
        known = fn in range(W.ROW_NUMBER, W.LEAD + 1)
        want.append((st, out, int(known and W.takes_input(fn)), int(known and W.nullable(fn))))
    assert got == want
    accepted = {(fn, t) for (fn, fr, t, off), (st, _, _, _) in zip(cases, got) if st == W.OK and W.takes_input(fn)}
    assert (W.SUM, 1) in accepted and (W.SUM, 5) in accepted and (W.SUM, 2) not in accepted  # no inexact fp64 prefix sum
    assert {t for fn, t in accepted if fn == W.LAG} == {1, 2, 5, 6, 7} == {t for fn, t in accepted if fn == W.MIN}
    assert {t for fn, t in accepted if fn == W.COUNT} == set(range(1, 8))
    refused = {st for (fn, fr, t, off), (st, _, _, _) in zip(cases, got) if st != W.OK}
    assert refused == {W.INVALID_ARG, W.UNSUPPORTED}


def test_shared_scans(driver):
    rng = np.random.default_rng(4)
    calls = [[], [(W.ROW_NUMBER, 0)], [(W.SUM, 1), (W.COUNT, 1), (W.RANK, 0), (W.MIN, 1), (W.MAX, 1), (W.SUM, 0)],
             [(W.LAG, 0), (W.LEAD, 0), (W.COUNT_STAR, 0)], [(W.MAX, i) for i in range(8)], [(W.MIN, 3)] * 8]
    for _ in range(40):
        calls.append([(int(rng.integers(1, 11)), int(rng.integers(0, 3))) for _ in range(int(rng.integers(1, 9)))])
    lines = [f"s {len(c)} " + " ".join(f"{fn} {inp}" for fn, inp in c) for c in calls]
    for line, call in zip(driver(lines), calls):
        v = [int(x) for x in line.split()]
        found, of_fn = W.scans([(fn, 0, inp, 0) for fn, inp in call])
        assert v[0] == len(found) <= len(call)
        assert list(zip(v[1:1 + 2 * v[0]:2], v[2:2 + 2 * v[0]:2])) == found
        assert v[1 + 2 * v[0]:] == of_fn


def test_working_memory_size(driver):
    tile, small, max_aggs = driver.constants()
    assert 0 < tile and tile <= small and max_aggs == W.MAX_AGGS
    ns = sorted({1, 2, 31, 32, 33, 63, 64, 65, small, small + 1, tile - 1, tile, tile + 1, 3 * tile + 17, 32 * tile, 32 * tile + 1,
                 10**6 + 3, 10**8, 2**31 - 1})
    cases = [(n, s, f) for n in ns for s in range(0, max_aggs + 1) for f in sorted({max(s, 1), max_aggs})]  # a scan per function at most
    got = [int(x) for x in driver([f"b {n} {s} {f}" for n, s, f in cases])]
    assert got == [W.work_bytes(n, s, f, tile) for n, s, f in cases]
    for (n, s, f), b in zip(cases, got):  # the inverse permutation, every scan's arrays and the staging records fit
        assert b % 256 == 0 and b >= 4 * n + s * 12 * n + 8 * n * (f + 1)
