"""CPU tests of the top-k selection's host rules: the threshold-bin pick, the highest varying digit,
the need bookkeeping, the stop rule and the QE_TOPK_AUTO rule of qe_topk_plan.hpp, compiled for the
host with g++ (once more with the address and undefined-behaviour sanitizers, as a stand-alone
program), against tests/topkref.py."""
import pathlib
import subprocess

import numpy as np
import pytest

import topkref as R

ROOT = pathlib.Path(__file__).resolve().parents[1]
SMALL_MAX = 2048  # any positive value serves: the rules take it as a number


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("topkplan") / f"topk_plan_host_{request.param}"
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=undefined"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", str(ROOT / "include"),
                    "-I", str(ROOT / "query-engines_amd" / "csrc"), str(ROOT / "tests" / "native" / "topk_plan_host.cpp"),
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


def _pick_line(hist, need):
    nz = [(b, c) for b, c in enumerate(hist) if c]
    return f"p {need} {len(nz)} " + " ".join(f"{b} {c}" for b, c in nz)


def _hist(pairs):
    h = [0] * 256
    for b, c in pairs.items():
        h[b] = c
    return h


def _pick_cases():
    big = 2**31 - 1
    cases = []
    for need in (1, 2, 999, 1000):
        cases.append((_hist({0: 1000}), need))  # all mass in bin 0
        cases.append((_hist({255: 1000}), need))  # all mass in bin 255
    edge = _hist({3: 10, 4: 5, 9: 7, 200: 1, 255: 2})
    for need in (1, 10, 11, 15, 16, 22, 23, 24, 25):  # at every cumulative edge and one past it, 1 and the total
        cases.append((edge, need))
    gaps = _hist({0: 4, 100: 1, 101: 0, 102: 0, 103: 3, 254: 2})  # empty bins around the threshold
    for need in (4, 5, 6, 8, 9, 10):
        cases.append((gaps, need))
    one = _hist({17: big})  # 2^31 - 1 rows in one bin
    cases += [(one, 1), (one, big)]
    wide = _hist({5: big, 6: big, 7: 3})  # the running sum passes 2^32
    cases += [(wide, big), (wide, big + 1), (wide, 2 * big), (wide, 2 * big + 1), (wide, 2 * big + 3)]
    for need in (0, -1, 1001):  # outside 1..total: no bin
        cases.append((_hist({0: 1000}), need))
    rng = np.random.default_rng(3)
    for _ in range(40):
        h = [int(x) for x in rng.integers(0, 50, 256) * (rng.random(256) < 0.3)]
        total = sum(h)
        for need in {1, total, int(rng.integers(1, max(total, 1) + 1))}:
            if total:
                cases.append((h, need))
    return cases


def test_threshold_bin_pick(driver):
    cases = _pick_cases()
    got = [tuple(int(x) for x in line.split()) for line in driver([_pick_line(h, need) for h, need in cases])]
    assert got == [R.pick_bin(h, need) for h, need in cases]
    for (h, need), (b, below, tied) in zip(cases, got):
        if 1 <= need <= sum(h):
            assert below < need <= below + h[b] and tied == h[b] and below == sum(h[:b])
        else:
            assert b == -1
    assert R.pick_bin(_hist({0: 1000}), 1000) == (0, 0, 1000) and R.pick_bin(_hist({255: 1000}), 1) == (255, 0, 1000)
    assert R.pick_bin(_hist({3: 10, 4: 5}), 10) == (3, 0, 10) and R.pick_bin(_hist({3: 10, 4: 5}), 11) == (4, 10, 5)
    big = 2**31 - 1
    assert R.pick_bin(_hist({5: big, 6: big, 7: 3}), 2 * big + 1) == (7, 2 * big, 3)


def test_highest_varying_digit(driver):
    def line(rows, h8):
        tr = [(g, b, c) for g in range(8) for b, c in enumerate(h8[g]) if c]
        return f"d {rows} {len(tr)} " + " ".join(f"{g} {b} {c}" for g, b, c in tr)

    def word_hist(words):
        h8 = [[0] * 256 for _ in range(8)]
        for w in words:
            for g in range(8):
                h8[g][(w >> (8 * g)) & 255] += 1
        return h8

    sets = [[0x0102030405060708] * 5,  # constant: no digit
            [0x0102030405060708, 0x0102030405060709],  # only the lowest digit varies
            [0x0102030405060708, 0xFF02030405060708],  # the highest
            [0x00000000000FFFFF, 0x0000000000012345, 0x0000000000000000],  # narrow range: digit 2
            [7], [0, 1 << 63]]
    want = [-1, 0, 7, 2, -1, 7]
    got = [int(x) for x in driver([line(len(ws), word_hist(ws)) for ws in sets])]
    assert got == want == [R.top_digit(word_hist(ws), len(ws)) for ws in sets]


def test_need_bookkeeping(driver):
    walks = [(10, 1000, [(3, 500), (0, 20), (6, 4)]), (1, 5, []), (5, 5, [(0, 5)]), (2**31 - 2, 2**31 - 1, [(2**30, 2**30)])]
    lines = [f"t {k} {tied} {len(p)} " + " ".join(f"{a} {b}" for a, b in p) for k, tied, p in walks]
    for out, (k, tied, picks) in zip(driver(lines), walks):
        v = [int(x) for x in out.split()]
        got = list(zip(v[::2], v[1::2]))
        assert got == R.walk(k, tied, picks)
        assert got[-1] == (got[-2][0], k)  # after the cut exactly k candidates remain
        assert all(c >= k for _, c in got)  # the list always holds the top-k


def test_stop_rule(driver):
    factor, _ = driver.constants()
    assert factor >= 1
    cases = [(c, k, s) for s in (1, 64, SMALL_MAX) for k in (0, 1, 10, s // factor, s, 10 * s, 2**31 - 1)
             for c in (0, 1, s - 1, s, s + 1, factor * k - 1, factor * k, factor * k + 1, 2**31 - 1) if c >= 0]
    got = [x == "1" for x in driver([f"s {c} {k} {s}" for c, k, s in cases])]
    assert got == [R.stop(c, k, s, factor) for c, k, s in cases]
    assert len(cases) > 100
    huge = [(c, k, s) for s in (1, SMALL_MAX) for k in (2**62, 2**62 + 1, 2**63 - 1) for c in (0, 1, s + 1, 2**31 - 1, 2**63 - 1)]
    got = [x == "1" for x in driver([f"s {c} {k} {s}" for c, k, s in huge])]  # factor * k is past int64: no product is formed
    assert got == [R.stop(c, k, s, factor) for c, k, s in huge] and all(got)


def test_auto_rule_properties(driver):
    _, div = driver.constants()
    assert div >= 2
    memo = {}

    def use_select(n, k):
        if (n, k) not in memo:
            memo[(n, k)] = driver([f"a {n} {k} {SMALL_MAX}"])[0] == "1"
        return memo[(n, k)]

    R.check_auto(use_select, SMALL_MAX)
    for n in (SMALL_MAX + 1, 4 * SMALL_MAX, 10**6 + 3, 10**8, 2**31 - 1):  # SELECT when k <= n / div
        for k in (1, n // div // 2, n // div):
            assert use_select(n, k) == (k < n), (n, k)
    assert use_select(10**8, 10**8 // div) and not use_select(SMALL_MAX, 1) and not use_select(10**6, 10**6)
