"""The GROUP BY path choice and buffer sizing as host functions (query-engines_amd/csrc/qe_agg_paths.hpp).

CPU: tests/native/agg_paths.cpp links libqe_hip.so, builds the C4, nullable fp64 MAX and exact fp64
SUM plans of tests/native/agg_plans.hpp without a GPU, and runs
  * the decision ladder over the grid of tests/golden/agg_paths.json. That file holds the notes
    (qe_hashagg_last_kernel_kind) of one ~300,000-row update per (plan, expected groups, knob
    setting), recorded on an MI355X from the commit before the ladder became a function; the first
    rung that applies must decide what the note says was decided (tests/aggpaths.py);
  * the sizing invariants over a few thousand random (rows, CUs, buckets or sub-buckets, record
    bytes, chunking) tuples;
  * the knob reader: which knobs clamp and which fall back when out of range.
The live notes of a GPU at the path changes of the C4 plan: tests/test_gpu_agg_paths.py."""
import json
import os
import pathlib
import subprocess

import pytest

import aggpaths

ROOT = pathlib.Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
KNOBS = aggpaths.KNOBS


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not present")
    if not (ROOT / "query-engines_amd" / "lib" / "libqe_hip.so").exists():
        pytest.skip("libqe_hip.so not built")
    out = tmp_path_factory.mktemp("aggpaths") / "agg_paths"  # per xdist worker: no shared build output
    csrc, lib = ROOT / "query-engines_amd" / "csrc", ROOT / "query-engines_amd" / "lib"
    subprocess.run([HIPCC, "-O1", "-std=c++17", f"-I{csrc}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "agg_paths.cpp"), f"-L{lib}", "-lqe_hip", f"-Wl,-rpath,{lib}",
                    "-o", str(out)], check=True, capture_output=True)
    return out


def _run(exe, args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env or {})
    return subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, env=e)


GOLD = aggpaths.golden()


def test_golden_is_the_recorded_sweep():
    assert GOLD["commit"] and GOLD["cus"] > 0
    assert set(GOLD["settings"]) >= {"default", "lds_compact0", "mp_spill0", "compact_spill0"}
    for name, s in GOLD["settings"].items():
        for plan in ("c4",) if name == "jit0" else ("c4", "f64max", "det"):
            grid = [r["groups"] for r in s["records"] if r["plan"] == plan]
            assert grid == sorted(grid) and grid[0] <= 256 and grid[-1] == 1 << 22
            assert all(b - a <= 256 for a, b in zip(grid, grid[1:]) if b <= 16384)
            assert all(b == 2 * a for a, b in zip(grid, grid[1:]) if a >= 16384)


@pytest.mark.parametrize("setting", sorted(GOLD["settings"]))
def test_ladder_decides_what_the_parent_did(exe, setting):
    s = GOLD["settings"][setting]
    grid = sorted({r["groups"] for r in s["records"]})
    r = _run(exe, ["ladder", GOLD["cus"], 0 if setting == "jit0" else 1, GOLD["rows"], ",".join(map(str, grid))], s["env"])
    assert r.returncode == 0, r.stderr
    plan = {(p["plan"], p["groups"]): aggpaths.planned(p) for p in map(json.loads, r.stdout.splitlines())}
    wrong = []
    for g in s["records"]:
        want = aggpaths.decided(g["note"], g["specialized"])
        got = plan[(g["plan"], g["groups"])]
        if want != got:
            wrong.append((g["plan"], g["groups"], want, got))
    assert not wrong, wrong[:10]
    assert len(s["records"]) >= len(grid)


def test_geometry_invariants(exe):
    r = _run(exe, ["geometry", 20261019, 6000])
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    stats = json.loads(r.stdout.splitlines()[-1])
    assert stats["violations"] == 0 and stats["tuples"] == 6000
    assert stats["chunked"] > 500 and stats["forced_below_one_workgroup"] > 50  # both kinds of tuple were drawn


def test_knobs_defaults_clamps_and_fallbacks(exe):
    k = json.loads(_run(exe, ["knobs"]).stdout)
    assert k == {"lds_compact": 1, "mp_spill": 1, "part_chunked": -1, "spill_load": 6, "compact_load": 98,
                 "compact_spill": 1, "compact_twopass": 0, "spill_maxpct": 70, "spill_subbuckets": 2, "mp_max": 2,
                 "lds_budget_kb": 0, "part_narrow": 1, "part_fill_shift": 0, "part_fast_fill": 0, "part_wg_per_cu": 2,
                 "pagg_slices_per_cu": 8, "fused_wg_per_cu": 0, "nn_implicit": 1}
    # out of range: these clamp to the nearest bound ...
    k = json.loads(_run(exe, ["knobs"], {"QE_SPILL_LOAD": "9", "QE_MP_MAX": "99", "QE_LDS_BUDGET_KB": "4",
                                         "QE_FUSED_WG_PER_CU": "0"}).stdout)
    assert (k["spill_load"], k["mp_max"], k["lds_budget_kb"], k["fused_wg_per_cu"]) == (7, 8, 16, 1)
    # ... and these fall back (QE_SPILL_MAXPCT to 0, round 4's rule; the others to their defaults)
    k = json.loads(_run(exe, ["knobs"], {"QE_COMPACT_LOAD": "100", "QE_SPILL_MAXPCT": "95", "QE_SPILL_SUBBUCKETS": "3",
                                         "QE_PART_FILL_SHIFT": "4", "QE_PART_FAST_FILL": "5", "QE_PART_WG_PER_CU": "33",
                                         "QE_PAGG_SLICES_PER_CU": "0"}).stdout)
    assert (k["compact_load"], k["spill_maxpct"], k["spill_subbuckets"], k["part_fill_shift"], k["part_fast_fill"],
            k["part_wg_per_cu"], k["pagg_slices_per_cu"]) == (98, 0, 2, 0, 0, 2, 8)
    # flags: only a leading 0 turns one off, only a leading 1 opts into the two compact passes
    k = json.loads(_run(exe, ["knobs"], {"QE_LDS_COMPACT": "0", "QE_MP_SPILL": "0", "QE_COMPACT_SPILL": "0",
                                         "QE_PART_NARROW": "0", "QE_NN_IMPLICIT": "0", "QE_COMPACT_TWOPASS": "1",
                                         "QE_PART_CHUNKED": "0"}).stdout)
    assert (k["lds_compact"], k["mp_spill"], k["compact_spill"], k["part_narrow"], k["nn_implicit"],
            k["compact_twopass"], k["part_chunked"]) == (0, 0, 0, 0, 0, 1, 0)
    k = json.loads(_run(exe, ["knobs"], {"QE_LDS_COMPACT": "no", "QE_COMPACT_TWOPASS": "yes", "QE_PART_CHUNKED": "yes"}).stdout)
    assert (k["lds_compact"], k["compact_twopass"], k["part_chunked"]) == (1, 0, 1)
