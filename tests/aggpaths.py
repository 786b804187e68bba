"""What a GROUP BY update's note (qe_hashagg_last_kernel_kind) says the path choice decided, in the
terms of the planner (qe_agg_paths.hpp), and the golden record of the notes (tests/golden/agg_paths.json).
Record counts and timings in a note are not part of the decision and are dropped."""
import json
import pathlib
import re

# every knob the path choice and the sizing read (AggKnobs, qe_agg_paths.hpp)
KNOBS = ["QE_LDS_COMPACT", "QE_COMPACT_LOAD", "QE_COMPACT_SPILL", "QE_COMPACT_TWOPASS", "QE_SPILL_MAXPCT",
         "QE_SPILL_SUBBUCKETS", "QE_SPILL_LOAD", "QE_MP_MAX", "QE_MP_SPILL", "QE_LDS_BUDGET_KB", "QE_PART_NARROW",
         "QE_PART_FILL_SHIFT", "QE_PART_FAST_FILL", "QE_PART_WG_PER_CU", "QE_PART_CHUNKED", "QE_PAGG_SLICES_PER_CU",
         "QE_FUSED_WG_PER_CU", "QE_NN_IMPLICIT"]
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "agg_paths.json"

_RECORDS = r"(?P<rb>\d+) B(?: records)? \((?P<words>column|value) words(?P<narrow>, 32-bit)?\)"
_SPILL = re.compile(r"^multi-pass: 2 buckets(?P<compact> \(compact kept table\))?, bucket 1 spilled"
                    r"(?: in (?P<sb>\d+) sub-buckets)? as " + _RECORDS + "$")
_PART = re.compile(r"^radix-partitioned: (?P<np>\d+) buckets, (?:(?P<chunked>chunked records)|\d+ records) of " + _RECORDS +
                   r"(?P<staged>, staged scatter)?$")
_PASSES = re.compile(r"^multi-pass: (?P<n>\d+) bucket passes(?P<compact> \(compact table\))?(?:; .*)?$")
_COMPACT = re.compile(r"^compact LDS table: (?P<slots>\d+) slots$")


def _records(m):
    return {"record_bytes": int(m["rb"]), "colmode": m["words"] == "column", "narrow": m["narrow"] is not None}


def decided(note: str, specialized: bool) -> dict:
    """The decided fields of a note: path, and what that path fixes."""
    m = _SPILL.match(note)
    if m:
        return {"path": "compact_spill" if m["compact"] else "spill", "sub_buckets": int(m["sb"] or 1), **_records(m)}
    m = _PART.match(note)
    if m:
        return {"path": "partition", "buckets": int(m["np"]), "chunked": m["chunked"] is not None, **_records(m)}
    m = _PASSES.match(note)
    if m:
        return {"path": "compact_twopass" if m["compact"] else "keyhash", "mp_n": int(m["n"])}
    m = _COMPACT.match(note)
    if m:
        return {"path": "compact", "compact_slots": int(m["slots"])}
    if note == "" and specialized:
        return {"path": "regular"}
    if "global-only launch" in note or "generic kernel: 0 KiB" in note:
        return {"path": "global"}
    if not specialized and note.startswith("jit disabled"):
        return {"path": "regular"}
    raise AssertionError(f"note not understood: {note!r} (specialized {specialized})")


def planned(rec: dict) -> dict:
    """The same fields from one line of tests/native/agg_paths.cpp's ladder output."""
    path = rec["path"]
    records = {"record_bytes": rec["record_bytes"], "colmode": bool(rec["colmode"]), "narrow": bool(rec["narrow"])}
    if path in ("compact_spill", "spill"):
        return {"path": path, "sub_buckets": rec["sub_buckets"], **records}
    if path == "partition":
        return {"path": path, "buckets": rec["buckets"], "chunked": bool(rec["chunked"]), **records}
    if path in ("compact_twopass", "keyhash"):
        return {"path": path, "mp_n": rec["mp_n"]}
    if path == "compact":
        return {"path": path, "compact_slots": rec["compact_slots"]}
    return {"path": path}


def golden() -> dict:
    return json.loads(GOLDEN.read_text())


def boundary_points(records, key=lambda d: d) -> list:
    """Grid points on either side of each change of key(decided fields), in grid order."""
    pts = []
    for a, b in zip(records, records[1:]):
        if key(decided(a["note"], a["specialized"])) != key(decided(b["note"], b["specialized"])):
            pts += [g for g in (a["groups"], b["groups"]) if g not in pts]
    return pts
