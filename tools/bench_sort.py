#!/usr/bin/env python3
"""ORDER BY measurements on one MI355X: qe_sort_indices against torch.sort(stable=True) on the same
device tensor, qe_take, and the single-workgroup path.

  python tools/bench_sort.py [--rows 10000000,100000000] [--reps 10] [--keys int64_full_range] [--out profiles/sort.json]

Times are device events on the ctx stream around one call (warm-up first, median of --reps, the two
contenders alternated inside one loop). A qe_sort_indices call reads one histogram back per key word,
so its event time includes those host round trips: it is the call's time, not a kernel sum.
torch.sort returns int64 indices and moves int64 values (8 + 8 bytes per row and pass, where
qe_sort_indices moves 8 + 4); torch has no multi-key sort, so the (UINT8, DATE32) pair is given to it
pre-packed into one int64 (the packing is not timed).
Algorithmic bytes of a sort = rows x [key bytes + 12 (encoded word and index written) + passes x
(8 counted + 12 read + 12 written) - 8 (the last pass of a word writes no words)], passes = the digits
that are not constant over all rows (computed here with torch from the same columns). qe_take of two
8-byte columns = rows x (4 + 2 x 8 + 2 x 8). TB/s = those bytes over the median; share = TB/s over
8 TB/s (HBM3E peak).
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "query-engines_amd"))

HBM_TBS = 8.0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="10000000,100000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--keys", default="", help="comma-separated key-set names to time (default: all)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sort.json"))
    args = ap.parse_args()

    import torch

    from kquery import native as N
    from kquery.columnar import Context, DeviceColumn
    from kquery.datasource import ColumnSpec, generate_column
    from kquery.operators import sort_indices, sort_layout, take

    if not torch.cuda.is_available():
        print("bench_sort needs a GPU (there is no CPU fallback)", file=sys.stderr)
        return 2
    ctx = Context.get(0)
    MIN64 = -(1 << 63)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def passes_of(word):  # digits of the encoded int64 word that vary over the rows
        return sum(int(((word >> (8 * g)) & 255).min().item() != ((word >> (8 * g)) & 255).max().item()) for g in range(8))

    def key_sets(n):
        full = generate_column(ColumnSpec("full", N.TYPE_INT64, N.GEN_RAW, 0, 0), n, 0, 7, ctx)
        narrow = generate_column(ColumnSpec("narrow", N.TYPE_INT64, N.GEN_MOD, 1 << 20, 1), n, 0, 7, ctx)
        f64 = generate_column(ColumnSpec("f64", N.TYPE_FLOAT64, N.GEN_UNIT53, 0, 2), n, 0, 7, ctx)
        u8 = DeviceColumn(N.TYPE_UINT8, n, (full.values[:n] & 0xFF).to(torch.uint8), None, None, ctx)
        d32 = DeviceColumn(N.TYPE_DATE32, n, (18000 + (narrow.values[:n] % 3650)).to(torch.int32), None, None, ctx)
        fb = f64.values[:n].view(torch.int64)
        packed = (u8.values.to(torch.int64) << 32) | (d32.values.to(torch.int64) + (1 << 31))
        yield "int64_full_range", [full], full.values[:n], full.values[:n] ^ MIN64, 8
        yield "int64_below_2^20", [narrow], narrow.values[:n], narrow.values[:n] ^ MIN64, 8
        yield "float64_unit53", [f64], f64.values[:n], torch.where(fb < 0, ~fb, fb | MIN64), 8
        yield "uint8_date32_packed", [u8, d32], packed, packed, 5

    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "layout": dict(zip(("tile_rows", "small_max"), sort_layout())),
               "note": "ms = median device-event time of one call; ratio = torch.sort(stable) ms / qe_sort_indices ms "
                       "(torch sorts int64 values and returns int64 indices)", "sort": [], "take": [], "small": {}}
    for n in [int(x) for x in args.rows.split(",")]:
        perm = None
        for name, cols, tkey, word, key_bytes in key_sets(n):
            if args.keys and name not in args.keys.split(","):
                continue
            passes = passes_of(word)
            flags = [0] * len(cols)
            ours, theirs = [], []
            for r in range(args.warmup + args.reps):
                ms, idx = timed(lambda: sort_indices(cols, flags))
                ms_t, (_, tidx) = timed(lambda: torch.sort(tkey, stable=True))
                if r >= args.warmup:
                    ours.append(ms)
                    theirs.append(ms_t)
            same = bool(torch.equal(idx.values[:n].to(torch.int64), tidx))
            del tidx
            perm = idx if perm is None else perm
            mo, mt = statistics.median(ours), statistics.median(theirs)
            nbytes = n * (key_bytes + 12 + passes * 32 - (8 if passes else 0))
            tbs = nbytes / (mo * 1e-3) / 1e12
            row = {"rows": n, "keys": name, "passes": passes, "qe_ms": round(mo, 4), "qe_ms_min": round(min(ours), 4),
                   "qe_ms_max": round(max(ours), 4), "torch_ms": round(mt, 4), "ratio": round(mt / mo, 3),
                   "algorithmic_bytes": nbytes, "tb_per_s": round(tbs, 3), "share_of_8tbs": round(tbs / HBM_TBS, 3),
                   "same_permutation_as_torch": same}
            results["sort"].append(row)
            print(json.dumps(row), flush=True)
        a = generate_column(ColumnSpec("a", N.TYPE_INT64, N.GEN_RAW, 0, 3), n, 0, 7, ctx)
        b = generate_column(ColumnSpec("b", N.TYPE_FLOAT64, N.GEN_UNIT53, 0, 4), n, 0, 7, ctx)
        ts = []
        for r in range(args.warmup + args.reps):
            ms, _ = timed(lambda: take(perm, [a, b]))
            if r >= args.warmup:
                ts.append(ms)
        m = statistics.median(ts)
        nbytes = n * (4 + 32)
        row = {"rows": n, "columns": "int64 + float64, a full-range key's permutation", "qe_ms": round(m, 4),
               "algorithmic_bytes": nbytes, "tb_per_s": round(nbytes / (m * 1e-3) / 1e12, 3),
               "share_of_8tbs": round(nbytes / (m * 1e-3) / 1e12 / HBM_TBS, 3),
               "note": "includes the output allocations of the Python wrapper and the call's one synchronisation"}
        results["take"].append(row)
        print(json.dumps(row), flush=True)
        del a, b, perm

    # single-workgroup path: wall time per call of a 1,024-row sort (what ORDER BY over a GROUP BY result costs)
    small = generate_column(ColumnSpec("s", N.TYPE_FLOAT64, N.GEN_UNIT53, 0, 5), 1024, 0, 7, ctx)
    calls = 200
    for fn, key in ((lambda: sort_indices([small], [0]), "qe_us_per_call"),
                    (lambda: torch.sort(small.values[:1024], stable=True), "torch_us_per_call")):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        results["small"][key] = round((time.perf_counter() - t0) / calls * 1e6, 2)
    results["small"]["rows"] = 1024
    results["small"]["note"] = "host wall time per call over 200 back-to-back calls ending in one synchronise"
    print(json.dumps(results["small"]), flush=True)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
