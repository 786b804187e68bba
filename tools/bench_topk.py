#!/usr/bin/env python3
"""ORDER BY ... LIMIT k measurements on one MI355X: qe_topk_indices in selection mode against the
truncated full sort (QE_TOPK_SORT, what qe_sort_indices(limit) does), and against torch.topk for the
single INT64 / FLOAT64 key.

  python tools/bench_topk.py [--rows 10000000,100000000] [--reps 7] [--keys int64_full_range] [--out profiles/topk.json]

Times are device events on the ctx stream around one call (warm-up first, median of --reps, the
contenders alternated inside one loop). Both qe_topk_indices modes read histograms back while they
run (qe_topk_last_stats counts the read-backs), so an event time includes those host round trips: it
is the call's time, not a kernel sum. torch.topk(largest=False, sorted=True) returns values and int64
indices and is not stable; it has no multi-key form, so the multi-key sets have no torch column.
k runs over 10, 1000, 100K, rows / 16 and rows / 4. Per row of the table: the selection's digit
steps, the candidates it handed to the final sort and its read-backs, and whether the two modes
returned the same bytes.
"""
import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "query-engines_amd"))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="10000000,100000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--keys", default="", help="comma-separated key-set names to time (default: all)")
    ap.add_argument("--ks", default="", help="comma-separated k values (default: 10,1000,100000,rows/16,rows/4)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "topk.json"))
    args = ap.parse_args()

    import torch

    from kquery import native as N
    from kquery.columnar import Context, DeviceColumn
    from kquery.datasource import ColumnSpec, generate_column
    from kquery.operators import sort_layout, topk_indices, topk_last_stats

    if not torch.cuda.is_available():
        print("bench_topk needs a GPU (there is no CPU fallback)", file=sys.stderr)
        return 2
    ctx = Context.get(0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def key_sets(n):
        full = generate_column(ColumnSpec("full", N.TYPE_INT64, N.GEN_RAW, 0, 0), n, 0, 7, ctx)
        narrow = generate_column(ColumnSpec("narrow", N.TYPE_INT64, N.GEN_MOD, 1 << 20, 1), n, 0, 7, ctx)
        f64 = generate_column(ColumnSpec("f64", N.TYPE_FLOAT64, N.GEN_UNIT53, 0, 2), n, 0, 7, ctx)
        u8 = DeviceColumn(N.TYPE_UINT8, n, (full.values[:n] & 0xFF).to(torch.uint8), None, None, ctx)
        d32 = DeviceColumn(N.TYPE_DATE32, n, (18000 + (narrow.values[:n] % 3650)).to(torch.int32), None, None, ctx)
        four = DeviceColumn(N.TYPE_INT64, n, (narrow.values[:n] & 3) * 1000, None, None, ctx)
        yield "int64_full_range", [full], full.values[:n]
        yield "int64_below_2^20", [narrow], narrow.values[:n]
        yield "uint8_date32_packed", [u8, d32], None
        yield "int64_4_values_then_float64", [four, f64], None

    layout = dict(zip(("tile_rows", "small_max"), sort_layout()))
    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "layout": layout,
               "note": "ms = median device-event time of one call; select = QE_TOPK_SELECT, sort = QE_TOPK_SORT (the full "
                       "sort, truncated); steps / candidates / read-backs from qe_topk_last_stats of the selection",
               "topk": []}
    for n in [int(x) for x in args.rows.split(",")]:
        ks = [int(x) for x in args.ks.split(",")] if args.ks else [10, 1000, 100_000, n // 16, n // 4]
        for name, cols, tkey in key_sets(n):
            if args.keys and name not in args.keys.split(","):
                continue
            flags = [0] * len(cols)
            for k in ks:
                k = min(k, n)
                sel, srt, tor = [], [], []
                for r in range(args.warmup + args.reps):
                    ms_a, a = timed(lambda: topk_indices(cols, flags, k, N.TOPK_SELECT))
                    st = topk_last_stats(ctx)
                    ms_b, b = timed(lambda: topk_indices(cols, flags, k, N.TOPK_SORT))
                    ms_t = None
                    if tkey is not None and not args.no_torch:
                        ms_t, _ = timed(lambda: torch.topk(tkey, k, largest=False, sorted=True))
                    if r >= args.warmup:
                        sel.append(ms_a)
                        srt.append(ms_b)
                        if ms_t is not None:
                            tor.append(ms_t)
                same = bool(torch.equal(a.values[:k], b.values[:k]))
                del a, b
                ms, mf = statistics.median(sel), statistics.median(srt)
                row = {"rows": n, "keys": name, "k": k, "select_ms": round(ms, 4), "select_ms_min": round(min(sel), 4),
                       "select_ms_max": round(max(sel), 4), "sort_ms": round(mf, 4), "sort_over_select": round(mf / ms, 3),
                       "torch_topk_ms": round(statistics.median(tor), 4) if tor else None, "path": st[0], "digit_steps": st[1],
                       "candidates": st[2], "read_backs": st[3], "same_indices_as_sort": same}
                results["topk"].append(row)
                print(json.dumps(row), flush=True)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
