#!/usr/bin/env python3
"""Window-function measurements on one MI355X: qe_window_boundaries (twice) + qe_window_eval beside
the qe_sort_indices call they follow, on the same keys in the same run.

  python tools/bench_window.py [--rows 100000000] [--partitions 1,1000,10000000] [--reps 5] [--functions all] [--out profiles/window.json]

The window is PARTITION BY p ORDER BY o with p = u mod partitions and o = u mod 2^20 (INT64, so there
are peers), over an INT64 input with 10 % nulls and a FLOAT64 input. Each function family runs alone
and all eight functions run together; the bounded-frame families (qe_window_eval_frames) are SUM, MIN and
FIRST_VALUE over ROWS BETWEEN lo AND hi at widths 3, 1001 and 1 000 001, centred on the current row
(`_c`) and trailing it (`_t`), beside `min_rows`, the running MIN they are compared with. Times are device events on the ctx stream around the calls
(warm-up first, median of --reps). qe_window_eval ends with its one read-back (the out-of-range flag),
and qe_sort_indices reads a histogram back per key word, so both times include those host round trips.
`stream_ms` is what the bytes the window calls touch would take at qe_stream_read_best's rate, by this
count of bytes per row (scattered 4- and 8-byte accesses counted at their size, not at the cache
line's): boundaries 2 x (4 + 8 per key) per call; inverse permutation 4 + 4; each scan 4 + 8 gathered,
12 staged, 12 read back and 12 written (a bounded MIN / MAX runs two scans and reads a value of each); evaluation
12 per scan value read (LAG / LEAD / FIRST_VALUE / LAST_VALUE: 4 + 8) and a
staging record of 8 per function + 8 written, read back once, then 8 per function written.
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
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--partitions", default="1,1000,10000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--functions", default="", help="comma-separated family names to time (default: all of them); the rows "
                    "that --out already holds for other families, of the same device and row count, are kept")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "window.json"))
    args = ap.parse_args()

    import torch

    from kquery import native as N
    from kquery.columnar import Context
    from kquery.datasource import ColumnSpec, generate_column
    from kquery.operators import sort_indices, window_boundaries, window_eval, window_eval_frames, window_layout

    if not torch.cuda.is_available():
        print("bench_window needs a GPU (there is no CPU fallback)", file=sys.stderr)
        return 2
    ctx = Context.get(0)
    n = args.rows

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    x = generate_column(ColumnSpec("x", N.TYPE_INT64, N.GEN_MOD, 1 << 30, 3, 100), n, 0, 7, ctx)
    f = generate_column(ColumnSpec("f", N.TYPE_FLOAT64, N.GEN_UNIT53, 0, 4), n, 0, 7, ctx)
    okey = generate_column(ColumnSpec("o", N.TYPE_INT64, N.GEN_MOD, 1 << 20, 2), n, 0, 7, ctx)
    families = {
        "ranks": [(N.WIN_ROW_NUMBER, 0, 0, 0), (N.WIN_RANK, 0, 0, 0), (N.WIN_DENSE_RANK, 0, 0, 0)],
        "counts": [(N.WIN_COUNT_STAR, N.FRAME_RANGE, 0, 0), (N.WIN_COUNT, N.FRAME_ROWS, 0, 0)],
        "sum": [(N.WIN_SUM, N.FRAME_ROWS, 0, 0)],
        "min_max": [(N.WIN_MIN, N.FRAME_ROWS, 1, 0), (N.WIN_MAX, N.FRAME_RANGE, 1, 0)],
        "lag_lead": [(N.WIN_LAG, 0, 0, 1), (N.WIN_LEAD, 0, 1, 1)],
    }
    families["all"] = [(N.WIN_ROW_NUMBER, 0, 0, 0), (N.WIN_RANK, 0, 0, 0), (N.WIN_DENSE_RANK, 0, 0, 0),
                       (N.WIN_COUNT_STAR, N.FRAME_RANGE, 0, 0), (N.WIN_SUM, N.FRAME_ROWS, 0, 0),
                       (N.WIN_MIN, N.FRAME_ROWS, 1, 0), (N.WIN_MAX, N.FRAME_RANGE, 1, 0), (N.WIN_LAG, 0, 0, 1)]

    families["min_rows"] = [(N.WIN_MIN, N.FRAME_ROWS, 1, 0)]
    # bounded frames: (fn, frame, input, offset, lo, hi), through qe_window_eval_frames
    for width in (3, 1001, 1_000_001):
        for shape, (lo, hi) in (("c", (-(width // 2), width // 2)), ("t", (-(width - 1), 0))):
            for name, fn, inp in (("sum", N.WIN_SUM, 0), ("min", N.WIN_MIN, 1), ("first", N.WIN_FIRST_VALUE, 1)):
                families[f"{name}_w{width}_{shape}"] = [(fn, N.FRAME_ROWS_BETWEEN, inp, 0, lo, hi)]

    ms = N.C.c_double()
    shape = N.C.create_string_buffer(128)
    cc = (N.QeColumn * 1)(okey.as_c())
    N.check(N.lib().qe_stream_read_best(ctx.handle, cc, 1, 5, N.C.byref(ms), shape, 128))
    read_gbs = 8 * n / (ms.value * 1e-3) / 1e9

    def bytes_per_row(fns):
        scans, reads = set(), 0
        for f in fns:
            fn, frame, inp = f[:3]
            if fn in (N.WIN_COUNT, N.WIN_SUM):
                scans.add((1, inp, 0))
                reads += 12
            elif fn in (N.WIN_MIN, N.WIN_MAX):
                two = frame == N.FRAME_ROWS_BETWEEN  # (the families here have two finite bounds)
                scans.update({(fn, inp, f[5] - f[4] + 1, d) for d in (0, 1)} if two else {(fn, inp, 0)})
                reads += 24 if two else 12
            elif fn in (N.WIN_LAG, N.WIN_LEAD, N.WIN_FIRST_VALUE, N.WIN_LAST_VALUE):
                reads += 12
        b = 2 * (4 + 8) + 2 * (4 + 16)  # the two boundary calls: one key, two keys
        b += 8 + len(scans) * (12 + 3 * 12) + 4 + 2 * 8 * (len(fns) + 1)
        return b + 8 * len(fns) + reads

    results = {"device": torch.cuda.get_device_name(0), "rows": n, "reps": args.reps,
               "layout": dict(zip(("tile_rows", "small_max"), window_layout())),
               "stream_read_best": {"gb_per_s": round(read_gbs, 1), "shape": shape.value.decode()},
               "note": "ms = median device-event time (eval_ms_min / eval_ms_max: the least and the greatest of the reps); window_ms = two qe_window_boundaries + one qe_window_eval; sort_ms = "
                       "qe_sort_indices over the same two INT64 keys; stream_ms = the window calls' bytes at stream_read_best's rate",
               "window": []}
    for parts in [int(p) for p in args.partitions.split(",")]:
        pkey = generate_column(ColumnSpec("p", N.TYPE_INT64, N.GEN_MOD, parts, 1), n, 0, 7, ctx)
        keys = [pkey, okey]
        sort_ms = []
        for r in range(args.warmup + args.reps):
            t, order = timed(lambda: sort_indices(keys, [0, 0]))
            if r >= args.warmup:
                sort_ms.append(t)
        for name, fns in families.items():
            if args.functions and name not in args.functions.split(","):
                continue
            bnd, ev = [], []
            for r in range(args.warmup + args.reps):
                tb, (ps, gs) = timed(lambda: (window_boundaries(keys[:1], order), window_boundaries(keys, order)))
                call = window_eval_frames if len(fns[0]) == 6 else window_eval
                te, outs = timed(lambda: call(order, ps, gs, [x, f], fns))
                del outs
                if r >= args.warmup:
                    bnd.append(tb)
                    ev.append(te)
            b, e, s = statistics.median(bnd), statistics.median(ev), statistics.median(sort_ms)
            row = {"partitions": parts, "functions": name, "nfns": len(fns), "boundaries_ms": round(b, 3), "eval_ms": round(e, 3),
                   "eval_ms_min": round(min(ev), 3), "eval_ms_max": round(max(ev), 3),
                   "window_ms": round(b + e, 3), "sort_ms": round(s, 3), "window_over_sort": round((b + e) / s, 3),
                   "stream_ms": round(bytes_per_row(fns) * n / read_gbs / 1e6, 3)}
            results["window"].append(row)
            print(json.dumps(row), flush=True)
        del order, pkey
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    if args.functions and out.exists():  # a run of some families keeps the file's rows of the others
        old = json.loads(out.read_text())
        if old.get("device") == results["device"] and old.get("rows") == n:
            timed = {(r["partitions"], r["functions"]) for r in results["window"]}
            results["window"] = [r for r in old["window"] if (r["partitions"], r["functions"]) not in timed] + results["window"]
    out.write_text(json.dumps(results, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
