#!/usr/bin/env python3
"""Equi-join measurements on one MI355X: qe_join_build and qe_join_probe against a torch formulation
of the same join on the same device tensors (sort the build keys once, then searchsorted per probe
batch and expand the runs).

  python tools/bench_join.py [--cases pkfk_1m,pkfk_64m,mod7,skew] [--reps 10] [--scale 1.0] [--out profiles/join.json]

Cases (INT64 keys, inner join, no nulls):
  pkfk_1m   100M probe rows against 1M unique build keys, every probe row matches once
  pkfk_64m  100M probe rows against 64M unique build keys
  mod7      10M probe rows against 1K build rows of key mod 7 (about 143 build rows per probe row)
  skew      200K build rows, a quarter of them one key; 30K probe rows on that key (1.5G pairs)
--scale multiplies every row count (rehearsals and smaller devices).

Times are device events on the ctx stream around one call (warm-up first, median of --reps, the two
contenders alternated inside one loop). Both of our calls read a count back (the build its longest
run, the probe its pair count), so an event time includes that host round trip and the Python
wrapper's output allocations: it is the call's time, not a kernel sum. The probe is given the exact
pair capacity, so it runs once (count, scan, emit).
Bytes a pass must move, from the shapes: build = rows x 8 (keys) + slots x 16 (the table written);
probe = 2 x probe rows x 8 (the count and the emit pass each read the keys) + pairs x 8 (two INT32
written) + pairs x 4 (rows[] read) when the build side has duplicate keys. The table gathers are
listed apart (gather_bytes = 2 x probe rows x one 64-byte line): they are served by the caches for a
table that fits them and by HBM otherwise. TB/s = the pass's bytes over its median time.

--marks adds, per case and inside the same loop (so on the same table, right after the untracked
probe): the tracked probe (QE_JOIN_INNER | QE_JOIN_TRACK, the same capacity; the table is fresh in
every repetition, so the time includes allocating and clearing the mark bitmap) and, after it,
join_build_rows(matched). New keys: qe_probe_tracked_ms (+ _min / _max), tracked_ratio = tracked ms /
untracked ms, matched_rows, build_rows_ms (+ _min / _max), build_rows_bytes and build_rows_gb_per_s.
build_rows_bytes is the least the call can move: the bitmap (slots / 8) and the slots (slots x 16)
read, rows[] read (build rows x 4) when the build side has duplicate keys, the matched indices written
(matched rows x 4); its working bytes (one per build row, written once and read twice) are on top.
The call reads its count back, so its time holds that round trip too.
"""
import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "query-engines_amd"))

ODD = 0x9E3779B97F4A7C15 - (1 << 64)  # an odd multiplier: i -> i * ODD is a bijection of the int64 values


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="pkfk_1m,pkfk_64m,mod7,skew")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "join.json"))
    ap.add_argument("--marks", action="store_true", help="also time the tracked probe and join_build_rows")
    args = ap.parse_args()

    import torch

    from kquery import native as N
    from kquery.columnar import Context, DeviceColumn
    from kquery.operators import join_build, join_build_rows, join_probe, join_stats

    if not torch.cuda.is_available():
        print("bench_join needs a GPU (there is no CPU fallback)", file=sys.stderr)
        return 2
    ctx = Context.get(0)
    dev = ctx.torch_device

    def rows(n):
        return max(1, int(n * args.scale))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    def col(t):
        return DeviceColumn(N.TYPE_INT64, t.numel(), t, None, None, ctx)

    def data(case):
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        if case in ("pkfk_1m", "pkfk_64m"):
            nb, m = rows(1_000_000 if case == "pkfk_1m" else 64_000_000), rows(100_000_000)
            b = torch.randperm(nb, device=dev, generator=g) * ODD
            return b, b[torch.randint(0, nb, (m,), device=dev, generator=g)]
        if case == "mod7":
            return (torch.randint(0, 7, (rows(1_000),), device=dev, generator=g),
                    torch.randint(0, 7, (rows(10_000_000),), device=dev, generator=g))
        nb, m = rows(200_000), rows(30_000)
        b = torch.randint(0, 7, (nb,), device=dev, generator=g)
        b[torch.randperm(nb, device=dev, generator=g)[: nb // 4]] = 1000
        return b, torch.full((m,), 1000, dtype=torch.int64, device=dev)

    def torch_build(b):
        return torch.sort(b, stable=True)

    def torch_probe(sk, perm, p):
        lo = torch.searchsorted(sk, p, right=False)
        cnt = torch.searchsorted(sk, p, right=True) - lo
        pi = torch.repeat_interleave(torch.arange(p.numel(), device=dev), cnt)
        first = torch.cumsum(cnt, 0) - cnt
        bi = perm[lo[pi] + (torch.arange(pi.numel(), device=dev) - first[pi])]
        return pi, bi

    results = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "scale": args.scale,
               "note": "ms = median device-event time of one call (its read-back and the wrapper's allocations included); "
                       "ratio = torch ms / qe ms; torch = sort the build keys (build), searchsorted + run expansion (probe), "
                       "with int64 indices", "cases": []}
    for case in [c for c in args.cases.split(",") if c]:
        b, p = data(case)
        bc, pc = col(b), col(p)
        table = join_build(bc)
        _, distinct, max_dup, slots = join_stats(table)
        pi, bi = join_probe(table, pc)
        pairs = pi.length
        table.close()
        row = {"case": case, "build_rows": b.numel(), "probe_rows": p.numel(), "pairs": pairs, "distinct": distinct,
               "max_dup": max_dup, "slots": slots}
        try:  # the torch formulation holds several int64 temporaries of `pairs` rows
            sk, perm = torch_build(b)
            tpi, tbi = torch_probe(sk, perm, p)
            row["same_pairs_as_torch"] = bool(torch.equal(pi.values[:pairs].to(torch.int64), tpi)
                                              and torch.equal(bi.values[:pairs].to(torch.int64), tbi))
            del tpi, tbi
            with_torch = True
        except RuntimeError as e:
            row["torch"] = f"not measured: {str(e).splitlines()[0][:120]}"
            with_torch = False
        del pi, bi
        qb, qp, tb, tp, qt, qr = [], [], [], [], [], []
        matched_rows = 0
        for r in range(args.warmup + args.reps):
            ms_b, table = timed(lambda: join_build(bc))
            ms_p, out = timed(lambda: join_probe(table, pc, N.JOIN_INNER, capacity=pairs))
            del out
            if args.marks:
                ms_t, out = timed(lambda: join_probe(table, pc, N.JOIN_INNER | N.JOIN_TRACK, capacity=pairs))
                del out
                ms_r, out = timed(lambda: join_build_rows(table, True))
                matched_rows = out.length
                del out
                if r >= args.warmup:
                    qt.append(ms_t)
                    qr.append(ms_r)
            table.close()
            if with_torch:
                ms_tb, (sk, perm) = timed(lambda: torch_build(b))
                ms_tp, out = timed(lambda: torch_probe(sk, perm, p))
                del out
            if r >= args.warmup:
                qb.append(ms_b)
                qp.append(ms_p)
                if with_torch:
                    tb.append(ms_tb)
                    tp.append(ms_tp)
        build_bytes = b.numel() * 8 + slots * 16
        probe_bytes = 2 * p.numel() * 8 + pairs * 8 + (pairs * 4 if max_dup > 1 else 0)
        mb, mp = statistics.median(qb), statistics.median(qp)
        row.update({"qe_build_ms": round(mb, 4), "qe_build_ms_min": round(min(qb), 4), "qe_build_ms_max": round(max(qb), 4),
                    "qe_probe_ms": round(mp, 4), "qe_probe_ms_min": round(min(qp), 4), "qe_probe_ms_max": round(max(qp), 4),
                    "build_bytes": build_bytes, "probe_bytes": probe_bytes, "gather_bytes": 2 * p.numel() * 64,
                    "build_tb_per_s": round(build_bytes / (mb * 1e-3) / 1e12, 4),
                    "probe_tb_per_s": round(probe_bytes / (mp * 1e-3) / 1e12, 4),
                    "probe_rows_per_us": round(p.numel() / (mp * 1e3), 2), "pairs_per_us": round(pairs / (mp * 1e3), 2)})
        if args.marks:
            mt, mr = statistics.median(qt), statistics.median(qr)
            rows_bytes = slots // 8 + slots * 16 + (b.numel() * 4 if max_dup > 1 else 0) + matched_rows * 4
            row.update({"qe_probe_tracked_ms": round(mt, 4), "qe_probe_tracked_ms_min": round(min(qt), 4),
                        "qe_probe_tracked_ms_max": round(max(qt), 4), "tracked_ratio": round(mt / mp, 4),
                        "matched_rows": matched_rows, "build_rows_ms": round(mr, 4), "build_rows_ms_min": round(min(qr), 4),
                        "build_rows_ms_max": round(max(qr), 4), "build_rows_bytes": rows_bytes,
                        "build_rows_gb_per_s": round(rows_bytes / (mr * 1e-3) / 1e9, 3)})
        if with_torch:
            mtb, mtp = statistics.median(tb), statistics.median(tp)
            row.update({"torch_build_ms": round(mtb, 4), "torch_probe_ms": round(mtp, 4),
                        "build_ratio": round(mtb / mb, 3), "probe_ratio": round(mtp / mp, 3)})
        results["cases"].append(row)
        print(json.dumps(row), flush=True)
        del b, p, bc, pc
        torch.cuda.empty_cache()
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
