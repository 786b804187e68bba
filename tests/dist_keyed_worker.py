"""Worker for tests/test_dist_keyed.py (launched by torch.distributed.run, 2 ranks sharing cuda:0,
gloo backend): each rank partial-aggregates its own rows of a string- and tuple-keyed table,
exchange_partials moves every group to its owner by key content, and rank 0 checks the union of
the owners' groups against the oracle over all rows."""
import json
import os
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "query-engines_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from oracle import semantics as S  # noqa: E402


def table(seed, n):
    rng = np.random.default_rng(seed)
    words = ["1", "2", "VTS", "", "Pärsson", "x" * 45]
    s = [None if rng.random() < 0.03 else words[i] for i in rng.integers(0, len(words), n)]
    k = rng.integers(-3, 4, n).astype(np.int64) * (2 ** 40)
    kv = rng.random(n) > 0.05
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    return s, k, kv, v


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from kquery import native as N
    from kquery.aggregate import HashAggregateState
    from kquery.columnar import Context, DeviceColumn
    from kquery.exchange import exchange_partials

    ctx = Context.get(0)
    results = {}
    for mode in ("utf8", "tuple"):
        s, k, kv, v = table(100 + rank, 30_000 + 7000 * rank)
        types = [N.TYPE_UTF8] if mode == "utf8" else [N.TYPE_UTF8, N.TYPE_INT64]
        aggs = [(N.AGG_SUM, N.TYPE_INT64), (N.AGG_COUNT_STAR, N.TYPE_INT64), (N.AGG_MIN, N.TYPE_INT64)]
        partial = HashAggregateState(ctx, types, aggs, 64)
        owner = HashAggregateState(ctx, types, aggs, 64)
        keys = [DeviceColumn.from_strings(s, ctx=ctx)]
        if mode == "tuple":
            keys.append(DeviceColumn.from_numpy(N.TYPE_INT64, k, kv, ctx=ctx))
        vc = DeviceColumn.from_numpy(N.TYPE_INT64, v, ctx=ctx)
        partial.update(keys, [vc, None, vc])
        exchange_partials(partial, owner)
        ko, ao = owner.finalize()
        cols = [c.to_pylist() for c in ko] + [c.to_pylist() for c in ao]
        mine = [list(r) for r in zip(*cols)]
        allrows = [None] * world
        dist.all_gather_object(allrows, mine)
        if rank == 0:
            got = {}
            for rows in allrows:
                for r in rows:
                    key = tuple(r[: len(types)])
                    assert key not in got, f"group {key} owned by two ranks"
                    got[key] = r[len(types):]
            ks, kk, kvs, vs = [], [], [], []
            for r in range(world):
                s2, k2, kv2, v2 = table(100 + r, 30_000 + 7000 * r)
                ks += s2
                kk += [int(x) if ok else None for x, ok in zip(k2, kv2)]
                vs += v2.tolist()
            kcols = [ks] if mode == "utf8" else [ks, kk]
            want = S.hash_aggregate_rows(kcols, [vs, [1] * len(vs), vs], [S.AGG_SUM, S.AGG_COUNT_STAR, S.AGG_MIN],
                                         [False] * 3)
            ok = len(got) == len(want) and all(got[key] == w for key, w in want.items())
            results[mode] = {"ok": ok, "groups": len(got)}
    # numeric keys: fixed-capacity slot exchange, and its fallback when a slot overflows
    for mode, cap in (("slots", None), ("slots_overflow", 50)):
        rng = np.random.default_rng(300 + rank)
        n = 50_000 + 1000 * rank
        k = rng.integers(0, 3000, n).astype(np.int64)
        kv = rng.random(n) > 0.01
        x = rng.normal(size=n)
        aggs = [(N.AGG_SUM, N.TYPE_INT64), (N.AGG_MAX, N.TYPE_FLOAT64), (N.AGG_COUNT_STAR, N.TYPE_INT64)]
        partial = HashAggregateState(ctx, [N.TYPE_INT64], aggs, 4096)
        owner = HashAggregateState(ctx, [N.TYPE_INT64], aggs, 4096)
        partial.set_row_base(rank * 10_000_000)
        kc = DeviceColumn.from_numpy(N.TYPE_INT64, k, kv, ctx=ctx)
        partial.update([kc], [kc, DeviceColumn.from_numpy(N.TYPE_FLOAT64, x, ctx=ctx), None])
        exchange_partials(partial, owner, slot_records=cap)
        ko, ao = owner.finalize()
        mine = [list(r) for r in zip(*([c.to_pylist() for c in ko] + [c.to_pylist() for c in ao]))]
        allrows = [None] * world
        dist.all_gather_object(allrows, mine)
        if rank == 0:
            got = {}
            for rows in allrows:
                for r in rows:
                    assert r[0] not in got, f"group {r[0]} owned by two ranks"
                    got[r[0]] = r[1:]
            kk, xs = [], []
            for r in range(world):
                g = np.random.default_rng(300 + r)
                n2 = 50_000 + 1000 * r
                k2 = g.integers(0, 3000, n2).astype(np.int64)
                kv2 = g.random(n2) > 0.01
                kk += [int(a) if ok else None for a, ok in zip(k2, kv2)]
                xs += g.normal(size=n2).tolist()
            want = S.hash_aggregate_rows([kk], [kk, xs, [1] * len(kk)], [S.AGG_SUM, S.AGG_MAX, S.AGG_COUNT_STAR],
                                         [False, True, False])
            ok = len(got) == len(want) and all(got[key[0]] == w for key, w in want.items())
            results[mode] = {"ok": ok, "groups": len(got)}
    # deterministic fp64 SUM / AVG across ranks: the exchanged partials carry exact fixed-point
    # limbs, so every group equals math.fsum over both ranks' rows bit for bit
    import math

    rng = np.random.default_rng(700 + rank)
    n = 60_000 + 5000 * rank
    k = rng.integers(0, 900, n).astype(np.int64)
    x = np.round(rng.normal(size=n) * np.exp2(rng.integers(-10, 25, n)) * 2.0 ** 50) * 2.0 ** -50
    aggs = [(N.AGG_SUM, N.TYPE_FLOAT64), (N.AGG_AVG, N.TYPE_FLOAT64), (N.AGG_COUNT_STAR, N.TYPE_INT64)]
    partial = HashAggregateState(ctx, [N.TYPE_INT64], aggs, 1024, deterministic=True)
    owner = HashAggregateState(ctx, [N.TYPE_INT64], aggs, 1024, deterministic=True)
    partial.set_row_base(rank * 10_000_000)
    partial.update([DeviceColumn.from_numpy(N.TYPE_INT64, k, ctx=ctx)],
                   [DeviceColumn.from_numpy(N.TYPE_FLOAT64, x, ctx=ctx)] * 2 + [None])
    exchange_partials(partial, owner)
    ko, ao = owner.finalize()
    mine = [(int(a), float(b), float(c), int(d)) for a, b, c, d in
            zip(ko[0].to_numpy(), ao[0].to_numpy(), ao[1].to_numpy(), ao[2].to_numpy())]
    allrows = [None] * world
    dist.all_gather_object(allrows, mine)
    if rank == 0:
        got = {r[0]: r[1:] for rows in allrows for r in rows}
        kk, xs = [], []
        for q in range(world):
            g = np.random.default_rng(700 + q)
            n2 = 60_000 + 5000 * q
            k2 = g.integers(0, 900, n2).astype(np.int64)
            x2 = np.round(g.normal(size=n2) * np.exp2(g.integers(-10, 25, n2)) * 2.0 ** 50) * 2.0 ** -50
            kk.append(k2)
            xs.append(x2)
        kk, xs = np.concatenate(kk), np.concatenate(xs)
        ok = len(got) == len(np.unique(kk))
        for key in np.unique(kk):
            v = xs[kk == key].tolist()
            s_, a_, c_ = got[int(key)]
            ok = ok and s_ == math.fsum(v) and a_ == math.fsum(v) / len(v) and c_ == len(v)
        results["deterministic"] = {"ok": bool(ok), "groups": len(got)}
    # global aggregate over rank shards: one all-gather of partials, identical merge on every rank
    from kquery.exchange import global_aggregate

    g = np.random.default_rng(500 + rank)
    n = 40_000 + 333 * rank
    x = g.normal(size=n)
    xv = g.random(n) > 0.05
    if rank == 1:
        x[:3] = [np.nan, -0.0, 5.0]  # NaN first in rank 1: rank 0's rows come first, so no seed
    r = global_aggregate(DeviceColumn.from_numpy(N.TYPE_FLOAT64, x, xv, ctx=ctx), row_base=rank * 10_000_000)
    mine = [r.rows, r.count, r.sum, r.min, r.max]
    everyone = [None] * world
    dist.all_gather_object(everyone, mine)
    if rank == 0:
        xs, vs = [], []
        for q in range(world):
            g2 = np.random.default_rng(500 + q)
            n2 = 40_000 + 333 * q
            x2 = g2.normal(size=n2)
            v2 = g2.random(n2) > 0.05
            if q == 1:
                x2[:3] = [np.nan, -0.0, 5.0]
            xs.append(x2)
            vs.append(v2)
        want = S.global_aggregate(np.concatenate(xs), np.concatenate(vs))
        from kquery.columnar import f64_from_bits

        same = all(e == everyone[0] for e in everyone)  # every rank merged to the same bits
        ok = (same and r.rows == want["rows"] and r.count == want["count"]
              and S.rows_equal(f64_from_bits(r.sum), want["sum"], 0.0)
              and S.rows_equal(f64_from_bits(r.min), want["min"]) and S.rows_equal(f64_from_bits(r.max), want["max"]))
        results["global"] = {"ok": bool(ok)}
    if rank == 0:
        print("RESULT " + json.dumps(results), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
