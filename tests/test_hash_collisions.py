"""The string and key-tuple dictionaries (qe_strdict.hip) under forged 64-bit hash collisions.

The dictionary finds a key by its hash and only then compares content: in dict_probe's eq()
(bytes_equal / tuple_eq), in the per-workgroup LDS cache (lc_find), in the wave's leader election
(wave_leader) and, implicitly, in k_dict_rebuild, which re-chains codes by their stored hashes.
Ordinary test strings never share a hash, so none of those comparisons ever has to say "no" after
a hash match. tests/hashforge.py forges classes of different keys with ONE hash; here they go
through encode / decode, the tuple dictionary, whole GROUP BYs and a keyed merge, and every result
is compared with a Python dict keyed by the raw bytes (or the tuples).

qe_hash_partition is the public window onto the device's str_hash: it is compared row for row with
the restatement, and every forged class must land in one partition of 2^31 - 1, so a change of the
device hash makes these tests fail instead of pass without collisions.

The forged strings are arbitrary bytes, not valid UTF-8: columns are built from raw bytes and
results are compared through offsets and values, never decoded to str.
"""
import functools

import numpy as np
import pytest

import hashforge as F

# (length, first of the two forged words). 40 / 41 sit on either side of LC_BYTES = 40 (the LDS
# cache and the leader election only take keys of at most 40 bytes) and differ inside the 40-byte
# head; 59 / 64 differ only in bytes 40..55, so their members share the whole head.
CLASS_SPECS = [(16, 0), (19, 0), (40, 3), (41, 3), (59, 5), (64, 5)]
CLASS_OLD, CLASS_NEW = 24, 8  # 24 > LC_PROBES = 8: most members of a class stay out of the LDS cache
BIG_OLD, BIG_NEW = 300, 20  # more than a wave of members; a chain well under MAX_PROBES
MAX_PROBES = 1024  # qe_strdict.hip MAX_PROBES: slots a lookup visits before it gives up
NPARTS_31 = (1 << 31) - 1


class Data:
    pass


def _random_keys(rng, count, taken):
    out = []
    while len(out) < count:
        b = rng.bytes(int(rng.integers(8, 71)))
        if b not in taken:
            taken.add(b)
            out.append(b)
    return out


def _rows(rng, pool, n, nulls):
    """n rows over `pool`, every member at least once, shuffled, a share of nulls (None)."""
    idx = np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), n - len(pool))])
    idx[len(pool):][rng.random(n - len(pool)) < nulls] = -1  # (never a member's one sure row)
    rng.shuffle(idx)
    return [None if i < 0 else pool[i] for i in idx]


@functools.lru_cache(maxsize=None)
def data() -> Data:
    rng = np.random.default_rng(20250117)
    d = Data()
    d.classes = {ln: F.forge_strings(rng.bytes(ln), blk, CLASS_OLD + CLASS_NEW, rng) for ln, blk in CLASS_SPECS}
    d.big = F.forge_strings(rng.bytes(16), 0, BIG_OLD + BIG_NEW, rng)
    d.chain = F.forge_strings(rng.bytes(16), 0, MAX_PROBES + 6, rng)
    taken = set(d.big) | set(d.chain) | {m for c in d.classes.values() for m in c}
    d.rand = _random_keys(rng, 200, taken)
    d.fresh = _random_keys(rng, 1500, taken)  # enough new codes to outgrow the first 1024
    d.pool1 = [m for c in d.classes.values() for m in c[:CLASS_OLD]] + d.big[:BIG_OLD] + d.rand
    d.batch1 = _rows(rng, d.pool1, 20_000, 0.03)
    d.values1 = rng.integers(-10**9, 10**9, len(d.batch1)).astype(np.int64)
    d.second1 = rng.integers(0, 3, len(d.batch1)).astype(np.int64)
    new = [m for c in d.classes.values() for m in c[CLASS_OLD:]] + d.big[BIG_OLD:]
    pool2 = [d.pool1[i] for i in rng.integers(0, len(d.pool1), 600)] + new + d.fresh
    d.batch2 = _rows(rng, pool2, 4000, 0.03)
    # one wave's first step: 64 different members of one class in rows 0..63
    tail = d.big[:64] + d.rand[:20]
    d.wave = d.big[:64] + [tail[i] for i in rng.integers(0, len(tail), 257 - 64)]
    # (int64, int64) key tuples: one forged class, random pairs, fresh pairs for growth
    d.tclass = F.forge_tuples(100 + 20, rng)
    pairs = {tuple(int(x) for x in p) for p in rng.integers(-2**63, 2**63 - 1, (3300, 2), dtype=np.int64)}
    pairs = sorted(pairs - set(d.tclass))[:3200]
    rng.shuffle(pairs)
    pairs = [tuple(int(x) for x in p) for p in pairs]
    d.tpool1 = d.tclass[:100] + pairs[:200]
    d.tbatch1 = [d.tpool1[i] for i in _rows(rng, list(range(len(d.tpool1))), 20_000, 0.0)]
    tpool2 = [d.tpool1[i] for i in rng.integers(0, len(d.tpool1), 300)] + d.tclass[100:] + pairs[200:]
    d.tbatch2 = [tpool2[i] for i in _rows(rng, list(range(len(tpool2))), 5000, 0.0)]
    return d


def _forged_string_classes(d):
    return list(d.classes.values()) + [d.big, d.chain]


# ---- CPU: the forger's own conditions, on the data the GPU tests use -------------------------------
def test_forged_string_classes_collide_and_differ():
    d = data()
    hashes = set()
    for members in _forged_string_classes(d):
        assert len(set(members)) == len(members)  # pairwise distinct
        assert len({len(m) for m in members}) == 1
        assert len(members[0]) >= 8  # longer than a packed wide code: every member enters the dictionary
        hs = {F.str_hash(m) for m in members}
        assert len(hs) == 1  # one restated hash per class
        hashes |= hs
    assert len(hashes) == len(CLASS_SPECS) + 2  # the classes themselves do not collide
    others = d.rand + d.fresh
    assert len(set(others)) == len(others) and all(len(b) >= 8 for b in others)
    assert hashes.isdisjoint({F.str_hash(b) for b in others})
    assert len(d.chain) == MAX_PROBES + 6 and len(d.big) < MAX_PROBES


def test_forged_string_classes_prefix_properties():
    d = data()
    for ln, blk in CLASS_SPECS:
        members = d.classes[ln]
        base = members[0]
        lo, hi = 8 * blk, 8 * blk + 16
        for m in members:
            assert len(m) == ln and m[:lo] == base[:lo] and m[hi:] == base[hi:]  # only the two words differ
        words = {m[lo:lo + 8] for m in members}
        assert len(words) == len(members)
    for ln in (59, 64):  # same 40-byte head (and same length, same hash): only bytes_equal separates them
        assert len({m[:40] for m in d.classes[ln]}) == 1
        assert len({m[40:56] for m in d.classes[ln]}) == len(d.classes[ln])
    for ln in (40, 41):  # differ inside the head, which ends at byte 40
        assert len({m[:40] for m in d.classes[ln]}) == len(d.classes[ln])
        assert len({m[40:] for m in d.classes[ln]}) == 1
    for ln in (16, 19):
        assert len({m[:16] for m in d.classes[ln]}) == len(d.classes[ln])
    assert d.wave[:64] == d.big[:64] and len(set(d.wave[:64])) == 64 and len(d.wave) == 257


def test_forged_tuple_class_collides_and_differs():
    d = data()
    assert len(set(d.tclass)) == len(d.tclass) == 120
    assert all(-2**63 <= x < 2**63 for p in d.tclass for x in p)
    assert len({F.tuple_hash([a, b, 0, 0, 0]) for a, b in d.tclass}) == 1
    rest = set(d.tbatch1 + d.tbatch2) - set(d.tclass)
    assert len(rest) >= 3000 + 200 - 50
    assert F.tuple_hash(d.tclass[0]) not in {F.tuple_hash(p) for p in rest}


def test_batches_hold_what_the_gpu_tests_rely_on():
    d = data()
    b1 = {k for k in d.batch1 if k is not None}
    assert b1 == set(d.pool1) and len(d.pool1) == 6 * CLASS_OLD + BIG_OLD + 200
    b2 = {k for k in d.batch2 if k is not None}
    new = b2 - b1
    assert len(b2 & b1) > 300 and len(b1) + len(new) > 1024  # old members again; past the first code capacity
    for members in list(d.classes.values()) + [d.big]:
        assert set(members) <= b1 | b2 and set(members) & new and set(members) & b1
    assert 0.01 < sum(k is None for k in d.batch1) / len(d.batch1) < 0.06
    assert set(d.tbatch1) == set(d.tpool1) and set(d.tclass[100:]) <= set(d.tbatch2) - set(d.tbatch1)
    assert len(set(d.tbatch1) | set(d.tbatch2)) > 1024


def test_restated_hashes_follow_their_definition():
    """Hand-unrolled cases of the restatement: lengths below, at and above one word."""
    f, m = F.fmix64, F.M64
    seed = lambda n: F.SEED ^ ((n * F.LEN_MUL) & m)  # noqa: E731
    assert F.str_hash(b"") == f(seed(0))
    assert F.str_hash(b"abc") == f(f(seed(3) ^ int.from_bytes(b"abc", "little") ^ (3 << 59)))
    w = int.from_bytes(b"abcdefgh", "little")
    assert F.str_hash(b"abcdefgh") == f((f(seed(8) ^ w) + F.STEP) & m)
    assert F.str_hash(b"abcdefghi") == f(f(((f(seed(9) ^ w) + F.STEP) & m) ^ ord("i") ^ (1 << 59)))
    assert F.str_hash(b"a") != F.str_hash(b"a\0")
    assert F.tuple_hash([1, 2]) == F.tuple_hash([1, 2, 0, 0, 0]) != F.tuple_hash([2, 1])
    assert F.partition([(F.TYPE_INT64, np.arange(50), None)], 1).tolist() == [0] * 50
    p = F.partition([(F.TYPE_FLOAT64, np.array([np.nan, -np.nan, 0.0, -0.0]), None)], NPARTS_31)
    assert p[0] == p[1] and p[2] != p[3]
    a = F.partition([(F.TYPE_INT32, np.array([-1], dtype=np.int32), None)], NPARTS_31)
    b = F.partition([(F.TYPE_INT64, np.array([0xFFFFFFFF]), None)], NPARTS_31)
    assert a[0] == b[0]  # INT32 members are zero-extended


# ---- device helpers ---------------------------------------------------------------------------------
def _bitmap(ctx, bits):
    import torch

    from kquery.columnar import bitmap_bytes

    buf = np.zeros(max(bitmap_bytes(len(bits)), 4), dtype=np.uint8)
    packed = np.packbits(np.asarray(bits, dtype=bool), bitorder="little")
    buf[: len(packed)] = packed
    return torch.from_numpy(buf).to(ctx.torch_device)


def ucol(ctx, keys):
    """UTF8 column from raw byte strings (any bytes); None is a null row of no bytes."""
    import torch

    from kquery import native as N
    from kquery.columnar import DeviceColumn

    vals = [k if k is not None else b"" for k in keys]
    offs = np.zeros(len(vals) + 1, dtype=np.int32)
    offs[1:] = np.cumsum(np.fromiter((len(v) for v in vals), dtype=np.int64, count=len(vals)))
    buf = np.frombuffer(b"".join(vals) or b"\0", dtype=np.uint8).copy()
    valid = _bitmap(ctx, [k is not None for k in keys]) if any(k is None for k in keys) else None
    return DeviceColumn(N.TYPE_UTF8, len(vals), torch.from_numpy(buf).to(ctx.torch_device), valid,
                        torch.from_numpy(offs).to(ctx.torch_device), ctx)


def raw_keys(col):
    """A UTF8 device column as raw bytes per row (None for nulls), through offsets and values."""
    n = col.length
    offs = col.offsets.cpu().numpy()[: n + 1]
    buf = col.values.cpu().numpy().tobytes()
    valid = col.valid_mask()
    return [buf[offs[i]:offs[i + 1]] if valid[i] else None for i in range(n)]


def _device_cols(ctx, cols):
    from kquery import native as N
    from kquery.columnar import DeviceColumn

    dev = [ucol(ctx, [v if ok else None for v, ok in zip(vals, valid if valid is not None else [True] * len(vals))])
           if t == N.TYPE_UTF8 else DeviceColumn.from_numpy(t, np.asarray(vals), valid, ctx=ctx)
           for t, vals, valid in cols]
    return dev


def device_partition(ctx, dev_cols, nparts):
    import torch

    from kquery import native as N

    n = dev_cols[0].length
    part = torch.full((max(n, 1),), -1, dtype=torch.int32, device=ctx.torch_device)
    arr = (N.QeColumn * len(dev_cols))(*[c.as_c() for c in dev_cols])
    N.check(N.lib().qe_hash_partition(ctx.handle, arr, len(dev_cols), int(nparts), part.data_ptr()))
    ctx.synchronize()
    return part.cpu().numpy()[:n]


# ---- qe_hash_partition against the restatement --------------------------------------------------------
def _partition_cases():
    rng = np.random.default_rng(77)
    n = 4099
    lens = np.concatenate([np.arange(71), [7, 8, 9, 40, 41] * 4, rng.integers(0, 71, n - 71 - 20)])
    rng.shuffle(lens)
    vals = []
    for ln in lens:
        b = bytearray(rng.bytes(int(ln)))
        for j in range(len(b)):  # embedded 0x00, also at the ends
            if rng.random() < 0.15:
                b[j] = 0
        vals.append(bytes(b))
    utf8 = [(F.TYPE_UTF8, vals, (rng.random(n) > 0.05).tolist())]
    bits = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,
                     0x7FF8000000000123, 0x0000000000000000, 0x8000000000000000, 0x3FF0000000000000,
                     0x7FF0000000000000, 0xFFF0000000000000], dtype=np.uint64).view(np.float64)
    f = bits[rng.integers(0, len(bits), n)]
    f[: len(bits)] = bits
    mixed = [(F.TYPE_FLOAT64, f, None),
             (F.TYPE_INT32, rng.integers(-2**31, 2**31, n).astype(np.int32), (rng.random(n) > 0.05).tolist()),
             (F.TYPE_UINT8, rng.integers(0, 256, n).astype(np.uint8), (rng.random(n) > 0.05).tolist()),
             (F.TYPE_BOOL, rng.random(n) < 0.5, (rng.random(n) > 0.05).tolist())]
    return {"utf8": utf8, "mixed": mixed}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["utf8", "mixed"])
def test_hash_partition_matches_restatement(gpu_ctx, case):
    cols = _partition_cases()[case]
    dev = _device_cols(gpu_ctx, cols)
    for nparts in (1, 2, 3, 7, NPARTS_31):
        got = device_partition(gpu_ctx, dev, nparts)
        want = F.partition(cols, nparts)
        assert got.dtype == np.int32 and got.shape == want.shape
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"nparts {nparts}: {bad.size} rows differ, first row {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.gpu
def test_forged_classes_collide_on_the_device(gpu_ctx):
    """One UTF8 column at 2^31 - 1 partitions is a bijective image of the top 31 bits of str_hash:
    every forged class lands in ONE partition, the one the restatement names. This ties the forger
    to the device's hash (random 16-byte keys in one partition: chance 2^-31 each)."""
    d = data()
    for members in _forged_string_classes(d):
        got = device_partition(gpu_ctx, [ucol(gpu_ctx, members)], NPARTS_31)
        want = F.partition([(F.TYPE_UTF8, members, None)], NPARTS_31)
        assert len(set(got.tolist())) == 1 and np.array_equal(got, want)
    got = device_partition(gpu_ctx, [ucol(gpu_ctx, d.rand)], NPARTS_31)
    assert len(set(got.tolist())) > 190  # and unforged keys do not


# ---- StringDictionary.encode / decode ---------------------------------------------------------------------
WIDE_DICT = 1 << 62


def _encode_check(ctx, d, keys, seen, wide):
    """Encodes `keys`, checks the dictionary's contract against `seen` (key -> code from earlier
    batches, updated in place) and that decode restores every row's bytes."""
    from kquery import native as N

    codes = d.encode(ucol(ctx, keys))
    assert codes.type == (N.TYPE_INT64 if wide else N.TYPE_INT32) and codes.length == len(keys)
    c = codes.to_numpy()
    valid = codes.valid_mask()
    assert valid.tolist() == [k is not None for k in keys]
    for k, code, ok in zip(keys, c.tolist(), valid.tolist()):
        if not ok:
            continue
        if wide:
            assert code >> 62 == 1, "a key of 8 bytes or more takes a dictionary code"
            code &= WIDE_DICT - 1
        assert seen.setdefault(k, code) == code  # equal bytes -> equal code, old codes unchanged
    by_code = {}
    for k, code in seen.items():
        assert by_code.setdefault(code, k) == k, f"code {code} stands for two different keys"
    assert d.size() == len(seen)  # one code per distinct key
    assert sorted(by_code) == list(range(len(seen)))  # dense 0..size-1
    out = d.decode(codes)
    assert out.length == len(keys) and raw_keys(out) == keys
    return codes


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["int32", "wide"])
def test_strdict_roundtrip_with_collisions(gpu_ctx, wide):
    from kquery.strdict import StringDictionary

    d = data()
    sd = StringDictionary(gpu_ctx, 16, wide=wide)
    seen = {}
    _encode_check(gpu_ctx, sd, d.batch1, seen, wide)
    assert len(seen) == len(d.pool1)
    first = dict(seen)
    # old members, new members of the same classes and enough fresh keys to outgrow the code arrays:
    # k_dict_rebuild re-chains the codes that share a hash
    _encode_check(gpu_ctx, sd, d.batch2, seen, wide)
    assert len(seen) > 1024 and all(seen[k] == c for k, c in first.items())
    # after growth the first batch still encodes to its codes
    _encode_check(gpu_ctx, sd, d.batch1, seen, wide)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["int32", "wide"])
def test_strdict_one_wave_of_colliding_new_keys(gpu_ctx, wide):
    """257 rows into an empty dictionary; rows 0..63 are 64 different keys with one hash, so the 64
    lanes of one wave contend for one chain at once: one claims, the others wait for its code, claim
    past it or are deferred to the later passes."""
    from kquery.strdict import StringDictionary

    d = data()
    seen = {}
    _encode_check(gpu_ctx, StringDictionary(gpu_ctx, 16, wide=wide), d.wave, seen, wide)
    assert len(seen) == len(set(d.wave))


# ---- encode_tuple / decode_tuple ------------------------------------------------------------------------
def _tuple_encode_check(ctx, d, pairs, seen):
    from kquery import native as N
    from kquery.columnar import DeviceColumn

    arr = np.array(pairs, dtype=np.int64)
    cols = [DeviceColumn.from_numpy(N.TYPE_INT64, arr[:, k].copy(), ctx=ctx) for k in range(2)]
    codes = d.encode_tuple(cols)
    c = codes.to_numpy()
    assert c.dtype == np.int32 and len(c) == len(pairs)
    for p, code in zip(pairs, c.tolist()):
        assert seen.setdefault(p, code) == code
    by_code = {}
    for p, code in seen.items():
        assert by_code.setdefault(code, p) == p, f"code {code} stands for two different tuples"
    assert d.size() == len(seen)
    assert sorted(by_code) == list(range(len(seen)))
    outs = d.decode_tuple(codes, [N.TYPE_INT64, N.TYPE_INT64])
    for k, o in enumerate(outs):
        assert o.valid_mask().all()
        assert np.array_equal(o.to_numpy(), arr[:, k])


@pytest.mark.gpu
def test_tuple_dict_roundtrip_with_collisions(gpu_ctx):
    from kquery.strdict import StringDictionary

    d = data()
    td = StringDictionary(gpu_ctx, 16)
    seen = {}
    _tuple_encode_check(gpu_ctx, td, d.tbatch1, seen)
    assert len(seen) == len(d.tpool1)
    first = dict(seen)
    _tuple_encode_check(gpu_ctx, td, d.tbatch2, seen)
    assert len(seen) > 1024 and all(seen[p] == c for p, c in first.items())
    _tuple_encode_check(gpu_ctx, td, d.tbatch1, seen)


# ---- GROUP BY end to end, against a Python dict keyed by the raw bytes / tuples ---------------------------
def _want_groups(keys, values):
    want = {}
    for k, v in zip(keys, values.tolist()):
        g = want.setdefault(k, [0, 0, v])
        g[0] += 1
        g[1] += v
        g[2] = max(g[2], v)
    return want


def _state(ctx, key_types):
    from kquery import native as N
    from kquery.aggregate import HashAggregateState

    aggs = [(N.AGG_COUNT_STAR, N.TYPE_INT64), (N.AGG_SUM, N.TYPE_INT64), (N.AGG_MAX, N.TYPE_INT64)]
    return HashAggregateState(ctx, key_types, aggs, 16)


def _update(ctx, st, key_cols, values):
    from kquery import native as N
    from kquery.columnar import DeviceColumn

    vc = DeviceColumn.from_numpy(N.TYPE_INT64, values, ctx=ctx)
    st.update(key_cols, [None, vc, vc])


def _got_groups(st, utf8_first):
    kout, aout = st.finalize()
    kcols = []
    for j, kc in enumerate(kout):
        if j == 0 and utf8_first:
            kcols.append(raw_keys(kc))
        else:
            valid = kc.valid_mask()
            kcols.append([int(x) if ok else None for x, ok in zip(kc.to_numpy().tolist(), valid.tolist())])
    for a in aout:
        assert a.valid_mask().all()
    acols = [a.to_numpy().tolist() for a in aout]
    got = {}
    for row in zip(*kcols, *acols):
        key = row[0] if len(kcols) == 1 else tuple(row[: len(kcols)])
        assert key not in got, "one key in two groups"
        got[key] = list(row[len(kcols):])
    return got


@pytest.mark.gpu
def test_group_by_lone_utf8_key_with_collisions(gpu_ctx):
    """Wide codes; then qe_hashagg_merge of two states fed disjoint halves into a third, so the
    members meet another dictionary in another order (import_keyed's re-encode)."""
    from kquery import native as N

    d = data()
    want = _want_groups(d.batch1, d.values1)
    st = _state(gpu_ctx, [N.TYPE_UTF8])
    assert st.device_key_types == [N.TYPE_INT64]
    _update(gpu_ctx, st, [ucol(gpu_ctx, d.batch1)], d.values1)
    assert _got_groups(st, True) == want
    h = len(d.batch1) // 2
    halves = []
    for a, b in ((0, h), (h, len(d.batch1))):
        s = _state(gpu_ctx, [N.TYPE_UTF8])
        _update(gpu_ctx, s, [ucol(gpu_ctx, d.batch1[a:b])], d.values1[a:b])
        halves.append(s)
    owner = _state(gpu_ctx, [N.TYPE_UTF8])
    owner.merge(halves[1])
    owner.merge(halves[0])
    assert _got_groups(owner, True) == want
    halves[1].merge(halves[0])  # and straight into the other half's dictionary
    assert _got_groups(halves[1], True) == want


@pytest.mark.gpu
def test_group_by_utf8_and_int64_keys_with_collisions(gpu_ctx):
    """Tuple codes over string codes: the INT32 string code is a member of the key tuple."""
    from kquery import native as N
    from kquery.columnar import DeviceColumn

    d = data()
    st = _state(gpu_ctx, [N.TYPE_UTF8, N.TYPE_INT64])
    assert st.key_layout == 2
    _update(gpu_ctx, st, [ucol(gpu_ctx, d.batch1), DeviceColumn.from_numpy(N.TYPE_INT64, d.second1, ctx=gpu_ctx)],
            d.values1)
    want = _want_groups(list(zip(d.batch1, d.second1.tolist())), d.values1)
    assert _got_groups(st, True) == want


@pytest.mark.gpu
def test_group_by_int64_pair_with_collisions(gpu_ctx):
    from kquery import native as N
    from kquery.columnar import DeviceColumn

    d = data()
    rng = np.random.default_rng(5)
    st = _state(gpu_ctx, [N.TYPE_INT64, N.TYPE_INT64])
    assert st.key_layout == 2
    pairs, values = [], []
    for batch in (d.tbatch1, d.tbatch2):  # the second batch grows the tuple dictionary
        arr = np.array(batch, dtype=np.int64)
        v = rng.integers(-10**9, 10**9, len(batch)).astype(np.int64)
        _update(gpu_ctx, st, [DeviceColumn.from_numpy(N.TYPE_INT64, arr[:, k].copy(), ctx=gpu_ctx) for k in range(2)], v)
        pairs += batch
        values.append(v)
    assert _got_groups(st, False) == _want_groups(pairs, np.concatenate(values))


# ---- the probe limit ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_probe_limit_raises_and_never_aliases(gpu_ctx):
    """MAX_PROBES + 6 = 1030 keys with one hash form one chain longer than a lookup walks at any table
    size. Every probe is bounded, growth cannot shorten the chain, and after 64 attempts encode
    gives up: the call raises ("key dictionary did not converge") rather than return codes that
    alias two keys. The context stays usable: a fresh dictionary works afterwards."""
    from kquery import native as N
    from kquery.strdict import StringDictionary

    d = data()
    assert len(d.chain) == 1024 + 6  # MAX_PROBES + 6
    sd = StringDictionary(gpu_ctx, 16)
    with pytest.raises(N.QueryEngineError, match="did not converge"):
        sd.encode(ucol(gpu_ctx, d.chain))
    sd.close()
    seen = {}
    keys = d.chain[:100] + d.rand[:50] + [None] + d.chain[:100]
    _encode_check(gpu_ctx, StringDictionary(gpu_ctx, 16), keys, seen, False)
    assert len(seen) == 150
