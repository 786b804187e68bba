"""qe_select_project on built selections (tests/selprojcases.py), through the C ABI, under every
tile-base scheme: register-resident, two-pass, scanned two-pass and the decoupled look-back.

Each case asks qe_select_project_layout for the tile size, block size and scheme of the call it is
about to make, asserts the scheme, places the selection relative to that tile, and after the call
compares with the oracle-based reference
  * the row count,
  * the values of rows [0, count) bit for bit where valid,
  * the whole validity bitmap of the n-row capacity byte for byte: the reference's bits inside
    [0, count); at and past count, padding included, 0 for an output that can be null and all ones
    for one that cannot (include/qe_hip.h),
  * that value rows [count, n) still hold the sentinel they were filled with.

Sizes come from the hook's tile size T and the device's CU count: 66 T + 1 rows are 67 tiles (tile
65 takes a second look-back round trip, the last tile is partial); 8 x 1024 x CUs + 1 rows give
the resident pass a second output group; (4 CUs + 3) T + 1 rows give the persistent look-back more
tiles than workgroups.

Eight value-only slips were applied, one at a time, to a scratch copy of the generator, and this
file (448 tests) run against each. Tests that failed:
  1 resident INT32 load zero-extended: 19, every S7 case of the default scheme
    (test_resident_output_groups[S7-*] 14, test_other_shapes_67_tiles[S7-default-*] 5)
  2 a predicate column's validity taken as 1: 20, every test_other_shapes_67_tiles[S8-*]
  3 the mask's validity ignored: 20, every test_other_shapes_67_tiles[S6v-*]
  4 staged odd-tail store out[tot - 1] omitted: 228, in every test function but
    test_resident_output_groups (the resident pass has its own tail store), for S1-S3 and S5-S8
  5 `whole` forced true in the validity-word loop: 67 (S3 41, S5 9, S8 12, async 4, persistent S3
    seq_31): the count-sequence, one-per-tile and uniform selections, from T + 1 rows up
  6 the `l0 < 0` branch shifting by 0: the same 67
  7 per-lane UINT8 store of x >> 8: 77, every S4 case that selects a row
  8 resident staging index off by one in the second output group: 18, test_resident_output_groups
    [*-2-*] for S1, S2, S7 except one_stripe_0 (which leaves the second group empty)
Measured on an MI355X: the file 22.5 s with its kernel compiles; slowest tests the two 16.8M-row
persistent look-back cases with seq_31 (2.2 s each), every other under 0.5 s.
"""
import zlib

import numpy as np
import pytest

import selprojcases as K

pytestmark = pytest.mark.gpu

SCHEME_ENV = {"default": None, "twopass": "1", "lookback": "0", "scanned": "2"}
RESIDENT_SHAPES = ("S1", "S2", "S7")  # plans the register-resident pass takes (nothing nullable, <= 2 wide outputs)


def _types(N):
    return {"i64": N.TYPE_INT64, "f64": N.TYPE_FLOAT64, "i32": N.TYPE_INT32, "u8": N.TYPE_UINT8,
            "date32": N.TYPE_DATE32, "bool": N.TYPE_BOOL}


def _cspec(N, spec):
    s = N.QeSelectSpec()
    s.mask_col = spec.mask_col
    s.nterms = len(spec.terms)
    for i, (col, op, rhs, lit) in enumerate(spec.terms):
        t = s.terms[i]
        t.col, t.op, t.rhs_col = col, op, rhs
        if lit is not None:
            t.lit = N.scalar(lit)
    s.nout = len(spec.outputs)
    for k, prog in enumerate(spec.outputs):
        s.outputs[k].ntokens = len(prog)
        for j, (op, arg, lit) in enumerate(prog):
            s.outputs[k].tokens[j] = N.QeToken(op, arg, N.scalar(lit) if lit is not None else N.QeScalar())
    return s


def _set_scheme(monkeypatch, scheme):
    if SCHEME_ENV[scheme] is None:
        monkeypatch.delenv("QE_SELPROJ_TWOPASS", raising=False)
    else:
        monkeypatch.setenv("QE_SELPROJ_TWOPASS", SCHEME_ENV[scheme])


def _expected_scheme(N, shape, scheme):
    if scheme == "default":
        return N.SELECT_RESIDENT if shape in RESIDENT_SHAPES else N.SELECT_TWOPASS
    return {"twopass": N.SELECT_TWOPASS, "lookback": N.SELECT_LOOKBACK_PERSISTENT, "scanned": N.SELECT_SCANNED}[scheme]


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


_scratch = {}


def _probe(ctx, shape, n):
    """The layout of `shape` over n rows, asked before any data exists: the columns have the
    shape's types and validity and point into one scratch buffer (the hook reads no device memory)."""
    import torch
    from kquery import native as N

    cols, spec = K.make_case(shape, np.zeros(8, dtype=bool), 0)
    need = max(n, 1) * 8
    if _scratch.get("bytes", 0) < need:
        _scratch["buf"] = torch.zeros(need, dtype=torch.uint8, device=ctx.torch_device)
        _scratch["bytes"] = need
    ptr = _scratch["buf"].data_ptr()
    ty = _types(N)
    cc = (N.QeColumn * len(cols))(*[N.QeColumn(ty[c.kind], 0, n, ptr if c.valid is not None else None, ptr, None)
                                   for c in cols])
    kinds = K.output_kinds(cols, spec)
    oc = (N.QeColumn * len(kinds))(*[N.QeColumn(ty[k], 0, n, ptr, ptr, None) for k, _ in kinds])
    lay = N.QeSelectLayout()
    N.check(N.lib().qe_select_project_layout(ctx.handle, cc, len(cols), N.C.byref(_cspec(N, spec)), oc, N.C.byref(lay)))
    return lay


def _plan_size(ctx, shape, n_of):
    """(n, layout) with n = n_of(T, layout) for the tile size T that the hook reports for n rows."""
    lay = _probe(ctx, shape, 1000)
    for _ in range(4):
        n = n_of(int(lay.tile_rows), lay)
        lay = _probe(ctx, shape, n)
        if n == n_of(int(lay.tile_rows), lay):
            break
    else:
        pytest.fail(f"{shape}: no size n = f(tile_rows(n)) found")
    assert lay.tile_rows in K.TILE_SIZES and lay.block in K.BLOCKS, (
        f"the generator reports tile_rows {lay.tile_rows} / block {lay.block}, outside selprojcases.TILE_SIZES / "
        f"BLOCKS: add it there (tests/test_selproj_cases.py checks the builders at every listed size)")
    assert lay.tiles == -(-n // lay.tile_rows)
    return n, lay


_SENTINEL = {8: 0x5A5A5A5A5A5A5A5A, 4: 0x5A5A5A5A, 1: 0x5A}


def _upload(ctx, cols):
    from kquery import native as N
    from kquery.columnar import DeviceColumn

    ty = _types(N)
    return [DeviceColumn.from_numpy(ty[c.kind], c.values, c.valid, ctx=ctx) for c in cols]


def _alloc_outs(ctx, kinds, n):
    """Outputs at capacity n: values filled with 0x5A bytes, validity with 0xA5 bytes."""
    import torch
    from kquery import native as N
    from kquery.columnar import DeviceColumn, bitmap_bytes

    ty = _types(N)
    outs = []
    for kind, _ in kinds:
        w = np.dtype(K._DTYPE[kind]).itemsize
        idt = {8: torch.int64, 4: torch.int32, 1: torch.uint8}[w]
        vals = torch.full((max(n, 1),), _SENTINEL[w], dtype=idt, device=ctx.torch_device)
        if kind == "f64":
            vals = vals.view(torch.float64)
        valid = torch.full((max(bitmap_bytes(n), 4),), 0xA5, dtype=torch.uint8, device=ctx.torch_device)
        outs.append(DeviceColumn(ty[kind], n, vals, valid, None, ctx))
    return outs


def _compare(outs, kinds, ref, n, cnt, what):
    from kquery.columnar import bitmap_bytes

    want_cnt = len(ref[0][0])
    assert cnt == want_cnt, f"{what}: count {cnt}, reference {want_cnt}"
    for k, (out, (kind, nullable), (val, valid)) in enumerate(zip(outs, kinds, ref)):
        w = np.dtype(K._DTYPE[kind]).itemsize
        it = {8: np.int64, 4: np.int32, 1: np.uint8}[w]
        got = out.values.cpu().numpy().view(it)[:n]
        bits = out.validity.cpu().numpy()[: bitmap_bytes(n)]
        if nullable:
            want_bits = np.zeros(bitmap_bytes(n), dtype=np.uint8)
            pk = np.packbits(valid, bitorder="little")
            want_bits[: len(pk)] = pk
        else:
            assert valid.all()
            want_bits = np.full(bitmap_bytes(n), 0xFF, dtype=np.uint8)
        bad = np.flatnonzero(bits != want_bits)
        assert len(bad) == 0, (f"{what}: output {k} validity byte {bad[0]} of {len(bits)} is {bits[bad[0]]:#x}, want "
                               f"{want_bits[bad[0]]:#x} ({len(bad)} bytes differ; count {cnt})")
        wv = val.view(it)
        bad = np.flatnonzero((got[:cnt] != wv) & valid)
        assert len(bad) == 0, f"{what}: output {k} row {bad[0]} is {got[bad[0]]}, want {wv[bad[0]]} ({len(bad)} rows differ)"
        bad = np.flatnonzero(got[cnt:] != it(_SENTINEL[w]))
        assert len(bad) == 0, f"{what}: output {k} row {cnt + bad[0]} past the count {cnt} was written ({len(bad)} rows)"


def _call(ctx, dcols, cspec, outs):
    from kquery import native as N

    cc = (N.QeColumn * len(dcols))(*[c.as_c() for c in dcols])
    oc = (N.QeColumn * len(outs))(*[o.as_c() for o in outs])
    cnt = N.C.c_int64(-1)
    N.check(N.lib().qe_select_project(ctx.handle, cc, len(dcols), N.C.byref(cspec), oc, N.C.byref(cnt)))
    return cnt.value, cc, oc


def _run(ctx, shape, builder, n, lay, want_scheme, T=None, calls=1):
    """One case: selection `builder` (a name in selprojcases.BUILDERS or a builder) placed on tiles
    of T (default: the layout's) rows, plan `shape`, compared after each of `calls` calls."""
    from kquery import native as N

    T = int(T or lay.tile_rows)
    name = builder if isinstance(builder, str) else getattr(builder, "__qualname__", "builder")
    seed = zlib.crc32(f"{shape}/{name}".encode()) & 0xFFFF
    if isinstance(builder, str):
        sel, cols, spec, ref = K.cached_case(shape, builder, n, T, int(lay.block), seed)
    else:
        sel = builder(n, T, int(lay.block), seed)
        cols, spec = K.make_case(shape, sel, seed, T, int(lay.block))
        ref = K.select_project_ref(cols, spec)
    kinds = K.output_kinds(cols, spec)
    dcols = _upload(ctx, cols)
    cspec = _cspec(N, spec)
    what = f"{shape} {name} n={n} T={T} block={lay.block} scheme={lay.scheme}"
    for call in range(calls):
        outs = _alloc_outs(ctx, kinds, n)
        real = N.QeSelectLayout()
        cc = (N.QeColumn * len(dcols))(*[c.as_c() for c in dcols])
        oc = (N.QeColumn * len(outs))(*[o.as_c() for o in outs])
        N.check(N.lib().qe_select_project_layout(ctx.handle, cc, len(dcols), N.C.byref(cspec), oc, N.C.byref(real)))
        assert (real.scheme, real.tile_rows, real.tiles, real.staged, real.block, real.group_rows) == \
            (lay.scheme, lay.tile_rows, lay.tiles, lay.staged, lay.block, lay.group_rows), what
        assert real.scheme == want_scheme, f"{what}: scheme {real.scheme}, expected {want_scheme}"
        cnt, _, _ = _call(ctx, dcols, cspec, outs)
        _compare(outs, kinds, ref, n, cnt, f"{what} call {call}")
    return int(sel.sum())


def _n66(T, lay):
    return 66 * T + 1


MATRIX = [(s, sch) for s, schs in (("S1", ("default", "twopass", "lookback", "scanned")),
                                   ("S3", ("twopass", "lookback", "scanned")),
                                   ("S4", ("twopass", "lookback", "scanned"))) for sch in schs]


@pytest.mark.parametrize("builder", sorted(K.BUILDERS))
@pytest.mark.parametrize("shape,scheme", MATRIX)
def test_every_builder_67_tiles(gpu_ctx, monkeypatch, shape, scheme, builder):
    """Every builder x S1 (wide), S3 (staged validity words), S4 (narrow, nullable, per-lane stores)
    x scheme at 66 T + 1 rows."""
    from kquery import native as N

    _set_scheme(monkeypatch, scheme)
    n, lay = _plan_size(gpu_ctx, shape, _n66)
    assert lay.staged == (0 if shape == "S4" else 1)
    _run(gpu_ctx, shape, builder, n, lay, _expected_scheme(N, shape, scheme))


SMALL = ["seq_31", "seq_33", "seq_mixed", "seq_123", "seq_full_short", "one_per_tile_first", "one_per_tile_last",
         "one_per_tile_rand"]


@pytest.mark.parametrize("size", ["T-1", "T", "T+1", "2T"])
@pytest.mark.parametrize("shape,scheme", MATRIX + [("S3", "default"), ("S4", "default")])
def test_count_sequences_around_one_tile(gpu_ctx, monkeypatch, shape, scheme, size):
    """count_sequence and one_per_tile at T - 1, T, T + 1 and 2 T rows: one tile short of full,
    exactly full, a one-row second tile, two full tiles."""
    from kquery import native as N

    _set_scheme(monkeypatch, scheme)
    f = {"T-1": lambda T, lay: T - 1, "T": lambda T, lay: T, "T+1": lambda T, lay: T + 1, "2T": lambda T, lay: 2 * T}[size]
    n, lay = _plan_size(gpu_ctx, shape, f)
    for b in SMALL:
        _run(gpu_ctx, shape, b, n, lay, _expected_scheme(N, shape, scheme))


@pytest.mark.parametrize("builder", ["uniform_50", "one_per_tile_rand", "seq_mixed", "alternate_tiles", "none"])
@pytest.mark.parametrize("scheme", list(SCHEME_ENV))
@pytest.mark.parametrize("shape", ["S2", "S5", "S6", "S6v", "S7", "S8"])
def test_other_shapes_67_tiles(gpu_ctx, monkeypatch, shape, scheme, builder):
    """S2 (two outputs), S5 (five wide outputs: per-lane 8-byte stores in the look-back), S6 / S6v
    (BOOL mask column, without and with validity), S7 (INT32 / fp64 / column-against-column terms)
    and S8 (nullable predicate column whose nulls carry passing values) at 66 T + 1 rows."""
    from kquery import native as N

    _set_scheme(monkeypatch, scheme)
    n, lay = _plan_size(gpu_ctx, shape, _n66)
    if shape == "S5" and scheme == "lookback":
        assert lay.staged == 0, "five wide outputs no longer take the unstaged 8-byte form in the look-back"
    _run(gpu_ctx, shape, builder, n, lay, _expected_scheme(N, shape, scheme))


@pytest.mark.parametrize("case", ["one_stripe_0", "one_stripe_last", "alternate_tiles@group", "alternate_groups",
                                  "seq_123", "last_only", "uniform_50"])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("shape", RESIDENT_SHAPES)
def test_resident_output_groups(gpu_ctx, monkeypatch, shape, groups, case):
    """The register-resident pass (default scheme) with one output group per tile (66 T + 1 rows)
    and with two: the smallest n with tile_rows > group_rows, 8 x 1024 x CUs + 1. Selections that
    leave whole stripes and whole groups empty; each case is called twice (epoch-tagged status words)."""
    from kquery import native as N

    _set_scheme(monkeypatch, "default")
    cus = _cus()
    n, lay = _plan_size(gpu_ctx, shape, _n66 if groups == 1 else (lambda T, lay: 8 * 1024 * cus + 1))
    assert lay.scheme == N.SELECT_RESIDENT and lay.block == 1024 and lay.group_rows in K.TILE_SIZES
    if groups == 1:
        assert lay.tile_rows == lay.group_rows
    else:
        assert lay.tile_rows > lay.group_rows
        assert _probe(gpu_ctx, shape, n - 1).tile_rows == lay.group_rows, "not the smallest n with two groups"
    G = int(lay.group_rows)
    if case == "alternate_tiles@group":
        _run(gpu_ctx, shape, "alternate_tiles", n, lay, N.SELECT_RESIDENT, T=G, calls=2)
    elif case == "alternate_groups":
        _run(gpu_ctx, shape, K.alternate_groups(G), n, lay, N.SELECT_RESIDENT, calls=2)
    else:
        _run(gpu_ctx, shape, case, n, lay, N.SELECT_RESIDENT, calls=2)


@pytest.mark.parametrize("builder", ["seq_31", "alternate_tiles"])
@pytest.mark.parametrize("shape", ["S2", "S3"])
def test_persistent_lookback_more_tiles_than_workgroups(gpu_ctx, monkeypatch, capfd, shape, builder):
    """(4 CUs + 3) T + 1 rows: the persistent grid holds at most 4 workgroups per CU, so some
    workgroup walks two tiles through the next-tile prefetch whatever the occupancy. No rerun."""
    from kquery import native as N

    _set_scheme(monkeypatch, "lookback")
    cus = _cus()
    n, lay = _plan_size(gpu_ctx, shape, lambda T, lay: (4 * cus + 3) * T + 1)
    assert lay.tiles == 4 * cus + 4 and lay.staged == 1
    _run(gpu_ctx, shape, builder, n, lay, N.SELECT_LOOKBACK_PERSISTENT)
    assert "rerunning" not in capfd.readouterr().err


@pytest.mark.parametrize("scheme", list(SCHEME_ENV))
def test_async_calls_with_different_selections(gpu_ctx, monkeypatch, scheme):
    """Four S3 calls with different selections queued before any wait: each returns its own count
    and outputs."""
    from kquery import native as N

    _set_scheme(monkeypatch, scheme)
    n, lay = _plan_size(gpu_ctx, "S3", _n66)
    queued = []
    for b in ("seq_33", "alternate_tiles", "one_per_tile_last", "uniform_99"):
        sel, cols, spec, ref = K.cached_case("S3", b, n, int(lay.tile_rows), int(lay.block), 1)
        kinds = K.output_kinds(cols, spec)
        dcols, outs, cspec = _upload(gpu_ctx, cols), _alloc_outs(gpu_ctx, kinds, n), _cspec(N, spec)
        cc = (N.QeColumn * len(dcols))(*[c.as_c() for c in dcols])
        oc = (N.QeColumn * len(outs))(*[o.as_c() for o in outs])
        p = N.C.c_void_p()
        N.check(N.lib().qe_select_project_async(gpu_ctx.handle, cc, len(dcols), N.C.byref(cspec), oc, N.C.byref(p)))
        queued.append((p, dcols, cc, oc, cspec, outs, kinds, ref, b))
    counts = []
    for p, *_ in queued:
        cnt = N.C.c_int64(-1)
        N.check(N.lib().qe_select_pending_wait(p, N.C.byref(cnt)))
        counts.append(cnt.value)
    gpu_ctx.synchronize()
    for cnt, (_, _, _, _, _, outs, kinds, ref, b) in zip(counts, queued):
        _compare(outs, kinds, ref, n, cnt, f"S3 {b} async {scheme}")
