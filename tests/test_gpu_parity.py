"""GPU parity tests: every HIP kernel family, through the C ABI (libqe_hip.so via kquery), against
the CPU oracle on the same seeded inputs. Bit-exact for integer/byte/index work, and for fp64
SUM/AVG: the correctly rounded exact sum, and that sum / count in one division (oracle _fsum). The
fp64 aggregate inputs of the GROUP BY tests come from tests/aggdata.py (finite, hard groups; NaN and
+-Inf in marked groups only), and each test asserts the generator's conditions on its own data."""
import functools
import math

import numpy as np
import pytest

import aggdata
from oracle import gen
from oracle import semantics as S

pytestmark = pytest.mark.gpu

from kquery import native as N  # noqa: E402
from kquery.aggregate import HashAggregateState  # noqa: E402
from kquery.columnar import DeviceColumn  # noqa: E402

# qe_agg_global's AVG of an int64 column is a compensated sum of the converted values, not certified
# (DESIGN §4): the one result of these tests outside the exact contract.
GLOBAL_INT_AVG_REL = 1e-9


def dcol(ctx, t, values, valid=None):
    return DeviceColumn.from_numpy(t, values, valid, ctx=ctx)


def col_values(c: DeviceColumn):
    return c.to_numpy(), c.valid_mask()


def _rand(rng, n, kind, null_rate=0.0):
    if kind == "i64":
        v = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    elif kind == "small":
        v = rng.integers(-4, 5, n).astype(np.int64)
    else:
        v = rng.normal(size=n) * 100
        v[rng.random(n) < 0.05] = np.nan
        v[rng.random(n) < 0.05] = 0.0
        v[rng.random(n) < 0.05] = -0.0
        v[rng.random(n) < 0.01] = np.inf
    valid = (rng.random(n) >= null_rate) if null_rate > 0 else None
    return v, valid


SIZES = [0, 1, 7, 8, 9, 1000, 8191, 8193, 100_003]


@pytest.fixture(params=["jit", "generic"])
def agg_ctx(request, gpu_ctx):
    """Hash-aggregate tests run through both kernels: the hipRTC plan-specialised one and the
    generic interpreting one; both must match the oracle exactly."""
    N.check(N.lib().qe_ctx_set_jit(gpu_ctx.handle, 1 if request.param == "jit" else 0))
    gpu_ctx.kernel_mode = request.param
    yield gpu_ctx
    N.check(N.lib().qe_ctx_set_jit(gpu_ctx.handle, 1))


def check_kernel_kind(ctx, st, lds_mode=True):
    spec, note = st.last_kernel_kind()
    if getattr(ctx, "kernel_mode", "jit") == "jit" and lds_mode:
        # plans whose on-chip table does not fit the LDS budget run global-only (generic kernel)
        assert spec or note.startswith("global-only launch"), f"expected the specialised kernel: {note}"
    elif getattr(ctx, "kernel_mode", "jit") == "generic":
        assert not spec


# ---- generator ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,param,t", [
    (N.GEN_MOD, 1024, N.TYPE_INT64), (N.GEN_RAW, 0, N.TYPE_INT64), (N.GEN_UNIT53, 0, N.TYPE_FLOAT64),
    (N.GEN_MOD_F64, 10000, N.TYPE_FLOAT64), (N.GEN_MOD, 1000, N.TYPE_INT32), (N.GEN_MOD, 3, N.TYPE_UINT8),
    (N.GEN_MOD, 2, N.TYPE_BOOL)])
def test_generator_bit_exact(gpu_ctx, dist, param, t):
    from kquery.datasource import ColumnSpec, generate_column

    n, row0 = 100_005, 777
    c = generate_column(ColumnSpec("x", t, dist, param, 5, null_permille=100), n, row0, 42, gpu_ctx)
    ref, valid = gen.generate(dist, param, 42, 5, row0, n, 100)
    got, gv = col_values(c)
    if t == N.TYPE_INT32:
        ref = ref.astype(np.int32)
    elif t == N.TYPE_UINT8:
        ref = ref.astype(np.uint8)
    elif t == N.TYPE_BOOL:
        ref = (ref & 1).astype(bool)
    assert np.array_equal(gv, valid)
    if t == N.TYPE_FLOAT64:
        assert np.array_equal(got.view(np.int64), ref.view(np.int64))
    else:
        assert np.array_equal(got, ref)


# ---- K1 arithmetic ---------------------------------------------------------------------------------
def _eval(ctx, fn_name, op, lhs, rhs, out):
    keep = []

    def operand(x):
        if isinstance(x, DeviceColumn):
            c = x.as_c()
            keep.append(c)
            return N.QeOperand(N.C.pointer(c), N.QeScalar())
        return N.QeOperand(None, N.scalar(x))

    a, b = operand(lhs), operand(rhs)
    oc = out.as_c()
    N.check(getattr(N.lib(), fn_name)(ctx.handle, op, N.C.byref(a), N.C.byref(b), N.C.byref(oc)))
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("op", [N.OP_ADD, N.OP_SUB, N.OP_MUL, N.OP_DIV])
def test_arith_int64(gpu_ctx, n, op):
    rng = np.random.default_rng(n * 10 + op)
    a = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    b = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    if n:
        b[rng.random(n) < 0.2] = rng.integers(-3, 4, 1)[0]
        b[: min(n, 3)] = [0, -1, 1][: min(n, 3)]
        a[0] = -2**63
    av = rng.random(n) > 0.1
    out = DeviceColumn.empty(N.TYPE_INT64, n, True, ctx=gpu_ctx)
    _eval(gpu_ctx, "qe_eval_arith", op, dcol(gpu_ctx, N.TYPE_INT64, a, av), dcol(gpu_ctx, N.TYPE_INT64, b), out)
    r, v = S.arith(op, a, av, b, None)
    got, gv = col_values(out)
    assert np.array_equal(gv, v)
    assert np.array_equal(got[v], r[v])


@pytest.mark.parametrize("op", [N.OP_ADD, N.OP_SUB, N.OP_MUL, N.OP_DIV])
def test_arith_f64_mixed_and_literals(gpu_ctx, op):
    rng = np.random.default_rng(op)
    n = 10_007
    x, xv = _rand(rng, n, "f64", 0.1)
    i = rng.integers(-1000, 1000, n).astype(np.int64)
    out = DeviceColumn.empty(N.TYPE_FLOAT64, n, True, ctx=gpu_ctx)
    _eval(gpu_ctx, "qe_eval_arith", op, dcol(gpu_ctx, N.TYPE_FLOAT64, x, xv), dcol(gpu_ctx, N.TYPE_INT64, i), out)
    r, v = S.arith(op, x, xv, i.astype(np.float64), None)
    got, gv = col_values(out)
    assert np.array_equal(gv, v)
    assert np.array_equal(got[v].view(np.int64), r[v].view(np.int64))
    # column op literal, literal op column
    out2 = DeviceColumn.empty(N.TYPE_INT64, n, True, ctx=gpu_ctx)
    _eval(gpu_ctx, "qe_eval_arith", op, dcol(gpu_ctx, N.TYPE_INT64, i), 7, out2)
    r2, v2 = S.arith(op, i, None, np.int64(7), None)
    g2, gv2 = col_values(out2)
    assert np.array_equal(g2[v2], r2[v2]) and np.array_equal(gv2, v2)
    out3 = DeviceColumn.empty(N.TYPE_FLOAT64, n, False, ctx=gpu_ctx)
    _eval(gpu_ctx, "qe_eval_arith", op, 1.5, dcol(gpu_ctx, N.TYPE_INT64, i + 2000), out3)
    r3, _ = S.arith(op, 1.5, None, (i + 2000).astype(np.float64), None)
    assert np.array_equal(out3.to_numpy().view(np.int64), r3.view(np.int64))


def test_arith_null_literal_and_errors(gpu_ctx):
    n = 100
    a = np.arange(n, dtype=np.int64)
    out = DeviceColumn.empty(N.TYPE_INT64, n, True, ctx=gpu_ctx)
    _eval(gpu_ctx, "qe_eval_arith", N.OP_ADD, dcol(gpu_ctx, N.TYPE_INT64, a), None, out)
    assert not out.valid_mask().any()
    with pytest.raises(N.IllegalArgumentException):  # int DIV can produce nulls: validity required
        _eval(gpu_ctx, "qe_eval_arith", N.OP_DIV, dcol(gpu_ctx, N.TYPE_INT64, a), 3,
              DeviceColumn.empty(N.TYPE_INT64, n, False, ctx=gpu_ctx))
    with pytest.raises(N.CapacityError):
        _eval(gpu_ctx, "qe_eval_arith", N.OP_ADD, dcol(gpu_ctx, N.TYPE_INT64, a), 3,
              DeviceColumn.empty(N.TYPE_INT64, n - 1, False, ctx=gpu_ctx))


# ---- K2 comparison ---------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [N.OP_EQ, N.OP_NE, N.OP_LT, N.OP_LE, N.OP_GT, N.OP_GE])
@pytest.mark.parametrize("kind", ["small", "f64", "mixed", "lit"])
def test_cmp(gpu_ctx, op, kind):
    rng = np.random.default_rng(op * 7 + len(kind))
    n = 20_011
    if kind == "small":
        a, av = _rand(rng, n, "small", 0.1)
        b, bv = _rand(rng, n, "small", 0.1)
        ta = tb = N.TYPE_INT64
    elif kind == "f64":
        a, av = _rand(rng, n, "f64", 0.1)
        b, bv = _rand(rng, n, "f64", 0.1)
        b[::3] = a[::3]
        ta = tb = N.TYPE_FLOAT64
    elif kind == "mixed":
        a, av = _rand(rng, n, "small", 0.1)
        b, bv = _rand(rng, n, "f64", 0.0)
        b[::2] = np.round(b[::2]) % 5
        ta, tb = N.TYPE_INT64, N.TYPE_FLOAT64
    else:
        a, av = _rand(rng, n, "small", 0.1)
        ta = N.TYPE_INT64
    out = DeviceColumn.empty(N.TYPE_BOOL, n, True, ctx=gpu_ctx)
    if kind == "lit":
        _eval(gpu_ctx, "qe_eval_cmp", op, dcol(gpu_ctx, ta, a, av), 1, out)
        r, v = S.cmp(op, a, av, np.int64(1), None)
    else:
        _eval(gpu_ctx, "qe_eval_cmp", op, dcol(gpu_ctx, ta, a, av), dcol(gpu_ctx, tb, b, bv), out)
        r, v = S.cmp(op, a, av, b, bv)
    got, gv = col_values(out)
    assert np.array_equal(gv, v)
    assert np.array_equal(got & gv, r)


def test_cmp_utf8_employee(gpu_ctx):
    """Config 1's predicate state = 'CA' on the reference fixture's column, on device."""
    import pathlib

    from oracle import csv_ref

    rows = csv_ref.read_csv(str(pathlib.Path(__file__).parent / "golden" / "employee.csv"))[0]
    states = rows["state"] + ["CA", None, "C", "CAX"]
    col = DeviceColumn.from_strings(states, ctx=gpu_ctx)
    for lit, op in (("CA", N.OP_EQ), ("Uppsala", N.OP_EQ), ("CA", N.OP_NE)):
        out = DeviceColumn.empty(N.TYPE_BOOL, len(states), True, ctx=gpu_ctx)
        litc = DeviceColumn.from_strings([lit], ctx=gpu_ctx)
        _eval(gpu_ctx, "qe_eval_cmp", op, col, litc, out)
        r, v = S.cmp_utf8(op, states, lit)
        got, gv = col_values(out)
        assert np.array_equal(gv, v) and np.array_equal(got & gv, r)
    # the reference fixture itself: state='CA' selects nothing (known answer)
    out = DeviceColumn.empty(N.TYPE_BOOL, 3, False, ctx=gpu_ctx)
    _eval(gpu_ctx, "qe_eval_cmp", N.OP_EQ, DeviceColumn.from_strings(rows["state"], ctx=gpu_ctx),
          DeviceColumn.from_strings(["CA"], ctx=gpu_ctx), out)
    assert not out.to_numpy().any()


# ---- K3a boolean -------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [N.OP_AND, N.OP_OR, N.OP_NOT, N.OP_IS_NULL, N.OP_IS_NOT_NULL])
@pytest.mark.parametrize("n", [1, 9, 64, 1000, 100_001])
def test_bool3(gpu_ctx, op, n):
    rng = np.random.default_rng(op + n)
    a = rng.random(n) < 0.5
    av = rng.random(n) < 0.8
    b = rng.random(n) < 0.5
    bv = rng.random(n) < 0.8
    A, B = dcol(gpu_ctx, N.TYPE_BOOL, a, av), dcol(gpu_ctx, N.TYPE_BOOL, b, bv)
    out = DeviceColumn.empty(N.TYPE_BOOL, n, True, ctx=gpu_ctx)
    ac, bc, oc = A.as_c(), B.as_c(), out.as_c()
    N.check(N.lib().qe_eval_bool(gpu_ctx.handle, op, N.C.byref(ac), N.C.byref(bc), N.C.byref(oc)))
    r, v = S.bool3(op, a, av, b, bv)
    got, gv = col_values(out)
    assert np.array_equal(gv, v)
    assert np.array_equal(got & gv, r & v)


# ---- K3b selection ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + [3_000_017])
@pytest.mark.parametrize("sel_rate", [0.0, 0.01, 0.5, 1.0])
def test_filter_order_preserving(gpu_ctx, n, sel_rate):
    from kquery.columnar import RecordBatch, Schema
    from kquery.operators import filter_batch

    rng = np.random.default_rng(n + int(sel_rate * 100))
    m = rng.random(n) < sel_rate
    mv = rng.random(n) > 0.05
    a = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    av = rng.random(n) > 0.3
    f = rng.normal(size=n)
    i32 = rng.integers(-2**31, 2**31, n).astype(np.int32)
    u8 = rng.integers(0, 256, n).astype(np.uint8)
    cols = [dcol(gpu_ctx, N.TYPE_INT64, a, av), dcol(gpu_ctx, N.TYPE_FLOAT64, f),
            dcol(gpu_ctx, N.TYPE_INT32, i32), dcol(gpu_ctx, N.TYPE_UINT8, u8)]
    out = filter_batch(RecordBatch(Schema([]), cols), dcol(gpu_ctx, N.TYPE_BOOL, m, mv))
    sel = S.select_mask(m, mv)
    assert out.rowCount() == int(sel.sum())
    ga, gav = col_values(out.field(0))
    assert np.array_equal(gav, av[sel]) and np.array_equal(ga[gav], a[sel][av[sel]])
    assert np.array_equal(out.field(1).to_numpy().view(np.int64), f[sel].view(np.int64))
    assert np.array_equal(out.field(2).to_numpy(), i32[sel])
    assert np.array_equal(out.field(3).to_numpy(), u8[sel])


# ---- K4a global aggregate ----------------------------------------------------------------------------
def _global(ctx, col, mask=None):
    r = N.QeGlobalAgg()
    c = col.as_c()
    mc = mask.as_c() if mask is not None else None
    N.check(N.lib().qe_agg_global(ctx.handle, N.C.byref(c), N.C.byref(mc) if mc is not None else None,
                                  N.C.byref(r)))
    return r


def _check_global(r, ref, is_f):
    from kquery.columnar import f64_from_bits

    assert r.rows == ref["rows"] and r.count == ref["count"]
    if ref["count"] == 0:
        assert r.valid == 0
        return
    assert r.valid == 1
    if is_f:
        assert S.rows_equal(f64_from_bits(r.sum), ref["sum"], 0.0), (f64_from_bits(r.sum), ref["sum"])
        assert S.rows_equal(f64_from_bits(r.min), ref["min"]), (f64_from_bits(r.min), ref["min"])
        assert S.rows_equal(f64_from_bits(r.max), ref["max"]), (f64_from_bits(r.max), ref["max"])
    else:
        assert (r.sum, r.min, r.max) == (ref["sum"], ref["min"], ref["max"])
    assert S.rows_equal(r.avg, ref["avg"], 0.0 if is_f else GLOBAL_INT_AVG_REL), (r.avg, ref["avg"])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["i64", "f64", "f64_nulls_mask", "f64_finite", "f64_finite_nulls_mask",
                                  "f64_one_special"])
def test_global_aggregate(gpu_ctx, n, kind):
    rng = np.random.default_rng(n + len(kind))
    if kind == "i64":
        x = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
        xv, m, mv = None, None, None
        t = N.TYPE_INT64
    else:
        if kind.startswith("f64_finite"):
            x = aggdata.global_values(n, n)
            aggdata.check_global_finite(x)
            xv = rng.random(n) >= 0.2 if kind.endswith("mask") else None
        elif kind == "f64_one_special":  # one NaN / +Inf / -Inf two thirds into the column
            x = aggdata.global_values(n, n, aggdata.GLOBAL_SPECIALS[n % 3] if n else None, n * 2 // 3)
            xv = None
        else:
            x, xv = _rand(rng, n, "f64", 0.0 if kind == "f64" else 0.2)
        m = rng.random(n) < 0.7 if kind.endswith("mask") else None
        mv = rng.random(n) < 0.9 if m is not None else None
        t = N.TYPE_FLOAT64
    r = _global(gpu_ctx, dcol(gpu_ctx, t, x, xv), dcol(gpu_ctx, N.TYPE_BOOL, m, mv) if m is not None else None)
    _check_global(r, S.global_aggregate(x, xv, m, mv), t == N.TYPE_FLOAT64)


@pytest.mark.parametrize("case", [[np.nan, 1.0, 2.0], [1.0, np.nan, 2.0], [-1.0, -0.0, 0.0], [0.0, -0.0],
                                  [-0.0, 0.0, 1.0], [np.nan, np.nan], [5.0]])
def test_global_max_order_semantics(gpu_ctx, case):
    """MaxAccumulator K:538-561 order rules, with the cases spread across lanes / blocks."""
    base = np.array(case, dtype=np.float64)
    for pad in (0, 1000, 70_000):
        x = np.concatenate([np.full(pad, np.nan), base, np.full(pad, -5.0)])
        xv = np.concatenate([np.zeros(pad, bool), np.ones(len(base), bool), np.ones(pad, bool)])
        r = _global(gpu_ctx, dcol(gpu_ctx, N.TYPE_FLOAT64, x, xv))
        _check_global(r, S.global_aggregate(x, xv), True)


# ---- K4b hash aggregate --------------------------------------------------------------------------------
def result_dict(keys, aggs):
    kv = [k.to_pylist() for k in keys]
    av = [a.to_pylist() for a in aggs]
    n = aggs[0].length if aggs else keys[0].length
    return {tuple(S.canon(k[i]) for k in kv): [a[i] for a in av] for i in range(n)}


def assert_groups_equal(got, ref, fns):
    assert len(got) == len(ref), (len(got), len(ref))
    gk = {tuple(S.canon(x) for x in k): v for k, v in got.items()}
    for k, want in ref.items():
        ck = tuple(S.canon(x) for x in k)
        assert ck in gk, k
        for j, (a, b) in enumerate(zip(gk[ck], want)):
            assert S.rows_equal(a, b, 0.0), (k, j, a, b)


ALL_FNS = [N.AGG_SUM, N.AGG_MIN, N.AGG_MAX, N.AGG_COUNT, N.AGG_COUNT_STAR, N.AGG_AVG]
MP_F64 = [N.AGG_SUM, N.AGG_COUNT, N.AGG_MAX]


@functools.lru_cache(maxsize=None)
def _f64_case(which, *shape):
    """(k, kv, x, xv, oracle result) of an fp64 GROUP BY case: generated, checked against the
    generator's conditions and aggregated by the oracle once for the kernel modes and record
    placements that run it (no test writes to them)."""
    make, seed, fns = {"int64_key": (aggdata.int64_key_data, lambda g: g, ALL_FNS),
                       "partitioned": (aggdata.partitioned_data, lambda g, e: g + e, ALL_FNS),
                       "multipass": (aggdata.multipass_data, lambda g, e: g * 3 + e, MP_F64),
                       "two_phase": (aggdata.two_phase_data, lambda: 9, TWO_PHASE_FNS)}[which]
    _, _, k, kv = make(*shape)
    x, xv = aggdata.group_values(k, kv, seed(*shape))
    aggdata.check_group_conditions(k, kv, x, xv)
    return k, kv, x, xv, S.group_aggregate([k], [kv], [x] * len(fns), [xv] * len(fns), fns)


TWO_PHASE_FNS = [N.AGG_MAX, N.AGG_MIN, N.AGG_SUM, N.AGG_COUNT, N.AGG_COUNT_STAR]


@pytest.mark.parametrize("ngroups,expected", [(1, 16), (10, 1024), (1000, 1024), (5000, 100), (200_000, 1024)])
@pytest.mark.parametrize("vtype", ["i64", "f64"])
def test_hashagg_int64_key(agg_ctx, ngroups, expected, vtype):
    rng, n, k, kv = aggdata.int64_key_data(ngroups)  # (the EMPTY sentinel value is a legal key)
    if vtype == "i64":
        x = rng.integers(-2**62, 2**62, n).astype(np.int64)
        xv = rng.random(n) > 0.1
        t = N.TYPE_INT64
        ref = None
    else:
        k, kv, x, xv, ref = _f64_case("int64_key", ngroups)
        t = N.TYPE_FLOAT64
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], [(f, t) for f in ALL_FNS], expected)
    K, X = dcol(agg_ctx, N.TYPE_INT64, k, kv), dcol(agg_ctx, t, x, xv)
    st.update([K], [X] * len(ALL_FNS))
    check_kernel_kind(agg_ctx, st, ngroups <= expected * 4)
    keys, aggs = st.finalize()
    if ref is None:
        ref = S.group_aggregate([k], [kv], [x] * 6, [xv] * 6, ALL_FNS)
    assert_groups_equal(result_dict(keys, aggs), ref, ALL_FNS)


def test_hashagg_f64_key_and_multibatch_order(agg_ctx):
    """fp64 keys (Double.equals: NaN one group, +0/-0 distinct) and MIN/MAX ties across batches:
    row order continues across update calls, like the reference's batch loop (K:617-620)."""
    rng = np.random.default_rng(5)
    n = 50_000
    k = rng.choice(np.array([np.nan, 0.0, -0.0, 1.5, -2.25, np.inf]), n)
    x = rng.choice(np.array([0.0, -0.0, -1.0, np.nan, -3.0]), n)
    xv = rng.random(n) > 0.2
    fns = [N.AGG_MAX, N.AGG_MIN, N.AGG_COUNT, N.AGG_SUM]
    st = HashAggregateState(agg_ctx, [N.TYPE_FLOAT64], [(f, N.TYPE_FLOAT64) for f in fns], 16)
    for s in range(0, n, 12_345):
        e = min(n, s + 12_345)
        st.update([dcol(agg_ctx, N.TYPE_FLOAT64, k[s:e])], [dcol(agg_ctx, N.TYPE_FLOAT64, x[s:e], xv[s:e])] * 4)
    keys, aggs = st.finalize()
    ref = S.group_aggregate([k], [None], [x] * 4, [xv] * 4, fns)
    assert_groups_equal(result_dict(keys, aggs), ref, fns)


def test_hashagg_multi_key_too_wide(gpu_ctx):
    """Two 32-bit keys + null bits exceed the packed 63-bit key: the C ABI groups by key-tuple
    codes instead (one INT32 device key; qe_hashagg_key_layout says so), as HashAggregateState
    does (tests/test_tuplekeys.py)."""
    kt = (N.C.c_int32 * 2)(N.TYPE_INT32, N.TYPE_DATE32)
    ad = (N.QeAggDesc * 1)(N.QeAggDesc(N.AGG_COUNT_STAR, N.TYPE_INT64))
    h = N.C.c_void_p()
    N.check(N.lib().qe_hashagg_create(gpu_ctx.handle, 2, kt, 1, ad, 16, N.C.byref(h)))
    try:
        dk, nk, types = N.C.c_int32(), N.C.c_int32(), (N.C.c_int32 * 4)()
        N.check(N.lib().qe_hashagg_key_layout(h, N.C.byref(dk), N.C.byref(nk), types))
        assert dk.value == 2 and nk.value == 1 and types[0] == N.TYPE_INT32  # key-tuple codes
    finally:
        N.check(N.lib().qe_hashagg_destroy(h))
    state = HashAggregateState(gpu_ctx, [N.TYPE_INT32, N.TYPE_DATE32], [(N.AGG_COUNT_STAR, N.TYPE_INT64)], 16)
    assert state.key_layout == 2 and state.device_key_types == [N.TYPE_INT32]


@pytest.mark.parametrize("types", [(N.TYPE_UINT8, N.TYPE_UINT8), (N.TYPE_INT32, N.TYPE_UINT8),
                                   (N.TYPE_UINT8, N.TYPE_DATE32, N.TYPE_UINT8)])
def test_hashagg_multi_key(agg_ctx, types):
    rng = np.random.default_rng(len(types))
    n = 200_000
    keys, kvs, dcols = [], [], []
    for t in types:
        if t == N.TYPE_UINT8:
            v = rng.integers(0, 3, n).astype(np.uint8)
        else:
            v = rng.integers(-5, 5, n).astype(np.int32)
        kv = rng.random(n) > 0.05
        keys.append(v.astype(np.int64))
        kvs.append(kv)
        dcols.append(dcol(agg_ctx, t, v, kv))
    x = rng.integers(-1000, 1000, n).astype(np.int64)
    st = HashAggregateState(agg_ctx, list(types), [(f, N.TYPE_INT64) for f in ALL_FNS], 256)
    st.update(dcols, [dcol(agg_ctx, N.TYPE_INT64, x)] * 6)
    kk, aa = st.finalize()
    ref = S.group_aggregate(keys, kvs, [x] * 6, [None] * 6, ALL_FNS)
    assert_groups_equal(result_dict(kk, aa), ref, ALL_FNS)


def test_hashagg_mask_and_no_keys(agg_ctx):
    rng = np.random.default_rng(11)
    n = 300_000
    x = rng.integers(-100, 100, n).astype(np.int64)
    m = rng.random(n) < 0.3
    mv = rng.random(n) > 0.1
    st = HashAggregateState(agg_ctx, [], [(f, N.TYPE_INT64) for f in ALL_FNS], 1)
    st.update([], [dcol(agg_ctx, N.TYPE_INT64, x)] * 6, dcol(agg_ctx, N.TYPE_BOOL, m, mv))
    kk, aa = st.finalize()
    ref = S.group_aggregate([], [], [x] * 6, [None] * 6, ALL_FNS, S.select_mask(m, mv))
    assert_groups_equal(result_dict(kk, aa), ref, ALL_FNS)
    # empty input: zero groups (Main.kt:637: the map stays empty)
    st2 = HashAggregateState(agg_ctx, [], [(N.AGG_MAX, N.TYPE_INT64)], 1)
    st2.update([], [dcol(agg_ctx, N.TYPE_INT64, x)], dcol(agg_ctx, N.TYPE_BOOL, np.zeros(n, bool)))
    assert st2.num_groups() == 0


def _c4_spec(threshold=1 << 19):
    """Slots: 0 k, 1 a, 2 b. WHERE a > threshold GROUP BY k: SUM(a+b), COUNT(*), MIN(a), MAX(b)."""
    spec = N.QeFusedSpec()
    spec.mask_col = -1
    spec.nterms = 1
    spec.terms[0].col = 1
    spec.terms[0].op = N.OP_GT
    spec.terms[0].rhs_col = -1
    spec.terms[0].lit = N.scalar(threshold)
    spec.key_cols[0] = 0
    p = spec.inputs[0]
    p.ntokens = 3
    p.tokens[0] = N.QeToken(N.TOK_COL, 1, N.QeScalar())
    p.tokens[1] = N.QeToken(N.TOK_COL, 2, N.QeScalar())
    p.tokens[2] = N.QeToken(N.TOK_ADD, 0, N.QeScalar())
    spec.inputs[2].ntokens = 1
    spec.inputs[2].tokens[0] = N.QeToken(N.TOK_COL, 1, N.QeScalar())
    spec.inputs[3].ntokens = 1
    spec.inputs[3].tokens[0] = N.QeToken(N.TOK_COL, 2, N.QeScalar())
    return spec


C4_AGGS = [(N.AGG_SUM, N.TYPE_INT64), (N.AGG_COUNT_STAR, N.TYPE_INT64), (N.AGG_MIN, N.TYPE_INT64),
           (N.AGG_MAX, N.TYPE_INT64)]
C4_FNS = [f for f, _ in C4_AGGS]


@pytest.mark.parametrize("n,row0", [(1, 0), (1000, 5), (10_000_000, 0)])
def test_fused_c4_vs_oracle(agg_ctx, n, row0):
    from kquery.datasource import C4_COLUMNS, generate_column

    cols = [generate_column(s, n, row0, 42, agg_ctx) for s in C4_COLUMNS]
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], C4_AGGS, 1024)
    st.update_fused(cols, _c4_spec())
    check_kernel_kind(agg_ctx, st)
    kk, aa = st.finalize()
    k, _ = gen.generate(gen.GEN_MOD, 1024, 42, 0, row0, n)
    a, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 1, row0, n)
    b, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 2, row0, n)
    ref = S.group_aggregate([k], [None], [S.arith(S.OP_ADD, a, None, b, None)[0], None, a, b], [None] * 4, C4_FNS,
                            a > (1 << 19))
    assert_groups_equal(result_dict(kk, aa), ref, C4_FNS)


def test_fused_equals_unfused_operators(agg_ctx):
    """Scan -> Selection -> Projection -> HashAggregate: per-family operators and the fused kernel
    give identical batches; both match the oracle (C2-shaped predicate, nullable inputs)."""
    from kquery.columnar import Field, Schema
    from kquery.datasource import InMemoryDataSource
    from kquery.expressions import (AddExpression, AndExpression, ColumnExpression, CountStarExpression,
                                    GtExpression, LiteralLongExpression, LtExpression, MaxExpression,
                                    MinExpression, MultiplyExpression, SumExpression, AvgExpression)
    from kquery.operators import (FusedHashAggregateExec, HashAggregateExec, ProjectionExec, ScanExec,
                                  SelectionExec, fuse)
    from kquery.columnar import RecordBatch

    rng = np.random.default_rng(3)
    n = 1_000_003
    k = rng.integers(0, 300, n).astype(np.int64)
    a = rng.integers(0, 1 << 20, n).astype(np.int64)
    av = rng.random(n) > 0.1
    b = rng.integers(-2**40, 2**40, n).astype(np.int64)
    schema = Schema([Field("k", N.TYPE_INT64), Field("a", N.TYPE_INT64), Field("b", N.TYPE_INT64)])
    batches = []
    for s in range(0, n, 300_000):
        e = min(n, s + 300_000)
        batches.append(RecordBatch(schema, [dcol(agg_ctx, N.TYPE_INT64, k[s:e]),
                                            dcol(agg_ctx, N.TYPE_INT64, a[s:e], av[s:e]),
                                            dcol(agg_ctx, N.TYPE_INT64, b[s:e])]))
    scan = ScanExec(InMemoryDataSource(schema, batches), ["k", "a", "b"])
    pred = AndExpression(GtExpression(ColumnExpression(1), LiteralLongExpression(1 << 18)),
                         LtExpression(ColumnExpression(2), LiteralLongExpression(2**39)))
    sel = SelectionExec(scan, pred)
    proj = ProjectionExec(sel, Schema([Field("k", N.TYPE_INT64), Field("ab", N.TYPE_INT64), Field("a", N.TYPE_INT64),
                                       Field("b3", N.TYPE_INT64)]),
                          [ColumnExpression(0), AddExpression(ColumnExpression(1), ColumnExpression(2)),
                           ColumnExpression(1), MultiplyExpression(ColumnExpression(2), LiteralLongExpression(3))])
    aggs = [SumExpression(ColumnExpression(1)), CountStarExpression(), MinExpression(ColumnExpression(2)),
            MaxExpression(ColumnExpression(3)), AvgExpression(ColumnExpression(1))]
    out_schema = Schema([Field("k", N.TYPE_INT64)] + [Field(x.name, N.TYPE_INT64) for x in aggs])
    plan = HashAggregateExec(proj, [ColumnExpression(0)], aggs, out_schema)
    fused = fuse(plan)
    assert isinstance(fused, FusedHashAggregateExec)
    r1 = next(plan.execute())
    r2 = next(fused.execute())
    d1 = result_dict(r1.fields[:1], r1.fields[1:])
    d2 = result_dict(r2.fields[:1], r2.fields[1:])
    fns = [x.fn for x in aggs]
    sel_m = (a > (1 << 18)) & av & (b < 2**39)
    ab, abv = S.arith(S.OP_ADD, a, av, b, None)
    b3, _ = S.arith(S.OP_MUL, b, None, np.int64(3), None)
    ref = S.group_aggregate([k], [None], [ab, None, a, b3, ab], [abv, None, av, None, abv], fns, sel_m)
    assert_groups_equal(d1, ref, fns)
    assert_groups_equal(d2, ref, fns)


def test_export_import_two_phase(agg_ctx):
    """main()'s two-phase aggregate (K:1309-1325): shard rows into partitions, partial-aggregate
    each, export records bucketed by hash(key) mod P, import every bucket into its owner, and the
    union of the owners' groups equals the single-pass result."""
    P = 3
    k, kv, x, xv, ref = _f64_case("two_phase")
    n, fns = len(k), TWO_PHASE_FNS
    aggs = [(f, N.TYPE_FLOAT64) for f in fns]
    owners = [HashAggregateState(agg_ctx, [N.TYPE_INT64], aggs, 4096) for _ in range(P)]
    bounds = np.linspace(0, n, P + 1).astype(int)
    for p in range(P):
        s, e = bounds[p], bounds[p + 1]
        st = HashAggregateState(agg_ctx, [N.TYPE_INT64], aggs, 4096)
        st.set_row_base(int(s))
        st.update([dcol(agg_ctx, N.TYPE_INT64, k[s:e], kv[s:e])], [dcol(agg_ctx, N.TYPE_FLOAT64, x[s:e], xv[s:e])] * 5)
        recs, counts = st.export(P)
        rb = st.record_bytes()
        off = 0
        for q in range(P):
            owners[q].import_records(recs[off * rb:(off + counts[q]) * rb], counts[q])
            off += counts[q]
    got = {}
    for o in owners:
        kk, aa = o.finalize()
        d = result_dict(kk, aa)
        assert not (set(d) & set(got))  # each group has exactly one owner
        got.update(d)
    assert_groups_equal(got, ref, fns)


def test_hashagg_growth_from_tiny_table(agg_ctx):
    """expected_groups far too small: the global table grows and deferred rows / overflow records
    are re-applied exactly once."""
    rng = np.random.default_rng(17)
    n = 2_000_000
    k = rng.integers(0, 300_000, n).astype(np.int64)
    x = rng.integers(0, 10, n).astype(np.int64)
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], [(N.AGG_SUM, N.TYPE_INT64), (N.AGG_COUNT_STAR, N.TYPE_INT64)], 8)
    st.update([dcol(agg_ctx, N.TYPE_INT64, k)], [dcol(agg_ctx, N.TYPE_INT64, x), None])
    kk, aa = st.finalize()
    ref = S.group_aggregate([k], [None], [x, None], [None, None], [N.AGG_SUM, N.AGG_COUNT_STAR])
    assert_groups_equal(result_dict(kk, aa), ref, [N.AGG_SUM, N.AGG_COUNT_STAR])


def check_partitioned(ctx, st):
    spec, note = st.last_kernel_kind()
    if getattr(ctx, "kernel_mode", "jit") == "jit":
        assert spec and note.startswith("radix-partitioned"), note


@pytest.fixture(params=["auto", "chunked", "counted"])
def part_mode(request, monkeypatch):
    """Both record placements of the partitioned update: chunks claimed from a device counter (the
    default for large batches; forced here at test sizes) and exact offsets from a count pass."""
    if request.param != "auto":
        monkeypatch.setenv("QE_PART_CHUNKED", "1" if request.param == "chunked" else "0")
    return request.param


@pytest.mark.parametrize("ngroups,expected", [(50_000, 50_000), (600_000, 20_000), (3, 100_000)])
@pytest.mark.parametrize("vtype", ["i64", "f64"])
def test_hashagg_partitioned(agg_ctx, part_mode, ngroups, expected, vtype):
    """Expected groups beyond the LDS table: rows are radix-partitioned by key hash and each
    workgroup aggregates a record slice in LDS. Nullable keys and inputs, the EMPTY sentinel as a
    key, fp64 MIN/MAX order ties across two batches, and far more groups than expected (records of
    groups that find no room are retried)."""
    rng, n, k, kv = aggdata.partitioned_data(ngroups, expected)
    if vtype == "i64":
        x = rng.integers(-2**62, 2**62, n).astype(np.int64)
        xv = rng.random(n) > 0.1
        t = N.TYPE_INT64
        ref = None
    else:
        k, kv, x, xv, ref = _f64_case("partitioned", ngroups, expected)
        t = N.TYPE_FLOAT64
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], [(f, t) for f in ALL_FNS], expected)
    half = 400_001
    for s, e in ((0, half), (half, n)):
        st.update([dcol(agg_ctx, N.TYPE_INT64, k[s:e], kv[s:e])], [dcol(agg_ctx, t, x[s:e], xv[s:e])] * len(ALL_FNS))
        check_partitioned(agg_ctx, st)
    keys, aggs = st.finalize()
    if ref is None:
        ref = S.group_aggregate([k], [kv], [x] * 6, [xv] * 6, ALL_FNS)
    assert_groups_equal(result_dict(keys, aggs), ref, ALL_FNS)


@pytest.fixture(params=["spill", "twopass"])
def mp_mode(request, monkeypatch):
    """Both two-bucket updates: one fused pass that spills the second bucket's rows as records for a
    partition-aggregate pass (default), and two fused passes (QE_MP_SPILL=0)."""
    monkeypatch.setenv("QE_MP_SPILL", "1" if request.param == "spill" else "0")
    monkeypatch.setenv("QE_LDS_COMPACT", "0")  # (the compact one-pass table has tests of its own)
    return request.param


def check_multipass(ctx, st, mode, buckets=2):
    note = st.last_kernel_kind()[1]
    if getattr(ctx, "kernel_mode", "jit") == "jit":
        assert note.startswith("multi-pass"), note
        if buckets == 2:
            assert ("spilled" in note) == (mode == "spill"), note


MP_I64 = [N.AGG_SUM, N.AGG_COUNT_STAR, N.AGG_MIN, N.AGG_MAX]


@pytest.mark.parametrize("vtype,ngroups,expected", [("i64", 4500, 4500), ("i64", 40_000, 4000),
                                                    ("f64", 1200, 1200), ("f64", 40_000, 1200)])
def test_hashagg_multipass(agg_ctx, mp_mode, vtype, ngroups, expected):
    """Expected groups just beyond one LDS table (the specialised kernel's table takes up to
    152 KiB: ~2.5K groups of the i64 shape, ~0.6K of the f64 one, whose exact SUM keeps a 24-byte
    window per slot): 2 passes of the fused kernel,
    each keeping one bucket of key hashes (also when far more groups turn up than expected:
    overflow records and deferred rows inside a pass). Nullable keys and inputs, fp64 MAX order
    across two batches."""
    rng, n, k, kv = aggdata.multipass_data(ngroups, expected)
    if vtype == "i64":
        fns, t = MP_I64, N.TYPE_INT64  # non-nullable: the LDS table then holds 4096 slots
        x = rng.integers(-2**62, 2**62, n).astype(np.int64)
        xv, ref = None, None
    else:
        fns, t = MP_F64, N.TYPE_FLOAT64
        k, kv, x, xv, ref = _f64_case("multipass", ngroups, expected)
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], [(f, t) for f in fns], expected)
    for s, e in ((0, 250_001), (250_001, n)):
        st.update([dcol(agg_ctx, N.TYPE_INT64, k[s:e], kv[s:e])],
                  [dcol(agg_ctx, t, x[s:e], None if xv is None else xv[s:e])] * len(fns))
        if s == 0:
            check_multipass(agg_ctx, st, mp_mode)
    keys, aggs = st.finalize()
    if ref is None:
        ref = S.group_aggregate([k], [kv], [x] * len(fns), [xv] * len(fns), fns)
    assert_groups_equal(result_dict(keys, aggs), ref, fns)


@pytest.mark.parametrize("case", ["fits", "wide_first", "wide_later"])
def test_multipass_spill_narrow_records(agg_ctx, monkeypatch, case):
    """The spilling first pass writes its records in 32-bit words while the spilled values fit int32;
    when one does not, the kept rows stand, the records are dropped, and the spilled rows (key hash
    at or above the kept share) are aggregated by one more fused pass over the columns; the state's
    records are 64-bit afterwards. Two batches; results equal the oracle."""
    monkeypatch.setenv("QE_MP_SPILL", "1")
    monkeypatch.setenv("QE_LDS_COMPACT", "0")
    rng = np.random.default_rng(len(case) + 99)
    n, groups = 600_000, 4000
    k = rng.integers(0, groups, n).astype(np.int64) * 104729 + 11
    x = rng.integers(-2**31, 2**31, n).astype(np.int64)
    half = 250_001
    if case == "wide_first":
        x[:half:50] = 2**40  # every 50th row of batch 0: some of them are spilled
    elif case == "wide_later":
        x[half::50] = -2**40
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], [(f, N.TYPE_INT64) for f in MP_I64], groups)
    notes = []
    for s, e in ((0, half), (half, n)):
        st.update([dcol(agg_ctx, N.TYPE_INT64, k[s:e])], [dcol(agg_ctx, N.TYPE_INT64, x[s:e])] * len(MP_I64))
        notes.append(st.last_kernel_kind()[1])
    if getattr(agg_ctx, "kernel_mode", "jit") == "jit":
        narrow = "spilled as 8 B records (column words, 32-bit)"
        wide = "spilled as 16 B records (column words)"
        expect = {"fits": [narrow, narrow], "wide_first": ["re-read", wide], "wide_later": [narrow, "re-read"]}[case]
        assert all(x in m for x, m in zip(expect, notes)), notes
    keys, aggs = st.finalize()
    ref = S.group_aggregate([k], [None], [x] * len(MP_I64), [None] * len(MP_I64), MP_I64)
    assert_groups_equal(result_dict(keys, aggs), ref, MP_I64)


def test_fused_c4_one_pass_large_table(agg_ctx):
    """2400 groups of the C4 shape: one pass of the specialised kernel over a 4096-slot table
    (152 KiB LDS budget of its 1024-thread workgroups); the generic kernel (80 KiB) partitions."""
    from kquery.datasource import C4_COLUMNS, ColumnSpec, generate_column

    n, groups = 1_000_003, 2400
    kspec = ColumnSpec("k", N.TYPE_INT64, N.GEN_MOD, groups, 0)
    cols = [generate_column(kspec, n, 0, 42, agg_ctx)] + [generate_column(s, n, 0, 42, agg_ctx) for s in C4_COLUMNS[1:]]
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], C4_AGGS, groups)
    st.update_fused(cols, _c4_spec())
    if agg_ctx.kernel_mode == "jit":
        assert st.last_kernel_kind() == (True, ""), st.last_kernel_kind()
    kk, aa = st.finalize()
    k, _ = gen.generate(gen.GEN_MOD, groups, 42, 0, 0, n)
    a, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 1, 0, n)
    b, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 2, 0, n)
    ref = S.group_aggregate([k], [None], [S.arith(S.OP_ADD, a, None, b, None)[0], None, a, b], [None] * 4, C4_FNS,
                            a > (1 << 19))
    assert_groups_equal(result_dict(kk, aa), ref, C4_FNS)


@pytest.mark.parametrize("groups", [3500, 4096, 5000, 5500, 6500, 7500, 8192, 9500, 12000])
def test_fused_c4_compact_vs_oracle(agg_ctx, groups):
    """Groups just past the regular LDS table: ONE fused pass over a compact table (32-bit keys,
    32-bit MIN / MAX of bare columns, ~6.4K slots in 152 KiB) instead of key-hash passes; past
    that table (to ~10.5K groups: a 6/8 kept share plus up to two spilled sub-buckets, each filling
    at most QE_SPILL_MAXPCT 70 of its aggregation table), one spilling pass whose kept share stays
    in the compact table; beyond, the partitioned update."""
    from kquery.datasource import C4_COLUMNS, ColumnSpec, generate_column

    n, row0 = 2_000_003, 5
    kspec = ColumnSpec("k", N.TYPE_INT64, N.GEN_MOD, groups, 0)
    cols = [generate_column(kspec, n, row0, 42, agg_ctx)] + [generate_column(s, n, row0, 42, agg_ctx)
                                                              for s in C4_COLUMNS[1:]]
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], C4_AGGS, groups)
    st.update_fused(cols, _c4_spec())
    if agg_ctx.kernel_mode == "jit":
        spec, note = st.last_kernel_kind()
        want = ("compact LDS table" if groups <= 5500 else "multi-pass: 2 buckets (compact kept table)"
                if groups <= 9500 else "radix-partitioned")
        assert spec and note.startswith(want), note
        assert ("2 sub-buckets" in note) == (groups in (8192, 9500)), note
    kk, aa = st.finalize()
    k, _ = gen.generate(gen.GEN_MOD, groups, 42, 0, row0, n)
    a, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 1, row0, n)
    b, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 2, row0, n)
    ref = S.group_aggregate([k], [None], [S.arith(S.OP_ADD, a, None, b, None)[0], None, a, b], [None] * 4, C4_FNS,
                            a > (1 << 19))
    assert_groups_equal(result_dict(kk, aa), ref, C4_FNS)


@pytest.mark.parametrize("case,spill", [("fits", 0), ("key_wide", 0), ("value_wide", 0), ("nullable", 0),
                                        ("fits", 1), ("key_wide", 1), ("value_wide", 1), ("fits", 2), ("value_wide", 2)])
def test_compact_table_speculation(agg_ctx, case, spill):
    """The compact table speculates that keys and MIN / MAX inputs fit 32 bits. A batch where one
    does not is still exact (those rows go to the global table) and the state's later batches take
    the bucket passes instead; null keys, INT32_MIN keys and nullable inputs keep their semantics.
    `spill` 1: 6,300 groups, past the one-pass table: the spilling pass over the compact kept table,
    where a wide key or value in the spilled share also makes its 32-bit records misfit; 2: 9,500
    groups, the spilled share in two sub-buckets."""
    rng = np.random.default_rng(len(case) * 7 + spill)
    # (nullable inputs add a non-null count per aggregate to the slot: fewer slots, fewer groups)
    n, groups = 400_000, 2600 if case == "nullable" else (9500 if spill == 2 else 6300 if spill else 4200)
    k = (rng.integers(0, groups, n).astype(np.int64) - groups // 2) * 1021
    k[::997] = -2**31  # the 32-bit table's empty marker is a real key here
    x = rng.integers(-2**31, 2**31, n).astype(np.int64)
    kv = xv = None
    half = n // 2
    if case == "key_wide":
        k[:half:5000] = 2**40 + 3
    elif case == "value_wide":
        x[:half:3000] = -2**45
    elif case == "nullable":
        kv = rng.random(n) > 0.02
        xv = rng.random(n) > 0.1
    fns = [N.AGG_SUM, N.AGG_COUNT_STAR, N.AGG_MIN, N.AGG_MAX, N.AGG_COUNT]
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], [(f, N.TYPE_INT64) for f in fns], groups)
    notes = []
    for s, e in ((0, half), (half, n)):
        st.update([dcol(agg_ctx, N.TYPE_INT64, k[s:e], None if kv is None else kv[s:e])],
                  [dcol(agg_ctx, N.TYPE_INT64, x[s:e], None if xv is None else xv[s:e])] * len(fns))
        notes.append(st.last_kernel_kind()[1])
    if agg_ctx.kernel_mode == "jit":
        want = "multi-pass: 2 buckets (compact kept table)" if spill else "compact LDS table"
        # (a misfit in the spilled share reruns that share and names it: "multi-pass: 2 buckets, ...")
        assert notes[0].startswith("multi-pass: 2 buckets" if spill and case != "fits" else want), notes
        if spill and case == "fits":
            assert ("in 2 sub-buckets" in notes[0]) == (spill == 2), notes
        if case in ("key_wide", "value_wide"):
            assert not notes[1].startswith(want), notes
        else:
            assert notes[1].startswith(want), notes
    kk, aa = st.finalize()
    ref = S.group_aggregate([k], [kv], [x] * len(fns), [xv] * len(fns), fns)
    assert_groups_equal(result_dict(kk, aa), ref, fns)


def test_fused_c4_multipass_vs_oracle(agg_ctx, mp_mode):
    from kquery.datasource import C4_COLUMNS, ColumnSpec, generate_column

    n, groups = 2_000_003, 4000
    kspec = ColumnSpec("k", N.TYPE_INT64, N.GEN_MOD, groups, 0)
    cols = [generate_column(kspec, n, 0, 42, agg_ctx)] + [generate_column(s, n, 0, 42, agg_ctx) for s in C4_COLUMNS[1:]]
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], C4_AGGS, groups)
    st.update_fused(cols, _c4_spec())
    check_multipass(agg_ctx, st, mp_mode)
    kk, aa = st.finalize()
    k, _ = gen.generate(gen.GEN_MOD, groups, 42, 0, 0, n)
    a, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 1, 0, n)
    b, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 2, 0, n)
    ref = S.group_aggregate([k], [None], [S.arith(S.OP_ADD, a, None, b, None)[0], None, a, b], [None] * 4, C4_FNS,
                            a > (1 << 19))
    assert_groups_equal(result_dict(kk, aa), ref, C4_FNS)


def test_hashagg_adapts_to_partitioned(agg_ctx, part_mode):
    """expected_groups left at its default while the batches hold 300K groups: the first batch
    grows the global table, and the later batches switch to the partitioned update by themselves."""
    rng = np.random.default_rng(23)
    n, nb = 1_500_000, 3
    k = rng.integers(0, 300_000, n).astype(np.int64) * 31 + 5
    x = rng.integers(-1000, 1000, n).astype(np.int64)
    fns = [N.AGG_SUM, N.AGG_COUNT_STAR, N.AGG_MIN, N.AGG_MAX]
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], [(f, N.TYPE_INT64) for f in fns])
    notes = []
    for s in range(0, n, n // nb):
        st.update([dcol(agg_ctx, N.TYPE_INT64, k[s:s + n // nb])], [dcol(agg_ctx, N.TYPE_INT64, x[s:s + n // nb])] * 4)
        notes.append(st.last_kernel_kind()[1])
    if agg_ctx.kernel_mode == "jit":
        assert not notes[0].startswith("radix-partitioned"), notes
        assert all(m.startswith("radix-partitioned") for m in notes[1:]), notes
    kk, aa = st.finalize()
    ref = S.group_aggregate([k], [None], [x] * 4, [None] * 4, fns)
    assert_groups_equal(result_dict(kk, aa), ref, fns)


@pytest.mark.parametrize("groups,threshold", [(100_000, 1 << 19), (1 << 20, 1 << 19), (100_000, 1 << 21)])
def test_fused_c4_partitioned_vs_oracle(agg_ctx, part_mode, groups, threshold):
    """C4 query shape with k = u mod G for large G (partitioned fused path), including a predicate
    no row passes (zero records, zero groups)."""
    from kquery.datasource import C4_COLUMNS, ColumnSpec, generate_column

    n, row0 = 3_000_001, 7
    kspec = ColumnSpec("k", N.TYPE_INT64, N.GEN_MOD, groups, 0)
    cols = [generate_column(kspec, n, row0, 42, agg_ctx)] + [generate_column(s, n, row0, 42, agg_ctx)
                                                              for s in C4_COLUMNS[1:]]
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], C4_AGGS, groups)
    st.update_fused(cols, _c4_spec(threshold))
    check_partitioned(agg_ctx, st)
    if groups == 1 << 20 and threshold < n and getattr(agg_ctx, "kernel_mode", "jit") == "jit":
        # half-full 4096-slot tables: 512 buckets of 24-byte column records, staged scatter
        assert "512 buckets" in st.last_kernel_kind()[1] and "staged" in st.last_kernel_kind()[1], st.last_kernel_kind()
    kk, aa = st.finalize()
    k, _ = gen.generate(gen.GEN_MOD, groups, 42, 0, row0, n)
    a, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 1, row0, n)
    b, _ = gen.generate(gen.GEN_MOD, 1 << 20, 42, 2, row0, n)
    ref = S.group_aggregate([k], [None], [S.arith(S.OP_ADD, a, None, b, None)[0], None, a, b], [None] * 4, C4_FNS,
                            a > threshold)
    assert_groups_equal(result_dict(kk, aa), ref, C4_FNS)
    if threshold >= 1 << 20:
        assert kk[0].length == 0


NARROW_FNS = [N.AGG_SUM, N.AGG_COUNT_STAR, N.AGG_MIN, N.AGG_MAX]


@pytest.mark.parametrize("case", ["fits", "edges", "wide_first", "wide_later"])
def test_partitioned_narrow_records(agg_ctx, part_mode, case):
    """Partitioned records in 32-bit words (Plan.part_narrow): integral words are stored narrow while
    every value of the update survives int32 (sign-extended, INT32_MIN / INT32_MAX included); one
    value outside it (here a single row, key or input) makes the scatter flag the update, the
    aggregation pass leaves the table alone and the update reruns with 64-bit words, which the state
    then keeps. Three batches; results equal the oracle either way."""
    rng = np.random.default_rng(len(case) * 7)
    n, groups = 900_000, 80_000
    k = (rng.integers(0, groups, n).astype(np.int64) - groups // 2) * 20011
    x = rng.integers(-2**31, 2**31, n).astype(np.int64)
    if case == "edges":
        x[::1000] = -2**31
        x[1::1000] = 2**31 - 1
        k[5] = 2**31 - 1
        k[6] = -2**31
    elif case == "wide_first":
        x[17] = 2**31  # one row of batch 0
    elif case == "wide_later":
        k[2 * n // 3 + 5] = -2**31 - 1  # one key of batch 2
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], [(f, N.TYPE_INT64) for f in NARROW_FNS], groups)
    notes = []
    for s in range(0, n, n // 3):
        st.update([dcol(agg_ctx, N.TYPE_INT64, k[s:s + n // 3])], [dcol(agg_ctx, N.TYPE_INT64, x[s:s + n // 3])] * 4)
        check_partitioned(agg_ctx, st)
        notes.append(st.last_kernel_kind()[1])
    if getattr(agg_ctx, "kernel_mode", "jit") == "jit":
        narrow = ["32-bit" in m for m in notes]
        assert narrow == {"fits": [True] * 3, "edges": [True] * 3, "wide_first": [False] * 3,
                          "wide_later": [True, True, False]}[case], notes
        if narrow[0]:
            assert "records of 8 B (column words, 32-bit)" in notes[0], notes  # key, x
    kk, aa = st.finalize()
    ref = S.group_aggregate([k], [None], [x] * 4, [None] * 4, NARROW_FNS)
    assert_groups_equal(result_dict(kk, aa), ref, NARROW_FNS)


@pytest.mark.parametrize("n", [1, 2, 3, 255, 257, 4097])
def test_partitioned_tiny_batches(agg_ctx, part_mode, n):
    """Partitioned updates of a few rows: the staged scatter's prefetch loads row pairs clamped to
    the column's last pair (n >= 2; one row goes to the direct scatter), so the odd last row of a
    batch must come from the pair's upper half. Every row selected, nullable key."""
    rng = np.random.default_rng(n)
    k = rng.integers(-2**30, 2**30, n).astype(np.int64)
    kv = rng.random(n) > 0.1
    x = rng.integers(-2**20, 2**20, n).astype(np.int64)
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], [(f, N.TYPE_INT64) for f in NARROW_FNS], 100_000)
    st.update([dcol(agg_ctx, N.TYPE_INT64, k, kv)], [dcol(agg_ctx, N.TYPE_INT64, x)] * 4)
    check_partitioned(agg_ctx, st)
    kk, aa = st.finalize()
    ref = S.group_aggregate([k], [kv], [x] * 4, [None] * 4, NARROW_FNS)
    assert_groups_equal(result_dict(kk, aa), ref, NARROW_FNS)


_NARROW_OFF_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/query-engines_amd"]
import numpy as np
from kquery import native as N
from kquery.aggregate import HashAggregateState
from kquery.columnar import Context, DeviceColumn
ctx = Context.get(0)
k = np.arange(300000, dtype=np.int64) % 100000
st = HashAggregateState(ctx, [N.TYPE_INT64], [(N.AGG_SUM, N.TYPE_INT64)], 100000)
st.update([DeviceColumn.from_numpy(N.TYPE_INT64, k, ctx=ctx)], [DeviceColumn.from_numpy(N.TYPE_INT64, 3 * k, ctx=ctx)])
note = st.last_kernel_kind()[1]
kk, aa = st.finalize()
got = dict(zip(kk[0].to_numpy().tolist(), aa[0].to_numpy().tolist()))
assert note.startswith("radix-partitioned") and "32-bit" not in note, note
assert got == {i: 9 * i for i in range(100000)}
print("ok")
"""


def test_partitioned_narrow_off():
    """QE_PART_NARROW=0 (read once per process, so run in a child process): 64-bit records."""
    import os
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parents[1]
    env = dict(os.environ, QE_PART_NARROW="0")
    r = subprocess.run([sys.executable, "-c", _NARROW_OFF_CHILD, str(root)], cwd=str(root), env=env,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


_KNOB_CHILD = """
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/query-engines_amd"]
import numpy as np
from kquery import native as N
from kquery.aggregate import HashAggregateState
from kquery.columnar import Context, DeviceColumn
from oracle import semantics as S
ctx = Context.get(0)
fns = [N.AGG_SUM, N.AGG_MIN, N.AGG_MAX, N.AGG_COUNT, N.AGG_COUNT_STAR]
rng = np.random.default_rng(7)
n = 700_001
k = rng.integers(0, 90_000, n).astype(np.int64) * 7919 - 3
kv = rng.random(n) > 0.01
k[rng.random(n) < 0.001] = -2**31  # the 32-bit EMPTY sentinel as a key
x = rng.integers(-2**31, 2**31, n).astype(np.int64)
xv = rng.random(n) > 0.1
st = HashAggregateState(ctx, [N.TYPE_INT64], [(f, N.TYPE_INT64) for f in fns], 100_000)
for s, e in ((0, 300_001), (300_001, n)):
    st.update([DeviceColumn.from_numpy(N.TYPE_INT64, k[s:e], kv[s:e], ctx=ctx)],
              [DeviceColumn.from_numpy(N.TYPE_INT64, x[s:e], xv[s:e], ctx=ctx)] * len(fns))
    note = st.last_kernel_kind()[1]
    assert note.startswith("radix-partitioned") and "32-bit" in note, note
kk, aa = st.finalize()
ref = S.group_aggregate([k], [kv], [x] * len(fns), [xv] * len(fns), fns)
got = {}
kl, avs = kk[0].to_pylist(), [a.to_pylist() for a in aa]
for i, key in enumerate(kl):
    got[(key,)] = tuple(a[i] for a in avs)
assert len(got) == len(ref), (len(got), len(ref))
for key, want in ref.items():
    assert tuple(got[key]) == tuple(want), (key, got[key], want)
print("ok")
"""


@pytest.mark.parametrize("knobs", [
    {"QE_PSCATTER_FAST": "1"},
    {"QE_PSCATTER_FAST": "1", "QE_PART_BLK64": "1"},
    {"QE_PAGG_TRANSPOSE": "0"},
    {"QE_PAGG_FAST_DEPTH": "4"},
    {"QE_PAGG_INTERLEAVE": "1"},
    {"QE_PAGG_FAST": "0"},
], ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_partitioned_layout_knobs(knobs):
    """The partitioned path's opt-in and opt-out layouts (knobs read once per process, so each in a
    child process): the record-regrouping scatter, 64-record blocks, direct lane loads in the fast
    aggregation pass, its 4-deep buffer rotation, and the general aggregation pass — chunked 32-bit
    records, nullable keys and inputs, INT32_MIN keys, two batches; bit-exact vs the oracle."""
    import os
    import pathlib
    import subprocess
    import sys

    root = pathlib.Path(__file__).resolve().parents[1]
    env = dict(os.environ, QE_PART_CHUNKED="1", **knobs)
    r = subprocess.run([sys.executable, "-c", _KNOB_CHILD, str(root)], cwd=str(root), env=env,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-3000:]


def _colrec_case(shape, rng, n):
    """(slot arrays, slot valids, slot types, aggs, programs, oracle inputs, predicate term)."""
    from kquery.workloads import _prog, _tok

    k, kv = aggdata.colrec_data(rng, n)
    if shape == "f64":
        x, xv = aggdata.group_values(k, kv, 3)
        aggdata.check_group_conditions(k, kv, x, xv)
        aggdata.check_group_conditions(k, kv, x, xv, xv & (x > -50.0), kinds=False)
        cols, valids, types = [k, x], [kv, xv], [N.TYPE_INT64, N.TYPE_FLOAT64]
        aggs = [(N.AGG_SUM, N.TYPE_FLOAT64), (N.AGG_MAX, N.TYPE_FLOAT64), (N.AGG_MIN, N.TYPE_FLOAT64),
                (N.AGG_AVG, N.TYPE_FLOAT64), (N.AGG_COUNT_STAR, N.TYPE_INT64)]
        progs = {0: [_tok(N.TOK_COL, 1), _tok(N.TOK_LIT, 0, 1.5), _tok(N.TOK_ADD)], 1: [_tok(N.TOK_COL, 1)],
                 2: [_tok(N.TOK_COL, 1)], 3: [_tok(N.TOK_COL, 1)]}
        s0 = S.arith(S.OP_ADD, x, xv, 1.5, None)
        ins = [s0, (x, xv), (x, xv), (x, xv), (None, None)]
        term, sel = N.QePredTerm(1, N.OP_GT, -1, 0, N.scalar(-50.0)), xv & (x > -50.0)
    else:
        a = rng.integers(-2**40, 2**40, n).astype(np.int64)
        av = rng.random(n) > 0.1
        c = rng.integers(-3, 4, n).astype(np.int64)
        cv = rng.random(n) > 0.1
        cols, valids, types = [k, a, c], [kv, av, cv], [N.TYPE_INT64] * 3
        if shape == "odd":  # key, a, flags: 3 words (values would take 5)
            aggs = [(N.AGG_SUM, N.TYPE_INT64), (N.AGG_MIN, N.TYPE_INT64), (N.AGG_COUNT, N.TYPE_INT64),
                    (N.AGG_COUNT_STAR, N.TYPE_INT64)]
            progs = {0: [_tok(N.TOK_COL, 1), _tok(N.TOK_COL, 1), _tok(N.TOK_ADD)], 1: [_tok(N.TOK_COL, 1)],
                     2: [_tok(N.TOK_COL, 1)]}
            ins = [S.arith(S.OP_ADD, a, av, a, av), (a, av), (a, av), (None, None)]
        else:  # key, a, c, flags: 4 words (values would take 6); division by zero is null
            aggs = [(N.AGG_SUM, N.TYPE_INT64), (N.AGG_MIN, N.TYPE_INT64), (N.AGG_MAX, N.TYPE_INT64),
                    (N.AGG_SUM, N.TYPE_INT64), (N.AGG_COUNT_STAR, N.TYPE_INT64)]
            progs = {0: [_tok(N.TOK_COL, 1), _tok(N.TOK_COL, 2), _tok(N.TOK_DIV)], 1: [_tok(N.TOK_COL, 1)],
                     2: [_tok(N.TOK_COL, 2), _tok(N.TOK_LIT, 0, 7), _tok(N.TOK_MUL)], 3: [_tok(N.TOK_COL, 2)]}
            ins = [S.arith(S.OP_DIV, a, av, c, cv), (a, av), S.arith(S.OP_MUL, c, cv, 7, None), (c, cv), (None, None)]
        term, sel = N.QePredTerm(1, N.OP_GT, -1, 0, N.scalar(-(2**39))), av & (a > -(2**39))
    return cols, valids, types, aggs, progs, ins, term, sel


@pytest.mark.parametrize("shape,width", [("odd", 24), ("even", 32), ("f64", 32)])
def test_fused_partitioned_column_records(agg_ctx, part_mode, shape, width):
    """Partitioned records that hold the columns the aggregate programs read, when that is narrower
    than the programs' values: the programs are re-evaluated in the aggregation pass. Nullable key
    and inputs, integer division by zero (null), literals, fp64 MIN/MAX row order, two batches."""
    rng = np.random.default_rng(len(shape))
    n = 1_000_000
    cols, valids, types, aggs, progs, ins, term, sel = _colrec_case(shape, rng, n)
    spec = N.QeFusedSpec()
    spec.mask_col = -1
    spec.nterms = 1
    spec.terms[0] = term
    spec.key_cols[0] = 0
    for j, toks in progs.items():
        p = spec.inputs[j]
        p.ntokens = len(toks)
        for i, t in enumerate(toks):
            p.tokens[i] = t
    st = HashAggregateState(agg_ctx, [N.TYPE_INT64], aggs, 60_000)
    half = 400_001
    for s0, e0 in ((0, half), (half, n)):
        st.update_fused([dcol(agg_ctx, t, v[s0:e0], m[s0:e0]) for t, v, m in zip(types, cols, valids)], spec)
        check_partitioned(agg_ctx, st)
        if getattr(agg_ctx, "kernel_mode", "jit") == "jit":
            assert f"records of {width} B (column words)" in st.last_kernel_kind()[1]
    kk, aa = st.finalize()
    fns = [f for f, _ in aggs]
    ref = S.group_aggregate([cols[0]], [valids[0]], [v for v, _ in ins], [m for _, m in ins], fns, sel)
    assert_groups_equal(result_dict(kk, aa), ref, fns)


@pytest.mark.slow
def test_c4_full_size_properties(gpu_ctx):
    """BASELINE config 4 at full size (1B rows, one GPU): size-independent properties.
    Sum over groups of COUNT(*) == rows passing the filter (qe_filter_count on the predicate);
    sum over groups of SUM(a+b) == global SUM of a+b over the selected rows (qe_agg_global);
    global MIN(a) / MAX(b) == min / max over the groups; exactly 1024 groups."""
    from kquery.datasource import C4_COLUMNS, generate_column

    n = 1_000_000_000
    cols = [generate_column(s, n, 0, 42, gpu_ctx) for s in C4_COLUMNS]
    st = HashAggregateState(gpu_ctx, [N.TYPE_INT64], C4_AGGS, 1024)
    st.update_fused(cols, _c4_spec())
    kk, aa = st.finalize()
    assert kk[0].length == 1024
    sums, counts, mins, maxs = (x.to_numpy() for x in aa)
    mask = DeviceColumn.empty(N.TYPE_BOOL, n, False, ctx=gpu_ctx)
    _eval(gpu_ctx, "qe_eval_cmp", N.OP_GT, cols[1], 1 << 19, mask)
    cnt = N.C.c_int64()
    mc = mask.as_c()
    N.check(N.lib().qe_filter_count(gpu_ctx.handle, N.C.byref(mc), N.C.byref(cnt)))
    assert int(counts.sum()) == cnt.value
    ab = DeviceColumn.empty(N.TYPE_INT64, n, False, ctx=gpu_ctx)
    _eval(gpu_ctx, "qe_eval_arith", N.OP_ADD, cols[1], cols[2], ab)
    g = _global(gpu_ctx, ab, mask)
    assert g.count == cnt.value
    assert int(sums.astype(np.uint64).sum(dtype=np.uint64).view(np.int64)) == g.sum
    ga = _global(gpu_ctx, cols[1], mask)
    gb = _global(gpu_ctx, cols[2], mask)
    assert int(mins.min()) == ga.min and int(maxs.max()) == gb.max


def test_export_partition_matches_oracle(gpu_ctx):
    """qe_hashagg_export buckets groups by the same hash(key) mod P as oracle/records.py."""
    import struct

    from oracle import records as R

    rng = np.random.default_rng(21)
    k = rng.integers(-10**12, 10**12, 100_000).astype(np.int64)
    st = HashAggregateState(gpu_ctx, [N.TYPE_INT64], [(N.AGG_COUNT_STAR, N.TYPE_INT64)], 1 << 17)
    st.update([dcol(gpu_ctx, N.TYPE_INT64, k)], [None])
    for P in (1, 3, 8):
        recs, counts = st.export(P)
        raw = recs.cpu().numpy().tobytes()
        rb = st.record_bytes()
        off = 0
        for p in range(P):
            for i in range(counts[p]):
                key = struct.unpack_from("<q", raw, (off + i) * rb)[0]
                assert R.partition_of(key, False, P) == p
            off += counts[p]
        assert off == len(np.unique(k))


@pytest.mark.parametrize("slot_records,expected,async_update", [(None, 8192, False), (10, 8192, False),
                                                                (None, 8192, True), (8192, 16, True)])
def test_exchange_rccl_single_rank(gpu_ctx, slot_records, expected, async_update):
    """The RCCL path of kquery.exchange (backend nccl = RCCL) end to end on one rank: fixed slots
    (None: capacity = expected groups), slots too small for the ~4990 groups (fallback), and a
    stream-ordered partial update exported before it is read back — (8192, 16): its table
    overflowed (deferred rows), so the slot headers must force the variable-size exchange, which
    settles the update first."""
    import os
    import socket

    import torch
    import torch.distributed as dist

    from kquery.exchange import exchange_partials

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        rng = np.random.default_rng(4)
        k = rng.integers(0, 5000, 200_000).astype(np.int64)
        x = rng.integers(-100, 100, 200_000).astype(np.int64)
        aggs = [(N.AGG_SUM, N.TYPE_INT64), (N.AGG_COUNT_STAR, N.TYPE_INT64)]
        part = HashAggregateState(gpu_ctx, [N.TYPE_INT64], aggs, expected, async_update=async_update)
        owner = HashAggregateState(gpu_ctx, [N.TYPE_INT64], aggs, 8192)
        K, X = dcol(gpu_ctx, N.TYPE_INT64, k), dcol(gpu_ctx, N.TYPE_INT64, x)
        part.update([K], [X, None])
        n = exchange_partials(part, owner, slot_records=slot_records)
        assert n == len(np.unique(k))
        kk, aa = owner.finalize()
        ref = S.group_aggregate([k], [None], [x, None], [None, None], [N.AGG_SUM, N.AGG_COUNT_STAR])
        assert_groups_equal(result_dict(kk, aa), ref, [N.AGG_SUM, N.AGG_COUNT_STAR])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n", [1_000_003, 4_000_000])
def test_fused_c5_lineitem_vs_oracle(agg_ctx, n):
    """BASELINE config 5 shape (Q1-like): date32 / fp64 / int64 predicates (one a range), two
    uint8 keys packed, nested fp64 expressions, AVG and COUNT(*)."""
    from kquery.datasource import C5_COLUMNS, generate_column
    from kquery.workloads import C5_AGGS, C5_KEY_TYPES, c5_spec

    row0 = 1234567
    cols = [generate_column(s, n, row0, 42, agg_ctx) for s in C5_COLUMNS]
    st = HashAggregateState(agg_ctx, C5_KEY_TYPES, C5_AGGS, 16)
    st.update_fused(cols, c5_spec())
    check_kernel_kind(agg_ctx, st)
    kk, aa = st.finalize()
    v = {s.name: gen.generate(s.dist, s.param, 42, s.col_id, row0, n)[0] for s in C5_COLUMNS}
    qty, price, disc, tax = v["l_quantity"], v["l_extendedprice"], v["l_discount"], v["l_tax"]
    flag, status = v["l_returnflag"].astype(np.uint8), v["l_linestatus"].astype(np.uint8)
    ship = v["l_shipdate"].astype(np.int32)
    sel = (ship <= 2400) & (disc >= 0.05) & (disc <= 0.07) & (qty < 24)
    dp = price * (1.0 - disc)
    dpt = dp * (1.0 + tax)
    fns = [f for f, _ in C5_AGGS]
    ref = S.group_aggregate([flag.astype(np.int64), status.astype(np.int64)], [None, None],
                            [qty, price, dp, dpt, price, None], [None] * 6, fns, sel)
    got = result_dict(kk, aa)
    assert_groups_equal(got, ref, fns)
    assert len(got) == 6


@pytest.mark.parametrize("state,field", [("CA", "filter_state_CA_project_id_first_name"),
                                         ("Uppsala", "filter_state_Uppsala_ids")])
def test_config1_employee_csv_on_device(gpu_ctx, state, field):
    """BASELINE config 1: employee.csv scan -> filter(state = lit) -> project(id, first_name),
    through the device operators (UTF-8 predicate + UTF-8 compaction), against the reference
    fixture's known answers."""
    import json
    import pathlib

    from kquery.csv_source import CsvDataSource
    from kquery.columnar import Field, Schema
    from kquery.expressions import ColumnExpression, EqExpression, LiteralStringExpression
    from kquery.operators import ProjectionExec, ScanExec, SelectionExec

    gold = pathlib.Path(__file__).parent / "golden"
    kat = json.loads((gold / "employee_kat.json").read_text())
    ds = CsvDataSource(str(gold / "employee.csv"), True, 1000, ctx=gpu_ctx)
    scan = ScanExec(ds, ["first_name", "id", "state"])
    sel = SelectionExec(scan, EqExpression(ColumnExpression(2), LiteralStringExpression(state)))
    proj = ProjectionExec(sel, Schema([Field("id", N.TYPE_UTF8), Field("first_name", N.TYPE_UTF8)]),
                          [ColumnExpression(1), ColumnExpression(0)])
    out = list(proj.execute())
    ids = [v for b in out for v in b.field(0).to_pylist()]
    names = [v for b in out for v in b.field(1).to_pylist()]
    if state == "CA":
        assert [[i, nm] for i, nm in zip(ids, names)] == kat[field]
    else:
        assert ids == kat[field] and names == ["Matte", "Other"]


@pytest.mark.parametrize("n", [1, 100, 8193, 200_001])
def test_filter_utf8_columns(gpu_ctx, n):
    from kquery.columnar import RecordBatch, Schema
    from kquery.operators import filter_batch

    rng = np.random.default_rng(n)
    words = ["", "a", "Pärsson", "Uppsala", "x" * 40, "tripdata", "VendorID"]
    strs = [None if rng.random() < 0.1 else words[rng.integers(len(words))] + str(rng.integers(1000)) for _ in range(n)]
    m = rng.random(n) < 0.4
    col = DeviceColumn.from_strings(strs, ctx=gpu_ctx)
    out = filter_batch(RecordBatch(Schema([]), [col, dcol(gpu_ctx, N.TYPE_INT64, np.arange(n, dtype=np.int64))]),
                       dcol(gpu_ctx, N.TYPE_BOOL, m))
    want = [s for s, keep in zip(strs, m) if keep]
    assert out.field(0).to_pylist() == want
    assert out.field(1).to_numpy().tolist() == np.nonzero(m)[0].tolist()


def _unfmix64(h: int) -> int:
    """Inverse of the murmur3 finaliser (qe_dev.hpp fmix64): a key whose table hash is `h`."""
    m = (1 << 64) - 1
    h ^= h >> 33
    h = (h * pow(0xC4CEB9FE1A85EC53, -1, 1 << 64)) & m
    h ^= h >> 33
    h = (h * pow(0xFF51AFD7ED558CCD, -1, 1 << 64)) & m
    h ^= h >> 33
    return h - (1 << 64) if h >= 1 << 63 else h


@pytest.mark.parametrize("path", ["slots", "records"])
def test_import_probe_limit_loses_no_group_silently(gpu_ctx, path):
    """300 keys whose global-table hash shares its low 32 bits form one probe chain longer than
    the probe limit (HA_GLOBAL_MAXP = 256) at every table size, so an import must drop groups.
    The loss must surface as CapacityError — on the slot path (k_import_slots runs without a
    read-back of its own) at the latest from finalize — never as a silently short result."""
    import torch

    from oracle import records as R

    keys = [_unfmix64((j << 32) | 0x1234) for j in range(1, 301)]
    assert all(R.fmix64(k) & 0xFFFFFFFF == 0x1234 for k in keys)
    fns = [R.AGG_SUM, R.AGG_COUNT_STAR]
    groups = {k: (1, [(k, 1), (0, 1)]) for k in keys}
    aggs = [(N.AGG_SUM, N.TYPE_INT64), (N.AGG_COUNT_STAR, N.TYPE_INT64)]
    st = HashAggregateState(gpu_ctx, [N.TYPE_INT64], aggs, 1024)
    with pytest.raises(N.CapacityError, match="lost"):
        if path == "slots":
            buf = R.encode_slots(groups, fns, 1, 512)
            dev = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(gpu_ctx.torch_device)
            assert st.import_slots(dev, 1, 512) == 300
            st.finalize()
        else:
            payload, counts = R.encode(groups, fns, 1)
            dev = torch.frombuffer(bytearray(payload), dtype=torch.uint8).to(gpu_ctx.torch_device)
            st.import_records(dev, counts[0])
    # the same keys spread over distinct chains import and finalise exactly
    st2 = HashAggregateState(gpu_ctx, [N.TYPE_INT64], aggs, 1024)
    spread = {j * 7919 + 1: (1, [(j, 1), (0, 1)]) for j in range(300)}
    buf = R.encode_slots(spread, fns, 1, 512)
    dev = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(gpu_ctx.torch_device)
    assert st2.import_slots(dev, 1, 512) == 300
    kc, res = st2.finalize()
    assert kc[0].length == 300 and int(res[1].to_numpy().sum()) == 300


def test_generic_kernel_lds_budget(gpu_ctx):
    """The 152 KiB LDS table budget belongs to the specialised 1024-thread kernel (one workgroup
    per CU). A state created with JIT on whose update then runs the generic 512-thread kernel (JIT
    switched off after create, as after a failed hipRTC compile) gets its table re-laid out within
    the 80 KiB budget: two workgroups per CU, not one, and the same results."""
    rng = np.random.default_rng(7)
    n = 400_000
    k = rng.integers(0, 2000, n).astype(np.int64)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    aggs = [(N.AGG_SUM, N.TYPE_INT64), (N.AGG_COUNT_STAR, N.TYPE_INT64), (N.AGG_MIN, N.TYPE_INT64),
            (N.AGG_MAX, N.TYPE_INT64)]
    st = HashAggregateState(gpu_ctx, [N.TYPE_INT64], aggs, 2000)
    kc, vc = dcol(gpu_ctx, N.TYPE_INT64, k), dcol(gpu_ctx, N.TYPE_INT64, v)
    N.check(N.lib().qe_ctx_set_jit(gpu_ctx.handle, 0))
    try:
        st.update([kc], [vc, None, vc, vc])
        spec, note = st.last_kernel_kind()
        keys, vals = st.finalize()
        gpu_ctx.synchronize()
    finally:
        N.check(N.lib().qe_ctx_set_jit(gpu_ctx.handle, 1))
    assert not spec and "2 workgroups per CU" in note, note
    ref = S.group_aggregate([k], [None], [v, None, v, v], [None] * 4,
                            [S.AGG_SUM, S.AGG_COUNT_STAR, S.AGG_MIN, S.AGG_MAX], None)
    kv = keys[0].to_numpy()
    cols = [c.to_numpy() for c in vals]
    got = {(int(kv[i]),): [int(c[i]) for c in cols] for i in range(len(kv))}
    assert got == ref
