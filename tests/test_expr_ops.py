"""The unfused expression and selection kernels (qe_expr.hip: K1 qe_eval_arith / qe_eval_arith_dlen,
K2 qe_eval_cmp, K3a qe_eval_bool; qe_filter.hip: K3b qe_filter_count / qe_filter_apply /
qe_filter_apply_async) held to the oracle through the C ABI, on the inputs of exprcases.py (whose
conditions tests/test_expr_cases.py asserts on the CPU).

Every comparison is exact: integers with array_equal, fp64 by bit pattern on the valid rows (any
NaN equal to any NaN: IEEE 754 leaves a result NaN's sign open, and the device returns x - NaN
with the sign flipped where numpy keeps it; a gathered value is a copy, NaN bits included),
validity and BOOL bitmaps byte for byte over the ceil(n / 8) bytes a kernel writes, so the padding
bits of the last byte must be 0. Output buffers are filled with 0xFF / a sentinel before each call
and input validity is uploaded with the padding bits of its last byte SET (Arrow leaves them
unspecified), so an unwritten byte or a padding bit passed through shows. One thing is not pinned:
the header leaves a comparison's VALUE bit under a null row unspecified, so K2 (and K3a) values are
compared as `values & validity`, as tests/test_gpu_parity.py does; their own padding bits must
still be 0.

What fails if the kernels are wrong in these ways. Each slip changes a computed value or bit only; it
was applied alone to a scratch copy of the sources, the library rebuilt and this file run against it
once on an MI355X (291 tests; the unmodified library passes all). Failures seen, by test:
  k_cmp comparing integers as uint64_t (35): test_cmp_matrix for the 15 pairs without an fp64 side or
      two UINT8 ones (opposite signs, INT64_MIN against INT64_MAX), test_cmp_literals for every integer
      kind, test_sizes[i32-i32 / u8-i64], test_grid_stride_i32_gt_literal, test_composed_predicate;
  load8's INT32 vector path zero-extending (102): test_arith_matrix (64) and test_cmp_matrix (16) with
      an "i32" or "d32" side, both literal tests for those kinds, test_sizes from 8 rows on (1 and 7
      rows take the scalar tail and pass), test_grid_stride_i32_gt_literal, test_composed_predicate;
  load8's tail mask `valid &= (1u << nrows) - 1` removed (152): every K1 / K2 test at a size with a
      tail (not 8 or 2,048 rows): the padding bits uploaded with the input validity come out in the
      last validity byte; the three arithmetic / comparison grid-stride cases;
  make_src leaving an int literal unconverted when the compute type is fp64 (4):
      test_arith_literals[f64-*] and test_cmp_literals[f64-*] (7, -1, the int64 extremes against fp64);
  k_bool's OR validity reduced to `la & lb` (4): test_bool3[OR-8 / 9 / 2049] (true OR null is true;
      one row holds no such pair), test_composed_predicate (c IS NULL keeps rows whose left side is null);
  flush_valid_bits storing plainly whenever l0 >= 0 (31): test_filter_tiles and
      test_filter_batch_of_11_columns for inside_word, empty_middle, ones, boundary_then_tail and
      light_after_heavy in all three mask forms, and test_composed_predicate: a tile's plain store of
      the word it shares with the next one clears that tile's bits when it lands second (a matter of
      timing: runs of ones lie across every seam in the columns of even phase, and light_after_heavy
      makes the order near certain: 40 rows finish long before 8,191)."""
import itertools

import numpy as np
import pytest

import exprcases as K
from oracle import semantics as S

pytestmark = pytest.mark.gpu

from kquery import native as N  # noqa: E402
from kquery.columnar import DeviceColumn, Field, RecordBatch, Schema, bitmap_bytes  # noqa: E402

TYPE = {"i64": N.TYPE_INT64, "f64": N.TYPE_FLOAT64, "i32": N.TYPE_INT32, "d32": N.TYPE_DATE32, "u8": N.TYPE_UINT8}
PAIRS = list(itertools.product(K.KINDS, K.KINDS))
SENTINEL = 0x5A5A5A5A5A5A5A5A
SENTINEL_F = -12345.5


# ---- device columns ------------------------------------------------------------------------------------
def _up(ctx, arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr)).to(ctx.torch_device)


def bitmap(bits, dirty=True) -> np.ndarray:
    """LSB-first bitmap padded to whole 32-bit words; dirty: the padding bits of the last used byte set."""
    n = len(bits)
    buf = np.zeros(max(bitmap_bytes(n), 4), dtype=np.uint8)
    packed = np.packbits(np.asarray(bits, dtype=bool), bitorder="little")
    buf[: len(packed)] = packed
    if dirty and n % 8:
        buf[(n - 1) // 8] |= (0xFF << (n % 8)) & 0xFF
    return buf


def dcol(ctx, kind, values, valid=None):
    c = DeviceColumn.from_numpy(TYPE[kind], values, None, ctx=ctx)
    if valid is not None:
        c.validity = _up(ctx, bitmap(valid))
    return c


def bcol(ctx, bits, valid=None, dirty=True):
    return DeviceColumn(N.TYPE_BOOL, len(bits), _up(ctx, bitmap(bits, dirty)),
                        _up(ctx, bitmap(valid, dirty)) if valid is not None else None, None, ctx)


def scol(ctx, offs, data, valid=None):
    return DeviceColumn(N.TYPE_UTF8, len(offs) - 1, _up(ctx, data), _up(ctx, bitmap(valid)) if valid is not None else None,
                        _up(ctx, offs), ctx)


def scol_of(ctx, values, null_bytes=b"zz", with_validity=True):
    offs, data, valid = K.utf8_arrays(values, null_bytes)
    return scol(ctx, offs, data, valid if with_validity else None)


def out_col(ctx, t, n, nullable):
    """An output whose buffers hold 0xFF bytes / a sentinel: what the kernel leaves must be its own."""
    c = DeviceColumn.empty(t, n, nullable, ctx=ctx)
    if t == N.TYPE_BOOL:
        c.values.fill_(0xFF)
    elif t == N.TYPE_FLOAT64:
        c.values.fill_(SENTINEL_F)
    elif t == N.TYPE_INT64:
        c.values.fill_(SENTINEL)
    else:
        c.values.fill_(0x5A)
    if nullable:
        c.validity.fill_(0xFF)
    return c


def out_utf8(ctx, n, nbytes, nullable):
    import torch

    dev = ctx.torch_device
    return DeviceColumn(N.TYPE_UTF8, n, torch.full((max(nbytes, 1),), 0x5A, dtype=torch.uint8, device=dev),
                        torch.full((max(bitmap_bytes(n), 4),), 0xFF, dtype=torch.uint8, device=dev) if nullable else None,
                        torch.full((n + 1,), -1, dtype=torch.int32, device=dev), ctx)


def raw(t, nbytes):
    return t[:nbytes].cpu().numpy()


def pack(bits):
    return np.packbits(np.asarray(bits, dtype=bool), bitorder="little")


def f64_bits(x):
    """Bit patterns with every NaN as one pattern: IEEE 754 leaves the sign and payload of a NaN
    result open (the device computes x - NaN as x + (-NaN) and returns the flipped sign, numpy the
    operand's). Everything else, -0.0 included, is compared bit for bit."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.int64).copy()
    b[np.isnan(x)] = 0x7FF8000000000000
    return b


def call2(ctx, fn, op, lhs, rhs, out, dlen=None) -> int:
    """qe_eval_arith / qe_eval_cmp / qe_eval_arith_dlen; returns the status."""
    keep = []

    def operand(x):
        if isinstance(x, DeviceColumn):
            c = x.as_c()
            keep.append(c)
            return N.QeOperand(N.C.pointer(c), N.QeScalar())
        return N.QeOperand(None, N.scalar(x.value, N.TYPE_FLOAT64 if x.is_f64 else N.TYPE_INT64))

    a, b, oc = operand(lhs), operand(rhs), out.as_c()
    args = [ctx.handle, op, N.C.byref(a), N.C.byref(b), N.C.byref(oc)]
    if dlen is not None:
        args.append(N.C.c_void_p(dlen.data_ptr()))
    return getattr(N.lib(), fn)(*args)


def call_bool(ctx, op, lhs, rhs, out) -> int:
    a, oc = lhs.as_c(), out.as_c()
    b = rhs.as_c() if rhs is not None else None
    return N.lib().qe_eval_bool(ctx.handle, op, N.C.byref(a), N.C.byref(b) if b is not None else None, N.C.byref(oc))


# ---- checks ------------------------------------------------------------------------------------------------
def check_validity(out, n, want):
    assert np.array_equal(raw(out.validity, (n + 7) // 8), pack(want[:n]))  # (padding bits 0)


def check_values(out, n, r, v, nullable):
    if nullable:
        check_validity(out, n, v)
    else:
        assert v.all()
    got = out.values[:n].cpu().numpy()
    if out.type == N.TYPE_FLOAT64:
        assert r.dtype == np.float64 and np.array_equal(f64_bits(got[v[:n]]), f64_bits(r[:n][v[:n]]))
    else:
        assert r.dtype != np.float64 and np.array_equal(got[v[:n]], r[:n][v[:n]])


def check_bits(out, n, r, v, nullable):
    nb = (n + 7) // 8
    vals = raw(out.values, nb)
    if n % 8:
        assert vals[-1] >> (n % 8) == 0  # the values' own padding bits
    if nullable:
        check_validity(out, n, v)
        vals = vals & raw(out.validity, nb)  # a value bit under a null row is unspecified
    else:
        assert v.all()
    assert np.array_equal(vals, pack(r & v))


def run_arith(ctx, op, lhs, rhs, r, v, n, need_valid):
    t = N.TYPE_FLOAT64 if r.dtype == np.float64 else N.TYPE_INT64
    for nullable in ([True] if need_valid else [False, True]):
        out = out_col(ctx, t, n, nullable)
        assert call2(ctx, "qe_eval_arith", op, lhs, rhs, out) == N.QE_OK, N.lib().qe_last_error()
        check_values(out, n, r, v, nullable)


def run_cmp(ctx, op, lhs, rhs, r, v, n, need_valid):
    for nullable in ([True] if need_valid else [False, True]):
        out = out_col(ctx, N.TYPE_BOOL, n, nullable)
        assert call2(ctx, "qe_eval_cmp", op, lhs, rhs, out) == N.QE_OK, N.lib().qe_last_error()
        check_bits(out, n, r, v, nullable)


# ---- K1 / K2: the operand matrix ---------------------------------------------------------------------------
def _arith_case(ctx, kl, kr, ops, n):
    a, av, b, bv = K.arith_pair(kl, kr, n)
    for ln, rn in K.NULL_COMBOS:
        lv, rv = (av if ln else None), (bv if rn else None)
        A, B = dcol(ctx, kl, a, lv), dcol(ctx, kr, b, rv)
        for op in ops:
            r, v = S.arith(op, a, lv, b, rv)
            run_arith(ctx, op, A, B, r, v, n, ln or rn or (r.dtype != np.float64 and op == S.OP_DIV))


def _cmp_case(ctx, kl, kr, ops, n):
    a, av, b, bv = K.cmp_pair(kl, kr, n)
    for ln, rn in K.NULL_COMBOS:
        lv, rv = (av if ln else None), (bv if rn else None)
        A, B = dcol(ctx, kl, a, lv), dcol(ctx, kr, b, rv)
        for op in ops:
            r, v = S.cmp(op, a, lv, b, rv)
            run_cmp(ctx, op, A, B, r, v, n, ln or rn)


@pytest.mark.parametrize("op", K.ARITH_OPS)
@pytest.mark.parametrize("kl,kr", PAIRS)
def test_arith_matrix(gpu_ctx, kl, kr, op):
    """Every ordered pair of operand kinds, each side with and without validity, 2,055 rows (a second
    block and a 7-row tail)."""
    _arith_case(gpu_ctx, kl, kr, [op], K.MATRIX_N)


@pytest.mark.parametrize("kl,kr", PAIRS)
def test_cmp_matrix(gpu_ctx, kl, kr):
    _cmp_case(gpu_ctx, kl, kr, K.CMP_OPS, K.MATRIX_N)


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("kl,kr", K.SIZE_PAIRS)
def test_sizes(gpu_ctx, kl, kr, n):
    """Every op at every size that reaches another path of load8 / store8."""
    _arith_case(gpu_ctx, kl, kr, K.ARITH_OPS, n)
    _cmp_case(gpu_ctx, kl, kr, K.CMP_OPS, n)


@pytest.mark.parametrize("side", ["lit_right", "lit_left"])
@pytest.mark.parametrize("kind", K.KINDS)
def test_arith_literals(gpu_ctx, kind, side):
    """Int and fp64 literals on either side, NaN / -0.0 / +-Inf, the int64 extremes, and a null
    literal of each type (all-null; FLOAT64 output for a null FLOAT64 literal)."""
    n = K.MATRIX_N
    for lit in K.LITERALS:
        a, av = K.column_around(kind, lit, n)
        for nulls in (True, False):
            lv = av if nulls else None
            A = dcol(gpu_ctx, kind, a, lv)
            for op in K.ARITH_OPS:
                if side == "lit_right":
                    r, v = S.arith(op, a, lv, K.ref_operand(lit), None)
                    lhs, rhs = A, lit
                else:
                    r, v = S.arith(op, K.ref_operand(lit), None, a, lv)
                    lhs, rhs = lit, A
                if lit.value is None:
                    assert not v.any() and (r.dtype == np.float64) == (lit.is_f64 or kind == "f64")
                need = nulls or lit.value is None or (r.dtype != np.float64 and op == S.OP_DIV)
                run_arith(gpu_ctx, op, lhs, rhs, r, v, n, need)


@pytest.mark.parametrize("side", ["lit_right", "lit_left"])
@pytest.mark.parametrize("kind", K.KINDS)
def test_cmp_literals(gpu_ctx, kind, side):
    n = K.MATRIX_N
    for lit in K.LITERALS:
        a, av = K.column_around(kind, lit, n)
        for nulls in (True, False):
            lv = av if nulls else None
            A = dcol(gpu_ctx, kind, a, lv)
            for op in K.CMP_OPS:
                if side == "lit_right":
                    r, v = S.cmp(op, a, lv, K.ref_operand(lit), None)
                    lhs, rhs = A, lit
                else:
                    r, v = S.cmp(op, K.ref_operand(lit), None, a, lv)
                    lhs, rhs = lit, A
                if lit.value is None:
                    assert not v.any()
                run_cmp(gpu_ctx, op, lhs, rhs, r, v, n, nulls or lit.value is None)


@pytest.mark.parametrize("order", ["int_fp", "fp_int"])
def test_cmp_int64_against_fp64_beyond_2_53(gpu_ctx, order):
    """Mixed comparison is done in fp64 (header): 2^53 + 1 = float(2^53), INT64_MAX = 2^63."""
    n = K.MATRIX_N
    i, d = K.mixed_precision_pairs(n)
    I, D = dcol(gpu_ctx, "i64", i), dcol(gpu_ctx, "f64", d)
    for op in K.CMP_OPS:
        if order == "int_fp":
            r, v = S.cmp(op, i, None, d, None)
            run_cmp(gpu_ctx, op, I, D, r, v, n, False)
        else:
            r, v = S.cmp(op, d, None, i, None)
            run_cmp(gpu_ctx, op, D, I, r, v, n, False)


def test_expression_refusals(gpu_ctx):
    """Argument checks that return before any launch."""
    ctx, n = gpu_ctx, 40
    rng = K.rng_for("refusals")
    a = dcol(ctx, "i64", K.column("i64", n, rng))
    an = dcol(ctx, "i64", K.column("i64", n, rng), K.validity(n, rng))
    f = dcol(ctx, "f64", K.column("f64", n, rng))
    short = dcol(ctx, "i64", K.column("i64", n - 1, rng))
    flag = bcol(ctx, rng.random(n) < 0.5)
    s = scol_of(ctx, K.utf8_values(b"CA", n))
    s_plain = scol_of(ctx, [b"CA"] * n, with_validity=False)
    one, two = scol_of(ctx, [b"CA"], with_validity=False), scol_of(ctx, [b"CA", b"NY"], with_validity=False)
    i64 = lambda rows=n, nullable=True: out_col(ctx, N.TYPE_INT64, rows, nullable)  # noqa: E731
    boo = lambda rows=n, nullable=True: out_col(ctx, N.TYPE_BOOL, rows, nullable)  # noqa: E731
    seven = K.Lit(7, False)
    arith = lambda *x: call2(ctx, "qe_eval_arith", *x)  # noqa: E731
    cmp_ = lambda *x: call2(ctx, "qe_eval_cmp", *x)  # noqa: E731
    # the wrong op family
    assert arith(S.OP_EQ, a, a, i64()) == N.QE_ERR_INVALID_ARG
    assert cmp_(S.OP_ADD, a, a, boo()) == N.QE_ERR_INVALID_ARG
    assert call_bool(ctx, S.OP_ADD, flag, flag, boo()) == N.QE_ERR_INVALID_ARG
    assert arith(S.OP_AND, a, a, i64()) == N.QE_ERR_INVALID_ARG
    # both operands literal
    assert arith(S.OP_ADD, seven, seven, i64()) == N.QE_ERR_INVALID_ARG
    assert cmp_(S.OP_EQ, seven, seven, boo()) == N.QE_ERR_INVALID_ARG
    # BOOL / UTF8 operands to K1
    assert arith(S.OP_ADD, flag, a, i64()) == N.QE_ERR_UNSUPPORTED
    assert arith(S.OP_ADD, a, s_plain, i64()) == N.QE_ERR_UNSUPPORTED
    # unequal lengths
    assert arith(S.OP_ADD, a, short, i64()) == N.QE_ERR_INVALID_ARG
    assert cmp_(S.OP_LT, short, a, boo()) == N.QE_ERR_INVALID_ARG
    # an output of the wrong type
    assert arith(S.OP_ADD, a, f, i64()) == N.QE_ERR_INVALID_ARG
    assert arith(S.OP_ADD, a, a, out_col(ctx, N.TYPE_FLOAT64, n, True)) == N.QE_ERR_INVALID_ARG
    assert cmp_(S.OP_LT, a, a, i64()) == N.QE_ERR_INVALID_ARG
    # too small an output
    assert arith(S.OP_ADD, a, a, i64(n - 1)) == N.QE_ERR_CAPACITY
    assert cmp_(S.OP_LT, a, seven, boo(n - 1)) == N.QE_ERR_CAPACITY
    assert call_bool(ctx, S.OP_NOT, flag, None, boo(n - 9)) == N.QE_ERR_CAPACITY
    # a result that can be null without an output validity buffer
    assert arith(S.OP_ADD, a, an, i64(n, False)) == N.QE_ERR_INVALID_ARG  # only the right side is nullable
    assert cmp_(S.OP_LT, a, an, boo(n, False)) == N.QE_ERR_INVALID_ARG
    assert arith(S.OP_DIV, a, seven, i64(n, False)) == N.QE_ERR_INVALID_ARG  # x / 0
    assert arith(S.OP_ADD, a, K.Lit(None, False), i64(n, False)) == N.QE_ERR_INVALID_ARG
    assert cmp_(S.OP_EQ, s, one, boo(n, False)) == N.QE_ERR_INVALID_ARG
    # UTF-8: only = and !=, a one-row literal column, on the right
    assert cmp_(S.OP_LT, s, one, boo()) == N.QE_ERR_UNSUPPORTED
    assert cmp_(S.OP_EQ, s, two, boo()) == N.QE_ERR_UNSUPPORTED
    assert cmp_(S.OP_EQ, one, s, boo()) == N.QE_ERR_UNSUPPORTED
    assert cmp_(S.OP_EQ, s, seven, boo()) == N.QE_ERR_UNSUPPORTED
    # and the same arguments put right run
    assert arith(S.OP_ADD, a, an, i64()) == N.QE_OK and cmp_(S.OP_EQ, s, one, boo()) == N.QE_OK


# ---- K2 on UTF-8 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.UTF8_SIZES)
@pytest.mark.parametrize("name", list(K.UTF8_LITERALS))
def test_cmp_utf8(gpu_ctx, name, n):
    lit = K.UTF8_LITERALS[name]
    vals = K.utf8_values(lit, n)
    litc = scol_of(gpu_ctx, [lit], with_validity=False)
    filled = [lit if v is None else v for v in vals]  # the form without validity: equal where a null was
    for values, nullable in ((vals, True), (filled, False)):
        col = scol_of(gpu_ctx, values, null_bytes=lit or b"x", with_validity=nullable)
        for op in (S.OP_EQ, S.OP_NE):
            r, v = S.cmp_utf8(op, values, lit)
            run_cmp(gpu_ctx, op, col, litc, r, v, n, nullable)


@pytest.mark.parametrize("n", [0] + K.UTF8_SIZES)
def test_cmp_utf8_null_literal_is_all_null(gpu_ctx, n):
    """A one-row UTF8 literal whose validity bit is clear is null, whatever bytes it spans: every
    row of the result is null (as with a null numeric literal), not a comparison with ""."""
    vals = K.utf8_values(b"", n)
    null_lit = scol_of(gpu_ctx, [None], null_bytes=b"CA")
    for with_validity in (True, False):
        col = scol_of(gpu_ctx, [b"" if v is None else v for v in vals] if not with_validity else vals,
                      with_validity=with_validity)
        for op in (S.OP_EQ, S.OP_NE):
            r, v = S.cmp_utf8(op, vals, None)
            assert not v.any()
            run_cmp(gpu_ctx, op, col, null_lit, r, v, n, True)
            assert call2(gpu_ctx, "qe_eval_cmp", op, col, null_lit,
                         out_col(gpu_ctx, N.TYPE_BOOL, n, False)) == N.QE_ERR_INVALID_ARG
    # a literal column WITH a validity buffer whose bit is set compares as usual
    valid_lit = scol(gpu_ctx, np.array([0, 0], dtype=np.int32), np.zeros(1, dtype=np.uint8), np.array([True]))
    col = scol_of(gpu_ctx, vals)
    r, v = S.cmp_utf8(S.OP_EQ, vals, b"")
    run_cmp(gpu_ctx, S.OP_EQ, col, valid_lit, r, v, n, True)


# ---- the second trip of the grid-stride loops ------------------------------------------------------------
@pytest.fixture(scope="module")
def big_n():
    """One row more than a grid of num_cus * 8 blocks x 256 threads x 8 rows covers in one trip, plus
    a whole block and a tail."""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 * 8 + 2048 + 5


def test_grid_stride_int64_add(gpu_ctx, big_n):
    rng = K.rng_for("gs-add")
    a = rng.integers(K.I64_MIN, K.I64_MAX, big_n, dtype=np.int64, endpoint=True)
    b = rng.integers(K.I64_MIN, K.I64_MAX, big_n, dtype=np.int64, endpoint=True)
    bv = rng.random(big_n) > 0.1
    r, v = S.arith(S.OP_ADD, a, None, b, bv)
    run_arith(gpu_ctx, S.OP_ADD, dcol(gpu_ctx, "i64", a), dcol(gpu_ctx, "i64", b, bv), r, v, big_n, True)


def test_grid_stride_i32_gt_literal(gpu_ctx, big_n):
    a, av = K.column_around("i32", K.Lit(-5, False), big_n)
    r, v = S.cmp(S.OP_GT, a, av, -5, None)
    run_cmp(gpu_ctx, S.OP_GT, dcol(gpu_ctx, "i32", a, av), K.Lit(-5, False), r, v, big_n, True)


def test_grid_stride_f64_mul_device_length(gpu_ctx, big_n):
    """qe_eval_arith_dlen with a device count below n, beyond one trip of the grid and no multiple of
    8: rows below it are computed, the last validity byte is cut at it, rows from it on are left."""
    import torch

    dn = big_n - 11
    assert dn % 8 and dn > big_n - 2048 - 5
    rng = K.rng_for("gs-mul")
    a = K.column("f64", big_n, rng)
    av = rng.random(big_n) > 0.1
    lit = K.Lit(1.0000000000000002, True)
    r, v = S.arith(S.OP_MUL, a, av, lit.value, None)
    out = out_col(gpu_ctx, N.TYPE_FLOAT64, big_n, True)
    cnt = torch.tensor([dn], dtype=torch.int64, device=gpu_ctx.torch_device)
    assert call2(gpu_ctx, "qe_eval_arith_dlen", S.OP_MUL, dcol(gpu_ctx, "f64", a, av), lit, out, cnt) == N.QE_OK
    check_values(out, dn, r, v, True)
    assert (out.values[dn:big_n].cpu().numpy() == SENTINEL_F).all()


def test_grid_stride_bool_and_is_null(gpu_ctx, big_n):
    rng = K.rng_for("gs-bool")
    a, b = rng.random(big_n) < 0.5, rng.random(big_n) < 0.5
    av, bv = rng.random(big_n) < 0.7, rng.random(big_n) < 0.7
    A, B = bcol(gpu_ctx, a, av), bcol(gpu_ctx, b, bv)
    for op, rhs, nullable in ((S.OP_AND, B, True), (S.OP_IS_NULL, None, False)):
        r, v = S.bool3(op, a, av, b, bv)
        out = out_col(gpu_ctx, N.TYPE_BOOL, big_n, nullable)
        assert call_bool(gpu_ctx, op, A, rhs, out) == N.QE_OK
        check_bits(out, big_n, r, v, nullable)


def test_grid_stride_utf8_eq(gpu_ctx, big_n):
    rng = K.rng_for("gs-utf8")
    pool = [b"CA", b"C", b"CAX", b"", b"NY", b"CB"]
    idx = rng.integers(0, len(pool), big_n)
    offs, data = K.utf8_from_pool(pool, idx)
    valid = rng.random(big_n) > 0.1
    col = scol(gpu_ctx, offs, data, valid)
    r = (idx == 0) & valid
    run_cmp(gpu_ctx, S.OP_EQ, col, scol_of(gpu_ctx, [b"CA"], with_validity=False), r, valid, big_n, True)


# ---- K3a ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.BOOL_SIZES)
@pytest.mark.parametrize("op", K.BOOL_OPS, ids=["AND", "OR", "NOT", "IS_NULL", "IS_NOT_NULL"])
def test_bool3(gpu_ctx, op, n):
    """Every op with validity on both sides, on one, on neither (the `avalid ? ... : 0xFF` arms); the
    unary ops with rhs = NULL. The value bit under a null operand is random."""
    binary = op in (S.OP_AND, S.OP_OR)
    for ln, rn in K.NULL_COMBOS:
        a, av, b, bv = K.bool_pair(n, ln, rn)
        A, B = bcol(gpu_ctx, a, av), bcol(gpu_ctx, b, bv)
        r, v = S.bool3(op, a, av, b, bv)
        need = (ln or (binary and rn)) and op not in (S.OP_IS_NULL, S.OP_IS_NOT_NULL)
        for nullable in ([True] if need else [False, True]):
            out = out_col(gpu_ctx, N.TYPE_BOOL, n, nullable)
            assert call_bool(gpu_ctx, op, A, B if binary else None, out) == N.QE_OK
            check_bits(out, n, r, v, nullable)


@pytest.mark.parametrize("n", K.BOOL_SIZES)
@pytest.mark.parametrize("kind", ["i64", "f64", "i32", "u8", "utf8"])
def test_null_tests_on_typed_columns(gpu_ctx, kind, n):
    """IS_NULL / IS_NOT_NULL read only the validity: any column type, with and without one."""
    rng = K.rng_for("isnull", kind, n)
    valid = K.validity(n, rng, 0.4)
    for with_validity in (True, False):
        vv = valid if with_validity else None
        if kind == "utf8":
            offs, data, _ = K.utf8_arrays(K.utf8_values(b"CA", n), b"zz")
            col = scol(gpu_ctx, offs, data, vv)
        else:
            col = dcol(gpu_ctx, kind, K.column(kind, n, rng), vv)
        for op in (S.OP_IS_NULL, S.OP_IS_NOT_NULL):
            r, v = S.bool3(op, np.zeros(n, dtype=bool), vv)
            for nullable in (False, True):
                out = out_col(gpu_ctx, N.TYPE_BOOL, n, nullable)
                assert call_bool(gpu_ctx, op, col, None, out) == N.QE_OK
                check_bits(out, n, r, v, nullable)
    flag = dcol(gpu_ctx, "i64", K.column("i64", n, rng))
    assert call_bool(gpu_ctx, S.OP_NOT, flag, None, out_col(gpu_ctx, N.TYPE_BOOL, n, True)) == N.QE_ERR_UNSUPPORTED


# ---- K3b: masks built tile by tile ---------------------------------------------------------------------------
MASK_FORMS = ["nullable", "plain", "raw_padded"]


def _mask(ctx, name, form):
    counts, tail, tail_sel = K.TILE_VECTORS[name]
    m, mv = K.mask_with_tile_counts(counts, tail, 0, tail_sel, form == "nullable")
    # raw_padded: the bytes as a producer may leave them, every padding bit of the last byte set
    return m, mv, bcol(ctx, m, mv, dirty=form != "plain")


def _filter_count(ctx, mask):
    cnt, mc = N.C.c_int64(-1), mask.as_c()
    assert N.lib().qe_filter_count(ctx.handle, N.C.byref(mc), N.C.byref(cnt)) == N.QE_OK
    return cnt.value


def _check_fixed(out, rows, kind, values, valid, sel):
    want_v = valid[sel] if valid is not None else np.ones(int(sel.sum()), dtype=bool)
    if valid is not None:
        check_validity(out, rows, want_v)
    got, want = out.values[:rows].cpu().numpy(), values[sel][:rows]
    keep = want_v[:rows]
    if kind == "f64":
        assert np.array_equal(got[keep].view(np.int64), want[keep].view(np.int64))  # a copy: NaN bits too
    else:
        assert np.array_equal(got[keep], want[keep])
    if valid is None:
        assert got.tobytes() == want.tobytes()


def _check_utf8(out, rows, offs, data, valid, sel):
    want_v = valid[sel] if valid is not None else np.ones(rows, dtype=bool)
    if valid is not None:
        check_validity(out, rows, want_v)
    go = out.offsets[:rows + 1].cpu().numpy().astype(np.int64)
    assert go[0] == 0 and (np.diff(go) >= 0).all() and go[-1] <= out.values.numel()
    gb = out.values.cpu().numpy().tobytes()
    src = data.tobytes()
    for k, i in enumerate(np.nonzero(sel)[0]):
        if want_v[k]:
            assert gb[go[k]:go[k + 1]] == src[offs[i]:offs[i + 1]], (k, i)


@pytest.mark.parametrize("form", MASK_FORMS)
@pytest.mark.parametrize("name", list(K.TILE_VECTORS))
def test_filter_tiles(gpu_ctx, name, form):
    """Each count vector against qe_filter_count, qe_filter_apply (8 columns in one call: five nullable
    fixed-width ones and three UTF-8, outputs sized for exactly the selected rows) and
    qe_filter_apply_async (8 fixed-width columns; nothing is asserted at or beyond the count)."""
    import torch

    ctx = gpu_ctx
    m, mv, mask = _mask(ctx, name, form)
    sel = S.select_mask(m, mv)
    n, total = len(m), int(sel.sum())
    assert _filter_count(ctx, mask) == total
    fixed, utf8 = K.filter_inputs(sel)
    mc = mask.as_c()
    # synchronous: nullable fixed-width and the UTF-8 columns, which share the pairs / tsum scratch
    names = [nm for nm, (_, _, vd) in fixed.items() if vd is not None] + list(utf8)
    ins, outs = [], []
    for nm in names:
        if nm in fixed:
            kind, values, valid = fixed[nm]
            ins.append(dcol(ctx, kind, values, valid))
            outs.append(out_col(ctx, TYPE[kind], total, True))
        else:
            offs, data, valid, _ = utf8[nm]
            ins.append(scol(ctx, offs, data, valid))
            outs.append(out_utf8(ctx, total, len(data), valid is not None))
    assert len(ins) == N.MAX_COLS
    ic = (N.QeColumn * len(ins))(*[c.as_c() for c in ins])
    oc = (N.QeColumn * len(outs))(*[o.as_c() for o in outs])
    got = N.C.c_int64(-1)
    assert N.lib().qe_filter_apply(ctx.handle, N.C.byref(mc), ic, len(ins), oc, N.C.byref(got)) == N.QE_OK, \
        N.lib().qe_last_error()
    ctx.synchronize()
    assert got.value == total and all(oc[k].length == total for k in range(len(ins)))
    for nm, out in zip(names, outs):
        if nm in fixed:
            _check_fixed(out, total, *fixed[nm], sel)
        else:
            _check_utf8(out, total, *utf8[nm][:3], sel)
    # stream-ordered: the 8 fixed-width columns, outputs sized by the mask
    ins = [dcol(ctx, kind, values, valid) for kind, values, valid in fixed.values()]
    outs = [out_col(ctx, TYPE[kind], n, valid is not None) for kind, _, valid in fixed.values()]
    ic = (N.QeColumn * len(ins))(*[c.as_c() for c in ins])
    oc = (N.QeColumn * len(outs))(*[o.as_c() for o in outs])
    cnt = torch.full((1,), -1, dtype=torch.int64, device=ctx.torch_device)
    assert N.lib().qe_filter_apply_async(ctx.handle, N.C.byref(mc), ic, len(ins), oc,
                                         N.C.c_void_p(cnt.data_ptr())) == N.QE_OK, N.lib().qe_last_error()
    ctx.synchronize()
    assert int(cnt.cpu().item()) == total
    for (kind, values, valid), out in zip(fixed.values(), outs):
        if valid is not None and total:  # the bits below the count (the last byte's other bits: unspecified)
            gv = np.unpackbits(raw(out.validity, (total + 7) // 8), bitorder="little")[:total].astype(bool)
            assert np.array_equal(gv, valid[sel])
        _check_fixed_rows(out, total, kind, values, valid, sel)


def _check_fixed_rows(out, rows, kind, values, valid, sel):
    got, want = out.values[:rows].cpu().numpy(), values[sel]
    keep = valid[sel] if valid is not None else np.ones(rows, dtype=bool)
    assert got[keep].tobytes() == want[keep].tobytes()


@pytest.mark.parametrize("form", MASK_FORMS)
@pytest.mark.parametrize("name", list(K.TILE_VECTORS))
def test_filter_batch_of_11_columns(gpu_ctx, name, form):
    """filter_batch over fixed-width and UTF-8 columns together: more than 8, so in two calls."""
    from kquery.operators import filter_batch

    ctx = gpu_ctx
    m, mv, mask = _mask(ctx, name, form)
    sel = S.select_mask(m, mv)
    total = int(sel.sum())
    fixed, utf8 = K.filter_inputs(sel)
    order = ["i64n", "s0n", "f64n", "i32n", "s2", "d32n", "u8n", "i64", "s1n", "i32", "u8"]
    cols = [dcol(ctx, *fixed[nm]) if nm in fixed else scol(ctx, *utf8[nm][:3]) for nm in order]
    out = filter_batch(RecordBatch(Schema([]), cols), mask)
    assert len(out.fields) == 11 and out.rowCount() == total
    for nm, col in zip(order, out.fields):
        assert col.length == total
        if nm in fixed:
            _check_fixed(col, total, *fixed[nm], sel)
        else:
            _check_utf8(col, total, *utf8[nm][:3], sel)


def test_filter_refusals(gpu_ctx):
    import torch

    ctx = gpu_ctx
    m, mv, mask = _mask(ctx, "aligned", "nullable")
    n, total = len(m), int(S.select_mask(m, mv).sum())
    rng = K.rng_for("filter-refusals")
    v, vv = K.column("i64", n, rng), K.validity(n, rng)
    mc = mask.as_c()
    cnt = torch.zeros(1, dtype=torch.int64, device=ctx.torch_device)

    def both(ins, outs):
        ic = (N.QeColumn * len(ins))(*[c.as_c() for c in ins])
        oc = [(N.QeColumn * len(outs))(*[o.as_c() for o in outs]) for _ in range(2)]  # (a call sets the lengths)
        return (N.lib().qe_filter_apply(ctx.handle, N.C.byref(mc), ic, len(ins), oc[0], None),
                N.lib().qe_filter_apply_async(ctx.handle, N.C.byref(mc), ic, len(ins), oc[1], N.C.c_void_p(cnt.data_ptr())))

    plain, nullable = dcol(ctx, "i64", v), dcol(ctx, "i64", v, vv)
    out = lambda rows=n, nl=True: out_col(ctx, N.TYPE_INT64, rows, nl)  # noqa: E731
    assert both([plain] * 9, [out() for _ in range(9)]) == (N.QE_ERR_UNSUPPORTED, N.QE_ERR_UNSUPPORTED)
    flag = bcol(ctx, m)  # a BOOL column cannot be gathered
    assert both([flag], [out_col(ctx, N.TYPE_BOOL, n, False)]) == (N.QE_ERR_UNSUPPORTED, N.QE_ERR_UNSUPPORTED)
    assert both([nullable], [out(n, False)]) == (N.QE_ERR_INVALID_ARG, N.QE_ERR_INVALID_ARG)
    assert both([plain], [out(total - 1, False)]) == (N.QE_ERR_CAPACITY, N.QE_ERR_CAPACITY)
    assert both([plain], [out(n - 1, False)])[1] == N.QE_ERR_CAPACITY  # the async form needs the mask's rows
    assert both([plain], [out_col(ctx, N.TYPE_FLOAT64, n, False)]) == (N.QE_ERR_INVALID_ARG, N.QE_ERR_INVALID_ARG)
    assert both([dcol(ctx, "i64", v[:-1])], [out()]) == (N.QE_ERR_INVALID_ARG, N.QE_ERR_INVALID_ARG)
    assert both([plain, nullable], [out(), out()]) == (N.QE_OK, N.QE_OK)
    ctx.synchronize()


# ---- a composed predicate through the operator classes -----------------------------------------------------
def test_composed_predicate(gpu_ctx):
    """((a > k) AND NOT (s = 'CA')) OR (c IS NULL) through SelectionExec: K2's bits under null rows go
    through K3a into K3b, against a row-at-a-time three-valued evaluation."""
    from kquery.datasource import InMemoryDataSource
    from kquery.expressions import (AndExpression, ColumnExpression, EqExpression, GtExpression, IsNullExpression,
                                    LiteralLongExpression, LiteralStringExpression, NotExpression, OrExpression)
    from kquery.operators import ScanExec, SelectionExec

    ctx = gpu_ctx
    b = K.predicate_batch()
    keep = K.predicate_rows(b)
    s_arr, p_arr = K.utf8_arrays(b["s"], b"CA"), K.utf8_arrays(b["pay_s"])
    cols = [dcol(ctx, "i32", b["a"], b["av"]), scol(ctx, *s_arr), dcol(ctx, "f64", b["c"], b["cv"]),
            dcol(ctx, "i64", b["pay_i"]), scol(ctx, p_arr[0], p_arr[1])]
    names = ["a", "s", "c", "pay_i", "pay_s"]
    schema = Schema([Field(nm, c.type) for nm, c in zip(names, cols)])
    scan = ScanExec(InMemoryDataSource(schema, [RecordBatch(schema, cols)]), names)
    pred = OrExpression(
        AndExpression(GtExpression(ColumnExpression(0), LiteralLongExpression(K.PREDICATE_K)),
                      NotExpression(EqExpression(ColumnExpression(1), LiteralStringExpression("CA")))),
        IsNullExpression(ColumnExpression(2)))
    out = list(SelectionExec(scan, pred).execute())
    assert len(out) == 1
    out = out[0]
    total = int(keep.sum())
    assert out.rowCount() == total
    _check_fixed(out.field(0), total, "i32", b["a"], b["av"], keep)
    _check_utf8(out.field(1), total, *s_arr, keep)
    _check_fixed(out.field(2), total, "f64", b["c"], b["cv"], keep)
    _check_fixed(out.field(3), total, "i64", b["pay_i"], None, keep)
    _check_utf8(out.field(4), total, p_arr[0], p_arr[1], None, keep)
