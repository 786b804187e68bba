"""CPU side of tests/test_expr_ops.py: the oracle's additions (null literals, byte strings) against
literal row loops, and the conditions every data set of exprcases.py must meet for its GPU test to
mean something. Nothing here touches the device; every assertion is on the references alone."""
import itertools
import math

import numpy as np
import pytest

import exprcases as K
from oracle import semantics as S

PAIRS = list(itertools.product(K.KINDS, K.KINDS))


def _same(got, want, f64):
    (r, v), (wr, wv) = got, want
    assert np.array_equal(v, wv)
    if f64:
        assert r.dtype == np.float64 and K.same_f64(r[v], wr[wv])
    else:
        assert r.dtype != np.float64 and np.array_equal(r[v], wr[wv])


def _row_arith(op, a, av, b, bv, n):
    f = K.is_f64(a) or K.is_f64(b)
    rows = [K.row_arith(op, x, y, f) for x, y in zip(K.rows_of(a, av, n), K.rows_of(b, bv, n))]
    return K.rows_result(rows, np.float64 if f else np.int64), f


def _row_cmp(op, a, av, b, bv, n):
    f = K.is_f64(a) or K.is_f64(b)
    rows = [K.row_cmp(op, x, y, f) for x, y in zip(K.rows_of(a, av, n), K.rows_of(b, bv, n))]
    return K.rows_result(rows, bool)


# ---- the oracle against the row loops ---------------------------------------------------------------
@pytest.mark.parametrize("kl,kr", PAIRS)
def test_oracle_arith_equals_row_loop(kl, kr):
    """Every ordered pair of kinds, narrow ones widened by value, at a size with a tail."""
    n = 57
    a, av, b, bv = K.arith_pair(kl, kr, n)
    for op in K.ARITH_OPS:
        want, f = _row_arith(op, a, av, b, bv, n)
        _same(S.arith(op, a, av, b, bv), want, f)


@pytest.mark.parametrize("kl,kr", PAIRS)
def test_oracle_cmp_equals_row_loop(kl, kr):
    n = 203
    a, av, b, bv = K.cmp_pair(kl, kr, n)
    for op in K.CMP_OPS:
        r, v = S.cmp(op, a, av, b, bv)
        wr, wv = _row_cmp(op, a, av, b, bv, n)
        assert np.array_equal(v, wv) and np.array_equal(r, wr & wv)


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("lit", K.LITERALS, ids=repr)
def test_oracle_literals_equal_row_loop(kind, lit):
    """Literals on either side: int against fp64 (the conversion), the int64 extremes, NaN, -0.0,
    +-Inf, and the null literal of each type (all-null; a null FLOAT64 literal makes the result fp64)."""
    n = 41
    a, av = K.column_around(kind, lit, n)
    for lhs, lv, rhs, rv in ((a, av, lit, None), (lit, None, a, av)):
        for op in K.ARITH_OPS:
            want, f = _row_arith(op, lhs, lv, rhs, rv, n)
            got = S.arith(op, K.ref_operand(lhs), lv, K.ref_operand(rhs), rv)
            _same(got, want, f)
            if lit.value is None:
                assert not got[1].any() and (got[0].dtype == np.float64) == (lit.is_f64 or kind == "f64")
        for op in K.CMP_OPS:
            r, v = S.cmp(op, K.ref_operand(lhs), lv, K.ref_operand(rhs), rv)
            wr, wv = _row_cmp(op, lhs, lv, rhs, rv, n)
            assert np.array_equal(v, wv) and np.array_equal(r, wr & wv)
            if lit.value is None:
                assert not v.any() and not r.any()


def test_oracle_cmp_utf8_bytes_and_null_literal():
    for lit in K.UTF8_LITERALS.values():
        vals = K.utf8_values(lit, 100)
        for op in (S.OP_EQ, S.OP_NE):
            for given in (lit, None):
                r, v = S.cmp_utf8(op, vals, given)
                rows = [K.row_cmp_utf8(op, x, given) for x in vals]
                wr, wv = K.rows_result(rows, bool)
                assert np.array_equal(v, wv) and np.array_equal(r, wr & wv)
                if given is None:
                    assert not v.any()
    # str input still works, and equals its encoded form
    r1, v1 = S.cmp_utf8(S.OP_EQ, ["Pärsson", None, "P"], "Pärsson")
    r2, v2 = S.cmp_utf8(S.OP_EQ, ["Pärsson".encode(), None, b"P"], "Pärsson".encode())
    assert r1.tolist() == r2.tolist() == [True, False, False] and v1.tolist() == v2.tolist()


def test_oracle_bool3_equals_row_loop():
    for ln, rn in K.NULL_COMBOS:
        a, av, b, bv = K.bool_pair(100, ln, rn)
        xs = [None if (av is not None and not av[i]) else bool(a[i]) for i in range(100)]
        ys = [None if (bv is not None and not bv[i]) else bool(b[i]) for i in range(100)]
        for op in K.BOOL_OPS:
            r, v = S.bool3(op, a, av, b, bv)
            wr, wv = K.rows_result([K.row_bool(op, x, y) for x, y in zip(xs, ys)], bool)
            assert np.array_equal(v, wv) and np.array_equal(r & v, wr & wv)


def test_row_references_by_hand():
    assert K.row_arith(S.OP_DIV, -7, 2, False) == -3 and K.row_arith(S.OP_DIV, 7, -2, False) == -3
    assert K.row_arith(S.OP_DIV, K.I64_MIN, -1, False) == K.I64_MIN and K.row_arith(S.OP_DIV, 5, 0, False) is None
    assert K.row_arith(S.OP_ADD, K.I64_MAX, 1, False) == K.I64_MIN
    assert K.row_arith(S.OP_MUL, K.I32_MIN, K.I32_MIN, False) == 1 << 62
    assert K.row_arith(S.OP_ADD, 255, K.I32_MIN, False) == K.I32_MIN + 255
    assert K.row_cmp(S.OP_EQ, (1 << 53) + 1, float(1 << 53), True) is True  # compares as fp64
    assert K.row_cmp(S.OP_LT, K.I64_MAX, 2.0 ** 63, True) is False
    assert K.row_cmp(S.OP_LT, K.I64_MIN, K.I64_MAX, False) is True
    assert K.row_cmp(S.OP_NE, math.nan, math.nan, True) is True and K.row_cmp(S.OP_EQ, 0.0, -0.0, True) is True
    assert K.row_bool(S.OP_AND, False, None) is False and K.row_bool(S.OP_AND, True, None) is None
    assert K.row_bool(S.OP_OR, None, True) is True and K.row_bool(S.OP_OR, None, False) is None
    assert K.row_bool(S.OP_NOT, None) is None and K.row_bool(S.OP_IS_NULL, None) is True


# ---- conditions on the data sets ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("n", [s for s in K.SIZES if s >= 2047])
def test_columns_hold_their_edges(kind, n):
    """With these values a missing sign extension (INT32) or a wrong zero extension (UINT8) changes
    the result; they sit in vector groups and, TAIL_EDGE, in the last row."""
    v = K.column(kind, n, K.rng_for("edges", kind, n))
    for e in K.EDGES[kind][:4]:
        assert (np.isnan(v).any() if isinstance(e, float) and math.isnan(e) else (v == e).any()), e
    full = v[: n - n % 8]
    if kind in ("i32", "d32"):
        assert (full < 0).any() and (full == K.I32_MIN).any() and (full == K.I32_MAX).any()
    if kind == "u8":
        assert (full >= 128).any() and (full == 255).any()
    if n % 8:
        assert v[n - 1] == K.TAIL_EDGE[kind]
        assert kind in ("f64",) or kind == "u8" or v[n - 1] < 0


@pytest.mark.parametrize("kl,kr,n", [(kl, kr, n) for kl, kr in PAIRS if "f64" not in (kl, kr)
                                      for n in K.SIZES if n >= 9 and (n == K.MATRIX_N or (kl, kr) in K.SIZE_PAIRS)])
def test_div_data_sets(kl, kr, n):
    """From 9 rows on every integer DIV data set has, as valid rows: x / 0; MIN / -1 where both kinds
    are signed (UINT8 holds neither); a quotient that truncates toward zero, negative wherever a
    side is signed (UINT8 / UINT8 has no negative quotient: an inexact positive one)."""
    a, av, b, bv = K.arith_pair(kl, kr, n)
    x, y = a.astype(object), b.astype(object)
    ok = av & bv
    assert (ok & (b == 0)).any()
    if kl in K.SIGNED and kr in K.SIGNED:
        assert (ok & (a == K.RANGE[kl][0]) & (b == -1)).any()
    nz = ok & (b != 0)
    inexact = np.array([bool(nz[i]) and x[i] % y[i] != 0 for i in range(n)])
    negative = np.array([bool(nz[i]) and (x[i] < 0) != (y[i] < 0) and x[i] != 0 for i in range(n)])
    assert (inexact & negative).any() if (kl in K.SIGNED or kr in K.SIGNED) else inexact.any()
    r, v = S.arith(S.OP_DIV, a, av, b, bv)
    assert not v[ok & (b == 0)].any() and v[nz].all()
    if n >= 16:  # the same rows again in the tail group
        tail = np.arange(n) >= n - 8
        assert (ok & (b == 0) & tail).any() and (inexact & tail).any()


@pytest.mark.parametrize("kl,kr", PAIRS)
def test_cmp_data_sets_yield_every_outcome(kl, kr):
    for n in ([K.MATRIX_N] if (kl, kr) not in K.SIZE_PAIRS else [s for s in K.SIZES if s >= 2047]):
        a, av, b, bv = K.cmp_pair(kl, kr, n)
        for nulls in K.NULL_COMBOS:
            shares = K.outcome_shares(a, av if nulls[0] else None, b, bv if nulls[1] else None)
            assert min(shares) >= 0.2, (n, nulls, shares)


def test_int64_cmp_data_set():
    a, av, b, bv = K.int64_cmp_pair(K.MATRIX_N)
    n = len(a)
    assert (a == b).sum() >= 0.2 * n and (np.abs(a.astype(object) - b.astype(object)) == 1).sum() >= 0.2 * n
    assert ((a < 0) != (b < 0)).sum() >= 0.3 * n
    both = av & bv
    assert (both & (a == K.I64_MIN) & (b == K.I64_MAX)).any() and (both & (a == K.I64_MAX) & (b == K.I64_MIN)).any()
    # an unsigned compare, or one through fp64, differs from the signed one on valid rows
    lt = S.cmp(S.OP_LT, a, None, b, None)[0]
    assert ((a.view(np.uint64) < b.view(np.uint64)) != lt)[both].sum() >= 0.2 * n
    assert ((a.astype(np.float64) < b.astype(np.float64)) != lt)[both].any()
    assert min(K.outcome_shares(a, av, b, bv)) >= 0.2


@pytest.mark.parametrize("kind", K.KINDS)
@pytest.mark.parametrize("lit", K.LITERALS, ids=repr)
def test_literal_data_sets(kind, lit):
    """Where the column's kind can sit below, on and above the literal, it does, on 20 % of the valid
    rows each, from either side. The other literals (NaN, +-Inf, the int64 extremes, a fraction against
    an integer column, null) cannot give all three; what they give is the row loop's (above)."""
    a, av = K.column_around(kind, lit, K.MATRIX_N)
    if K.literal_admits_all(kind, lit):
        assert min(K.outcome_shares(a, av, K.ref_operand(lit), None)) >= 0.2
        assert min(K.outcome_shares(K.ref_operand(lit), None, a, av)) >= 0.2
    elif lit.value is not None and not (isinstance(lit.value, float) and math.isnan(lit.value)):
        assert max(K.outcome_shares(a, av, K.ref_operand(lit), None)) >= 0.2


def test_mixed_precision_pairs():
    """int64 against fp64 beyond 2^53: exact comparison and comparison as fp64 disagree here, and the
    header pins the latter."""
    i, d = K.mixed_precision_pairs(K.MATRIX_N)
    assert min(K.outcome_shares(i, None, d, None)) >= 0.2 and np.isnan(d).any()
    assert {(1 << 53) + k for k in range(-2, 3)} <= set(i.tolist()) and {-(1 << 53) - k for k in range(-2, 3)} <= set(i.tolist())
    assert {float(1 << 53), float((1 << 53) + 2), float((1 << 53) - 1), 2.0 ** 63, -(2.0 ** 63)} <= set(d[~np.isnan(d)].tolist())
    eq = S.cmp(S.OP_EQ, i, None, d, None)[0]
    exact = np.array([(not math.isnan(y)) and x == int(y) for x, y in zip(i.tolist(), d.tolist())])
    assert (eq & ~exact).any() and not (exact & ~eq).any()  # e.g. 2^53 + 1 = float(2^53); I64_MAX = 2^63


@pytest.mark.parametrize("name", list(K.UTF8_LITERALS))
@pytest.mark.parametrize("n", K.UTF8_SIZES)
def test_utf8_data_sets(name, n):
    lit = K.UTF8_LITERALS[name]
    vals = K.utf8_values(lit, n)
    assert len(vals) == n
    if n >= 9:
        want = set(K.utf8_classes(lit)) - ({"empty"} if lit == b"" else set())
        assert {K.utf8_class_of(v, lit) for v in vals} == want
        assert vals[n - 1] is None  # the tail group ends in nulls
        for g in range(0, n - 7, 8):  # every whole validity byte mixes null / equal / unequal
            grp = vals[g:g + 8]
            assert any(v is None for v in grp) and any(v == lit for v in grp) and any(v not in (None, lit) for v in grp)
    if n == 2049 and len(lit) > 1:
        assert {lit[:k] for k in range(1, len(lit))} <= set(vals)
    offs, data, valid = K.utf8_arrays(vals, null_bytes=lit or b"x")
    assert offs[-1] == len(data) or (offs[-1] == 0 and len(data) == 1)
    assert all((offs[i + 1] > offs[i]) for i in range(n) if not valid[i])  # null rows span bytes


def test_utf8_pool_builder():
    pool = [b"", b"CA", b"C", b"CAX"]
    idx = np.array([1, 0, 3, 2, 1, 0, 0], dtype=np.int64)
    offs, data = K.utf8_from_pool(pool, idx)
    assert [bytes(data[offs[i]:offs[i + 1]]) for i in range(len(idx))] == [pool[i] for i in idx]


@pytest.mark.parametrize("n", [s for s in K.BOOL_SIZES if s >= 8])
def test_bool_data_sets(n):
    """Two nullable operands: true, false and null results on at least 10 % of the rows, for AND and
    for OR. (One row cannot; without validity on both sides there is less to reach: asserted below.)"""
    a, av, b, bv = K.bool_pair(n, True, True)
    for op in (S.OP_AND, S.OP_OR):
        assert min(K.state_shares(*S.bool3(op, a, av, b, bv))) >= 0.1
    for ln, rn in K.NULL_COMBOS[1:]:
        a, av, b, bv = K.bool_pair(n, ln, rn)
        assert (av is None) == (not ln) and (bv is None) == (not rn)
        for op in (S.OP_AND, S.OP_OR):
            t, f, nl = K.state_shares(*S.bool3(op, a, av, b, bv))
            assert t >= 0.1 and f >= 0.1 and (nl >= 0.1 or not (ln or rn))


@pytest.mark.parametrize("name", list(K.TILE_VECTORS))
@pytest.mark.parametrize("nullable", [False, True])
def test_tile_count_vectors_are_met(name, nullable):
    counts, tail, tail_sel = K.TILE_VECTORS[name]
    mask, mv = K.mask_with_tile_counts(counts, tail, 0, tail_sel, nullable)
    assert len(mask) == len(counts) * K.TILE + tail
    assert K.tile_counts(mask, mv, len(counts)) == list(counts) + [tail_sel]
    sel = S.select_mask(mask, mv)
    if nullable and (~sel).sum() >= 100:  # the unselected rows come in all three forms
        assert (~mask & mv).any() and (mask & ~mv).any() and (~mask & ~mv).any()
    fixed, utf8 = K.filter_inputs(sel)
    assert len(fixed) == 8 and sum(v[2] is not None for v in fixed.values()) == 5
    total = int(sel.sum())
    starts = np.cumsum([0] + K.tile_counts(mask, mv, len(counts)))
    for phase, (kind, vals, valid) in enumerate(fixed.values()):
        if valid is None or total == 0:
            continue
        out = valid[sel]
        if total >= 200:
            assert 0.3 <= out.mean() <= 0.7
        for i, p in enumerate(starts[:-1]):  # a run of equal bits across every tile's first selected row
            run = out[max(p - 20, 0):min(p + 20, total)]
            later = [q for q in starts[i + 1:] if q - 20 < p + 20 and q != p]
            if not later and len(run):
                assert (run == run[0]).all() and (len(run) >= 40 or p < 20 or p + 20 > total)
    for offs, data, valid, idx in utf8.values():
        lens = np.diff(offs)
        assert (lens == 0).any() and (lens == 40).any()
        assert valid is None or (lens[~valid] > 0).any()  # null rows whose offsets span bytes


def test_predicate_batch_reaches_every_branch():
    b = K.predicate_batch()
    keep = K.predicate_rows(b)
    n = K.PREDICATE_N
    assert 0.2 * n <= keep.sum() <= 0.8 * n
    a_null, s_null, c_null = ~b["av"], np.array([s is None for s in b["s"]]), ~b["cv"]
    gt = b["a"] > K.PREDICATE_K
    ca = np.array([s == b"CA" for s in b["s"]])
    for cond in (a_null & ~c_null, s_null & gt & ~a_null & ~c_null, c_null & a_null, gt & ca & ~a_null, gt & ~ca & ~s_null & ~a_null & ~c_null,
                 ~gt & ~a_null & s_null & ~c_null):
        assert cond.sum() >= 50
    # null AND false is false, not null: rows with a null `s` and a <= k are dropped without c
    assert not keep[~gt & ~a_null & s_null & ~c_null].any() and keep[c_null].all()
