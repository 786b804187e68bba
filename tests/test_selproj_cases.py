"""CPU checks of tests/selprojcases.py: the two references agree on every plan shape, and every
selection builder meets the condition it is named for at every tile size the select-project
generator can report (tests/test_selproj_shapes.py fails, not skips, on a tile size outside
selprojcases.TILE_SIZES)."""
import numpy as np
import pytest

import selprojcases as K
from oracle import semantics as S

GEOMS = [(T, b) for T in K.TILE_SIZES for b in K.BLOCKS if T % b == 0]


def _same(a, b):
    (av, ao), (bv, bo) = a, b
    assert av.dtype == bv.dtype and len(av) == len(bv)
    assert (ao == bo).all()
    w = 8 if av.dtype.itemsize == 8 else av.dtype.itemsize
    view = {8: np.int64, 4: np.int32, 1: np.uint8}[w]
    assert (av.view(view)[ao] == bv.view(view)[bo]).all()


@pytest.mark.parametrize("shape", K.shape_names())
@pytest.mark.parametrize("builder", ["uniform_50", "seq_mixed", "one_per_tile_rand"])
def test_row_loop_equals_vectorised_reference(shape, builder):
    n = 5000
    sel = K.BUILDERS[builder](n, 1024, 256, 7)
    cols, spec = K.make_case(shape, sel, 7, 1024, 256)
    rows, ref = K.select_project_rows(cols, spec), K.select_project_ref(cols, spec)
    assert len(rows) == len(ref) == len(spec.outputs)
    for a, b in zip(rows, ref):
        _same(a, b)
        assert len(a[0]) == int(sel.sum())
    assert (K.selection_of(cols, spec) == sel).all()


def test_row_loop_division_and_wrap():
    """What no shape uses but the references promise: x / 0 -> null, truncation, int64 wrap."""
    x = K.Col("i64", [7, -7, K.I32_MIN, -(1 << 63), 5, (1 << 63) - 1], [True, True, True, True, False, True])
    y = K.Col("i64", [2, 2, 0, -1, 1, 1])
    spec = K.Spec([], [K._bin(K.TOK_DIV, K._col(0), K._col(1)), K._bin(K.TOK_ADD, K._col(0), K._lit(1)),
                       K._bin(K.TOK_MUL, K._col(0), K._lit(1.5))])
    rows, ref = K.select_project_rows([x, y], spec), K.select_project_ref([x, y], spec)
    for a, b in zip(rows, ref):
        _same(a, b)
    assert list(rows[0][0][[0, 1, 3]]) == [3, -3, -(1 << 63)] and list(rows[0][1]) == [True, True, False, True, False, True]
    assert rows[1][0][5] == -(1 << 63) and rows[2][0].dtype == np.float64


@pytest.mark.parametrize("T,block", GEOMS)
@pytest.mark.parametrize("extra", [1, 0])
def test_builders_meet_their_conditions(T, block, extra):
    n = 66 * T + extra
    nt = (n + T - 1) // T
    rows_in = np.minimum(T, n - np.arange(nt) * T)
    B = lambda name: K.BUILDERS[name](n, T, block, 3)
    assert B("none").sum() == 0 and B("all").all()
    assert list(np.flatnonzero(B("first_only"))) == [0] and list(np.flatnonzero(B("last_only"))) == [n - 1]
    tt = B("tail_tile_only")
    assert tt.sum() == n % T and (n % T == 0 or tt[-(n % T):].all())
    for pos in ("first", "last", "rand"):
        s = B("one_per_tile_" + pos)
        assert (K.tile_counts(s, T) == 1).all()
        loc = np.flatnonzero(s) % T
        assert pos != "first" or (loc == 0).all()
        assert pos != "last" or (loc == rows_in - 1).all()
        assert pos != "rand" or len(set(loc)) > 8
        # output rows 0..nt-1: one validity word holds min(32, nt) >= 3 tiles
        assert np.bincount(K.tile_bases(s, T) >> 5).max() >= 3
    alt = K.tile_counts(B("alternate_tiles"), T)
    assert (alt[0::2] == rows_in[0::2]).all() and (alt[1::2] == 0).all()
    for name, seq in (("seq_31", [31]), ("seq_33", [33]), ("seq_mixed", K.SEQ_MIXED), ("seq_123", [1, 2, 3])):
        s = B(name)
        want = np.minimum(np.resize(seq, nt), rows_in)
        assert (K.tile_counts(s, T) == want).all(), name
        bases = K.tile_bases(s, T)
        if name in ("seq_31", "seq_33"):  # the output base passes through every bit offset
            assert set(bases & 31) == set(range(32)), name
        if name == "seq_mixed":
            # its period sums to 160 = 5 x 32, so the bases only take bit offsets 0 and 1: what it adds
            # is counts of 0, 1, a whole word, a word and a bit, and 63 at those two offsets
            assert set(bases & 31) == {0, 1}
        assert set(bases & 1) == {0, 1}, name  # both 16-byte parities of an 8-byte output
    assert {int(K.BUILDERS["seq_123"](m, T, block, 3).sum()) & 1 for m in (T, T + 1, 2 * T)} == {0, 1}  # odd and even totals
    fs = K.tile_counts(B("seq_full_short"), T)
    assert fs[3] == T - 1 and (np.delete(fs, 3) == np.delete(rows_in, 3)).all()
    # wave / stripe / lane builders under the stripe map: row = base + r * block + t
    row = np.arange(n)
    loc = row % T
    for name, want in (("one_wave_0", (loc % block) // 64 == 0), ("one_wave_last", (loc % block) // 64 == block // 64 - 1),
                       ("one_stripe_0", loc // block == 0), ("one_stripe_last", loc // block == T // block - 1),
                       ("lane0_only", loc % 64 == 0), ("lane63_only", loc % 64 == 63)):
        assert (B(name) == want).all(), name
    for name, p in (("uniform_01", 0.01), ("uniform_50", 0.5), ("uniform_99", 0.99)):
        assert abs(B(name).mean() - p) < 0.01


def test_resident_groups():
    """Group-sized placement (8 stripes of 1024 rows inside a resident tile): alternate_tiles at
    T = group size empties whole groups, one_stripe hits one stripe of every group."""
    G = 8 * 1024
    n = 3 * 12288 + 5
    alt = K.tile_counts(K.alternate_tiles(n, G, 1024), G)
    assert (alt[1::2] == 0).all() and (alt[0::2] > 0).all()
    s = K.one_stripe(-1)(n, G, 1024)
    assert (np.flatnonzero(s) % G >= G - 1024).all() and s.any()
    g = K.alternate_groups(G)(n, 12288, 1024).reshape(-1)[: 3 * 12288].reshape(3, 12288)
    assert g[0, :G].all() and not g[0, G:].any() and not g[1, :G].any() and g[1, G:].all() and g[2, :G].all()


@pytest.mark.parametrize("T,block", GEOMS)
def test_s7_data(T, block):
    n = 20 * T + 5
    sel = K.uniform(0.5)(n, T, block, 11)
    cols, spec = K.make_case("S7", sel, 11, T, block)
    p, q, b = (c.values for c in cols)
    terms = []
    for col, op, rhs, lit in spec.terms:
        m, mv = S.cmp(op, cols[col].values, None, cols[rhs].values if rhs >= 0 else lit, None)
        terms.append(S.select_mask(m, mv))
    assert (terms[0] & terms[1] & terms[2] == sel).all()
    for k in range(3):
        assert (~terms[k]).mean() >= 0.1, k
    others_q = terms[0] & terms[2]
    qb = q.view(np.int64)
    for v in K.S7_SPECIAL_Q:
        assert (others_q & (qb == np.float64(v).view(np.int64))).any(), v
    others_p = terms[1] & terms[2]
    for v in (-1, K.I32_MAX):
        assert (others_p & (p == v)).any(), v
    assert ((p == K.I32_MIN) & terms[1]).any()  # (INT32_MIN < b needs b above it: the third term is free)
    # whole stripes and the tail
    stripes = p[: (n // block) * block].reshape(-1, block)
    for v in (-1, K.I32_MAX):
        assert (stripes == v).all(axis=1).any(), v
    tail = p[(n // T) * T:]
    assert {-1, K.I32_MAX, K.I32_MIN} & set(tail.tolist())
    unsel = ~sel[: (n // block) * block].reshape(-1, block)
    assert (((stripes == K.I32_MIN) | ~unsel).all(axis=1) & unsel.any(axis=1)).any()


@pytest.mark.parametrize("shape", ["S6v", "S8"])
def test_null_rows_carry_passing_values(shape):
    n = 50_000
    sel = K.uniform(0.5)(n, 4096, 256, 5)
    cols, spec = K.make_case(shape, sel, 5)
    if shape == "S6v":
        m = cols[2]
        trap = ~m.valid & m.values
    else:
        a = cols[0]
        trap = ~a.valid & (a.values > spec.terms[0][3])
    assert trap.mean() >= 0.05 and not (trap & sel).any()
    assert (K.selection_of(cols, spec) == sel).all()


def test_s4_values_under_nulls():
    sel = K.uniform(0.5)(20_000, 2048, 256, 2)
    cols, _ = K.make_case("S4", sel, 2)
    assert set(cols[1].values[~cols[1].valid].tolist()) == {K.I32_MIN, -1}
    assert set(cols[2].values[~cols[2].valid].tolist()) == {128, 255}
    assert set(cols[3].values[~cols[3].valid].tolist()) == {K.I32_MIN, -1}
