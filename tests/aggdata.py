"""Aggregate test data that can fail: value columns for the fp64 SUM / AVG parity tests.

A column with NaN sprinkled over every row makes every group of a few hundred rows sum to NaN, and
a comparison of two NaNs checks nothing of the accumulator. Here NaN, +Inf and -Inf appear only on
the rows of MARKED groups; every other group is finite and hard to sum.

group_values(k, kv, seed) -> (values, valid) for a key column:

* marked groups: groups // 8 of the distinct keys (the null key is a group), one when there are 2
  to 7, none for a single group; never the largest group. The marked groups take the kinds of
  KINDS in turn — NaN as the first non-null row (the sticky seed of MIN / MAX), +Inf alone, -Inf
  alone, +Inf with -Inf (NaN), NaN alone — so all five are there from 40 groups on, and the first
  groups // 8 of them below that (the 1/8 budget comes first).
* every other group: normal * 100 with +-0.0; in every second group (and the largest) +2^60 on its
  first non-null row and -2^60 on its last, which lie in different workgroups and, in the tests
  that update in two batches, in different batches (the other groups keep MIN / MAX and the +-0.0
  ties meaningful); in about a tenth (and the largest), inputs outside the LDS window of the
  specialised kernels and inputs for the full-range words: 1e-30, 3e19, 1e-40, 5e-324 * 77, 2^190
  and a +-1e300 pair.

global_values(n, seed, special, at): the same mix without keys, finite, or with one special value
at a chosen row.

check_group_conditions / the asserts of the tests state what the data must be for a comparison to
mean something; they are computed from the inputs alone (a group of finite values has a finite
exact sum: fewer than 2^24 rows of at most 1e300). tests/test_aggdata.py runs every call the GPU
tests make, with their seeds and shapes, on the CPU.
"""
import math

import numpy as np

KINDS = ("nan_first", "pos_inf", "neg_inf", "both_inf", "nan")
EXTRAS = ((1e-30,), (3e19,), (1e-40,), (5e-324 * 77,), (2.0 ** 190,), (1e300, -1e300))
BIG = 2.0 ** 60


def _base(rng, n):
    x = rng.normal(size=n) * 100
    x[rng.random(n) < 0.05] = 0.0
    x[rng.random(n) < 0.05] = -0.0
    return x


def _groups(k, kv, xv):
    """(group id per row, groups, rows with a non-null value ordered by group then row, bounds)."""
    n = len(k)
    uniq, gid = np.unique(k, return_inverse=True)
    gid = gid.reshape(-1).astype(np.int64)
    ng = len(uniq)
    if kv is not None and not np.all(kv):
        gid = np.where(kv, gid, ng)
        used = np.unique(gid)  # (a key may occur on null-key rows only)
        gid = np.searchsorted(used, gid)
        ng = len(used)
    vr = np.arange(n) if xv is None else np.nonzero(xv)[0]
    order = np.argsort(gid[vr], kind="stable")
    rows = vr[order]
    bounds = np.searchsorted(gid[vr][order], np.arange(ng + 1))
    return gid, ng, rows, bounds


def group_values(k, kv, seed, null_rate=0.1):
    k = np.asarray(k)
    n = len(k)
    rng = np.random.default_rng([int(seed), 0xA99])
    x = _base(rng, n)
    xv = (rng.random(n) >= null_rate) if null_rate > 0 else None
    if n == 0:
        return x, xv
    gid, ng, rows, bounds = _groups(k, kv, xv)
    cnt = np.diff(bounds)
    largest = int(np.argmax(cnt))
    # marked groups (never the largest; groups with two values or more first)
    nmark = ng // 8 if ng >= 8 else (1 if ng > 1 else 0)
    cand = np.array([g for g in rng.permutation(ng) if g != largest], dtype=np.int64)
    cand = np.concatenate([cand[cnt[cand] >= 2], cand[cnt[cand] < 2]])
    marked = cand[:nmark]
    for i, g in enumerate(marked.tolist()):
        r = rows[bounds[g]:bounds[g + 1]]
        m = len(r)
        if m == 0:
            continue
        kind = KINDS[i % len(KINDS)]
        more = r[1:][rng.random(m - 1) < 0.05]
        if kind == "nan_first":
            x[r[0]] = np.nan
            x[more] = np.nan
        elif kind == "both_inf":
            x[more] = np.where(rng.random(len(more)) < 0.5, np.inf, -np.inf)
            two = rng.choice(m, size=min(m, 2), replace=False)
            x[r[two[0]]] = np.inf
            if m > 1:
                x[r[two[1]]] = -np.inf
        else:
            v = {"pos_inf": np.inf, "neg_inf": -np.inf, "nan": np.nan}[kind]
            x[more] = v
            x[r[int(rng.integers(1, m))] if m > 1 else r[0]] = v
    finite = np.ones(ng, dtype=bool)
    finite[marked] = False
    # the cancelling pair
    pair = finite & (cnt >= 3) & ((np.arange(ng) % 2 == 0) | (np.arange(ng) == largest))
    x[rows[bounds[:-1][pair]]] = BIG
    x[rows[bounds[1:][pair] - 1]] = -BIG
    # inputs outside the LDS window and for the full-range words
    fg = np.nonzero(finite & (cnt >= 4))[0]
    if len(fg):
        hard = set(rng.choice(fg, size=max(1, len(fg) // 10), replace=False).tolist())
        if cnt[largest] >= 4:
            hard.add(largest)
        for g in sorted(hard):
            mid = rows[bounds[g] + 1:bounds[g + 1] - 1]
            vals = [v for e in EXTRAS if g == largest or rng.random() < 0.5 for v in e]
            if len(vals) > len(mid):
                vals = vals[:len(mid)]
                if vals and vals[-1] == 1e300:  # never half of the pair
                    vals.pop()
            x[rng.choice(mid, size=len(vals), replace=False)] = vals
    return x, xv


def group_stats(k, kv, x, xv, sel=None):
    """Per-group facts of the reference inputs (rows of sel only): counts of non-null values and
    which groups hold NaN / +Inf / -Inf / a NaN as their first non-null row."""
    n = len(k)
    use = np.ones(n, dtype=bool) if xv is None else np.asarray(xv, dtype=bool).copy()
    if sel is not None:
        use &= sel
    gid, ng, rows, bounds = _groups(k, kv, use)
    cnt = np.diff(bounds)

    def has(m):
        return np.bincount(gid[use & m], minlength=ng) > 0

    first_nan = np.zeros(ng, dtype=bool)
    ne = cnt > 0
    first_nan[ne] = np.isnan(x[rows[bounds[:-1][ne]]])
    return {"ng": ng, "cnt": cnt, "nan": has(np.isnan(x)), "pinf": has(x == np.inf), "ninf": has(x == -np.inf),
            "first_nan": first_nan, "rows": int(use.sum())}


def check_group_conditions(k, kv, x, xv, sel=None, kinds=True):
    """The conditions under which a parity test over this column can fail (module docstring).
    kinds=False: under a selection on the values themselves (x > c drops every NaN and -Inf) the
    special kinds are a property of the generator's output, checked without the selection."""
    s = group_stats(k, kv, x, xv, sel)
    cnt, ng = s["cnt"], s["ng"]
    nonnull = cnt > 0
    finite = nonnull & ~s["nan"] & ~s["pinf"] & ~s["ninf"]
    assert 2 * int(finite.sum()) >= int(nonnull.sum()), (int(finite.sum()), int(nonnull.sum()))
    if nonnull.any():
        big = int(cnt[finite].max()) if finite.any() else 0
        if s["rows"] >= 1000 * int(nonnull.sum()):
            assert big >= 1000, big
        else:
            assert big == int(cnt.max()), (big, int(cnt.max()))
    present = {
        "nan_first": bool(s["first_nan"].any()),
        "pos_inf": bool((s["pinf"] & ~s["ninf"] & ~s["nan"]).any()),
        "neg_inf": bool((s["ninf"] & ~s["pinf"] & ~s["nan"]).any()),
        "both_inf": bool((s["pinf"] & s["ninf"] & ~s["nan"]).any()),
        "nan": bool((s["nan"] & ~s["first_nan"] & ~s["pinf"] & ~s["ninf"]).any()),
    }
    nmark = ng // 8 if ng >= 8 else (1 if ng > 1 else 0)
    for kind in KINDS[:min(nmark, len(KINDS))] if kinds else ():
        assert present[kind], (kind, ng)
    return {"groups": int(nonnull.sum()), "finite": int(finite.sum()),
            "largest_finite": int(cnt[finite].max()) if finite.any() else 0}


def global_values(n, seed, special=None, at=None):
    """A finite column with the mix of the finite groups; `special` (NaN, +Inf or -Inf) at row `at`."""
    rng = np.random.default_rng([int(seed), 0xA9B])
    x = _base(rng, n)
    if n >= 2:
        m = max(1, n // 100)
        x[:m] = BIG
        x[n - m:] = -BIG
    if n >= 16:
        vals = [v for e in EXTRAS for v in e]
        x[rng.choice(np.arange(1, n - 1), size=len(vals), replace=False)] = vals
    if special is not None:
        x[at] = special
    return x


def check_global_finite(x):
    """The finite form's condition: a finite reference sum (fewer than 2^24 rows of at most 1e300)."""
    assert np.isfinite(x).all() and len(x) < 2 ** 24


# ---- the GPU tests' calls: keys as the tests always made them, values from the generator -----------
def int64_key_data(ngroups):
    """tests/test_gpu_parity.py test_hashagg_int64_key[f64-*]."""
    rng = np.random.default_rng(ngroups)
    n = 400_000
    k = rng.integers(0, ngroups, n).astype(np.int64) * 7919 - 3
    kv = rng.random(n) > 0.01
    k[rng.random(n) < 0.001] = -2**63  # the EMPTY sentinel value is a legal key
    return rng, n, k, kv


def partitioned_data(ngroups, expected):
    """test_hashagg_partitioned[*-f64-*]."""
    rng = np.random.default_rng(ngroups + expected)
    n = 1_000_000
    k = rng.integers(0, ngroups, n).astype(np.int64) * 7919 - 3
    kv = rng.random(n) > 0.01
    k[rng.random(n) < 0.001] = -2**63
    return rng, n, k, kv


def multipass_data(ngroups, expected):
    """test_hashagg_multipass[*-f64-*]."""
    rng = np.random.default_rng(ngroups * 3 + expected)
    n = 600_000
    k = rng.integers(0, ngroups, n).astype(np.int64) * 104729 + 11
    kv = rng.random(n) > 0.01
    return rng, n, k, kv


def two_phase_data():
    """test_export_import_two_phase."""
    rng = np.random.default_rng(9)
    n = 600_000
    k = rng.integers(0, 5000, n).astype(np.int64)
    kv = rng.random(n) > 0.01
    return rng, n, k, kv


def colrec_data(rng, n):
    """test_fused_partitioned_column_records[*-f64-32] (_colrec_case)."""
    k = rng.integers(0, 60_000, n).astype(np.int64) * 7919 - 3
    kv = rng.random(n) > 0.01
    return k, kv


INT64_KEY = [(1, 16), (10, 1024), (1000, 1024), (5000, 100), (200_000, 1024)]
PARTITIONED = [(50_000, 50_000), (600_000, 20_000), (3, 100_000)]
MULTIPASS_F64 = [(1200, 1200), (40_000, 1200)]
GLOBAL_SPECIALS = (math.nan, math.inf, -math.inf)


def group_calls():
    """(name, k, kv, x, xv, sel) of every group_values call of the GPU tests."""
    for ngroups, _ in INT64_KEY:
        _, _, k, kv = int64_key_data(ngroups)
        yield (f"int64_key[{ngroups}]", k, kv) + group_values(k, kv, ngroups) + (None,)
    for ngroups, expected in PARTITIONED:
        _, _, k, kv = partitioned_data(ngroups, expected)
        yield (f"partitioned[{ngroups}]", k, kv) + group_values(k, kv, ngroups + expected) + (None,)
    for ngroups, expected in MULTIPASS_F64:
        _, _, k, kv = multipass_data(ngroups, expected)
        yield (f"multipass[{ngroups}]", k, kv) + group_values(k, kv, ngroups * 3 + expected) + (None,)
    _, _, k, kv = two_phase_data()
    yield ("two_phase", k, kv) + group_values(k, kv, 9) + (None,)
    k, kv = colrec_data(np.random.default_rng(len("f64")), 1_000_000)
    x, xv = group_values(k, kv, 3)
    yield ("colrec[f64]", k, kv, x, xv, xv & (x > -50.0))


# ---- rounding boundaries of the exact fp64 SUM / AVG ------------------------------------------------
# One group per case (tests/test_fx_sum.py on the host build of the accumulator,
# tests/test_fp64_sum_gpu.py on every kernel path). The expected value is the oracle's _fsum of the
# rows, AVG that sum / count. W: the 256-bit fixed-point words (units 2^-128); E: the full-range words.
DBL_MAX = 1.7976931348623157e308
TINY = 2.2250738585072014e-308  # the smallest normal
_H = 2.0 ** -53  # half an ulp of 1.0
_W = 2.0 ** -120  # a bit in the low word of W
_E = 5e-324  # a bit in E
BOUNDARY_CASES = [
    ("tie_down", [1.0, _H]),  # a tie: to even, 1.0
    ("tie_up_even", [1.0, 2.0 ** -52, _H]),  # a tie: up to even
    ("tie_plus_w", [1.0, _H, _W]),
    ("tie_minus_w", [1.0, _H, -_W]),
    ("tie_plus_e", [1.0, _H, _E]),
    ("tie_minus_e", [1.0, _H, -_E]),
    ("tie_w_cancelled", [1.0, _H, _W, -_W]),  # the deciding term cancelled in another row
    ("tie_up_w_cancelled", [1.0, 2.0 ** -52, _H, -_W, _W]),
    ("tie_e_cancelled", [1.0, _H, _E, -_E]),
    ("tie_up_e_cancelled", [1.0, 2.0 ** -52, _H, -_E, _E]),
    ("overflow_tie", [DBL_MAX, 2.0 ** 970]),  # half way to 2^1024: +Inf
    ("below_overflow", [DBL_MAX, 2.0 ** 969]),  # DBL_MAX
    ("neg_overflow_tie", [-DBL_MAX, -(2.0 ** 970)]),
    ("neg_below_overflow", [-DBL_MAX, -(2.0 ** 969)]),
    ("normal_minus_subnormal", [TINY, -_E]),  # the largest subnormal
    ("zero_among_neg_zeros", [3.7e-5, -0.0, -3.7e-5, -0.0]),  # +0.0
    ("avg_third", [0.5, 0.25, 0.25]),  # AVG 1 / 3
    ("avg_half_subnormal", [_E, 0.0]),  # AVG 5e-324 / 2: a tie, to even, 0.0
    # a lost carry out of W's low word: 2^-65 + 2^-65 = 2^-64 decides the tie upwards
    ("carry_low_word", [1.0, _H, 2.0 ** -65, 2.0 ** -65, -(2.0 ** -64) + 2.0 ** -110]),
]
