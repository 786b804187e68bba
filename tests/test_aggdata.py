"""The aggregate-data generator (tests/aggdata.py) meets its own conditions for every call the GPU
tests make, with their seeds and shapes — checked here on the CPU, from the inputs alone — and the
premise of it: the columns those tests used before (NaN on 5 % of all rows) leave the regular
GROUP BY shapes without a single finite sum."""
import math

import numpy as np
import pytest

import aggdata


def test_group_generator_conditions():
    seen = 0
    for name, k, kv, x, xv, sel in aggdata.group_calls():
        full = aggdata.check_group_conditions(k, kv, x, xv)
        assert full["finite"] >= 1, name
        if sel is not None:
            aggdata.check_group_conditions(k, kv, x, xv, sel, kinds=False)
        # specials only on rows of marked groups: at most 1/8 of the groups (one below 8) hold any
        s = aggdata.group_stats(k, kv, x, xv)
        special = s["nan"] | s["pinf"] | s["ninf"]
        assert int(special.sum()) <= max(s["ng"] // 8, 1), name
        seen += 1
    assert seen == len(aggdata.INT64_KEY) + len(aggdata.PARTITIONED) + len(aggdata.MULTIPASS_F64) + 2


def test_group_generator_is_deterministic_and_keeps_keys():
    _, _, k, kv = aggdata.multipass_data(1200, 1200)
    k0 = k.copy()
    a = aggdata.group_values(k, kv, 5)
    b = aggdata.group_values(k, kv, 5)
    assert np.array_equal(k, k0)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("ngroups", [1, 2, 7, 8, 39, 40, 1000])
def test_group_generator_small_shapes(ngroups):
    rng = np.random.default_rng(ngroups)
    k = rng.integers(0, ngroups, 20_000).astype(np.int64)
    k[:ngroups] = np.arange(ngroups)
    x, xv = aggdata.group_values(k, None, ngroups)
    st = aggdata.check_group_conditions(k, None, x, xv)
    s = aggdata.group_stats(k, None, x, xv)
    special = int((s["nan"] | s["pinf"] | s["ninf"]).sum())
    assert special == (ngroups // 8 if ngroups >= 8 else (1 if ngroups > 1 else 0))
    assert st["finite"] == ngroups - special
    # the finite groups are hard: a cancelling pair and the full-range inputs are there
    assert (x == aggdata.BIG).sum() == (x == -aggdata.BIG).sum() >= 1
    assert (np.abs(x) == 1e300).sum() >= 2 and (x == 1e-40).any()


def test_global_generator():
    for n in (0, 1, 7, 1000, 100_003):
        x = aggdata.global_values(n, n)
        aggdata.check_global_finite(x)
        if n >= 16:
            assert (x == aggdata.BIG).sum() == (x == -aggdata.BIG).sum() == max(1, n // 100)
            assert (x == 1e300).sum() == (x == -1e300).sum() == 1
    x = aggdata.global_values(1000, 3, math.inf, 666)
    assert np.isinf(x).sum() == 1 and x[666] == math.inf


def test_premise_old_columns_have_no_finite_groups():
    """The column the parity tests used (NaN on 5 % of rows, +Inf on 1 %) at test_hashagg_int64_key's
    1000-group shape: no group has a finite sum."""
    rng, n, k, kv = aggdata.int64_key_data(1000)
    v = rng.normal(size=n) * 100
    v[rng.random(n) < 0.05] = np.nan
    v[rng.random(n) < 0.05] = 0.0
    v[rng.random(n) < 0.05] = -0.0
    v[rng.random(n) < 0.01] = np.inf
    xv = rng.random(n) >= 0.1
    s = aggdata.group_stats(k, kv, v, xv)
    assert not ((s["cnt"] > 0) & ~s["nan"] & ~s["pinf"] & ~s["ninf"]).any()
