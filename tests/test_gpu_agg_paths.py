"""The live GROUP BY notes at the path changes that tests/golden/agg_paths.json records (the CPU side:
tests/test_agg_paths.py, which says what the golden file is)."""
import pytest

import aggpaths

pytestmark = pytest.mark.gpu

GOLD = aggpaths.golden()


def test_live_notes_at_the_path_changes(gpu_ctx, monkeypatch):
    """C4 plan, default knobs, ~300,000 rows per update: at the golden grid points on either side of
    each path change the live note decides what the golden note did. Plan-specialised kernels; with
    the generic kernel (jit off) only the golden's path and pass count."""
    from kquery import native as N
    from kquery.aggregate import HashAggregateState
    from kquery.datasource import ColumnSpec, generate_column
    from kquery.workloads import C4_AGGS, c4_spec

    for kn in aggpaths.KNOBS:
        monkeypatch.delenv(kn, raising=False)
    rows = GOLD["rows"]
    ab = [generate_column(ColumnSpec(n, N.TYPE_INT64, N.GEN_MOD, 1 << 20, i), rows, 0, 42, gpu_ctx)
          for i, n in ((1, "a"), (2, "b"))]

    def live(groups):
        k = generate_column(ColumnSpec("k", N.TYPE_INT64, N.GEN_MOD, groups, 0), rows, 0, 42, gpu_ctx)
        st = HashAggregateState(gpu_ctx, [N.TYPE_INT64], C4_AGGS, groups)
        st.update_fused([k] + ab, c4_spec(1 << 16))
        sp, note = st.last_kernel_kind()
        st.close()
        return aggpaths.decided(note, sp)

    try:
        for setting, jit in (("default", 1), ("jit0", 0)):
            if setting not in GOLD["settings"]:
                continue
            N.check(N.lib().qe_ctx_set_jit(gpu_ctx.handle, jit))
            recs = [r for r in GOLD["settings"][setting]["records"] if r["plan"] == "c4"]
            by_groups = {r["groups"]: r for r in recs}
            # a path change: another path, sub-bucket count or number of passes (the radix partition's
            # bucket count doubles many times more: checked at these points and at the grid's ends)
            pts = aggpaths.boundary_points(recs, lambda d: (d["path"], d.get("sub_buckets"), d.get("mp_n")))
            assert len(pts) >= (8 if jit else 4), pts
            pts = [recs[0]["groups"]] + pts + [recs[-1]["groups"]]
            for g in pts:
                want = aggpaths.decided(by_groups[g]["note"], by_groups[g]["specialized"])
                assert live(g) == want, (setting, g, by_groups[g]["note"])
    finally:
        N.check(N.lib().qe_ctx_set_jit(gpu_ctx.handle, 1))
