"""The global aggregate over pieces, as a caller runs it (shared by tests/test_global_partial.py and
tests/test_global_exact_gpu.py): qe_agg_global_partial per piece with its row base,
qe_agg_global_merge, and — when the merge cannot certify the fp64 sum and returns QE_NEED_EXACT —
the exact round: qe_agg_global_exact_partial per piece and qe_agg_global_merge_exact."""


def partials(ctx, pieces, t):
    """pieces: [(values, valid or None)]. Returns (partial buffers, device columns) — the columns
    are held by the caller until the kernels are done, and serve the exact round."""
    import torch

    from kquery import native as N
    from kquery.columnar import DeviceColumn

    parts, cols = [], []
    base = 0
    for x, xv in pieces:
        p = torch.empty(N.GLOBAL_PARTIAL_BYTES, dtype=torch.uint8, device=ctx.torch_device)
        cols.append(DeviceColumn.from_numpy(t, x, xv, ctx=ctx))
        c = cols[-1].as_c()
        N.check(N.lib().qe_agg_global_partial(ctx.handle, N.C.byref(c), None, base, N.C.c_void_p(p.data_ptr())))
        parts.append(p)
        base += len(x)
    ctx.synchronize()
    return parts, cols


def merge(ctx, parts, cols, t):
    """Returns (QeGlobalAgg, whether the exact round ran)."""
    import torch

    from kquery import native as N

    buf = torch.cat(parts)
    out = N.QeGlobalAgg()
    st = N.lib().qe_agg_global_merge(ctx.handle, t, N.C.c_void_p(buf.data_ptr()), len(parts), N.C.byref(out))
    words = []
    if st == N.QE_NEED_EXACT:
        for c in cols:
            w = torch.empty(N.GLOBAL_EXACT_BYTES, dtype=torch.uint8, device=ctx.torch_device)
            cc = c.as_c()
            N.check(N.lib().qe_agg_global_exact_partial(ctx.handle, N.C.byref(cc), None, N.C.c_void_p(w.data_ptr())))
            words.append(w)
        allw = torch.cat(words)
        st = N.lib().qe_agg_global_merge_exact(ctx.handle, N.C.c_void_p(allw.data_ptr()), len(parts), N.C.byref(out))
    N.check(st)
    return out, bool(words)
