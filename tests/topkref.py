"""Reference for the top-k selection's host rules (csrc/qe_topk_plan.hpp), restated in Python: the
threshold-bin pick, the `need` bookkeeping, the stop rule, and the properties QE_TOPK_AUTO must have
(not its constant). The ORDER oracle of top-k is sortref.order(keys, flags, limit=k): the first k
entries of the stable order."""


def pick_bin(hist, need):
    """(bin, below, tied): the bin b with below(b) < need <= below(b) + hist[b]; (-1, total, 0) when
    need is outside 1..total. Python integers: no width to overflow."""
    below = 0
    if need >= 1:
        for b, c in enumerate(hist):
            if need <= below + c:
                return b, below, c
            below += c
    return -1, below, 0


def top_digit(hist8, rows):
    """The highest digit g (7 = most significant) whose 256-bin histogram hist8[g] does not hold all
    `rows` rows in one bin; -1 when every digit is constant."""
    for g in range(7, -1, -1):
        if rows not in hist8[g]:
            return g
    return -1


def stop(candidates, k, small_max, factor):
    return candidates <= max(small_max, factor * k)


def header_constants():
    """(stop factor, AUTO divisor) as qe_topk_plan.hpp defines them: build-time numbers the device
    tests need to say which path AUTO must take, read from the header and not restated."""
    import pathlib
    import re

    text = (pathlib.Path(__file__).resolve().parents[1] / "query-engines_amd" / "csrc" / "qe_topk_plan.hpp").read_text()
    return tuple(int(re.search(rf"#define {name} (\d+)", text).group(1)) for name in ("QE_TOPK_STOP_FACTOR", "QE_TOPK_AUTO_DIV"))


def use_select(n, k, small_max, div):
    """topk_use_select with the divisor as a parameter."""
    return n > small_max and k < n and k <= n // div


def walk(k, tied, picks):
    """The need bookkeeping over a list of (below, tied) picks and a final cut: the (need,
    candidates) pairs before the first pick, after every pick and after the cut."""
    sure, out = 0, []
    out.append((k - sure, sure + tied))
    for below, t in picks:
        sure, tied = sure + below, t
        out.append((k - sure, sure + tied))
    tied = k - sure
    out.append((k - sure, sure + tied))
    return out


def check_auto(use_select, small_max, div_bound=None):
    """The properties of the AUTO rule `use_select(n, k)`: the full sort when n <= small_max or
    k >= n; selection for some small k on a large n; monotone in k (once it sorts, it sorts for every
    larger k). Returns the largest selecting k per probed n."""
    last = {}
    for n in (0, 1, small_max - 1, small_max, small_max + 1, 4 * small_max, 10**6 + 3, 10**8, 2**31 - 1):
        ks = sorted({0, 1, 2, 10, 1000, n // 1024, n // 64, n // 32, n // 17, n // 16, n // 16 + 1, n // 8, n // 4,
                     n // 2, n - 1, n, n + 1, n + 5} - {-1})
        seen_sort = False
        for k in ks:
            sel = use_select(n, k)
            if n <= small_max or k >= n:
                assert not sel, (n, k)
            if seen_sort:
                assert not sel, f"not monotone in k at n={n}, k={k}"
            seen_sort |= not sel
            if sel:
                last[n] = k
        if n > 64 * small_max:
            assert use_select(n, 1) and use_select(n, 10) and use_select(n, n // 1024), n
    return last
