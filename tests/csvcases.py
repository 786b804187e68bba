"""Inputs, expected values and the raw-bytes entry for the CSV scan's shape tests
(tests/test_csv_shapes.py): files of just over one segment-plan block assembled from pieces the
oracle parses once, wide records, small files for every-cut runs, and the hostile-alphabet fuzz.
Everything here is deterministic, so the CPU tests can assert the conditions each input must meet."""
import collections
import functools
import random

import numpy as np

from oracle import csv_ref as R

SEG = 16 * 1024  # qe_csv.hip: bytes per wave task
SP_TILE = 2048  # qe_csv.hip: segments per block of the segment plan
BLOCK = SP_TILE * SEG  # the first byte of the plan's second block
COMMA = 0x2C

Column = collections.namedtuple("Column", "offsets values max_len")  # int32 [rows + 1], uint8 [bytes], int


# ---- the device entry -----------------------------------------------------------------------------
def upload(ctx, data: bytes):
    import torch

    if not data:
        return torch.empty(1, dtype=torch.uint8, device=ctx.torch_device)[:0]
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(ctx.torch_device)


def parse_bytes(ctx, data, delim, has_header, fields, partial=False):
    """(columns of the projected field indices, bytes consumed) of one qe_csv_parse over `data`
    (bytes, or a uint8 device tensor already uploaded), the way CsvDataSource._parse_region calls
    the library: no file, no header-name lookup, 32 fields per call."""
    import torch

    from kquery import native as N

    dev = data if isinstance(data, torch.Tensor) else upload(ctx, data)
    nbytes = dev.numel()
    L, C = N.lib(), N.C
    out, consumed, nrows = [], nbytes, None
    for s in range(0, len(fields), 32):
        part = list(fields[s:s + 32])
        fi = (C.c_int32 * len(part))(*part)
        opt = N.QeCsvOptions(delim, 1 if has_header else 0, len(part), N.CSV_PARTIAL_TAIL if partial else 0, fi)
        h = C.c_void_p()
        N.check(L.qe_csv_parse(ctx.handle, C.c_void_p(dev.data_ptr()), nbytes, C.byref(opt), C.byref(h)))
        try:
            rows, used = C.c_int64(), C.c_int64()
            N.check(L.qe_csv_rows(h, C.byref(rows)))
            N.check(L.qe_csv_consumed(h, C.byref(used)))
            assert nrows in (None, rows.value) and (s == 0 or consumed == used.value)  # every call sees the same records
            nrows, consumed = rows.value, used.value
            for c in range(len(part)):
                nb, ml = C.c_int64(), C.c_int64()
                N.check(L.qe_csv_column_bytes(h, c, C.byref(nb)))
                N.check(L.qe_csv_column_max_len(h, c, C.byref(ml)))
                vals = torch.empty(max(1, nb.value), dtype=torch.uint8, device=ctx.torch_device)
                offs = torch.empty(nrows + 1, dtype=torch.int32, device=ctx.torch_device)
                cc = N.QeColumn(N.TYPE_UTF8, 0, nrows, None, vals.data_ptr(), offs.data_ptr())
                N.check(L.qe_csv_column_copy(h, c, C.byref(cc)))
                out.append(Column(offs.cpu().numpy(), vals[:nb.value].cpu().numpy(), ml.value))
        finally:
            L.qe_csv_destroy(h)
    return out, consumed


# ---- expected values --------------------------------------------------------------------------------
def project_rows(rows, fields):
    """Oracle rows -> rows of the projected fields (a missing field reads as b"")."""
    return [[r[f] if f < len(r) else b"" for f in fields] for r in rows]


def device_rows(columns):
    """Device columns -> rows of byte values (small results only)."""
    n = len(columns[0].offsets) - 1
    cols = [[c.values[c.offsets[i]:c.offsets[i + 1]].tobytes() for i in range(n)] for c in columns]
    return [list(r) for r in zip(*cols)]


def piece_columns(pieces, fields):
    """Expected columns of a file assembled from `pieces` = [(oracle rows of the piece, repeat
    count)]: per field the value lengths tiled and the value bytes repeated, never row by row."""
    out = []
    for f in fields:
        lens, vals = [np.zeros(0, dtype=np.int64)], []
        for rows, count in pieces:
            v = [r[f] if f < len(r) else b"" for r in rows]
            lens.append(np.tile(np.array([len(x) for x in v], dtype=np.int64), count))
            vals.append(b"".join(v) * count)
        offs = np.zeros(1 + sum(len(x) for x in lens), dtype=np.int64)
        np.cumsum(np.concatenate(lens), out=offs[1:])
        out.append(Column(offs.astype(np.int32), np.frombuffer(b"".join(vals), dtype=np.uint8), None))
    return out


def head_columns(columns, n):
    """The first n rows of expected columns."""
    return [Column(c.offsets[:n + 1], c.values[:c.offsets[n]], None) for c in columns]


def assert_columns(got, want, what=""):
    """Whole-array comparison of device columns with expected ones; on a mismatch names the first
    differing row. The parse's longest-value figure must be exact."""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g.offsets) == len(w.offsets), f"{what} column {i}: {len(g.offsets) - 1} rows, expected {len(w.offsets) - 1}"
        if not np.array_equal(g.offsets, w.offsets):
            r = int(np.flatnonzero(g.offsets != w.offsets)[0])
            raise AssertionError(f"{what} column {i}: offsets differ first at entry {r}: {g.offsets[r]} != {w.offsets[r]}")
        if not np.array_equal(g.values, w.values):
            b = int(np.flatnonzero(g.values != w.values)[0])
            r = int(np.searchsorted(w.offsets, b, side="right")) - 1
            a, e = int(w.offsets[r]), int(w.offsets[r + 1])
            raise AssertionError(f"{what} column {i}: row {r} is {g.values[a:e].tobytes()!r}, expected {w.values[a:e].tobytes()!r}")
        longest = int(np.diff(w.offsets).max()) if len(w.offsets) > 1 else 0
        assert g.max_len == longest, f"{what} column {i}: max_len {g.max_len}, longest value {longest}"


# ---- record units (random_csv-style, '\n'-terminated pieces) -------------------------------------------
PLAIN_WORDS = ["a", "b c", "Uppsala", "Sthlm", "Pärsson", "1337", "", "  padded  ", "€uro", "tab\there", "x#y", "0.25"]
QUOTE_WORDS = ["x,y", 'he said "hi"', "line\nbreak", '"', " in quotes "]
CR_WORDS = ["crlf\r\nin", "cr\rin"]
NCOLS = 5


def record_unit(seed, nbytes, quotes=False, cr=False, skips=False):
    """About `nbytes` of records of NCOLS fields (one in ten ragged), ending in '\\n'. quotes: quoted
    fields (balanced) holding delimiters, '\\n' and "" pairs; cr: also '\\r' inside quotes and
    '\\r\\n' / lone '\\r' terminators; skips: blank and comment lines. Without skips every line is a
    kept record."""
    rng = random.Random(seed)
    words = PLAIN_WORDS + (QUOTE_WORDS if quotes else []) + (CR_WORDS if quotes and cr else [])
    out, size = [], 0
    while size < nbytes:
        r = rng.random()
        if skips and r < 0.03:
            line = ""
        elif skips and r < 0.05:
            line = "   \t "
        elif skips and r < 0.07:
            line = "#comment, with, delims"
        else:
            k = NCOLS if rng.random() < 0.9 else rng.randint(1, NCOLS + 2)
            f = []
            for _ in range(k):
                w = rng.choice(words)
                if any(ch in w for ch in ',\n\r"') or (quotes and rng.random() < 0.2):
                    w = '"' + w.replace('"', '""') + '"'
                f.append(w)
            line = ",".join(f)
            if not R.kept(line.encode()):
                line = "k" + line
        nl = rng.choice(["\n", "\r\n", "\r"]) if cr else "\n"
        out.append(line + nl)
        size += len(out[-1].encode())
    out[-1] = out[-1].rstrip("\r\n") + "\n"
    return "".join(out).encode()


def filler(nbytes):
    """Exactly nbytes (>= 16) of short plain lines."""
    assert nbytes >= 16
    return b"fill,er\n" * (nbytes // 8 - 1) + b"fill,er" + b"x" * (nbytes % 8) + b"\n"


SegFile = collections.namedtuple("SegFile", "data pieces special_start rows_before_special close_quote")
HEADER = b"c0,c1,c2,c3,c4\n"


def _finish(parts, special_at=None, close_quote=None):
    """parts = [(bytes of a piece, repeat count)] after the header -> SegFile; each piece's rows
    come from one oracle parse of the piece on its own."""
    pieces = [(R.rows(p, COMMA, False), n) for p, n in parts]
    data = HEADER + b"".join(p * n for p, n in parts)
    start = before = None
    if special_at is not None:
        start = len(HEADER) + sum(len(p) * n for p, n in parts[:special_at])
        before = sum(len(rows) * n for rows, n in pieces[:special_at])
    return SegFile(data, pieces, start, before, close_quote)


def seg_file(name, block=BLOCK, seg=SEG, unit_bytes=64 << 10, tail_bytes=1 << 20):
    """The three files that reach the segment plan's second block (`block` bytes in; the defaults
    are the library's sizes, smaller ones give the same construction for the oracle to parse whole).
      plain:    no '"' and no '\\r' anywhere, every line a record, a record across `block`, the last
                record unterminated (the classify path);
      straddle: no '\\r' before `block`; one quoted field opens 40 bytes before `block` and closes
                more than `seg` bytes after it, holding '\\n', '\\r\\n', delimiters and "" pairs (its
                first seg / 2 bytes after `block` only '\\n' and delimiters: a chunk cut there has its
                only '"' bytes in block 0 and its block 1 wholly inside quotes); then records with
                all three terminators, the last one unterminated;
      late:     plain before `block` (with blank and comment lines), the file's first '"' and
                '\\r' after it."""
    tail = record_unit(12, unit_bytes, quotes=True, cr=True, skips=name == "late")
    treps = max(1, tail_bytes // len(tail))
    if name == "plain":
        unit = record_unit(10, unit_bytes)
        reps = (block + tail_bytes) // len(unit) + 1
        for pad in range(64):  # the filler line's length puts `block` strictly inside a record
            fill = b"f" * pad + b",fill\n"
            at = (block - len(HEADER) - len(fill)) % len(unit)
            if at >= 1 and unit[at - 1] != 0x0A and unit[at] != 0x0A:
                break
        return _finish([(fill, 1), (unit, reps), (b"last,, no newline ,x,y,z,w", 1)])
    if name == "straddle":
        unit = record_unit(11, unit_bytes, quotes=True)
        start = block - 43  # the record's first byte; its field's opening quote sits at block - 40
        reps = (start - len(HEADER) - 16) // len(unit)
        fill = filler(start - len(HEADER) - reps * len(unit))
        rng = random.Random(13)
        body = b""
        while len(body) < 39:  # up to `block`: no '\r'
            t = rng.choice([b"x", b",", b"\n", b'""', b" y"])
            body += t if len(body) + len(t) <= 39 else b"x"
        while len(body) < 40 + seg + 200:
            # (plain bytes where the segment after `block` ends, so that no "" pair sits across it)
            near_end = abs(len(body) - (39 + seg)) <= 2
            if len(body) < 39 + seg // 2 + 16:  # to half a segment past `block`: no '"', no '\r' (see the cut there)
                body += rng.choice([b"x", b",", b"\n", b" y", b"line"])
            else:
                body += b"x" if near_end else rng.choice([b"x", b",", b"\n", b'""', b" y", b"\r\n", b"\r\n", b"\r", b"line"])
        special = b'S0,"' + body + b'",s2\n'
        return _finish([(fill, 1), (unit, reps), (special, 1), (tail, treps), (b'z9,"un""terminated" , tail', 1)],
                       special_at=2, close_quote=start + 4 + len(body))
    if name == "late":
        unit = record_unit(14, unit_bytes, skips=True)
        reps = (block + 64) // len(unit) + 1
        return _finish([(unit, reps), (b'late,"first ""quote""", cr\r\n', 1), (tail, treps), (b"end,of,file", 1)])
    raise ValueError(name)


# ---- wide records ---------------------------------------------------------------------------------------
_B36 = "0123456789abcdefghijklmnopqrstuvwxyz"


def _b36(i):
    s = ""
    while True:
        s = _B36[i % 36] + s
        i //= 36
        if not i:
            return s


@functools.lru_cache(maxsize=None)
def wide_csv(nlines, nfields, quoted, ragged):
    """(bytes, oracle rows) of a headed file of `nlines` lines of `nfields` fields with values of
    0-3 bytes (field 0: the line number in base 36, so every line is a kept record and a shifted
    row shows); every tenth line has ragged[...] fields instead, every seventh is all empty fields.
    quoted: one quoted field per 50 lines (the general passes); otherwise no '"' and no '\\r' (the
    classify path)."""
    rng = random.Random(nlines * 7919 + nfields + (1 if quoted else 0))
    vals = ["", "", "a", "bc", "def", " x", "7 ", "é", "0", "#"]
    lines = [",".join(f"h{i}" for i in range(nfields))]
    for i in range(nlines):
        if i % 10 == 0:
            f = [rng.choice(vals) for _ in range(ragged[(i // 10) % len(ragged)])]
            f[0] = _b36(i)
        elif i % 7 == 0:
            f = [""] * nfields
        else:
            f = [rng.choice(vals) for _ in range(nfields)]
            f[0] = _b36(i)
        if quoted and i % 50 == 25:
            j = rng.choice([0, 31, 63, 64, 65, nfields - 1, rng.randrange(nfields)]) % len(f)
            f[j] = '" q,""%d\n"' % i
        lines.append(",".join(f))
    data = ("\n".join(lines) + "\n").encode()
    return data, R.rows(data, COMMA, True)


# ---- small files for every cut ----------------------------------------------------------------------------
CUT_SAMPLES = [
    b'h1,h2,h3\r\n\r\n  \n#c,d\n" a "" b ",  x  ,1\r"q\nq",,2\n1,2,3\r\n"x\r\ny",z\n\n4,"5""",6\r7,8',
    # a quoted header holding a delimiter and a CRLF
    b'"na,me" , "b\r\n2",c\r\n1,"2\n" ,3\r\r\n"",x\n#no\n  \r"a""b",,\r\n9,"8\r"\r\n\n7',
    # blank and comment lines first: early cuts hold no kept record
    b'\n \t\r\n#c1\r#c2,x\n\r\r\nk,v\n#"q\n"\n  "a, b" ,1\r\n\n2,"u\r"\r3,4\n5,6 ,7',
]
CUT_FIELDS = [0, 1, 2, 3]


def has_kept_record(data):
    return any(R.kept(r) for r in R.split_records(data))


def host_record_end(prefix):
    """qe_csv_record_end with eof = 0 from the oracle: record_cut, except that a '\\r' at the very
    end does not count (a '\\n' may follow)."""
    cut = R.record_cut(prefix)
    return R.record_cut(prefix[:-1]) if cut == len(prefix) and prefix.endswith(b"\r") else cut


# ---- grammar fuzz ---------------------------------------------------------------------------------------------
ALPHABET = [b"a", b"b", b" ", b'"', b'"', b",", b",", b"\n", b"\n", b"\r", b"#", b"\t", "ä".encode(), b'""']
FUZZ_FIELDS = [0, 1, 2, 3]


@functools.lru_cache(maxsize=None)
def fuzz_cases(n=600, seed=2024):
    rng = random.Random(seed)
    return [b"".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 160))) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def fuzz_straddle_cases(n=150, seed=2025):
    """[(bytes, offset of the fuzzed part)]: 40-200 tokens of the alphabet behind plain lines, placed
    so that they straddle the first 16 KiB segment boundary."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        case = b"".join(rng.choice(ALPHABET) for _ in range(rng.randint(40, 200)))
        at = SEG - rng.randint(1, len(case) - 1)
        out.append((filler(at) + case, at))
    return out


def _quote_states(data):
    """Per byte: inside quotes (the state a terminator or delimiter at that byte would see)."""
    inq, st = False, []
    for c in data:
        if c == 0x22:
            inq = not inq
        st.append(inq)
    return st


def fuzz_traits(data):
    """Which of the grammar's corners a case reaches (test_fuzz_cases_are_not_trivial)."""
    st = _quote_states(data)
    recs = R.split_records(data)
    keep = [r for r in recs if R.kept(r)]
    raws = [R._trim(f) for r in keep for f in R.split_fields(r, COMMA)]
    wrapped = [v for v in raws if len(v) >= 2 and v[0] == 0x22 and v[-1] == 0x22]
    return {
        "terminator_in_quotes": any(st[i] and c in (0x0A, 0x0D) for i, c in enumerate(data)),
        "unclosed_quote": data.count(b'"') % 2 == 1,
        "skipped_record": len(keep) < len(recs),
        "lone_cr": any(c == 0x0D and not st[i] and data[i + 1:i + 2] != b"\n" for i, c in enumerate(data)),
        "two_records": len(keep) >= 2,
        "wrapped_value": bool(wrapped),
        "escaped_pair": any(b'""' in R._trim(v[1:-1]) for v in wrapped),
        "ragged_rows": len({len(R.split_fields(r, COMMA)) for r in keep}) > 1,
    }
