"""The CSV scan (qe_csv.hip) where the random files of test_csv.py never go: the segment plan's
second block of 2048 segments on the classify path and the general one, records of up to 1,024
fields, QE_CSV_PARTIAL_TAIL at every cut of small files, and byte strings over a hostile alphabet
(the grammar of oracle/csv_ref.py defines a result for every one). The CPU tests assert what each
input must hold for its GPU test to mean something; inputs and expected values are in csvcases.py.

What would fail if the kernels were wrong in these ways (traced by reading, nothing was broken to
check):
  k_csv_seg_apply reading t[0] / last[0] whatever the parity P of the earlier blocks' quotes:
      second_segment_block[straddle] — block 0 ends inside the field (P = 1), so the line count
      (row count assertion) and, at the cut, `consumed == start` (last[0] is a '\n' inside the field);
  the earlier blocks' flags not ORed in: second_segment_block[straddle] at the cut — the chunk's only
      '"' bytes are in block 0, the scan would stay on the classify path (row count, consumed);
      [late] holds the other half, a flag set only in the last block;
  `last` not carried from earlier blocks: second_segment_block[straddle] at the cut — block 1 has
      no terminator outside quotes, `consumed` would be 0;
  record_field applying low_mask to fields >= 64: 100_fields[*-64], [*-99], 1100_fields ([1023]) —
      the column comes back empty (offsets differ at entry 1);
  nth_delim always selecting from d0: 100_fields[general-*] — a wanted delimiter in bytes 8-15 of its
      chunk (test_wide_files_meet_their_conditions checks there are such) gives wrong value bounds;
  consumed = nbytes under QE_CSV_PARTIAL_TAIL: every_cut at the first k that is not a record end,
      and both cuts of second_segment_block."""
import numpy as np
import pytest

import csvcases as K
from oracle import csv_ref as R
from test_csv import _gpu_scan

COMMA = K.COMMA
SEG_FILES = ["plain", "straddle", "late"]
ALL5 = list(range(K.NCOLS))


# ---- CPU: the oracle's additions ----------------------------------------------------------------------
def test_record_cut_by_hand():
    for data, want in [(b"", 0), (b"a\r", 2), (b"a\r\nb", 3), (b'"a\n', 0), (b'x\n"a\n', 2), (b"a\r\n", 3),
                       (b"a\rb\r\n\r", 6), (b'"\r\n"\n"\n', 5), (b"no terminator", 0)]:
        assert R.record_cut(data) == want, data


def test_rows_is_parse_with_the_delimiter_given():
    data = b'h1,h2\r\n\r\n  \n#c,d\n" a "" b ",  x  \r"q\nq",\n1,2,3\n4'
    assert R.rows(data, COMMA, True) == R.parse(data)[2]
    assert R.rows(data, COMMA, False) == R.parse(data, False)[2]
    assert R.rows(b"a;b,c\n1;2,3", ord(";"), True) == [[b"1", b"2,3"]]  # (parse() would detect ',')
    assert R.rows(b"", COMMA, True) == [] and R.rows(b"\n#x\n", COMMA, False) == []


# ---- A: two blocks of the segment plan ------------------------------------------------------------------
@pytest.mark.parametrize("name", SEG_FILES)
def test_piecewise_expectation_equals_one_oracle_parse(name):
    """What the 33 MiB files rest on: for '\\n'-terminated, quote-balanced pieces the rows of
    header + pieces are the pieces' own rows in order — here on a small instance of each
    construction (8 KiB 'block', 512-byte 'segment'), which the oracle parses whole."""
    f = K.seg_file(name, block=8192, seg=512, unit_bytes=2048, tail_bytes=4096)
    rows = R.rows(f.data, COMMA, True)
    assert rows == [r for piece, n in f.pieces for r in piece * n]
    assert len(f.pieces) >= 3 and any(n >= 2 for _, n in f.pieces) and len(f.data) > 8192 + 512
    # and the array form the GPU tests compare with
    want = K.piece_columns(f.pieces, ALL5)
    direct = K.project_rows(rows, ALL5)
    for c, col in enumerate(want):
        assert col.values.tobytes() == b"".join(r[c] for r in direct)
        assert list(np.diff(col.offsets)) == [len(r[c]) for r in direct]
    if name == "straddle":
        assert R.record_cut(f.data[:8192 + 256]) == f.special_start
        assert R.rows(f.data[:f.special_start], COMMA, True) == rows[:f.rows_before_special]
        assert f.data[f.close_quote] == 0x22 and f.close_quote > 8192 + 512


@pytest.mark.parametrize("name", SEG_FILES)
def test_segment_block_files_meet_their_conditions(name):
    B = K.BLOCK
    assert B == 2048 * 16384
    f = K.seg_file(name)
    data = f.data
    assert len(data) > B + 16384 and len(data) < B + (2 << 20)
    assert sum(len(rows) * n for rows, n in f.pieces) > 100_000
    if name == "plain":
        assert data.count(b'"') == 0 and data.count(b"\r") == 0
        assert data[B - 1] != 0x0A and data[B] != 0x0A  # a record straddles B
        assert data[-1] != 0x0A
        # no skipped line (header + rows = lines): the bitmap line walk's rows are the result
        assert 1 + sum(len(rows) * n for rows, n in f.pieces) == data.count(b"\n") + 1
    elif name == "straddle":
        assert data.count(b'"', 0, B) % 2 == 1 and data.find(b"\r", 0, B) == -1
        assert data[f.close_quote] == 0x22 and f.close_quote > B + 16384
        opening = f.special_start + 3
        assert data[opening] == 0x22 and opening <= B - 16 and data[f.special_start - 1] == 0x0A
        field = data[opening + 1:f.close_quote]
        assert field.count(b'"') % 2 == 0 and all(t in field for t in (b"\n", b"\r\n", b",", b'""'))
        # a chunk cut at B + 8192 has no '"' and no '\r' in its block 1 (the flags come from block 0
        # alone), and terminator bytes there, all inside the field
        assert data.count(b'"', B, B + 8192) == 0 and data.find(b"\r", 0, B + 8192) == -1
        assert data.count(b"\n", B, B + 8192) > 100
        assert data[opening + 1:B].count(b'"') % 2 == 0  # segment 2048 starts inside the field ...
        assert data[opening + 1:B + 16384].count(b'"') % 2 == 0  # ... and ends inside it
        assert data.find(b"\r\n", f.close_quote) > 0 and data[-1] not in (0x0A, 0x0D)
    else:
        assert data.find(b'"', 0, B) == -1 and data.find(b"\r", 0, B) == -1
        assert data.find(b'"', B) > 0 and data.find(b"\r", B) > 0
        assert 0 < data.find(b"\n#") < B and 0 < data.find(b"\n\n") < B  # the kept-line path


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEG_FILES)
def test_gpu_csv_second_segment_block(gpu_ctx, name):
    """2049+ segments: k_csv_seg_reduce / k_csv_seg_apply carry quote parity, terminator counts, the
    last terminator and the '"' / '\\r' flags from block 0 into block 1."""
    B = K.BLOCK
    f = K.seg_file(name)
    want = K.piece_columns(f.pieces, ALL5)
    nrows = len(want[0].offsets) - 1
    dev = K.upload(gpu_ctx, f.data)
    got, consumed = K.parse_bytes(gpu_ctx, dev, COMMA, True, ALL5)
    assert consumed == len(f.data)
    assert len(got[0].offsets) - 1 == nrows
    K.assert_columns(got, want, name)
    for c in (0, K.NCOLS - 1):
        got1, _ = K.parse_bytes(gpu_ctx, dev, COMMA, True, [c])
        K.assert_columns(got1, [want[c]], f"{name} [{c}]")
    if name == "late":
        return
    # a chunk cut 8 KiB into block 1
    cut = B + 8192
    if name == "plain":
        start = f.data.rfind(b"\n", 0, cut) + 1
        n = f.data.count(b"\n", 0, start) - 1  # every line a record; less the header
    else:  # inside the quoted field: block 1 then holds only in-quote terminators
        assert f.special_start < B < cut < f.close_quote
        start, n = f.special_start, f.rows_before_special
    got, consumed = K.parse_bytes(gpu_ctx, dev[:cut], COMMA, True, ALL5, partial=True)
    assert consumed == start
    K.assert_columns(got, K.head_columns(want, n), f"{name} cut")


# ---- B: wide records ----------------------------------------------------------------------------------------
RAGGED100 = (1, 63, 64, 65, 99)
RAGGED1100 = (1000, 1023, 1024, 1025)
PROJ100 = [[0], [63], [64], [63, 64, 65], [99], [0, 31, 32, 99], list(range(100)), [99, 0]]


@pytest.mark.parametrize("quoted", [False, True])
def test_wide_files_meet_their_conditions(quoted):
    for nlines, nfields, ragged in [(3000, 100, RAGGED100), (200, 1100, RAGGED1100)]:
        data, rows = K.wide_csv(nlines, nfields, quoted, ragged)
        assert len(rows) == nlines  # every line a record
        assert ((b'"' in data) == quoted) and b"\r" not in data
        counts = {len(r) for r in rows}
        assert counts == set(ragged) | {nfields}
        if nfields == 100:
            assert len(data) > 20 * 8192 and any(r == [b""] * 100 for r in rows)  # many 8 KiB line blocks
            assert max(len(v) for r in rows for v in r) <= (3 if not quoted else 16)
        if nfields == 100:
            # the delimiter that ends field 64 falls in both halves of its 16-byte chunk (quote-free lines)
            at, halves = 0, set()
            for ln in data.split(b"\n"):
                commas = [i for i, c in enumerate(ln) if c == COMMA]
                if len(commas) > 64 and b'"' not in ln:
                    halves.add((at + commas[64]) % 16 >= 8)
                at += len(ln) + 1
            assert halves == {False, True}
        if quoted:
            assert sum(1 for r in rows for v in r if b"q," in v) == nlines // 50


@pytest.mark.gpu
@pytest.mark.parametrize("fields", PROJ100, ids=lambda p: "all" if len(p) == 100 else "-".join(map(str, p)))
@pytest.mark.parametrize("quoted", [False, True], ids=["classify", "general"])
def test_gpu_csv_100_fields(gpu_ctx, quoted, fields):
    """Field indices on both sides of the 64-bit low_mask, several fields ending in one 16-byte
    chunk / one bitmap word, ragged lines that stop at fields 1, 63, 64, 65 and 99."""
    data, rows = K.wide_csv(3000, 100, quoted, RAGGED100)
    got, consumed = K.parse_bytes(gpu_ctx, data, COMMA, True, fields)
    assert consumed == len(data)
    K.assert_columns(got, K.piece_columns([(rows, 1)], fields), f"fields {fields}")


@pytest.mark.gpu
@pytest.mark.parametrize("quoted", [False, True], ids=["classify", "general"])
def test_gpu_csv_1100_fields(gpu_ctx, quoted):
    from kquery import native as N

    data, rows = K.wide_csv(200, 1100, quoted, RAGGED1100)
    dev = K.upload(gpu_ctx, data)
    for fields in ([1023], [0, 1023]):
        got, _ = K.parse_bytes(gpu_ctx, dev, COMMA, True, fields)
        K.assert_columns(got, K.piece_columns([(rows, 1)], fields), f"fields {fields}")
    with pytest.raises(N.IllegalStateException, match="out of range"):
        K.parse_bytes(gpu_ctx, dev, COMMA, True, [1024])
    with pytest.raises(N.IllegalArgumentException, match="twice"):
        K.parse_bytes(gpu_ctx, dev, COMMA, True, [5, 7, 5])


@pytest.mark.gpu
@pytest.mark.parametrize("quoted", [False, True], ids=["classify", "general"])
def test_gpu_csv_40_columns_by_name(gpu_ctx, tmp_path, quoted):
    """CsvDataSource's schema and name projection past its 32-field calls."""
    data, rows = K.wide_csv(300, 40, quoted, (1, 32, 33, 39))
    names, _, cols, _ = _gpu_scan(gpu_ctx, tmp_path, data)
    assert names == [f"h{i}" for i in range(40)] == R.parse(data)[0]
    assert cols == R.project(rows, range(40))
    _, _, cols, _ = _gpu_scan(gpu_ctx, tmp_path, data, ["h32", "h39"])
    assert cols == R.project(rows, [32, 39])


# ---- C: every cut of a small file -----------------------------------------------------------------------------
def _cuts(data):
    return range(len(data) + 1)


def test_cut_samples_meet_their_conditions():
    a, b, c = K.CUT_SAMPLES
    assert len(a) == 78 and all(len(s) < 300 for s in K.CUT_SAMPLES)
    assert R.split_fields(R.split_records(b)[0], COMMA)[1].count(b"\r\n") == 1  # a quoted header over two lines
    early = [k for k in _cuts(c) if R.record_cut(c[:k]) > 0 and not K.has_kept_record(c[:R.record_cut(c[:k])])]
    assert len(early) >= 10 and K.has_kept_record(c)
    for s in K.CUT_SAMPLES:
        st = K._quote_states(s)
        assert any(st[k] for k in range(len(s)))  # cuts inside a quoted field
        assert any(s[k - 1:k + 1] == b"\r\n" and not st[k] for k in range(1, len(s)))  # between '\r' and '\n'
        assert len(R.rows(s, COMMA, True)) >= 4 and max(len(r) for r in R.rows(s, COMMA, True)) <= 3


@pytest.mark.parametrize("sample", range(len(K.CUT_SAMPLES)))
def test_oracle_rows_concatenate_at_every_cut(sample):
    """Chunked parsing on the oracle alone: the rows up to record_cut of a prefix, then the rows of
    the rest (headed only if no kept record came before), are the rows of one parse — at value level,
    the cut between '\\r' and '\\n' included."""
    data = K.CUT_SAMPLES[sample]
    whole = R.rows(data, COMMA, True)
    for k in _cuts(data):
        cut = R.record_cut(data[:k])
        assert cut <= k and (cut == 0 or data[cut - 1] in (0x0A, 0x0D))
        first = R.rows(data[:cut], COMMA, True)
        rest = R.rows(data[cut:], COMMA, not K.has_kept_record(data[:cut]))
        assert first + rest == whole, k


@pytest.mark.gpu
@pytest.mark.parametrize("sample", range(len(K.CUT_SAMPLES)))
def test_gpu_csv_every_cut(gpu_ctx, sample):
    data = K.CUT_SAMPLES[sample]
    whole = K.project_rows(R.rows(data, COMMA, True), K.CUT_FIELDS)
    for k in _cuts(data):
        cols, consumed = K.parse_bytes(gpu_ctx, data[:k], COMMA, True, K.CUT_FIELDS, partial=True)
        assert consumed == R.record_cut(data[:k]), k
        first = K.device_rows(cols)
        assert first == K.project_rows(R.rows(data[:consumed], COMMA, True), K.CUT_FIELDS), k
        if consumed > 0:
            cols, used = K.parse_bytes(gpu_ctx, data[consumed:], COMMA, not K.has_kept_record(data[:consumed]),
                                       K.CUT_FIELDS)
            assert used == len(data) - consumed
            assert first + K.device_rows(cols) == whole, k


def test_host_record_end_at_every_cut():
    """qe_csv_record_end is host code: the library loads and the call runs without a GPU."""
    from kquery import native as N

    assert K.host_record_end(b"a\r") == 0 and K.host_record_end(b"a\r\r") == 2 and K.host_record_end(b'"\r') == 0
    for data in K.CUT_SAMPLES:
        buf = (N.C.c_uint8 * max(1, len(data))).from_buffer_copy(data)
        for k in _cuts(data):
            cut = N.C.c_int64(-1)
            N.check(N.lib().qe_csv_record_end(buf, k, 0, N.C.byref(cut)))
            assert cut.value == K.host_record_end(data[:k]), k
            N.check(N.lib().qe_csv_record_end(buf, k, 1, N.C.byref(cut)))
            assert cut.value == k


# ---- D: grammar fuzz ---------------------------------------------------------------------------------------------
def test_fuzz_cases_are_not_trivial():
    cases = K.fuzz_cases()
    assert len(cases) == 600 and len(set(cases)) > 590
    traits = [K.fuzz_traits(c) for c in cases]
    shares = {t: sum(x[t] for x in traits) / len(cases) for t in traits[0]}
    print(shares)
    assert len(shares) == 8
    for t, share in shares.items():
        assert share >= 0.30, (t, share)


def test_fuzz_straddle_cases_cross_the_first_segment_boundary():
    cases = K.fuzz_straddle_cases()
    assert len(cases) == 150
    for data, at in cases:
        head, case = data[:at], data[at:]
        assert at < K.SEG < len(data) and 40 <= len(case)
        assert b'"' not in head and b"\r" not in head and head.endswith(b"\n")
        assert any(c in case for c in (b'"', b"\r"))


# what well-formed random files never hold, one case each with a hand-written answer (no header)
NAMED_CASES = [
    (b'x,a"b,c"d,y\n', [[b"x", b'a"b,c"d', b"y"]]),  # stray quotes mid-field hide a delimiter
    (b'"a"x,1\n', [[b'"a"x', b"1"]]),  # not wrapped: the quotes stay
    (b'"a" \t,1\n', [[b"a", b"1"]]),  # a quoted field followed by blanks
    (b'1,"open\n2,3\n4,5', [[b"1", b'"open\n2,3\n4,5']]),  # an unclosed quote swallows the later lines
    (b"  #x,1\n#y\n \t\n", [[b"#x", b"1"]]),  # '#' after blanks is no comment
    (b"a\rb\r\nc\r\rd\n", [[b"a"], [b"b"], [b"c"], [b"d"]]),  # lone '\r' next to '\r\n'
]


def test_named_grammar_cases_on_the_oracle():
    for data, want in NAMED_CASES:
        assert R.rows(data, COMMA, False) == want, data


@pytest.mark.gpu
def test_gpu_csv_named_grammar_cases(gpu_ctx):
    for data, _ in NAMED_CASES:
        _fuzz_check(gpu_ctx, data)


def _fuzz_check(ctx, data):
    want = K.project_rows(R.rows(data, COMMA, False), K.FUZZ_FIELDS)
    for has_header in (False, True):
        cols, consumed = K.parse_bytes(ctx, data, COMMA, has_header, K.FUZZ_FIELDS)
        assert consumed == len(data)
        # (rows() with a header is rows() without one less the first kept record: one oracle pass)
        assert K.device_rows(cols) == want[1 if has_header else 0:], (data, has_header)


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(6))
def test_gpu_csv_fuzz(gpu_ctx, part):
    """Stray quotes mid-field, '"a"x', blanks after a closing quote, unclosed quotes that swallow the
    lines after them, '#' after blanks, lone '\\r' beside '\\r\\n': one parse per case."""
    for data in K.fuzz_cases()[part * 100:(part + 1) * 100]:
        _fuzz_check(gpu_ctx, data)


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(3))
def test_gpu_csv_fuzz_across_a_segment_boundary(gpu_ctx, part):
    for data, _ in K.fuzz_straddle_cases()[part * 50:(part + 1) * 50]:
        _fuzz_check(gpu_ctx, data)
