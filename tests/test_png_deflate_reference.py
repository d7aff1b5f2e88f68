"""The CPU statement of the compressing PNG export (tests/png_deflate_reference.py) must be right before it judges the kernel
(tests/test_gpu_png_stream.py): zlib inflates its streams to the Paeth-filtered canvas, the product's own decoder and PIL read its
files, its code rule is the one tools/sim_code_lengths.py states, and every input of the GPU tests reaches the regime it was built
for - shown by mutating the reference: a near miss of the design (matches off, a wrong tie, ...) still gives a valid stream, and it
must give OTHER bytes on at least one input of the group that covers the regime, or that group tests nothing."""
import io
import os
import sys
import zlib

import numpy as np
import pytest

import imagestitching_amd as ist
from tests import png_deflate_reference as R
from tests import png_stream_cases as C
from tests.test_png_code_rule import _histograms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sim_code_lengths as S  # noqa: E402

GROUPS = {"grid": C.grid_cases, "runs": C.runs_cases, "boundary": C.boundary_cases, "pads": C.pad_cases, "code": C.code_cases,
          "slabs": lambda: [C.slab_case()], "limit": lambda: [C.limit_case()]}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_streams_inflate_and_files_decode(group):
    from PIL import Image
    for name, a in GROUPS[group]():
        rep = C.report(name, a)
        h, w = a.shape[:2]
        assert rep.filtered == R.filtered_rows(a).tobytes() and len(rep.filtered) == h * (4 * w + 1), name
        assert zlib.decompress(rep.stream) == rep.filtered, name
        assert sum(c.nbytes for c in rep.chunks) + 9 == len(rep.stream) and all(c.nbytes % 16 == 0 for c in rep.chunks), name
        png = R.file_bytes(a, rep.stream)
        assert png.index(b"IDAT") + 4 == 64, name
        assert np.array_equal(ist.decode_png(png), a), name
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGBA")), a), name


def test_paeth_filter_against_a_scalar_statement():
    """PNG specification 9.4, pixel by pixel, on a small translucent canvas"""
    a = C.noise(3, 7, 9)
    a[2:4, 3:6] = a[1, 2]                                           # some ties
    want = bytearray()
    for y in range(7):
        want.append(4)
        for x in range(9):
            for ch in range(4):
                left = int(a[y, x - 1, ch]) if x else 0
                up = int(a[y - 1, x, ch]) if y else 0
                ul = int(a[y - 1, x - 1, ch]) if x and y else 0
                p = left + up - ul
                pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
                pred = left if pa <= pb and pa <= pc else (up if pb <= pc else ul)
                want.append((int(a[y, x, ch]) - pred) & 255)
    assert R.filtered_rows(a).tobytes() == bytes(want)


def test_length_rule_is_the_one_sim_code_lengths_states():
    """one rule, stated twice (integer arithmetic here, floating-point log2 there): equal lengths and rounds on every histogram
    of test_png_code_rule.py"""
    for counts in _histograms(1500, 5):
        length, rounds = R.code_lengths(counts)
        want, want_rounds = S.shannon_complete(counts)
        assert want is not None and length is not None
        assert {s: l for s, l in enumerate(length) if l} == want and rounds == want_rounds, counts


def test_sim_code_lengths_tokenises_as_the_reference_does():
    rows = [np.frombuffer(C.report(name, a).filtered, np.uint8) for name, a in C.runs_cases()]
    rows += [R.filtered_rows(C.photo_like(5, 3, 300))[2], R.filtered_rows(C.flat_with_lines(6, 4, 2000))[1]]
    for row in rows:
        assert S.tokens(row) == [R.symbol_of(int(t)) for t in R.tokenise(row)] + [256]


def test_length_symbols_are_rfc_1951s():
    """the reference's table (the standard's base lengths and extra-bit counts, written out) against the closed form the kernel's
    len_code and tools/sim_code_lengths.py use: symbol, extra-bit count and value of every length"""
    for n in range(3, 259):
        sym, eb, ev = R.LENGTH[n]
        if n == 258:
            assert (sym, eb, ev) == (285, 0, 0)
        elif n < 11:
            assert (sym, eb, ev) == (254 + n, 0, 0)
        else:
            e = (n - 3).bit_length() - 3
            assert (sym, eb, ev) == (257 + 4 * (e + 1) + (((n - 3) >> e) & 3), e, (n - 3) & ((1 << e) - 1))
    assert [S.length_symbol(n) for n in range(3, 64)] == [R.LENGTH[n][0] for n in range(3, 64)]


def test_inputs_reach_their_regimes():
    C.check_grid_regimes()
    C.check_runs_regimes()
    C.check_boundary_regimes()
    C.check_code_regimes()
    C.check_slab_regimes()
    C.check_pad_regimes()


def test_idat_layout_rule():
    assert R.idat_limit(None) == 1 << 30 and R.idat_limit("4095") == 1 << 30 and R.idat_limit("4097") == 4096 and R.idat_limit("65536") == 65536
    assert R.idat_lengths([160, 160, 160]) == [489]
    assert R.idat_lengths([4080, 16, 16], limit=4096) == [4080, 41]          # 4080 + 16 + 9 > 4096: the second chunk opens an IDAT
    assert R.idat_lengths([4064, 16, 16], limit=4096) == [4080, 25]          # (4064 + 16 + 9 <= 4096)
    assert R.idat_lengths([8000, 16], limit=4096) == [8000, 25]              # a chunk larger than the limit stands alone
    assert R.idat_lengths([16] * 5, slabs=[3, 2]) == [48, 41]
    assert R.host_slabs(1) == [1] and R.host_slabs(768) == [768] and R.host_slabs(5000) == [768, 4096, 136]


# ---- discriminating power: each near miss of the design against the group of inputs that covers its regime ---------------------
MUTATIONS = {
    "matches off": (R.RULES._replace(matches=False), "runs", "all-zero 64 px row"),
    "minimum run 5 instead of 4": (R.RULES._replace(min_run=5), "runs", "runs of 3 and of 4"),
    "runs across a span boundary": (R.RULES._replace(cross_span=True), "runs", "runs through span boundaries"),
    "stored / Huffman tie flipped": (R.RULES._replace(tie_stored=False), "boundary", "boundary tie 0, chunk 1"),
    "slack handed back in reverse symbol order": (R.RULES._replace(slack_reverse=True), "code", "many equal counts"),
    "one extra pad block": (R.RULES._replace(extra_pads=1), "pads", "pads 0"),
    "grid switches to pieces one pixel late": (R.RULES._replace(grid_late=True), "grid", "grid photo 4096x2"),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_inputs_tell_the_design_from_a_near_miss(mutation):
    rules, group, must_differ = MUTATIONS[mutation]
    differ = []
    for name, a in GROUPS[group]():
        true = C.report(name, a)
        bent = R.encode(a, rules)
        assert zlib.decompress(bent.stream) == true.filtered, name       # still a valid stream of the same bytes ...
        if bent.stream != true.stream:
            differ.append(name)
    assert must_differ in differ, differ                                  # ... and other bytes where the regime is reached
    if group == "boundary":
        assert all("tie" in name for name in differ), differ               # (one byte smaller: Huffman either way)
    if group == "grid":
        assert all("4096x2" in name for name in differ), differ            # (only the first width of the pieces regime moves)


def test_a_minimum_run_of_3_cannot_be_written_and_is_seen():
    """A run of 3 as literal + match would be a match of 2 bytes, which deflate has no symbol for: this near miss has no valid
    stream to compare (its decodable neighbour, a minimum of 5, is among the mutations above).  What it does to the tokens is
    still visible on the runs inputs, and the reference refuses to write them."""
    rules = R.RULES._replace(min_run=3)
    name, a = [c for c in C.runs_cases() if c[0] == "runs of 3 and of 4"][0]
    data = C.report(name, a).chunks[0].data
    bent = R.tokenise(data, rules)
    assert R.MATCH + 2 in bent.tolist() and bent.tolist() != C.report(name, a).chunks[0].tokens.tolist()
    with pytest.raises(KeyError):
        R.encode(a, rules)
