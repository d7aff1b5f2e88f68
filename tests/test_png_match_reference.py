"""The CPU statement of the PNG window matches (tests/png_match_reference.py) and its inputs (tests/png_match_cases.py), judged without a
GPU: the streams inflate to the filtered bytes, the files open to the canvas in both colour forms and with either row filter, no file
is larger than the default setting's, chunks that keep the run or the stored form are the default reference's bytes, every input
reaches the regime it was built for, every near miss of the rule changes some file, and rendered text shrinks to at most 75 per cent.
Reference anchor: wx.canvasToTempFilePath({fileType: 'png'}) (utils/canvas.js:205-242, pages/index/index.js:1577-1579) - a file that
decodes to the same pixels."""
import io
import zlib

import numpy as np
import pytest

from tests import png_deflate_reference as R
from tests import png_match_cases as K
from tests import png_match_reference as M

CASES = K.shape_cases()
NAMES = [n for n, _ in CASES]


def _bpp(a):
    return 3 if a.shape[1] == K.RGB_SHAPE[0] else 4


@pytest.mark.parametrize("name", NAMES)
def test_stream_inflates_and_file_opens_and_is_no_larger(name):
    from PIL import Image
    a = K.by_name()[name]
    forms = [(_bpp(a), False)] + ([(3, True), (4, True), (3, False)] if a.shape[:2] in ((70, 64), (12, 720)) else [])
    for bpp, adaptive in forms:
        rep = K.report(name, a, bpp, adaptive)
        run = M.encode_run(a, bpp, adaptive)
        assert zlib.decompressobj(-15).decompress(rep.stream[2:]) == rep.filtered == run.filtered, (name, bpp, adaptive)
        assert zlib.decompress(rep.stream) == rep.filtered
        im = Image.open(io.BytesIO(M.file_bytes_window(a, bpp, rep.stream, adaptive)))
        assert im.mode == ("RGB" if bpp == 3 else "RGBA") and np.array_equal(np.asarray(im), a[..., :bpp]), (name, bpp, adaptive)
        assert len(rep.stream) <= len(run.stream), (name, bpp, adaptive)
        assert len(rep.chunks) == len(run.chunks)
        at = 0
        for c, d in zip(rep.chunks, run.chunks):
            assert c.nbytes <= d.nbytes and c.offset == at
            if c.form != "window":                       # the run or the stored form: the default setting's chunk, byte for byte
                assert c.form == d.form and rep.stream[at:at + c.nbytes] == run.stream[d.offset:d.offset + d.nbytes], (name, bpp, adaptive)
            at += c.nbytes


def test_every_regime_is_reached_by_the_case_built_for_it():
    reached = {n: K.regimes(K.report(n, a, _bpp(a))) for n, a in CASES}
    want = {"match text 64x70": {"form window", "short last chunk", "distance slack rounds", "ragged last span", "cut by the span end"},
            "match text 720x12": {"form window", "short last chunk"},
            "match text over photo 720x12": {"run beside window"},
            "match text 4200x3": {"run beside window"},
            "match noise 64x70": {"form stored"}, "match noise 720x12": {"form stored"},
            "match flat 64x70": {"form huff"}, "match photo 720x12": {"form huff"},
            "match text|noise 64x70": {"form window", "hash collision"},
            "match one distance 1024x1": {"one distance symbol", "candidate at position 0", "capped at 63"},
            "match period 3 257x1": {"overlapping copy", "one distance symbol", "ragged last span"},
            "match period 67 300x1": {"cut by the span end", "hash collision"}}
    for name, regs in want.items():
        assert regs <= reached[name], (name, regs - reached[name])
    assert set().union(*reached.values()) == K.ALL_REGIMES
    for name in ("match text 1x1", "match text 3x1"):      # fewer than 4 bytes have no key; a chunk of one span has no earlier span
        a = K.by_name()[name]
        c = K.report(name, a).chunks[0]
        assert all(t.kind != M.WIN for t in c.win_tokens) and (M.candidates(c.data) == -1).all()
    assert len(M.hashes(np.zeros(3, np.uint8))) == 0 and len(M.hashes(np.zeros(4, np.uint8))) == 1
    single = K.report("match one distance 1024x1", K.by_name()["match one distance 1024x1"]).chunks[0]
    assert single.dist_symbols == [13] and single.dist_rounds == 0          # distance 128: symbol 13, length 1 without a round


@pytest.mark.parametrize("miss", sorted(M.NEAR_MISSES))
def test_the_inputs_tell_the_rule_from_a_near_miss(miss):
    rule = M.NEAR_MISSES[miss]
    changed = [n for n, a in CASES if M.encode_window(a, _bpp(a), False, rule).stream != K.report(n, a, _bpp(a)).stream]
    assert changed, miss
    for n in changed[:3]:                                   # a near miss is still a valid stream - only another one
        a = K.by_name()[n]
        bent = M.encode_window(a, _bpp(a), False, rule)
        assert zlib.decompress(bent.stream) == bent.filtered


def test_the_choice_keeps_the_default_chunk_unless_the_window_chunk_is_smaller():
    """chunks are compared with their lead bytes and pads; the inputs hold a tie, and a window body that is smaller but pads to more"""
    seen_tie = seen_pad = 0
    for n, a in CASES:
        for k, c in enumerate(K.report(n, a, _bpp(a)).chunks):
            lead = 2 if k == 0 else 0
            base = ("huff", c.huff_size) if c.huff_size is not None and c.huff_size < c.stored_size else ("stored", c.stored_size)
            if c.win_size is None:
                assert c.form == base[0]
                continue
            mine, theirs = M.padded(lead + c.win_size), M.padded(lead + base[1])
            assert c.form == ("window" if mine < theirs else base[0]), (n, k)
            assert c.nbytes == min(mine, theirs)
            seen_tie += mine == theirs
            seen_pad += c.win_size < base[1] and mine > theirs
    assert seen_tie >= 1 and seen_pad >= 1, (seen_tie, seen_pad)
    assert M.padded(234) == 304 and M.padded(236) == 256


def test_distance_symbols_follow_rfc_1951():
    assert [M.dist_code(d) for d in (1, 4, 5, 6, 7, 9, 12, 13, 128, 129, 8193, 12288, 12289, 16383)] == \
        [(0, 0, 0), (3, 0, 0), (4, 1, 0), (4, 1, 1), (5, 1, 0), (6, 2, 0), (6, 2, 3), (7, 2, 0), (13, 5, 31), (14, 6, 0), (26, 12, 0), (26, 12, 4095), (27, 12, 0), (27, 12, 4094)]
    assert len(M.DIST_BASE) == len(M.DIST_EXTRA) == M.NDIST


def test_rendered_text_shrinks_to_at_most_three_quarters():
    """the size gate: 720 x 360 RGBA, white with dark text in PIL's default font, vocabulary 300.  Measured with this rule: 59.3 per cent
    (110009 against 185401 bytes of zlib stream)."""
    a = K.rendered_text(1, 720, 360, 300)
    win, run = len(M.encode_window(a).stream), len(R.encode(a).stream)
    print("window %d bytes, run %d bytes, ratio %.1f %%" % (win, run, 100.0 * win / run))
    assert win <= 0.75 * run, (win, run)
