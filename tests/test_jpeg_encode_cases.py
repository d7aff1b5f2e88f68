"""The cases of tests/jpeg_encode_cases.py, judged on the CPU: for each layout and kind of table the union of what they reach is exactly
the set written out here, so a case that stops reaching its regime (a changed generator, a changed table rule) fails this test and not
silently the strength of tests/test_gpu_jpeg_encode_regimes.py.  PIL decodes every reference file."""
import io

import numpy as np
import pytest

from tests import jpeg_encode_cases as JC

EXPECTED_444 = {
    "several batches", "partial byte carried", "batch ends on a byte", "0xFF completed from carried bits",
    "0xFF last whole byte of a batch", "padded last byte is 0xFF", "unpadded last byte is 0xFF", "interval ends without padding",
    "full last batch", "two-block last batch", "one-block last batch", "single batch of 255 blocks", "span 4", "span 8",
    "span above 8", "idle threads in the stuffing", "0xFF at the start of a thread's span", "0xFF at the end of a thread's span",
    "part of exactly 128 blocks", "part of one block", "part whose last wave step is partial", "DC predictor read across a part edge",
    "run of 16..31", "run of 32..47", "run of 48..62", "coefficient 63 set (no EOB)", "block of zeros only", "DC size 11"}
# 4:2:0: an interval has 6 m blocks, an even number: never 1 or 255 modulo 256, never 1 modulo 128.  'part of one block' is left out for
# that reason and not after a search: no input can reach it.
EXPECTED_420 = {
    "several batches", "partial byte carried", "batch ends on a byte", "0xFF completed from carried bits",
    "0xFF last whole byte of a batch", "padded last byte is 0xFF", "unpadded last byte is 0xFF", "interval ends without padding",
    "full last batch", "two-block last batch", "span 4", "span 8",
    "span above 8", "idle threads in the stuffing", "0xFF at the start of a thread's span", "0xFF at the end of a thread's span",
    "part of exactly 128 blocks", "part whose last wave step is partial", "DC predictor read across a part edge",
    "run of 16..31", "run of 32..47", "run of 48..62", "coefficient 63 set (no EOB)", "block of zeros only", "DC size 11"}
EXPECTED = {"444": EXPECTED_444, "420": EXPECTED_420}
COMBINATIONS = [(layout, tables) for layout in ("444", "420") for tables in ("std", "optimal")]


def test_the_expected_sets_are_the_modules_names():
    assert EXPECTED_444 == JC.ALL_REGIMES and len(JC.ENTROPY_REGIMES + JC.HISTOGRAM_REGIMES) == len(JC.ALL_REGIMES) == 28
    assert EXPECTED_420 == JC.ALL_REGIMES - JC.ONLY_444


@pytest.mark.parametrize("layout,tables", COMBINATIONS)
def test_the_cases_reach_exactly_the_expected_regimes(layout, tables):
    union, names = set(), set()
    for name, a, quality in JC.cases(layout):
        assert a.dtype == np.uint8 and a.shape[0] == (16 if layout == "420" else 8) and a.shape[1] <= 2048 and a.shape[2] == 4, name
        assert name not in names
        names.add(name)
        union |= JC.regimes(a, quality, layout, tables)
    assert union == EXPECTED[layout], (sorted(EXPECTED[layout] - union), sorted(union - EXPECTED[layout]))


@pytest.mark.parametrize("layout,tables", COMBINATIONS)
def test_each_directed_case_reaches_what_it_was_searched_for(layout, tables):
    target = {"seam": "0xFF last whole byte of a batch", "end": "unpadded last byte is 0xFF"}
    found = 0
    for name, a, quality in JC.cases(layout):
        for kind in target:
            if name == "directed %s for %s tables" % (kind, tables):
                found += 1
                assert target[kind] in JC.regimes(a, quality, layout, tables), name
                if kind == "end":           # ... and the file says the same: a stuffed 0xFF directly in front of EOI
                    assert JC.reference(a, quality, layout, tables).endswith(b"\xff\x00\xff\xd9"), name
    assert found == 2


def test_the_restated_loops_agree_with_the_file():
    """regimes() walks the unstuffed stream in batches; the bytes it walks, stuffed, are the file's scan"""
    from tests import jpeg_writer as JW
    from tests.test_jpeg_optimize_abi import header_length
    for layout, tables in COMBINATIONS:
        for name, a, quality in JC.cases(layout):
            data, tr = JC.coded(a, quality, layout, tables)
            stream = JW._pack_bits(tr["codes"], tr["lens"])
            assert len(tr["block"]) == len(tr["codes"]) == len(tr["lens"]) and np.all(np.diff(tr["block"]) >= 0), name
            assert bytes(stream).replace(b"\xff", b"\xff\x00") == data[header_length(data):-2], (name, layout, tables)
            c = JC.counts(a, quality, layout)
            blocks = int(tr["block"][-1]) + 1
            assert c[:16].sum() + c[272:288].sum() == blocks and c.sum() == int((tr["comp"] >= 0).sum()), name


@pytest.mark.parametrize("layout,tables", COMBINATIONS)
def test_pil_decodes_every_reference_file(layout, tables):
    """also the files with a 0x00 directly in front of a marker: it is what libjpeg expects"""
    from PIL import Image
    for name, a, quality in JC.cases(layout):
        im = Image.open(io.BytesIO(JC.reference(a, quality, layout, tables)))
        im.load()
        assert im.size == (a.shape[1], a.shape[0]) and im.mode == "RGB", name
