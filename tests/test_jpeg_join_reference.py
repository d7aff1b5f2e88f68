"""The join reference (tests/jpeg_join_reference.py) judged by a witness that knows nothing of it: Pillow (libjpeg-turbo) decodes
expected_file(...) and decodes the sources, and the joined picture must be the sources laid side by side.

4:4:4: equal at every pixel.  4:2:0: equal at every pixel except the one pixel row (vertical) or column (horizontal) on each side of
each seam - libjpeg's triangle chroma filter reaches one chroma sample across the seam, which is the neighbour image's in the joined
file and the image's own (replicated) edge in the source.  That exclusion is a cap, not a tolerance: at most 2 rows or columns per
seam and nothing else.  Found on the CPU for every case of the list, vertical and horizontal alike (the horizontal form needs no
other count: the filter is the same along x): 4:4:4 has no differing row or column at all, 4:2:0 differs in a subset of {s - 1, s}
per seam s.  CPU only."""
import pytest

from tests import jpeg_join_reference as JR
from tests.jpeg_writer import write_jpeg

pytest.importorskip("PIL")


@pytest.mark.parametrize("optimize", (False, True))
@pytest.mark.parametrize("name", JR.CASE_NAMES)
def test_the_joined_file_decodes_to_the_sources_side_by_side(name, optimize):
    _, layout, direction, _, _ = next(c for c in JR.CASES if c[0] == name)
    frames = JR.case_frames(name)
    differing, allowed = JR.witness_mismatch(JR.expected_file(frames, direction, optimize), [write_jpeg(f) for f in frames], direction, layout)
    assert set(differing) <= allowed, (name, differing, sorted(allowed))
    if layout == "444":
        assert differing == []


def test_the_issues_three_vertical_shapes_differ_in_exactly_the_seam_rows():
    """W = 40, heights (16, 32, 9); W = 16, heights (16, 16); W = 17, heights (48, 16, 1): 4:2:0 differs in exactly rows s - 1 and s"""
    for name in ("partial column and row 420", "one MCU each 420", "narrow, last row of one pixel 420"):
        frames = JR.case_frames(name)
        differing, allowed = JR.witness_mismatch(JR.expected_file(frames, "vertical"), [write_jpeg(f) for f in frames], "vertical", "420")
        assert set(differing) == allowed, (name, differing, sorted(allowed))


def test_the_joined_frame_keeps_every_source_block_where_the_rule_puts_it():
    import numpy as np
    for name in ("partial column and row 420", "horizontal 420", "horizontal 444"):
        _, layout, direction, _, _ = next(c for c in JR.CASES if c[0] == name)
        frames = JR.case_frames(name)
        J = JR.join(frames, direction)
        at = 0
        for f in frames:
            for cj, cf in zip(J.comps, f.comps):
                by, bx = cf["coef"].shape[:2]
                per = (cf["v"] if direction == "vertical" else cf["h"])
                o = at * per
                got = cj["coef"][o:o + by] if direction == "vertical" else cj["coef"][:, o:o + bx]
                assert np.array_equal(got, cf["coef"])
                assert np.array_equal(cj["q"], cf["q"])
            mcu = 16 if layout == "420" else 8
            at += -(-(f.height if direction == "vertical" else f.width) // mcu)
        assert (J.width, J.height) == ((frames[0].width, sum(f.height for f in frames)) if direction == "vertical"
                                       else (sum(f.width for f in frames), frames[0].height))
