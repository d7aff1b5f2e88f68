"""The numpy restatement of the overlap contract (tests/overlap_reference.py) recovers the true header, footer and overlap of synthetic
scrolled screenshots.  CPU only; the GPU and the C rules are held to this reference in test_gpu_overlap.py and test_overlap_abi.py."""
import numpy as np
import pytest

from tests import overlap_reference as R

HEADER, FOOTER, BODY, W = 44, 50, 546, 360


def _hfk(p):
    return (p["header"], p["footer"], p["overlap"])


@pytest.mark.parametrize("noise", [0, 2])
@pytest.mark.parametrize("step", [100, 333, 530, 546, 600])
def test_scroll_steps_give_back_the_true_bars_and_overlap(step, noise):
    shots = R.synth_shots(W, HEADER, FOOTER, [BODY, BODY], [0, step], seed=step, noise=noise)
    want = R.truth(HEADER, FOOTER, [BODY, BODY], [0, step])[0]
    assert want[2] == (BODY - step if BODY - step >= 16 else 0)
    p = R.pair(*shots)
    assert _hfk(p) == want
    assert p["cost"] <= 8 * W * p["overlap"]                  # (0 without an overlap)


@pytest.mark.parametrize("noise", [0, 2])
def test_an_overlap_of_min_rows_is_found_and_one_row_less_is_not(noise):
    for step, k in ((BODY - 16, 16), (BODY - 15, 0)):
        shots = R.synth_shots(W, HEADER, FOOTER, [BODY, BODY], [0, step], seed=7, noise=noise)
        assert _hfk(R.pair(*shots)) == (HEADER, FOOTER, k)
    shots = R.synth_shots(W, HEADER, FOOTER, [BODY, BODY], [0, BODY - 15], seed=7, noise=noise)
    assert _hfk(R.pair(*shots, min_rows=15)) == (HEADER, FOOTER, 15)


def test_a_blank_pair_has_no_overlap():
    blank = np.full((90, 64, 4), 255, np.uint8)
    p = R.pair(blank, blank)
    assert p["overlap"] == 0 and p["cost"] == 0
    assert p["header"] == 45 and p["footer"] == 45          # every row matches: the bars take the whole search range


def test_rows_without_information_do_not_make_an_overlap():
    # bodies of one flat colour under real bars: every k costs nothing, and none has eight informative rows
    shots = R.synth_shots(64, 6, 5, [60, 60], [0, 30], seed=3, indicator=False)
    for s in shots:
        s[6:66] = 200
    p = R.pair(*shots)
    assert p["overlap"] == 0


def test_unequal_widths_give_nothing():
    a = R.synth_shots(64, 6, 5, [40], [0], seed=1)[0]
    b = R.synth_shots(65, 6, 5, [40], [0], seed=1)[0]
    assert R.pair(a, b) == {"header": 0, "footer": 0, "overlap": 0, "cost": 0}


@pytest.mark.parametrize("w", [5, 31, 33, 64, 130])
def test_narrow_widths_and_unequal_heights(w):
    bodies, offsets = [40, 60, 50], [0, 20, 45]
    shots = R.synth_shots(w, 6, 5, bodies, offsets, seed=w)
    assert len({s.shape[0] for s in shots}) == 3
    got = [_hfk(p) for p in R.find_overlaps(shots)]
    assert got == R.truth(6, 5, bodies, offsets) == [(6, 5, 20), (6, 5, 35)]


def test_signature_cells_cover_every_pixel_once():
    for w in (1, 5, 31, 32, 33, 100, 1170):
        img = np.random.default_rng(w).integers(0, 256, (3, w, 4), dtype=np.uint8)
        s = R.signatures(img)
        px = img.astype(np.int64)
        v = px[..., 0] + 2 * px[..., 1] + px[..., 2]
        assert np.array_equal(s.sum(axis=1), v.sum(axis=1)), w
        # the cell that owns pixel x is floor((32 x + 31) / w)
        own = np.zeros_like(s)
        for x in range(w):
            own[:, (32 * x + 31) // w] += v[:, x]
        assert np.array_equal(own, s), w


def test_the_crop_rule():
    rec = lambda h, f, k: {"header": h, "footer": f, "overlap": k, "cost": 0}
    assert R.overlap_rows([rec(44, 50, 100)], [640, 640]) == [(0, 590), (144, 640)]
    assert R.overlap_rows([rec(44, 50, 0)], [640, 640]) == [(0, 640), (0, 640)]
    # the middle image would keep nothing: its lower pair is voided
    assert R.overlap_rows([rec(10, 10, 40), rec(10, 10, 30)], [60, 60, 60]) == [(0, 50), (50, 60), (0, 60)]
    assert R.overlap_rows([], [17]) == [(0, 17)]


def test_cropped_shots_concatenate_to_the_page():
    bodies, offsets = [60, 60, 60], [0, 25, 70]
    shots = R.synth_shots(130, 6, 5, bodies, offsets, seed=11, clock=False, indicator=False)
    strip = np.concatenate(R.crop(shots), axis=0)
    # header once, page rows 0 .. 85 (pairs 0 | 1 overlap by 35), then - no overlap between shots 1 and 2 - footer, header and shot 2 whole
    assert strip.shape[0] == 6 + 85 + 5 + shots[2].shape[0]
    assert np.array_equal(strip[:6 + 60, :, :3], shots[0][:66, :, :3])
    assert np.array_equal(strip[66:66 + 25, :, :3], shots[1][6 + 35:6 + 60, :, :3])
