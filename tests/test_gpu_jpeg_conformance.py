"""JPEG decode on hand-built streams (tests/jpeg_writer.py): every layout at every small size, every scan / table /
restart / marker-noise / coefficient variant of the writer, and two files large enough for several GPU Huffman
workgroups, through the three entry points - ist.decode_image (host Huffman), ist.decode_files_device (GPU Huffman where
the file qualifies) and ist.stitch_files (the file pipeline, also reconstructing straight into the canvas).  Each output
must equal PIL's bit for bit and lie within the writer's pinned bound of the float64 reference; the GPU Huffman counter
must move by exactly the number of files the GPU decoder's intake takes, so a silent host fall-back cannot hide a bug."""
import io

import numpy as np
import pytest
from PIL import Image

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import jpeg_writer as JW
from tests import util as U
from tests.test_jpeg_writer import REF_BOUND

pytestmark = pytest.mark.gpu

GROUPS = ["size_" + k for k in JW.SIZE_LAYOUTS] + ["variant_" + k for k in JW.VARIANT_LAYOUTS] + ["large", "pillow_rgb"]


def _cases(group):
    if group.startswith("size_"):
        return JW.size_cases(group[5:])
    if group.startswith("variant_"):
        return JW.variant_cases(group[8:])
    return JW.large_cases() if group == "large" else JW.pillow_keep_rgb_cases()


def _pil(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))


def _expect(c, got, what):
    want = _pil(c["data"])
    assert got.shape == want.shape, (c["name"], what)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() == 0, "%s (%s): max diff %d in %d px, first at %s" % (c["name"], what, d.max(), int((d.max(-1) > 0).sum()),
                                                                       tuple(np.argwhere(d.max(-1) > 0)[0]))
    if c["frame"] is not None:
        err = np.abs(got[..., :3].astype(np.float64) - JW.reference_rgb(c["frame"])).max()
        assert err <= REF_BOUND, "%s (%s): %d LSB from the float64 reference" % (c["name"], what, err)


def _gpu_files():
    return L.lib.ist_debug_gpu_entropy_files()


@pytest.mark.parametrize("group", GROUPS)
def test_decode_image(group):
    for c in _cases(group):
        _expect(c, ist.decode_image(c["data"]), "decode_image")


@pytest.mark.parametrize("group", GROUPS)
def test_decode_files_device(group):
    cases = _cases(group)
    for k in range(0, len(cases), 64):
        batch = cases[k:k + 64]
        before = _gpu_files()
        out, imgs = ist.decode_files_device([c["data"] for c in batch])
        assert _gpu_files() - before == sum(c["gpu"] for c in batch), group
        for c, t, d in zip(batch, out, imgs):
            assert (d["width"], d["height"]) == (c["width"], c["height"])
            _expect(c, t.cpu().numpy(), "decode_files_device")


@pytest.mark.parametrize("group", GROUPS)
def test_stitch_files(tmp_path, group):
    """same-width files stitched vertically with the nearest filter: the PNG is the concatenation of PIL's bitmaps"""
    by_width = {}
    for c in _cases(group):
        by_width.setdefault(c["width"], []).append(c)
    for w, cases in by_width.items():
        paths = []
        for k, c in enumerate(cases):
            p = tmp_path / ("%d_%d.jpg" % (w, k))
            p.write_bytes(c["data"])
            paths.append(str(p))
        before = _gpu_files()
        res = ist.stitch_files(paths, "vertical", {"filter": "nearest"})
        assert _gpu_files() - before == sum(c["gpu"] for c in cases), (group, w)
        got = ist.decode_png(res["png"])
        want = np.concatenate([_pil(c["data"]) for c in cases], 0)
        assert got.shape == want.shape, (group, w)
        row = 0
        for c in cases:
            _expect(c, got[row:row + c["height"]], "stitch_files")
            row += c["height"]


def test_original_mode_reconstructs_straight_into_the_canvas(tmp_path):
    """mode 'original': the JPEGs are reconstructed into their boxes of the canvas (ist_debug_direct_images)"""
    pick = ["420_3x9", "420_4x17", "422_2x15", "rgb_7x8", "rgbids_17x16", "440_5x3", "grey22_9x9"]
    cases = {c["name"]: c for g in ("size_420", "size_422", "size_rgb", "size_rgbids", "size_440", "size_grey22") for c in _cases(g)}
    chosen = [cases[n] for n in pick] + [c for c in JW.variant_cases("440") if c["name"] in ("440_scans_y_then_cbcr", "440_edges")]
    paths = []
    for k, c in enumerate(chosen):
        p = tmp_path / ("o%d.jpg" % k)
        p.write_bytes(c["data"])
        paths.append(str(p))
    opts = {"filter": "nearest", "mode": "original", "gap": 3}
    before = L.lib.ist_debug_direct_images()
    res = ist.stitch_files(paths, "vertical", opts)
    assert L.lib.ist_debug_direct_images() - before == len(chosen)
    ref, _, _ = U.oracle_stitch([_pil(c["data"]) for c in chosen], "vertical", opts, orientations=[1] * len(chosen))
    got = ist.decode_png(res["png"])
    assert got.shape == ref.shape and np.array_equal(got, ref)


def test_refused_layouts_never_return_pixels(tmp_path):
    for c in JW.refused_cases():
        with pytest.raises(ist.StitchError) as e:
            ist.decode_image(c["data"])
        assert e.value.code == -7, c["name"]
        with pytest.raises(ist.StitchError) as e:
            ist.decode_files_device([c["data"]])
        assert e.value.code == -7, c["name"]
        p = tmp_path / (c["name"] + ".jpg")
        p.write_bytes(c["data"])
        with pytest.raises(ist.StitchError) as e:
            ist.stitch_files([str(p)], "vertical")
        assert e.value.code == -7, c["name"]
