"""The Python host's marshalling rules (imagestitching_amd/stitch.py: _rgba, _host_rows, _host_sources, _check_canvas, _file_out), without
a device.  Every entry point marshals before it asks for its context, and without a device a call that gets past marshalling fails
with StitchError -5 (IST_E_NO_DEVICE): the exception type of each case below is therefore also the proof of that order."""
import importlib

import numpy as np
import pytest
import torch

import imagestitching_amd as ist

S = importlib.import_module("imagestitching_amd.stitch")      # (the package exports the function `stitch` under the module's name)

OK = np.zeros((4, 4, 4), np.uint8)
BAD_TYPES = {"float32": np.zeros((4, 4, 4), np.float32), "rgb": np.zeros((4, 4, 3), np.uint8), "2-D": np.zeros((4, 16), np.uint8)}
TOO_SMALL = {"bmpHeight": {"data": OK, "bmpHeight": 400}, "bmpWidth": {"data": OK, "bmpWidth": 9}}

# every entry point that takes a request's host pixels, called with one image (a batch: one request of one image)
REQUESTS = {
    "stitch": lambda im: ist.stitch([im], "vertical"),
    "stitch_png": lambda im: ist.stitch_png([im], "vertical"),
    "stitch_jpeg": lambda im: ist.stitch_jpeg([im], "vertical"),
    "stitch_batch": lambda im: ist.stitch_batch([([im], "vertical")]),
    "stitch_png_batch": lambda im: ist.stitch_png_batch([([im], "vertical")]),
    "stitch_jpeg_batch": lambda im: ist.stitch_jpeg_batch([([im], "vertical")]),
    "upload_bitmap": ist.upload_bitmap,
}
PIXELS = {
    "encode_png": ist.encode_png,
    "encode_jpeg": ist.encode_jpeg,
    "render_ops": lambda a: S.render_ops(4, 4, None, 0, S._descs([OK]), [a]),
}


@pytest.mark.parametrize("bad", sorted(BAD_TYPES))
@pytest.mark.parametrize("entry", sorted(REQUESTS) + sorted(PIXELS))
def test_pixels_that_are_not_rgba8_are_a_type_error(entry, bad):
    call = REQUESTS.get(entry) or PIXELS[entry]
    with pytest.raises(TypeError, match="expected an HxWx4 uint8 RGBA array"):
        call(BAD_TYPES[bad])
    if entry in REQUESTS:
        with pytest.raises(TypeError, match="expected an HxWx4 uint8 RGBA array"):
            call({"width": 4, "height": 4, "data": BAD_TYPES[bad]})


@pytest.mark.parametrize("bad", sorted(TOO_SMALL))
@pytest.mark.parametrize("entry", sorted(REQUESTS))
def test_pixels_smaller_than_the_stored_size_are_a_value_error(entry, bad):
    with pytest.raises(ValueError, match=r"the pixels \(4x4\) are smaller than the bitmap \((4x400|9x4)\)") as e:
        REQUESTS[entry](TOO_SMALL[bad])
    if entry != "upload_bitmap":
        assert "image 0: " in str(e.value) and ("request 0, " in str(e.value)) == entry.endswith("_batch")


@pytest.mark.parametrize("entry", sorted(REQUESTS))
def test_missing_pixels_are_the_decode_failure(entry):
    with pytest.raises(ist.StitchError) as e:
        REQUESTS[entry]({"width": 4, "height": 4, "data": None})
    assert e.value.code == -6 and e.value.reason == ("request 0: " if entry.endswith("_batch") else "") + "图片0解码异常"


def test_valid_pixels_get_as_far_as_the_context():
    """the other half of the proof: a valid image gets past marshalling (no device here: -5; with one, the call succeeds)"""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    for entry, call in sorted(REQUESTS.items()) + [(k, PIXELS[k]) for k in ("encode_png", "encode_jpeg")]:
        with pytest.raises(ist.StitchError) as e:
            call(OK)
        assert e.value.code == -5, entry


def test_a_view_goes_as_it_is_and_anything_else_is_copied_once():
    big = np.random.default_rng(5).integers(0, 256, (16, 40, 4), dtype=np.uint8)
    view = big[:, 3:27]
    descs, ptrs, pitches, keep = S._host_sources([view])
    assert (descs[0].width, descs[0].height) == (24, 16)
    assert ptrs[0] == view.ctypes.data and pitches[0] == 160 and keep[0] is view
    row = big[0, :24]
    for v in (view[::-1], np.broadcast_to(row, (16, 24, 4)), big[:, ::2]):
        assert v.strides[0] < 4 * v.shape[1] or v.strides[1] != 4
        descs, ptrs, pitches, keep = S._host_sources([{"width": v.shape[1], "height": 16, "data": v}])
        assert keep[0] is not v and keep[0].flags.c_contiguous and ptrs[0] == keep[0].ctypes.data
        assert pitches[0] == 4 * v.shape[1] and np.array_equal(keep[0], v)
    # JPEG's extra condition on top of the rule: a row pitch that is a multiple of 4
    odd = np.zeros((4, 4 * 4 + 1), np.uint8)[:, :16].reshape(4, 4, 4)
    assert odd.strides == (17, 4, 1)
    assert S._host_rows(odd)[2] == 17 and S._host_rows(odd, align=4)[2] == 16
    # a hole of render_ops stays a NULL source
    descs, ptrs, pitches, keep = S._host_sources([None, view], descs=S._descs([view, view]), holes=True)
    assert not ptrs[0] and ptrs[1] == view.ctypes.data and len(keep) == 1


# ------------------------------------------------------------------------------------------------ device canvases and file outputs
DEVICE_CALLS = {
    "preview_device": lambda t: ist.preview_device(t, 2, 2),
    "thumbnails_device": lambda t: ist.thumbnails_device([t], (2, 2)),
    "encode_png_device": ist.encode_png_device,
    "encode_jpeg_device": ist.encode_jpeg_device,
    "encode_png_batch_device": lambda t: ist.encode_png_batch_device([t]),
    "encode_jpeg_batch_device": lambda t: ist.encode_jpeg_batch_device([t]),
}


@pytest.mark.parametrize("entry", sorted(DEVICE_CALLS))
def test_a_canvas_is_a_cuda_tensor_of_rgba8(entry):
    with pytest.raises(TypeError, match="CUDA tensor"):
        DEVICE_CALLS[entry](torch.zeros((4, 4, 4), dtype=torch.uint8))
    for bad in (torch.zeros((4, 4, 4), dtype=torch.float32), torch.zeros((4, 4, 3), dtype=torch.uint8), torch.zeros((4, 8, 4), dtype=torch.uint8)[:, ::2],
                np.zeros((4, 4, 4), np.uint8)):
        with pytest.raises(TypeError, match="expected an HxWx4 uint8 CUDA tensor with dense pixels"):
            DEVICE_CALLS[entry](bad)


def test_a_batch_names_the_canvas():
    ok = torch.zeros((4, 4, 4), dtype=torch.uint8)
    for call in (ist.encode_png_batch_device, ist.encode_jpeg_batch_device):
        with pytest.raises(TypeError, match="canvas 1: expected"):
            call([ok, torch.zeros((4, 4), dtype=torch.uint8)])
        with pytest.raises(TypeError, match="canvas 0: .*CUDA tensor"):
            call([ok, ok])


def test_an_encoders_output_is_a_dense_cuda_byte_tensor_or_allocated():
    for bad in (torch.zeros(64, dtype=torch.uint8), torch.zeros((8, 8), dtype=torch.uint8), torch.zeros(128, dtype=torch.uint8)[::2],
                torch.zeros(64, dtype=torch.int8), np.zeros(64, np.uint8)):
        with pytest.raises(TypeError, match="out must be"):
            S._file_out(bad, 10, "cpu")
    for cap in (0, 1, 1000, -4):
        out, off, ptr, capacity = S._file_out(None, cap, "cpu")
        assert out.dtype == torch.uint8 and out.numel() == max(cap, 0) + 16
        assert 0 <= off < 16 and ptr == out.data_ptr() + off and ptr % 16 == 0 and capacity == out.numel() - off >= max(cap, 0)
