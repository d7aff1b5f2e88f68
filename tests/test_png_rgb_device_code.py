"""The RGB instantiation of the compressing PNG kernel (ist_png_deflate_rgb_kernel, ist_png_deflate_rgb_batch_kernel) ships in the
gfx950 code objects of libimagestitch.so beside the RGBA kernels, costs the LDS they cost, and has left them what they were.  CPU
only: llvm-readelf notes of the code objects, as tests/test_png_batch_device_code.py reads them.  Reference anchor of what the kernels
compute: the PNG export of onStitch (utils/canvas.js:205-242)."""
import os
import re
import shutil

import pytest

from tests import test_png_batch_device_code as B

pytestmark = pytest.mark.skipif(not os.path.exists(B.READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")
RGB = {"single": "ist_png_deflate_rgb_kernel", "batch": "ist_png_deflate_rgb_batch_kernel"}
RGBA = {"single": "ist_png_deflate_kernel", "batch": "ist_png_deflate_batch_kernel"}
# .vgpr_count, .group_segment_fixed_size, .private_segment_fixed_size of the two RGBA kernels in the library of the commit before
# the RGB form existed (built from that commit with the same compiler and read with llvm-readelf --notes).  The 68 bytes of
# private segment are 16 spilled VGPRs (.vgpr_spill_count 16): under amdgpu_waves_per_eu(7) the kernel has 72 registers, and the top
# byte of each of a thread's sixteen span words, taken in step B, waits in scratch for the stored form's copy in step D.
RGBA_BEFORE = {".vgpr_count": 72, ".group_segment_fixed_size": 21544, ".private_segment_fixed_size": 68}

_cache = {}


def _one(tmp, name):
    if "ks" not in _cache:
        _cache["ks"] = B._kernels(tmp)
    found = [v for k, v in _cache["ks"].items() if re.search(r"\d%s[A-Z]" % name, k)]      # (the mangled length prefix, then the argument list)
    assert len(found) == 1, (name, sorted(_cache["ks"]))
    return found[0]


def test_the_rgb_kernels_ship_with_the_lds_of_the_rgba_kernels(tmp_path):
    for form in ("single", "batch"):
        rgb, rgba = _one(str(tmp_path), RGB[form]), _one(str(tmp_path), RGBA[form])
        assert rgb[".group_segment_fixed_size"] == rgba[".group_segment_fixed_size"] == 21544, (form, rgb, rgba)


def test_single_and_batch_twin_of_the_rgb_form_cost_the_same(tmp_path):
    single, batch = _one(str(tmp_path), RGB["single"]), _one(str(tmp_path), RGB["batch"])
    for key in B.KEYS:
        assert single[key] == batch[key], (key, single, batch)


def test_the_rgba_kernels_are_what_they_were(tmp_path):
    for form in ("single", "batch"):
        assert _one(str(tmp_path), RGBA[form]) == RGBA_BEFORE, form


def test_the_rgb_kernels_have_no_private_segment(tmp_path):
    """The RGBA kernels spill 16 VGPRs under the 72-register cap of amdgpu_waves_per_eu(7) (RGBA_BEFORE above) and the RGB instantiation
    of the same body would spill the same sixteen; it is built for 5 waves instead (96 VGPRs, none spilled), at the measured price
    written beside the kernel in ist_png_deflate.hip."""
    for form in ("single", "batch"):
        assert _one(str(tmp_path), RGB[form])[".private_segment_fixed_size"] == 0, form
