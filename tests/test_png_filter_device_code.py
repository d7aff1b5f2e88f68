"""The kernels of the adaptive PNG row filters ship in the gfx950 code objects of libimagestitch.so: the row-filter pre-pass in both
colour forms and the four adaptive twins of the compressing kernels, with the LDS of the kernels they are twins of and no private
segment; and the four compressing kernels that existed before are what they were.  CPU only: llvm-readelf notes of the code objects,
as tests/test_png_batch_device_code.py reads them.  Reference anchor of what the kernels compute: the PNG export of onStitch
(utils/canvas.js:205-242)."""
import os
import shutil

import pytest

from tests import test_png_batch_device_code as B
from tests import test_png_rgb_device_code as D

pytestmark = pytest.mark.skipif(not os.path.exists(B.READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")
PREPASS = ("ist_png_row_filter_kernel", "ist_png_row_filter_rgb_kernel")
ADAPT = {"rgba": {"single": "ist_png_deflate_adapt_kernel", "batch": "ist_png_deflate_adapt_batch_kernel"},
         "rgb": {"single": "ist_png_deflate_adapt_rgb_kernel", "batch": "ist_png_deflate_adapt_rgb_batch_kernel"}}
# .vgpr_count, .group_segment_fixed_size, .private_segment_fixed_size of the four compressing kernels in the library of the commit
# before the filter setting existed (built from that commit with the same compiler and read with llvm-readelf --notes, as RGBA_BEFORE
# of tests/test_png_rgb_device_code.py was).  The instruction streams of the four were compared too (hipcc -S --cuda-device-only of
# ist_png_deflate.hip at both commits, comments stripped): identical.
BEFORE = {"ist_png_deflate_kernel": {".vgpr_count": 72, ".group_segment_fixed_size": 21544, ".private_segment_fixed_size": 68},
          "ist_png_deflate_batch_kernel": {".vgpr_count": 72, ".group_segment_fixed_size": 21544, ".private_segment_fixed_size": 68},
          "ist_png_deflate_rgb_kernel": {".vgpr_count": 96, ".group_segment_fixed_size": 21544, ".private_segment_fixed_size": 0},
          "ist_png_deflate_rgb_batch_kernel": {".vgpr_count": 96, ".group_segment_fixed_size": 21544, ".private_segment_fixed_size": 0}}


def test_the_pre_pass_ships_with_no_private_segment_and_only_its_reduction_words(tmp_path):
    for name in PREPASS:
        k = D._one(str(tmp_path), name)
        assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 4 * 5 * 4, (name, k)


def test_the_adaptive_kernels_ship_with_the_lds_of_the_body_and_no_private_segment(tmp_path):
    for color, forms in ADAPT.items():
        for form, name in forms.items():
            k = D._one(str(tmp_path), name)
            assert k[".group_segment_fixed_size"] == 21544 and k[".private_segment_fixed_size"] == 0, (name, k)


def test_single_and_batch_twin_of_the_adaptive_kernels_cost_the_same(tmp_path):
    for color, forms in ADAPT.items():
        single, batch = D._one(str(tmp_path), forms["single"]), D._one(str(tmp_path), forms["batch"])
        for key in B.KEYS:
            assert single[key] == batch[key], (color, key, single, batch)


def test_the_compressing_kernels_of_before_are_what_they_were(tmp_path):
    for name, want in BEFORE.items():
        assert D._one(str(tmp_path), name) == want, name
