"""The kernels of the PNG window matches (pngMatch 'window': ist_ctx_set_png_match, IST_PNG_MATCH_WINDOW) ship in the gfx950 code objects
of libimagestitch.so: one kernel for a file and its batch twin, each serving both colour forms and both row-filter settings, with at
most 80 KiB of LDS - two workgroups stay resident on a CU of 160 KiB - and the same cost.  CPU only: the resource notes of the code
objects (llvm-readelf --notes), as tests/test_png_batch_device_code.py reads them; no instruction stream is looked at.  Reference anchor
of what the kernels compute: the PNG export of onStitch (utils/canvas.js:205-242)."""
import os
import shutil

import pytest

from tests import test_png_batch_device_code as B
from tests import test_png_rgb_device_code as D

pytestmark = pytest.mark.skipif(not os.path.exists(B.READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")
WINDOW = {"single": "ist_png_deflate_window_kernel", "batch": "ist_png_deflate_window_batch_kernel"}
LDS_LIMIT = 81920


def test_the_window_kernels_ship_with_at_most_80_kib_of_lds(tmp_path):
    for form, name in WINDOW.items():
        k = D._one(str(tmp_path), name)
        print(name, k)
        assert 0 < k[".group_segment_fixed_size"] <= LDS_LIMIT, (name, k)


def test_single_and_batch_twin_of_the_window_kernels_cost_the_same(tmp_path):
    single, batch = D._one(str(tmp_path), WINDOW["single"]), D._one(str(tmp_path), WINDOW["batch"])
    for key in B.KEYS:
        assert single[key] == batch[key], (key, single, batch)
