"""The batch twins of the preview kernels (ist_preview_partial_batch_kernel, ist_preview_finish_batch_kernel: many reduces per launch,
the thumbnails of the grid of chosen images, pages/index/index.wxml:4-22) ship in the gfx950 code objects of libimagestitch.so in both
forms and cost what their single-image twins cost: the same VGPR count, the same LDS and the same private segment (none), so the same
number of workgroups fits on a CU.  The item lookup and the item's arguments, read through the constant address space, were measured at
build time to cost the twins scalar registers only: the comparison is an equality.  CPU only: llvm-readelf notes of the code objects."""
import os
import re
import shutil

import pytest

from tests.test_png_batch_device_code import KEYS, READELF, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")
TWINS = {"ist_preview_partial_batch_kernel": "ist_preview_partial_kernel", "ist_preview_finish_batch_kernel": "ist_preview_finish_kernel"}


def test_thumbnail_batch_kernels_ship_in_both_forms_and_cost_what_their_single_image_twins_cost(tmp_path):
    ks = _kernels(str(tmp_path))
    for batch, single in TWINS.items():
        for form in ("ILb0E", "ILb1E"):                      # translucent and opaque instantiation (the template argument in the mangled name)
            b = [v for k, v in ks.items() if batch + form in k]
            s = [v for k, v in ks.items() if re.search(r"\d%s%s" % (single, form), k)]      # (the mangled length prefix: not the batch name)
            assert len(b) == 1 and len(s) == 1, (batch, form, sorted(k for k in ks if "preview" in k))
            for key in KEYS:
                assert b[0][key] == s[0][key], (batch, form, key, b[0], s[0])
            assert b[0][".private_segment_fixed_size"] == 0
