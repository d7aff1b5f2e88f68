"""The batch twins of the JPEG encoder's kernels (ist_jpeg_transform_batch_kernel, ist_jpeg_entropy_batch_kernel,
ist_jpeg_gather_batch_kernel) ship in the gfx950 code objects of libimagestitch.so and cost what their single-file kernels cost: the
same LDS, the same (empty) private segment and the same VGPR count - or, where the compiler will not give equal VGPRs, a count within
the single-file kernel's 8-register allocation step, so that the same number of waves fits on a SIMD.  The single-file kernels,
whose bodies became shared __device__ functions, stay within what DESIGN.md records for them.  CPU only: llvm-readelf notes.
Reference anchor of what they compute: the export seam (utils/canvas.js:205-221) for many requests at once.

Counts of this tree (single / twin): transform 42 / 42, entropy 68 / 68, gather 5 / 6 VGPRs."""
import os
import re
import shutil

import pytest

from tests import test_png_batch_device_code as P

pytestmark = pytest.mark.skipif(not os.path.exists(P.READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")
TWINS = {"ist_jpeg_transform_batch_kernel": "ist_jpeg_transform_kernel", "ist_jpeg_entropy_batch_kernel": "ist_jpeg_entropy_kernel",
         "ist_jpeg_gather_batch_kernel": "ist_jpeg_gather_kernel"}
# what DESIGN.md section 7 records for the single-file kernels: (VGPRs, LDS bytes; None: not recorded)
RECORDED = {"ist_jpeg_transform_kernel": (42, 9216), "ist_jpeg_entropy_kernel": (68, 55344), "ist_jpeg_gather_kernel": (5, None)}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return P._kernels(str(tmp_path_factory.mktemp("jpeg_batch_code")))


def _pair(ks, batch, single):
    b = [v for k, v in ks.items() if batch in k]
    s = [v for k, v in ks.items() if re.search(r"\d%s" % single, k)]      # (the mangled length prefix: not the batch name)
    assert len(b) == 1 and len(s) == 1, (batch, sorted(ks))
    return b[0], s[0]


def test_jpeg_batch_kernels_ship_and_cost_what_their_single_file_kernels_cost(kernels):
    for batch, single in TWINS.items():
        b, s = _pair(kernels, batch, single)
        print(batch, b, single, s)
        assert b[".group_segment_fixed_size"] == s[".group_segment_fixed_size"], (batch, b, s)
        assert b[".private_segment_fixed_size"] == s[".private_segment_fixed_size"] == 0, (batch, b, s)
        step = lambda v: (v + 7) // 8
        assert b[".vgpr_count"] == s[".vgpr_count"] or step(b[".vgpr_count"]) == step(s[".vgpr_count"]), (batch, b, s)


def test_single_file_jpeg_kernels_cost_no_more_than_recorded(kernels):
    for batch, single in TWINS.items():
        _, s = _pair(kernels, batch, single)
        vgprs, lds = RECORDED[single]
        assert s[".vgpr_count"] <= vgprs, (single, s)
        if lds is not None:
            assert s[".group_segment_fixed_size"] <= lds, (single, s)
        assert s[".private_segment_fixed_size"] == 0, (single, s)
