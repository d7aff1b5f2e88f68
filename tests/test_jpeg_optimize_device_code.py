"""The kernels of the JPEG export's optimised Huffman tables ship in the gfx950 code objects of libimagestitch.so: the histogram
(ist_jpeg_histogram_kernel and its batch twin) and the entropy kernel's wide instantiation (ist_jpeg_entropy_wide_kernel and its
twin: a block of up to 1665 bits).  None has a private segment, each fits the 64 KiB of LDS a workgroup may have, and a twin sits
within one 8-register allocation step of its single-file kernel, so the same number of waves fits on a SIMD.  The standard kernels
are held to their recorded cost by tests/test_jpeg_batch_device_code.py.  CPU only: llvm-readelf notes.

Counts of this tree (single / twin): histogram 42 / 42 VGPRs, 8704 B of LDS; wide entropy 74 / 74 VGPRs, 55760 B of LDS."""
import os
import re
import shutil

import pytest

from tests import test_png_batch_device_code as P

pytestmark = pytest.mark.skipif(not os.path.exists(P.READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")
TWINS = {"ist_jpeg_histogram_batch_kernel": "ist_jpeg_histogram_kernel", "ist_jpeg_entropy_wide_batch_kernel": "ist_jpeg_entropy_wide_kernel"}
# the wide image: (7 + 256 x 1665 + 31) // 32 + 2 words, beside the 2176 B of code tables (32 DC + 512 AC words) (the standard kernel's: 1660 bits a block)
WIDE_IMAGE_BYTES = ((7 + 256 * 1665 + 31) // 32 + 2) * 4


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return P._kernels(str(tmp_path_factory.mktemp("jpeg_optimize_code")))


def _one(ks, pattern):
    found = [v for k, v in ks.items() if re.search(pattern, k)]
    assert len(found) == 1, (pattern, sorted(ks))
    return found[0]


def test_optimize_kernels_ship_and_fit(kernels):
    for batch, single in TWINS.items():
        b, s = _one(kernels, r"\d%s" % batch), _one(kernels, r"\d%s" % single)      # (the mangled length prefix: the whole name)
        print(batch, b, single, s)
        for k in (b, s):
            assert k[".private_segment_fixed_size"] == 0, (batch, k)
            assert k[".group_segment_fixed_size"] <= 65536, (batch, k)
        assert b[".group_segment_fixed_size"] == s[".group_segment_fixed_size"], (batch, b, s)
        step = lambda v: (v + 7) // 8
        assert abs(step(b[".vgpr_count"]) - step(s[".vgpr_count"])) <= 1, (batch, b, s)


def test_the_wide_image_lives_in_the_new_kernels_only(kernels):
    wide, std = _one(kernels, r"\dist_jpeg_entropy_wide_kernel"), _one(kernels, r"\dist_jpeg_entropy_kernel")
    assert wide[".group_segment_fixed_size"] >= WIDE_IMAGE_BYTES + 2176 > std[".group_segment_fixed_size"]
    assert std[".group_segment_fixed_size"] <= 55344 and std[".vgpr_count"] <= 68      # (what DESIGN.md section 7 records for it)
