"""The reduced-size JPEG reconstruction kernels (csrc/ist_jpeg_scaled.hip) ship in the gfx950 code objects of libimagestitch.so: the
reduced IDCT in its three instantiations (S = 4, 2, 1) and the planes -> RGBA8 kernel, none of them with a private segment (no
scratch memory: every array they index is unrolled into registers).  The two IDCTs that pass rows and columns through LDS hold the
32 block images + the quantisation table the full-size IDCT holds; the 1 x 1 one holds none.  CPU only: llvm-readelf notes."""
import os
import re
import shutil

import pytest

from tests.test_png_batch_device_code import READELF, _kernels

pytestmark = pytest.mark.skipif(not os.path.exists(READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")


def test_the_reduced_idcts_and_the_planes_kernel_ship_without_a_private_segment(tmp_path):
    ks = _kernels(str(tmp_path))
    lds = {}
    for s in (4, 2, 1):
        k = [v for name, v in ks.items() if re.search(r"\d+ist_jpeg_scaled_idct_kernelILi%dEE" % s, name)]
        assert len(k) == 1, (s, sorted(n for n in ks if "scaled" in n))
        assert k[0][".private_segment_fixed_size"] == 0, (s, k[0])
        lds[s] = k[0][".group_segment_fixed_size"]
    full = [v for name, v in ks.items() if re.search(r"\d+ist_jpeg_idct_kernel", name)]
    assert len(full) == 1
    assert lds[4] == lds[2] == full[0][".group_segment_fixed_size"] == 4 * (32 * 72 + 72) and lds[1] == 0
    p = [v for name, v in ks.items() if "ist_jpeg_scaled_planes_kernel" in name]
    assert len(p) == 1 and p[0][".private_segment_fixed_size"] == 0 and p[0][".group_segment_fixed_size"] == 0, p
