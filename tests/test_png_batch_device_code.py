"""The batch twins of the PNG kernels (ist_png_deflate_batch_kernel, ist_png_gather_batch_kernel, ist_png_rows_batch_kernel) ship in
the gfx950 code objects of libimagestitch.so and cost what their single-file twins cost: the same VGPR count, the same LDS and the
same private segment, so the same number of workgroups fits on a CU.  CPU only: llvm-readelf notes of the code objects.
Reference anchor of what they compute: the export step of onStitch (utils/canvas.js:205-242) for many requests at once."""
import os
import re
import shutil
import subprocess

import pytest

from tests import test_device_code as D

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
pytestmark = pytest.mark.skipif(not os.path.exists(READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")
KEYS = (".vgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")
TWINS = {"ist_png_deflate_batch_kernel": "ist_png_deflate_kernel", "ist_png_gather_batch_kernel": "ist_png_gather_kernel",
         "ist_png_rows_batch_kernel": "ist_png_rows_kernel"}


def _kernels(tmp):
    out = {}
    for o in D._code_objects(tmp):
        notes = subprocess.run([READELF, "--notes", o], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name:
                out[name.group(1)] = {k: int(v) for k, v in re.findall(r"(%s):\s+(\d+)" % "|".join(re.escape(k) for k in KEYS), block)}
    return out


def test_png_batch_kernels_ship_and_cost_what_their_single_file_twins_cost(tmp_path):
    ks = _kernels(str(tmp_path))
    for batch, single in TWINS.items():
        b = [v for k, v in ks.items() if batch in k]
        s = [v for k, v in ks.items() if re.search(r"\d%s" % single, k)]      # (the mangled length prefix: not the batch name)
        assert len(b) == 1 and len(s) == 1, (batch, sorted(ks))
        for key in KEYS:
            assert b[0][key] == s[0][key], (batch, key, b[0], s[0])
    assert not [k for k in ks if "ist_stitch_batch" in k and "png" in k]
