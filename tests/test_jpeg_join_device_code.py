"""The join kernel (csrc/ist_jpeg_join.hip) ships in the gfx950 code objects of libimagestitch.so without a private segment and
without a spilled register: it moves 16 bytes per lane each way and holds nothing else.  Its LDS is the 32 block images of a workgroup
(144 bytes each: 128 + 16, so that the eight blocks of a wave start on different banks) and the 129 prefix sums of the image table.
CPU only: llvm-readelf notes of the code objects."""
import os
import re
import shutil
import subprocess

import pytest

from tests import test_device_code as D

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
pytestmark = pytest.mark.skipif(not os.path.exists(READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")
KEYS = (".vgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_spill_count")


def test_the_join_kernel_ships_without_a_private_segment_or_spills(tmp_path):
    found = []
    for o in D._code_objects(str(tmp_path)):
        notes = subprocess.run([READELF, "--notes", o], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and re.search(r"\d+ist_jpeg_join_kernel", name.group(1)):
                found.append({k: int(v) for k, v in re.findall(r"(%s):\s+(\d+)" % "|".join(re.escape(k) for k in KEYS), block)})
    assert len(found) == 1, found
    k = found[0]
    assert k[".private_segment_fixed_size"] == 0 and k[".sgpr_spill_count"] == 0 and k[".vgpr_spill_count"] == 0, k
    assert k[".group_segment_fixed_size"] == 32 * 144 + 4 * 129, k
    assert k[".vgpr_count"] <= 64, k                     # (eight waves per SIMD)
