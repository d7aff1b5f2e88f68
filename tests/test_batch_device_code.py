"""The batch kernels (ist_stitch_batch_kernel / ist_stitch_batch_area_kernel, ist_kernels.hip) ship in the gfx950 code objects of
libimagestitch.so, one per kernel form, and cost what the single-job kernel of the same form costs: the same VGPR count and the same
private segment (none, except the streamed box filter's form, whose single-job twin is held to 5 waves per SIMD and spills 3
registers by design - the batch twin keeps exactly that, no more).  CPU only: llvm-readelf notes of the code objects.
Reference anchor of what they compute: N x utils/canvas.js:153-202 (drawImage) for N independent onStitch calls."""
import os
import re
import shutil
import subprocess

import pytest

from tests import test_device_code as D

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
pytestmark = pytest.mark.skipif(not os.path.exists(READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")


def _kernels(tmp):
    """{kernel symbol: {'.vgpr_count': n, '.private_segment_fixed_size': n, ...}} over every gfx950 code object"""
    out = {}
    for o in D._code_objects(tmp):
        notes = subprocess.run([READELF, "--notes", o], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if not name:
                continue
            vals = {k: int(v) for k, v in re.findall(r"(\.vgpr_count|\.private_segment_fixed_size|\.sgpr_count):\s+(\d+)", block)}
            out[name.group(1)] = vals
    return out


def test_batch_kernels_ship_and_cost_what_their_single_job_twins_cost(tmp_path):
    ks = _kernels(str(tmp_path))
    batch = {k: v for k, v in ks.items() if "ist_stitch_batch" in k}
    # one per kernel form: fill/copy, + resampling, + box filter, + quarter turns / paint stacks, everything
    forms = {3: False, 7: False, 39: True, 31: False, 63: True}
    assert len(batch) == len(forms), sorted(batch)
    for paths, area in forms.items():
        b = [v for k, v in batch.items() if ("area_kernel" in k) == area and re.search(r"kernelILi%dELi0EEE" % paths, k)]
        twin = "ist_stitch_area_kernel" if area else "ist_stitch_kernel"
        single = "_ZN3ist%d%sILi%dELi0ELb0EEEvNS_10LaunchArgsEl" % (len(twin), twin, paths)      # the shipped single-job form
        assert len(b) == 1 and single in ks, (paths, sorted(batch), single)
        assert b[0][".vgpr_count"] == ks[single][".vgpr_count"], (paths, b[0], ks[single])
        assert b[0][".private_segment_fixed_size"] == ks[single][".private_segment_fixed_size"], (paths, b[0], ks[single])
        if not area:
            assert b[0][".private_segment_fixed_size"] == 0, (paths, b[0])
