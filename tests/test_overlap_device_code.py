"""Checks on the gfx950 machine code of the overlap kernels in libimagestitch.so (CPU only: llvm-objdump and llvm-readelf on the code
objects of the .hip_fatbin section): the three kernels ship, none has a private segment or a spill, and their LDS is what DESIGN.md
states (512 bytes for the signatures, none for the other two)."""
import os
import re
import shutil
import subprocess

import pytest

from tests import util as U
from tests.test_device_code import OBJDUMP, _code_objects

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
pytestmark = pytest.mark.skipif(not os.path.exists(OBJDUMP) or not os.path.exists(READELF) or shutil.which("objcopy") is None,
                                reason="needs llvm-objdump, llvm-readelf and objcopy")

KERNELS = {"ist_overlap_signature_kernel": 512, "ist_overlap_edge_kernel": 0, "ist_overlap_cost_kernel": 0}      # name -> LDS bytes


def _overlap_object(tmp):
    for o in _code_objects(tmp):
        names = subprocess.run([OBJDUMP, "-t", o], capture_output=True, text=True, check=True).stdout
        if "ist_overlap_signature_kernel" in names:
            return o, names
    return None, ""


def test_the_overlap_kernels_ship_for_gfx950(tmp_path):
    obj, names = _overlap_object(str(tmp_path))
    assert obj is not None, "no gfx950 code object holds the overlap kernels"
    for k in KERNELS:
        assert re.search(r"\S*%s\S*" % k, names), k


def test_the_overlap_kernels_have_no_private_segment_no_spills_and_the_stated_lds(tmp_path):
    obj, _ = _overlap_object(str(tmp_path))
    assert obj is not None
    notes = subprocess.run([READELF, "--notes", obj], capture_output=True, text=True, check=True).stdout
    seen = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:          # one block of the metadata per kernel
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        for k, lds in KERNELS.items():
            if k in name:
                seen[k] = True
                assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, k
                assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1)) == 0, k
                assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, k
                assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)) == lds, k
    assert sorted(seen) == sorted(KERNELS)
    dis = subprocess.run([OBJDUMP, "-d", obj], capture_output=True, text=True, check=True).stdout
    assert "global_load_dwordx4" in dis                    # the 16-byte row loads
    assert "scratch_" not in dis                           # private memory is never touched


def test_the_design_notes_state_the_resources():
    text = open(os.path.join(U.ROOT, "DESIGN.md"), encoding="utf-8").read()
    assert "ist_overlap.hip" in text and "512 bytes" in text
