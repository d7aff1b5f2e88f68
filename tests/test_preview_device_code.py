"""Checks on the gfx950 machine code of the preview kernels in libimagestitch.so (CPU only: llvm-objdump on the code objects of the
.hip_fatbin section).  What they compute: the redraw into the preview node (pages/index/index.js:1597-1603).  The reduce promises the
same bytes for the same input, so its partial sums are plain stores added in a fixed order: no float atomic may appear in it."""
import os
import re
import shutil
import subprocess

import pytest

from tests import util as U
from tests.test_device_code import OBJDUMP, _code_objects

pytestmark = pytest.mark.skipif(not os.path.exists(OBJDUMP) or shutil.which("objcopy") is None, reason="needs llvm-objdump and objcopy")

KERNELS = ("ist_preview_partial_kernel", "ist_preview_finish_kernel")


def _preview_object(tmp):
    for o in _code_objects(tmp):
        names = subprocess.run([OBJDUMP, "-t", o], capture_output=True, text=True, check=True).stdout
        if KERNELS[0] in names:
            return o, names
    return None, ""


def test_the_preview_kernels_ship_for_gfx950_in_both_forms(tmp_path):
    obj, names = _preview_object(str(tmp_path))
    assert obj is not None, "no gfx950 code object holds the preview kernels"
    for k in KERNELS:
        # opaque and translucent instantiation of each (template argument b1 / b0 in the mangled name)
        assert len(set(re.findall(r"\S*%sILb[01]E\S*" % k, names))) >= 2, k


def test_the_preview_kernels_use_no_float_atomics_and_no_scratch(tmp_path):
    obj, _ = _preview_object(str(tmp_path))
    assert obj is not None
    dis = subprocess.run([OBJDUMP, "-d", obj], capture_output=True, text=True, check=True).stdout
    assert "global_load_dwordx4" in dis                    # the 16-byte source loads
    for bad in ("global_atomic_add_f32", "global_atomic_pk_add", "flat_atomic_add_f32", "buffer_atomic_add_f32", "ds_add_f32", "ds_add_rtn_f32"):
        assert bad not in dis, bad
    assert "scratch_" not in dis and "buffer_store_dword" not in dis      # no spills (private memory is never touched)
