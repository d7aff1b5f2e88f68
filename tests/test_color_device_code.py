"""The colour conversion kernel (csrc/ist_color.hip) ships in the gfx950 code objects of libimagestitch.so with no private segment and no
spilled register: its tables live in LDS (enc 4096 + dec 768 dwords = 19456 bytes, eight workgroups of 256 threads per CU) and every
array it indexes is unrolled into registers.  CPU only: llvm-readelf notes of the code objects."""
import re
import subprocess

from tests import test_device_code as D
from tests.test_png_batch_device_code import READELF

KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count",
        ".kernarg_segment_size", ".max_flat_workgroup_size")


def _kernel(tmp, needle):
    found = []
    for o in D._code_objects(tmp):
        notes = subprocess.run([READELF, "--notes", o], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if name and needle in name.group(1):
                found.append({k: int(v) for k, v in re.findall(r"(%s):\s+(\d+)" % "|".join(re.escape(k) for k in KEYS), block)})
    return found


def test_the_colour_kernel_ships_without_a_private_segment_or_spills(tmp_path):
    k = _kernel(str(tmp_path), "ist_color_convert_kernel")
    assert len(k) == 1, k
    k = k[0]
    print(k)
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k
    assert k[".group_segment_fixed_size"] == 4 * (4096 + 768)
    assert k[".max_flat_workgroup_size"] == 256
    assert k[".kernarg_segment_size"] >= 24 + 1576          # the tables travel by value
    assert k[".vgpr_count"] <= 64                            # eight waves per SIMD: the LDS (8 workgroups x 19 KiB) is what bounds a CU, not registers
