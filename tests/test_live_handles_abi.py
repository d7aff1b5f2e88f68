"""ist_debug_live_handles without a device: the argument rule, and four zeros in a process that never touched one (the counts move
only where the library makes or releases a device block, a pinned block, a stream or an event)."""
import os
import subprocess
import sys

from imagestitching_amd import _lib as L


def test_null_output_is_refused():
    assert L.lib.ist_debug_live_handles(None) == -1                      # IST_E_INVALID
    assert b"ist_debug_live_handles" in L.lib.ist_last_error()


def test_four_zeros_in_a_process_that_never_touched_a_device():
    code = ("import ctypes as C\n"
            "from imagestitching_amd import _lib as L\n"
            "out = (C.c_int64 * 4)(7, 7, 7, 7)\n"
            "assert L.lib.ist_debug_live_handles(out) == L.IST_OK\n"
            "print(list(out))\n")
    got = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert got.stdout.strip() == "[0, 0, 0, 0]"
