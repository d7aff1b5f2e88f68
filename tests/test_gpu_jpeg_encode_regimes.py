"""The JPEG entropy coder and the symbol histogram on the GPU at every edge of their loops: the cases of tests/jpeg_encode_cases.py
(one MCU row each; tests/test_jpeg_encode_cases.py lists what they reach: carried bits that complete a 0xFF, a 0xFF that ends a batch
or the interval, full, one-block and two-block last batches, every span of the stuffing, every part size of the histogram, runs of 16
to 62, blocks without an EOB) through every encoder, each at the quality at which it was judged.  Every file equals the numpy contract
byte for byte, with the Annex K tables and with the file's own; the 544 symbol counts that an optimised encode leaves in the context
(ist_debug_jpeg_counts) equal the counts of the contract's events, which a file can hide: a miscount that changes no code length
changes no byte."""
import ctypes as C
import sys

import numpy as np
import pytest

from tests import jpeg_encode_cases as JC
from tests.test_gpu_jpeg_encode import first_difference

pytestmark = pytest.mark.gpu

LAYOUTS = ("444", "420")
CASES = [(layout, name) for layout in LAYOUTS for name, _, _ in JC.cases(layout)]
COUNTERS = 2 * (16 + 256)


@pytest.fixture(scope="module")
def ist():
    import imagestitching_amd
    return imagestitching_amd


def case(layout, name):
    return next(c for c in JC.cases(layout) if c[0] == name)


def context():
    """the context of device 0, which every encode of the package uses"""
    import imagestitching_amd  # noqa: F401
    return sys.modules["imagestitching_amd.stitch"]._ctx(0)      # (the package's attribute `stitch` is the function)


def gpu_counts(files=1):
    """the counters of the last optimised encode on device 0: `files` blocks of 544"""
    from imagestitching_amd import _lib as L
    out = np.full(files * COUNTERS, -1, np.int64)
    L.check(L.lib.ist_debug_jpeg_counts(context(), out.ctypes.data_as(C.POINTER(C.c_int64)), out.size))
    return out


def same_counts(got, want, what):
    bad = np.nonzero(got != want)[0]
    slot, at = divmod(int(bad[0]) % COUNTERS, 16 + 256) if len(bad) else (0, 0)
    where = "DC size %d" % at if at < 16 else "AC symbol 0x%02X" % (at - 16)
    assert not len(bad), "%s: %d counters differ, the first is %s of slot %d: %d, the contract has %d" % (
        what, len(bad), where, slot, got[bad[0]], want[bad[0]])


def same_file(got, want, what):
    assert got == want, "%s: %s" % (what, first_difference(got, want))


@pytest.mark.parametrize("layout,name", CASES)
def test_a_case_equals_the_contract_with_both_kinds_of_table_and_in_its_counts(ist, layout, name):
    _, a, q = case(layout, name)
    what = "%s, Q%d %s" % (name, q, layout)
    same_file(ist.encode_jpeg(a, q, layout), JC.reference(a, q, layout, "std"), what + ", Annex K tables")
    got = ist.encode_jpeg(a, q, layout, optimize=True)
    counts = gpu_counts()
    same_file(got, JC.reference(a, q, layout, "optimal"), what + ", optimised tables")
    same_counts(counts, JC.counts(a, q, layout), what)


def batch(ist, files):
    """[(canvas, quality, layout, optimize)] through one encode_jpeg_batch_device call -> the files"""
    import torch
    from imagestitching_amd import _lib as L
    cans = [torch.from_numpy(a).cuda() for a, _, _, _ in files]
    before = L.lib.ist_debug_jpeg_batch_launches()
    res = ist.encode_jpeg_batch_device(cans, [f[1] for f in files], [f[2] for f in files], optimize=[f[3] for f in files])
    torch.cuda.synchronize()
    assert L.lib.ist_debug_jpeg_batch_launches() == before + 1            # one round
    out = []
    for t, n in res:
        out.append(t.cpu().numpy().tobytes())
        assert len(out[-1]) == n
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("optimised", ("even files", "odd files", "no file"))
def test_all_cases_in_one_batch_call(ist, layout, optimised):
    """a round with an optimised file runs the wide batch entropy kernel on all of its files, a round without one the other: alternating
    either way shows every seam to the wide kernel with both kinds of table, and the batch of standard files shows them to the other;
    the batch gather lays every file out"""
    first = {"even files": 0, "odd files": 1, "no file": 2}[optimised]
    files = [(a, q, layout, first < 2 and k % 2 == first) for k, (_, a, q) in enumerate(JC.cases(layout))]
    for (name, _, _), (a, q, _, o), got in zip(JC.cases(layout), files, batch(ist, files)):
        same_file(got, JC.reference(a, q, layout, "optimal" if o else "std"), "%s, Q%d %s, %s" % (name, q, layout, "optimised" if o else "standard"))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_counts_of_a_batch_with_two_optimised_files_among_three(ist, layout):
    """six full parts (2048 wide) and a last part of two blocks (688 wide) around a standard file of the other layout, which is not counted"""
    other = "420" if layout == "444" else "444"
    (_, a0, q0), (_, a1, q1), (_, a2, q2) = case(layout, "noise 2048"), case(other, "photo 688 quality 50"), case(layout, "sparse 688")
    files = [(a0, q0, layout, True), (a1, q1, other, False), (a2, q2, layout, True)]
    got = batch(ist, files)
    counts = gpu_counts(2)
    for k, (a, q, lay, o) in enumerate(files):
        same_file(got[k], JC.reference(a, q, lay, "optimal" if o else "std"), "file %d" % k)
    same_counts(counts, np.concatenate([JC.counts(a0, q0, layout), JC.counts(a2, q2, layout)]), "files 0 and 2")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_seam_cases_from_a_pitched_device_canvas(ist, layout):
    import torch
    for name in ("directed seam for std tables", "directed end for optimal tables"):
        _, a, q = case(layout, name)
        h, w = a.shape[:2]
        wide = torch.full((h, w + 13, 4), 0xEE, dtype=torch.uint8, device="cuda")
        wide[:, :w] = torch.from_numpy(a).cuda()
        canvas = wide[:, :w]
        assert canvas.stride(0) == 4 * (w + 13)
        for tables in ("std", "optimal"):
            t, n = ist.encode_jpeg_device(canvas, q, layout, optimize=tables == "optimal")
            torch.cuda.synchronize()
            got, want = t.cpu().numpy().tobytes(), JC.reference(a, q, layout, tables)
            assert n == len(want)
            same_file(got, want, "%s, %s, %s tables" % (name, layout, tables))
            if tables == "optimal":
                same_counts(gpu_counts(), JC.counts(a, q, layout), name)


def test_debug_counts_refuses_more_than_the_block_holds(ist):
    from imagestitching_amd import _lib as L
    _, a, q = case("444", "constant 688")
    ist.encode_jpeg(a, q, "444", optimize=True)                               # the block exists
    out = np.zeros(COUNTERS, np.int64)
    p = out.ctypes.data_as(C.POINTER(C.c_int64))
    before = L.lib.ist_debug_jpeg_encode_launches(), L.lib.ist_debug_jpeg_histogram_launches(), L.lib.ist_debug_device_allocs()
    assert L.lib.ist_debug_jpeg_counts(context(), p, COUNTERS * 4097) == -1 and "holds" in L.last_error()      # (a batch is at most 4096 files)
    assert L.lib.ist_debug_jpeg_counts(context(), p, COUNTERS + 1) == -1
    assert L.lib.ist_debug_jpeg_counts(context(), p, 0) == 0
    assert L.lib.ist_debug_jpeg_counts(context(), p, COUNTERS) == 0
    same_counts(out, JC.counts(a, q, "444"), "constant 688")
    assert before == (L.lib.ist_debug_jpeg_encode_launches(), L.lib.ist_debug_jpeg_histogram_launches(), L.lib.ist_debug_device_allocs())
