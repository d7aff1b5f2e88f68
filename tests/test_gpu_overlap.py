"""The overlap search on the GPU (ist_bitmaps_overlap, ist_overlap_device; ist_overlap.hip) against the numpy restatement of the contract
(tests/overlap_reference.py): every record equal, cost included - the arithmetic is integer, so there is no tolerance."""
import ctypes as C
import sys

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import overlap_reference as R

pytestmark = pytest.mark.gpu
S = sys.modules["imagestitching_amd.stitch"]      # (the package's attribute `stitch` is the function)


def _upload(shots):
    return [ist.upload_bitmap(s) for s in shots]


def _close(bms):
    for b in bms:
        b.close()


def _check(shots, want=None, **opts):
    """find_overlaps(uploaded shots) == the reference's records (== the synthetic truth, where given)"""
    ref = R.find_overlaps(shots, **opts)
    if want is not None:
        assert [(p["header"], p["footer"], p["overlap"]) for p in ref] == want
    bms = _upload(shots)
    try:
        got = ist.find_overlaps(bms, **opts)
    finally:
        _close(bms)
    assert got == ref
    return got


def _signatures(rows):
    out = np.empty((rows, 32), np.uint32)
    L.check(L.lib.ist_debug_overlap_signatures(S._ctx(0), out.ctypes.data_as(C.POINTER(C.c_uint32)), rows))
    return out


@pytest.mark.parametrize("w", [5, 31, 33, 64, 130, 1170])
def test_three_shots_of_unequal_heights_at_every_width(w):
    bodies, offsets = [40, 60, 50], [0, 20, 45]                # heights 51, 71, 61
    shots = R.synth_shots(w, 6, 5, bodies, offsets, seed=w)
    _check(shots, R.truth(6, 5, bodies, offsets))
    # the signature table of the call: every row of every image, also where the width is no multiple of 4 and rows are not 16-byte aligned
    sig = _signatures(sum(s.shape[0] for s in shots))
    assert np.array_equal(sig.astype(np.int64), np.concatenate([R.signatures(s) for s in shots]))


def test_a_tall_pair_crosses_every_workgroup_boundary():
    # 2100 rows: 525 signature workgroups per image, k up to 2000 (500 cost workgroups of 4), r up to 2000 (32 steps of 64 per wave),
    # 9 flag workgroups of 256, 9 edge workgroups
    bodies, offsets = [2089, 2085], [0, 703]
    shots = R.synth_shots(96, 6, 5, bodies, offsets, seed=5)
    got = _check(shots, [(6, 5, 2089 - 703)])
    assert got[0]["cost"] > 0                                  # the scroll indicator moved


@pytest.mark.parametrize("step", [100, 530, 531, 600])
def test_the_noisy_case(step):
    shots = R.synth_shots(360, 44, 50, [546, 546], [0, step], seed=step, noise=2)
    _check(shots, R.truth(44, 50, [546, 546], [0, step]))


def test_options_reach_the_rule():
    shots = R.synth_shots(360, 44, 50, [546, 546], [0, 531], seed=9, noise=2)
    assert _check(shots)[0]["overlap"] == 0
    assert _check(shots, min_rows=15)[0]["overlap"] == 15
    assert _check(shots, min_rows=15, min_informative=16)[0]["overlap"] == 0
    _check(shots, tolerance=0, min_rows=1)                     # with noise nothing matches exactly: whatever the reference says


def test_a_blank_pair():
    blank = np.full((90, 64, 4), 255, np.uint8)
    assert _check([blank, blank]) == [{"header": 45, "footer": 45, "overlap": 0, "cost": 0}]


def test_mixed_widths_in_one_call():
    a = R.synth_shots(64, 6, 5, [40, 60], [0, 20], seed=1)
    b = R.synth_shots(65, 6, 5, [50, 60], [0, 30], seed=2)
    got = _check([a[0], a[1], b[0], b[1]])
    assert got[1] == {"header": 0, "footer": 0, "overlap": 0, "cost": 0}
    assert got[0]["overlap"] == 20 and got[2]["overlap"] == 20


def test_device_tensors_with_padded_rows_give_the_same_records():
    import torch
    shots = R.synth_shots(33, 6, 5, [40, 60], [0, 20], seed=4)
    tensors = []
    for s in shots:
        t = torch.zeros((s.shape[0], 40, 4), dtype=torch.uint8, device="cuda")[:, 3:36]      # pitch 160, rows 12 bytes into a line
        t.copy_(torch.from_numpy(s))
        tensors.append(t)
    assert ist.find_overlaps_device(tensors) == R.find_overlaps(shots)


def test_launches_and_allocations_of_a_repeated_shape():
    shots = R.synth_shots(130, 6, 5, [40, 60, 50], [0, 20, 45], seed=8)
    bms = _upload(shots)
    first = ist.find_overlaps(bms)
    live = (C.c_int64 * 4)()
    L.lib.ist_debug_live_handles(live)
    before = (L.lib.ist_debug_overlap_launches(), L.lib.ist_debug_device_allocs(), list(live))
    assert ist.find_overlaps(bms) == first
    L.lib.ist_debug_live_handles(live)
    assert (L.lib.ist_debug_overlap_launches(), L.lib.ist_debug_device_allocs(), list(live)) == (before[0] + 3, before[1], before[2])
    _close(bms)


def test_refusals():
    a = R.synth_shots(64, 6, 5, [40], [0], seed=1)[0]
    b = ist.upload_bitmap(a)
    turned = ist.upload_bitmap({"width": 64, "height": 51, "data": a, "orientation": 3})
    launches = L.lib.ist_debug_overlap_launches()
    with pytest.raises(ist.StitchError) as e:
        ist.find_overlaps([b])
    assert e.value.code == -1
    with pytest.raises(ist.StitchError) as e:
        ist.find_overlaps([b, turned])
    assert e.value.code == -7 and "image 1" in str(e.value)
    with pytest.raises(ist.StitchError) as e:
        ist.find_overlaps([b, b], tolerance=-1)
    assert e.value.code == -1
    out = (L.Overlap * 1)()
    assert L.lib.ist_bitmaps_overlap(S._ctx(0), None, 2, None, out) == -1
    assert L.lib.ist_bitmaps_overlap(S._ctx(0), (C.c_void_p * 2)(b.handle(), None), 2, None, out) == -6
    assert L.lib.ist_debug_overlap_launches() == launches       # refused before anything is enqueued
    assert ist.find_overlaps([b, b])[0]["overlap"] == 0         # the same shot twice: the bars take everything, no row is left to overlap
    _close([b, turned])
