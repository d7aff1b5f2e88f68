"""The GPU Huffman decoder (csrc/ist_jpeg_gpu.hip) where its synchronisation passes do not settle at once.  The files come from
tests/jpeg_sync_model.py (tests/test_jpeg_sync_model.py holds each to the regime it is named for, on the CPU); all are valid JPEGs.
Every file goes through ist.decode_files_device - the GPU-files counter must move, so a silent host fall-back cannot hide a bug -
and through the coefficient read-back (ist_debug_jpeg_gpu_coefficients): the coefficients must equal the writer's Frame EXACTLY, DC
included (the scans of the tallies, and the checkpoint's "new first leg + old second leg"), and the pixels PIL's bit for bit.  Where
a file's IDCT leaves frame_edges' range (the dense +-1 file, the blocks of 63 category-10 values) the clamp could hide a wrong
coefficient and PIL is no witness: those files are compared by coefficients only.  Pillow's own files have no Frame: pixels only.

The tests assert only brackets for the synchronisation launches (ist_debug_gpu_entropy_sync_launches), those that follow from
kInnerPasses and kMaxPasses.  Measured on an MI355X (LAB_NOTES.md section 1.2; in brackets what the CPU replay of the host loop,
tools/sim_slot_sync.cpp, gives for the files without restart intervals - the same everywhere):

  (a) pillow_keep_rgb_300x200 14 [14]   shared_420_300x200 3 [3]   shared_444_300x200 4 [4]   shared_420_restart40 3
      dense_pm1_deep_160x160 3 [3] (its DC values in +-40 instead of +-8: 2 [2])      control pillow_ycbcr_300x200 2 [2]
      dense_and_photo_stretches 4 [4, with 7 re-decodes that meet a checkpoint recorded in an earlier launch]
  (b) shared_444_noise_496 64 [64, no fixed point], the GPU hands it back; in a batch with four ordinary files 64, and the GPU keeps 0 of the 4
  (c) dense_pm1_deep_160x160 as in (a)   max_blocks_margin 3 [3]
  (d) deep_420 / deep_440, plain and restart7: 2 each      (e) dc_ramp_420, plain and restart500: 2 each
  (f) grey_127 / 128 / 129 / 256 / 257_sub, grey_tail_0, grey_tail_8, grey_restart1_short: 2 each
  (g) the 22 files of (a), (c), (d), (e), (f) in one call: 14, the slowest file's count
The whole module runs in 4 s.  A scratch library whose checkpoint forgot its luma DC sum between launches passed every JPEG test
that existed before this module, and every case here but dense_and_photo_stretches, whose coefficients it got wrong.

FINDING (b), recorded and not pinned: a file that has not reached the fixed point after kMaxPasses launches leaves EVERY ok[] of
its batch at 0, so today the four ordinary files decoded in one call with it all go to the host decoder (the GPU-files counter
moves by 0); the test asserts only that their pixels are right and that the counter moves by 0 to 4."""
import io

import numpy as np
import pytest
from PIL import Image

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import jpeg_sync_model as M

pytestmark = pytest.mark.gpu


def _pil(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))


def _counters():
    return L.lib.ist_debug_gpu_entropy_files(), L.lib.ist_debug_gpu_entropy_sync_launches()


def _moved(before):
    return tuple(b - a for a, b in zip(before, _counters()))


def _check_pixels(c, got):
    want = _pil(c["data"])
    assert got.shape == want.shape, c["name"]
    if not c["pixels"]:
        return                                           # coefficients only: the IDCT saturates
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() == 0, "%s: max diff %d in %d px, first at %s" % (c["name"], d.max(), int((d.max(-1) > 0).sum()), tuple(np.argwhere(d.max(-1) > 0)[0]))


def _check_coefficients(c, planes):
    if c["frame"] is None:
        return
    assert len(planes) == len(c["frame"].comps), c["name"]
    for k, (got, comp) in enumerate(zip(planes, c["frame"].comps)):
        want = comp["coef"]
        assert got.shape == want.shape, (c["name"], k)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%s: component %d: %d wrong coefficients, first at block (%d, %d) index %d: %d, expected %d" % (
            c["name"], k, len(bad), bad[0][0], bad[0][1], bad[0][2], got[tuple(bad[0])], want[tuple(bad[0])])


_ALONE = {}


def _alone(c):
    """one file by itself through both entry points, checked; the result is kept for the batch test"""
    if c["name"] in _ALONE:
        return _ALONE[c["name"]]
    before = _counters()
    out, imgs = ist.decode_files_device([c["data"]])
    files, launches = _moved(before)
    px = out[0].cpu().numpy()
    assert (imgs[0]["width"], imgs[0]["height"]) == (c["width"], c["height"]), c["name"]
    before = _counters()
    co = ist.debug_jpeg_gpu_coefficients(c["data"])
    assert _moved(before) == (0, co["launches"]), c["name"]                  # (the read-back counts launches, not files)
    assert co["launches"] == launches, (c["name"], co["launches"], launches)  # the same file alone: the same walk
    print("sync launches: %-28s %2d  (GPU took it: %s)" % (c["name"], launches, bool(files)))
    r = {"px": px, "files": files, "launches": launches, "ok": co["ok"], "planes": co["planes"]}
    _ALONE[c["name"]] = r
    if files:
        assert co["ok"], c["name"]
        _check_coefficients(c, co["planes"])
    _check_pixels(c, px)
    return r


def _taken(cases):
    for c in cases:
        r = _alone(c)
        assert r["files"] == 1 and r["ok"], "%s: the GPU decoder handed the file back" % c["name"]
        assert 2 <= r["launches"] <= M.K_MAX_PASSES, (c["name"], r["launches"])


SLOW = ("pillow_keep_rgb_300x200", "shared_420_300x200", "shared_444_300x200", "dense_pm1_deep_160x160", "shared_420_restart40")


@pytest.mark.parametrize("name", SLOW)
def test_a_several_launches_with_state_carried_across_them(name):
    """the four slow files, and shared tables with restart intervals longer than kInnerPasses subsequences: some workgroup needs more
    than kInnerPasses passes, so the second launch starts from start_p / checks / tally, the tid == 0 hand-over and the !settled flag
    of the first; the bracket is 3 <= launches <= kMaxPasses.

    The dense +-1 file reaches the bracket with its DC values in +-8; with +-40 the same file needs more than kInnerPasses passes
    in a workgroup too, but its re-decodes die out before any workgroup's last lane and 2 launches suffice, on the MI355X as in the
    CPU replay of the host loop (tools/sim_slot_sync.cpp; tests/jpeg_sync_model.py, _dense_pm1)."""
    (c,) = [c for c in M.slow_cases() if c["name"] == name]
    _taken([c])
    assert 3 <= _alone(c)["launches"] <= M.K_MAX_PASSES, (name, _alone(c)["launches"])


def test_a_checkpoint_recorded_in_an_earlier_launch():
    """dense stretches between photo stretches: re-decodes of a later launch meet checkpoints an earlier one recorded (7 in the
    CPU replay, several with four to six block starts in their first leg), so their tallies - block counts and DC sums - are the new first leg + the old second leg out of `checks` and `tally`"""
    _taken([M.carried_checkpoint_case()])


def test_a_control_settles_at_once():
    """the same picture with two table sets: its count is printed, not asserted"""
    _taken([M.control_case()])


def test_b_no_fixed_point_within_the_launch_budget():
    """alone: kMaxPasses launches, the file goes to the host decoder and its pixels are PIL's.  With four ordinary files in one call:
    every file's pixels are right; how many the GPU keeps (today: none, see the module docstring) is not pinned."""
    c = M.unsettled_case()
    r = _alone(c)
    assert r["launches"] == M.K_MAX_PASSES and r["files"] == 0 and not r["ok"]
    others = [M.deep_cases()[0], M.dc_cases()[0], M.geometry_cases()[2], M.control_case()]
    batch = others[:2] + [c] + others[2:]
    before = _counters()
    out, _ = ist.decode_files_device([x["data"] for x in batch])
    files, launches = _moved(before)
    print("sync launches: %-28s %2d  (GPU kept %d of the 4 ordinary files)" % ("batch with " + c["name"], launches, files))
    assert 0 <= files <= 4 and launches == M.K_MAX_PASSES
    for x, t in zip(batch, out):
        _check_pixels(x, t.cpu().numpy())


def test_c_blocks_longer_than_a_subsequence():
    """subsequences without a block start; a maximal block that starts in the last 64 bits of a workgroup and runs into the staged
    margin; a maximal block as the last of the scan (coefficients only)"""
    _taken(M.long_block_cases())


def test_d_general_step_at_scale():
    """codes of 10-16 bits in all four tables over several workgroups, plain and with restart intervals that start in mid-row"""
    _taken(M.deep_cases())


def test_e_dc_integration_across_workgroups():
    """DC ramps between -1016 and +1016 interleaved with the +-1016 alternation, over more than two workgroups, with and without
    restart intervals"""
    _taken(M.dc_cases())


def test_f_unit_geometry():
    """127 / 128 / 129 / 256 / 257 subsequences, whole subsequences, 8 bits behind a boundary, units shorter than the checkpoint"""
    _taken(M.geometry_cases())


def test_g_one_batch_equals_the_files_one_at_a_time():
    """(a), (c), (d), (e) and (f) in one call: byte-equal bitmaps, every file on the GPU, and as many launches as the slowest file
    alone - a unit's workgroups see only their own unit's state, and a settled unit raises no flag - not the sum"""
    cases = M.batch_cases()
    assert len(cases) <= 64
    alone = [_alone(c) for c in cases]
    before = _counters()
    out, _ = ist.decode_files_device([c["data"] for c in cases])
    files, launches = _moved(before)
    assert files == len(cases) == sum(r["files"] for r in alone)
    assert launches == max(r["launches"] for r in alone), (launches, [r["launches"] for r in alone])
    for c, t, r in zip(cases, out, alone):
        assert np.array_equal(t.cpu().numpy(), r["px"]), c["name"]
