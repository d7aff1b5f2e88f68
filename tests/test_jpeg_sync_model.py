"""The CPU model of the GPU Huffman decoder's geometry (tests/jpeg_sync_model.py) and the files built from it, held to their word
before any GPU sees them: the restated constants against the kernel's source text, the model's bit counts against the bytes the
writer actually wrote, every case against the regime it is named for, and - for the files that cannot settle in one launch - the
CPU replay of the kernel's pass iteration (tools/sim_slot_sync.cpp).  tests/test_gpu_jpeg_sync_regimes.py decodes the same files."""
import ctypes as C
import io
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_sync_model as M
from tests import jpeg_writer as JW
from tests.test_jpeg_writer import REF_BOUND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "imagestitching_amd", "csrc")


def test_constants_restate_the_kernel_source():
    src = open(os.path.join(CSRC, "ist_jpeg_gpu.hip"), encoding="utf-8").read()
    hdr = open(os.path.join(CSRC, "ist_jpeg.h"), encoding="utf-8").read()

    def define(name, text):
        return int(re.search(r"#define %s (\d+)\n" % name, text).group(1))

    def constant(name):
        return re.search(r"constexpr (?:int|uint32_t) %s = ([\w]+);" % name, src).group(1)

    assert constant("kSubBits") == "IST_SUB_BITS" and define("IST_SUB_BITS", src) == M.K_SUB_BITS
    assert constant("kSyncThreads") == "IST_SYNC_THREADS" and define("IST_SYNC_THREADS", src) == M.K_SYNC_THREADS
    assert int(constant("kInnerPasses")) == M.K_INNER_PASSES
    assert int(constant("kMaxPasses")) == M.K_MAX_PASSES
    assert int(constant("kCheckBits")) == M.K_CHECK_BITS
    assert int(constant("kMarginWords")) == M.K_MARGIN_WORDS
    assert re.search(r"constexpr int kJpegDcLookBits = (\d+), kJpegAcLookBits = IST_AC_LOOK_BITS;", hdr).group(1) == str(M.K_LOOK_BITS)
    assert define("IST_AC_LOOK_BITS", hdr) == M.K_LOOK_BITS
    # what the cases lean on: the pass loops are bounded by exactly these names
    assert "for (int it = 0; it < kInnerPasses; ++it)" in src and "for (int pass = 0; pass < kMaxPasses; ++pass)" in src


def _scan_units_from_bytes(data):
    """bits of every restart interval of the file's (single) scan, from the bytes: stuffing removed, RSTn cut, whole bytes"""
    at = data.index(b"\xff\xda")
    at += 2 + int.from_bytes(data[at + 2:at + 4], "big")
    units, n = [], 0
    while True:
        b = data[at]
        if b != 0xFF:
            n += 1; at += 1
        elif data[at + 1] == 0x00:
            n += 1; at += 2
        elif 0xD0 <= data[at + 1] <= 0xD7:
            units.append(8 * n); n = 0; at += 2
        elif data[at + 1] == 0xFF:
            at += 1
        else:
            units.append(8 * n)
            return units


GROUPS = {"slow": M.slow_cases, "carried": lambda: [M.carried_checkpoint_case()], "control": lambda: [M.control_case()], "unsettled": lambda: [M.unsettled_case()], "long_block": M.long_block_cases,
          "deep": M.deep_cases, "dc": M.dc_cases, "geometry": M.geometry_cases}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_file_is_what_the_model_says(group):
    """PIL decodes every file (to the writer's float64 reference where the IDCT stays in range), and the model's bits per unit are
    the bytes on disk"""
    for case in GROUPS[group]():
        _check_file(case)


def _check_file(case):
    px = np.asarray(Image.open(io.BytesIO(case["data"])).convert("RGB"))
    assert px.shape == (case["height"], case["width"], 3)
    if case["model"] is None:
        return
    assert [u["bits"] for u in case["model"]["units"]] == _scan_units_from_bytes(case["data"])
    assert JW.gpu_eligible(case["frame"], {}) and len(case["model"]["units"]) <= 2048
    if case["pixels"]:
        assert np.abs(px - JW.reference_rgb(case["frame"])).max() <= REF_BOUND


def test_a_slow_files_cannot_settle_in_one_launch():
    """regime: every MCU slot shares both tables (or no end of block marks the blocks), and a unit is longer than kInnerPasses
    subsequences - the truth walks it one subsequence per inner pass, so a third launch is needed"""
    for c in M.slow_cases():
        m = c["model"]
        if m is None:
            continue                                    # Pillow's file: the replay below is its witness
        assert m["max_unit_sub"] > M.K_INNER_PASSES, c["name"]
        assert m["n_sub"] <= M.K_INNER_PASSES * (M.K_MAX_PASSES - 2), c["name"]        # ... and it can be walked before kMaxPasses
        if c["name"].startswith("shared"):
            assert m["shared_tables"] and m["slots"] >= 3, c["name"]
        else:
            assert m["slots"] == 1 and min(u["longest_block"] for u in m["units"]) > M.K_SUB_BITS, c["name"]
    r = {c["name"]: c for c in M.slow_cases()}["shared_420_restart40"]["model"]
    assert len(r["units"]) >= 6 and sum(u["n_sub"] > M.K_INNER_PASSES for u in r["units"]) >= 5


def test_b_unsettled_file_outruns_the_launch_budget():
    """regime: shared tables and a quarter more subsequences than kMaxPasses launches of kInnerPasses passes can walk"""
    c = M.unsettled_case()
    m = c["model"]
    assert m["shared_tables"] and m["slots"] == 3 and len(m["units"]) == 1
    assert m["n_sub"] >= M.K_MAX_PASSES * M.K_INNER_PASSES * 5 // 4
    assert m["n_sub"] <= M.K_MAX_PASSES * M.K_INNER_PASSES * 3 // 2 and max(c["width"], c["height"]) <= 640     # ... and no larger than that takes


def test_c_blocks_longer_than_a_subsequence():
    dense, edge = M.long_block_cases()
    u = dense["model"]["units"][0]
    assert u["longest_block"] > M.K_SUB_BITS and len(u["subs_without_block_start"]) >= 10
    assert dense["model"]["long_codes"][(1, 0)] == 1.0                       # every AC code takes the general step
    u = edge["model"]["units"][0]
    starts, at = u["block_start"], edge["target_block"]
    lengths = np.diff(np.append(starts, u["coded_bits"]))
    wg_end = M.K_SYNC_THREADS * M.K_SUB_BITS
    # a block of the maximum length under the Annex K tables: a DC difference of category 11 (9 + 11 bits) and 63 x (16 + 10)
    assert lengths[at] == 20 + 63 * 26 == u["longest_block"]
    assert wg_end - 64 <= starts[at] < wg_end, "the block starts in the last 64 bits of the first workgroup"
    assert starts[at] + lengths[at] > wg_end + M.K_SUB_BITS and starts[at] + lengths[at] <= wg_end + 32 * M.K_MARGIN_WORDS
    assert lengths[-1] == 20 + 63 * 26 and u["workgroups"] == 2, "... and another one ends the scan"
    assert len(u["subs_without_block_start"]) >= 10


def test_d_deep_tables_miss_the_look_ahead_in_all_four_tables():
    for c in M.deep_cases():
        m = c["model"]
        assert sorted(m["long_codes"]) == [(0, 0), (0, 1), (1, 0), (1, 1)], c["name"]
        assert all(share > 0.05 for share in m["long_codes"].values()), (c["name"], m["long_codes"])
        if "restart" in c["name"]:
            mcus_x = -(-c["width"] // (8 * c["frame"].hmax))
            assert 7 % mcus_x != 0 and len(m["units"]) > 30, c["name"]      # intervals start in mid-row
        else:
            assert m["workgroups"] >= 3, c["name"]


def test_e_dc_ramps_span_workgroups():
    plain, restart = M.dc_cases()
    assert plain["model"]["workgroups"] > 2 and len(plain["model"]["units"]) == 1
    assert len(restart["model"]["units"]) == 3 and max(u["workgroups"] for u in restart["model"]["units"]) >= 2
    for comp in plain["frame"].comps:
        dc = comp["coef"][..., 0].reshape(-1)
        assert dc.min() == -1016 and dc.max() == 1016
        assert np.abs(np.diff(dc)).max() == 2032                             # DC differences of category 11
        assert len(np.unique(dc)) > 100                                      # ... and a ramp in between


def test_f_unit_geometry():
    cases = {c["name"]: c["model"]["units"] for c in M.geometry_cases()}
    for n_sub in (127, 128, 129, 256, 257):
        (u,) = cases["grey_%d_sub" % n_sub]
        assert u["n_sub"] == n_sub and u["workgroups"] == -(-n_sub // M.K_SYNC_THREADS)
    assert cases["grey_tail_0"][0]["whole_subsequences"] and cases["grey_tail_0"][0]["n_sub"] == 5
    assert cases["grey_tail_8"][0]["tail_bits"] == 8 and cases["grey_tail_8"][0]["n_sub"] == 6
    short = cases["grey_restart1_short"]
    assert len(short) >= 8 and all(u["short"] and u["blocks"] == 1 for u in short)


def test_g_batch_fits_one_call():
    names = [c["name"] for c in M.batch_cases()]
    assert len(names) == len(set(names)) and 20 <= len(names) <= 64


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    d = tmp_path_factory.mktemp("sim")
    exe = str(d / "sim_slot_sync")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "sim_slot_sync.cpp"),
                    os.path.join(CSRC, "ist_jpeg.cpp"), "-o", exe, "-lpthread"], check=True, capture_output=True, timeout=300)

    def run(case):
        p = d / (case["name"] + ".jpg")
        p.write_bytes(case["data"])
        out = subprocess.run([exe, str(p)], check=True, capture_output=True, text=True, timeout=120).stdout
        m = re.search(r"^SYNC nsub=(\d+) slots=(\d+) worst_passes=(\d+) pass_cap=(\d+) launches=(\d+) fixed_point=([01]) carried_checkpoint_hits=(\d+) at=\[([\d,]*)\] slot_wrong_exit_slot_wrong=([0-9.]+) guess_exit_true=([0-9.]+)$", out, re.M)
        assert m, out
        return {"nsub": int(m.group(1)), "slots": int(m.group(2)), "worst": int(m.group(3)), "cap": int(m.group(4)),
                "launches": int(m.group(5)), "fixed_point": m.group(6) == "1", "carried_hits": int(m.group(7)), "carried_at": [int(x) for x in m.group(8).split(",") if x],
                "slot_wrong": float(m.group(9)), "guess_true": float(m.group(10))}
    return run


def test_replay_agrees_that_the_slow_files_are_slow(replay):
    """the kernel's pass iteration, replayed on the CPU: some workgroup of every slow file needs more than kInnerPasses passes, the
    control settles in a handful, and a shared-table file started in a wrong slot ALWAYS leaves in a wrong slot"""
    slow = [c for c in M.slow_cases() if "restart" not in c["name"]] + [M.unsettled_case(), M.long_block_cases()[1]]      # (the replay takes scans without intervals)
    for c in slow:
        r = replay(c)
        assert r["worst"] > M.K_INNER_PASSES and r["cap"] >= r["worst"], (c["name"], r)
        if c["model"] is not None:
            assert r["nsub"] == c["model"]["n_sub"] and r["slots"] == c["model"]["slots"], (c["name"], r)
        if c["name"].startswith(("shared", "pillow_keep_rgb")):
            assert r["slot_wrong"] == 1.0, (c["name"], r)
        else:
            assert r["guess_true"] < 0.2, (c["name"], r)
        # the host loop replayed (the replay also checks that its fixed point is the true states).  A slot-ambiguous file walks to
        # the last lane of every workgroup, so a third launch follows; so do the dense +-1 file's chains with its DC values in +-8
        # (with +-40 they die out inside the workgroups and 2 launches suffice: jpeg_sync_model._dense_pm1)
        if c is M.unsettled_case():
            assert not r["fixed_point"] and r["launches"] == M.K_MAX_PASSES, (c["name"], r)
        else:
            assert r["fixed_point"] and 3 <= r["launches"] <= M.K_MAX_PASSES, (c["name"], r)
    r = replay(M.control_case())
    assert r["worst"] < M.K_INNER_PASSES // 4 and r["slot_wrong"] == 0.0 and r["fixed_point"] and r["launches"] == 2, r
    assert replay(M.slow_cases()[0])["nsub"] > M.K_INNER_PASSES * 3           # Pillow's RGB file: no model, the replay counts


def test_replay_meets_checkpoints_recorded_in_an_earlier_launch(replay):
    """regime: a re-decode in a later launch arrives at its checkpoint in the state an earlier launch recorded, so its tally is made
    from `checks` and `tally` carried across launches.  The slot-ambiguous files never do (their re-decodes differ in the slot)."""
    c = M.carried_checkpoint_case()
    r = replay(c)
    assert r["fixed_point"] and r["carried_hits"] >= 4 and 3 <= r["launches"] <= M.K_MAX_PASSES, r
    # ... and the first legs of some of them hold several block starts (DC symbols): the DC sums of the tally are handed over too
    starts = c["model"]["units"][0]["block_start"]
    in_first_leg = [int(((starts >= i * M.K_SUB_BITS) & (starts < i * M.K_SUB_BITS + M.K_CHECK_BITS)).sum()) for i in set(r["carried_at"])]
    assert sum(n >= 4 for n in in_first_leg) >= 3, (r["carried_at"], in_first_leg)
    for c in M.slow_cases()[1:3]:
        assert replay(c)["carried_hits"] == 0, c["name"]


def test_coefficient_read_back_abi_without_a_device():
    """declared, bound, laid out alike; the geometry query needs no device; argument errors first; never a CPU fall-back"""
    import torch
    from imagestitching_amd import _lib as L
    import imagestitching_amd as ist
    src = open(os.path.join(ROOT, "include", "imagestitch.h"), encoding="utf-8").read()
    for name in ("ist_debug_gpu_entropy_sync_launches", "ist_debug_jpeg_gpu_coefficients"):
        assert re.search(r"IST_API\s+\w+\s+%s\(" % name, src) and hasattr(L.lib, name)
    assert C.sizeof(L.JpegCoefInfo) == 40
    assert isinstance(L.lib.ist_debug_gpu_entropy_sync_launches(), int)
    c = M.dc_cases()[0]
    info = L.JpegCoefInfo()
    assert L.lib.ist_debug_jpeg_gpu_coefficients(None, c["data"], len(c["data"]), None, None, C.byref(info)) == 0
    assert info.ncomp == 3 and [(info.blocks_y[k], info.blocks_x[k]) for k in range(3)] == [comp["coef"].shape[:2] for comp in c["frame"].comps]
    assert L.lib.ist_debug_jpeg_gpu_coefficients(None, None, 0, None, None, C.byref(info)) == -1
    assert L.lib.ist_debug_jpeg_gpu_coefficients(None, c["data"], len(c["data"]), None, None, None) == -1
    planes = [np.zeros(comp["coef"].shape, np.int16) for comp in c["frame"].comps]
    ptrs = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    small = (C.c_int64 * 3)(planes[0].size - 1, planes[1].size, planes[2].size)
    assert L.lib.ist_debug_jpeg_gpu_coefficients(None, c["data"], len(c["data"]), ptrs, small, C.byref(info)) == -1 and "plane 0" in L.last_error()
    full = (C.c_int64 * 3)(*[p.size for p in planes])
    assert L.lib.ist_debug_jpeg_gpu_coefficients(None, c["data"], len(c["data"]), ptrs, full, C.byref(info)) == -4          # no context
    two_scans = JW.write_jpeg(c["frame"], scans=[[0], [1, 2]])
    assert L.lib.ist_debug_jpeg_gpu_coefficients(None, two_scans, len(two_scans), None, None, C.byref(info)) == -7
    if not torch.cuda.is_available():
        with pytest.raises(ist.StitchError) as e:
            ist.debug_jpeg_gpu_coefficients(c["data"])
        assert e.value.code == -5
