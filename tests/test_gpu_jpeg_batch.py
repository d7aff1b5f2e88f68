"""Batched JPEG export on the GPU (ist_jpeg_encode_batch_device / encode_jpeg_batch_device, ist_stitch_jpeg_batch /
stitch_jpeg_batch): every file of a batch equals tests/jpeg_encode_reference.py byte for byte, and so the file the single-file encoder
writes.  Each file is the export step of one unchanged onStitch with fileType 'jpg' (utils/canvas.js:205-221).

Shapes are the smallest that reach each thing that can go wrong in a batch: one-workgroup files first, last and between larger ones
(the edges of the piece search), partial MCUs, more than eight intervals, an interval of eight entropy batches, pitched canvases,
rounds that split a file and rounds that hold several files, sub-batches that reuse both halves."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import jpeg_encode_reference as R
from tests import util as U
from tests.test_gpu_jpeg_encode import checker, first_difference, noise, photo

pytestmark = pytest.mark.gpu

ROOT = U.ROOT
LAYOUTS = ("420", "444")
J = {"444": 0, "420": 1}


@pytest.fixture(scope="module")
def ist():
    import imagestitching_amd
    return imagestitching_amd


def _lib():
    from imagestitching_amd import _lib as L
    return L


def _counters():
    L = _lib()
    return L.lib.ist_debug_jpeg_batch_launches(), L.lib.ist_debug_jpeg_encode_launches()


def _same(got, want, what):
    assert got == want, "%s: %s" % (what, first_difference(got, want))


def _encode_batch(ist, files, pitched=False):
    """files: [(pixels, quality, layout)] -> the batch's files as bytes (canvases pitched on request: every other one)"""
    import torch
    cans = []
    for k, (a, _, _) in enumerate(files):
        h, w = a.shape[:2]
        if pitched and k % 2 == 0:
            wide = torch.full((h, w + 3 + k, 4), 0xEE, dtype=torch.uint8, device="cuda")
            wide[:, :w] = torch.from_numpy(a).cuda()
            cans.append(wide[:, :w])
            assert cans[-1].stride(0) == 4 * (w + 3 + k)
        else:
            cans.append(torch.from_numpy(a).cuda())
    res = ist.encode_jpeg_batch_device(cans, [q for _, q, _ in files], [s for _, _, s in files])
    torch.cuda.synchronize()
    out = []
    for t, n in res:
        b = t.cpu().numpy().tobytes()
        assert len(b) == n
        out.append(b)
    return out, cans


def _mixed_files():
    """one-workgroup files (1x1, 7x9, 16x16 in 4:2:0; 1x1, 7x9 in 4:4:4) first, last and between the larger ones; layouts and qualities
    interleaved per file"""
    return [(photo(1, 1), 1, "420"), (photo(33, 170), 50, "444"), (photo(7, 9), 90, "420"), (noise(100, 150), 100, "420"),
            (photo(16, 16), 100, "420"), (photo(100, 150), 50, "444"), (photo(1, 1), 50, "444"), (checker(48, 40), 100, "420"),
            (photo(17, 33), 1, "444"), (photo(33, 170), 90, "420"), (np.full((40, 50, 4), 200, np.uint8), 50, "420"), (noise(100, 150), 100, "444"),
            (photo(17, 33), 90, "420"), (photo(100, 150), 50, "420"), (checker(48, 40), 100, "444"), (np.full((40, 50, 4), 200, np.uint8), 1, "444"),
            (photo(16, 16), 50, "444"), (photo(7, 9), 100, "444")]


def test_one_mixed_call(ist):
    import torch
    files = _mixed_files()
    assert {q for _, q, _ in files} == {1, 50, 90, 100}
    batch, single = _counters()
    got, cans = _encode_batch(ist, files)
    assert _counters() == (batch + 1, single)
    for k, ((a, q, layout), g, c) in enumerate(zip(files, got, cans)):
        what = "file %d (%dx%d Q%d %s)" % (k, a.shape[1], a.shape[0], q, layout)
        _same(g, R.encode(a, q, layout), what)
        t, n = ist.encode_jpeg_device(c, q, layout)
        torch.cuda.synchronize()
        _same(g, t.cpu().numpy().tobytes(), what + " against encode_jpeg_device")
    # what the contents are there for
    assert b"\xff\x00" in got[3] and got[9].count(b"\xff\xd0") >= 2 and got[1].count(b"\xff\xd7") >= 1


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_long_interval_between_two_small_files(ist, layout):
    """4805 x 19: one interval of eight batches of the entropy kernel"""
    files = [(photo(7, 9), 90, layout), (photo(4805, 19), 50, layout), (photo(17, 33), 100, layout)]
    got, _ = _encode_batch(ist, files)
    for k, ((a, q, s), g) in enumerate(zip(files, got)):
        _same(g, R.encode(a, q, s), "file %d" % k)


def test_pitched_views_and_alpha(ist):
    rng = np.random.default_rng(11)
    files = []
    for k, (w, h) in enumerate(((37, 21), (7, 9), (50, 33), (16, 16), (33, 40), (1, 1))):
        a = photo(w, h, seed=k)
        if k % 4 < 2:                                       # random alpha in half the files, pitched or not: alpha is not read
            a[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
        files.append((a, (90, 50, 100)[k % 3], LAYOUTS[k % 2]))
    got, _ = _encode_batch(ist, files, pitched=True)
    for k, ((a, q, s), g) in enumerate(zip(files, got)):
        opaque = a.copy()
        opaque[..., 3] = 255
        _same(g, R.encode(opaque, q, s), "file %d" % k)


ROUND_SIZES = ((33, 170), (7, 9), (33, 700), (17, 33))
ROUND_BUDGET = 40000


def _layout(sizes, budget):
    """[(file, round, mcu_row0, mcu_rows)] of ist_jpeg_batch_layout"""
    L = _lib()

    class Piece(C.Structure):
        _fields_ = [("file", C.c_int32), ("round", C.c_int32), ("mcu_row0", C.c_int32), ("mcu_rows", C.c_int32)]

    n = len(sizes)
    w, h, ss = (C.c_int64 * n)(*[s[0] for s in sizes]), (C.c_int64 * n)(*[s[1] for s in sizes]), (C.c_int * n)(*[J[s[2]] for s in sizes])
    count = L.lib.ist_jpeg_batch_layout(w, h, ss, n, budget, None, 0)
    assert count > 0
    buf = (Piece * count)()
    assert L.lib.ist_jpeg_batch_layout(w, h, ss, n, budget, C.cast(buf, C.c_void_p), count) == count
    return [(p.file, p.round, p.mcu_row0, p.mcu_rows) for p in buf]


def test_rounds(tmp_path):
    """a 40 000 byte budget: files that span rounds, rounds that hold several files.  The override is read once, in tuning mode, so the
    encodes run in a process of their own."""
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import torch
import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests.test_gpu_jpeg_batch import ROUND_SIZES, LAYOUTS, _layout
from tests.test_gpu_jpeg_encode import photo
sizes = [(w, h, s) for s in LAYOUTS for w, h in ROUND_SIZES]
cans = [torch.from_numpy(photo(w, h)).cuda() for w, h, s in sizes]
before = L.lib.ist_debug_jpeg_batch_launches(), L.lib.ist_debug_jpeg_encode_launches()
res = ist.encode_jpeg_batch_device(cans, [90, 50, 100, 1] * 2, [s for w, h, s in sizes])
torch.cuda.synchronize()
print("launches", L.lib.ist_debug_jpeg_batch_launches() - before[0], L.lib.ist_debug_jpeg_encode_launches() - before[1])
print("rounds", _layout(sizes, 0)[-1][1] + 1)
np.savez(sys.argv[1], **{"f%%d" %% k: t.cpu().numpy() for k, (t, n) in enumerate(res)})
""" % (ROOT,)
    sizes = [(w, h, s) for s in LAYOUTS for w, h in ROUND_SIZES]
    pieces = _layout(sizes, ROUND_BUDGET)
    rounds = pieces[-1][1] + 1
    assert any(len({r for f, r, _, _ in pieces if f == k}) > 1 for k in range(len(sizes)))          # a file spans rounds
    assert any(len({f for f, r, _, _ in pieces if r == k}) > 1 for k in range(rounds))              # a round holds several files
    env = dict(os.environ, IST_TUNING="1", IST_JPEG_ENC_BUDGET=str(ROUND_BUDGET))
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "launches %d 0\n" % rounds in r.stdout and "rounds %d\n" % rounds in r.stdout, (rounds, r.stdout)
    got = np.load(tmp_path / "out.npz")
    for k, ((w, h, s), q) in enumerate(zip(sizes, [90, 50, 100, 1] * 2)):
        _same(got["f%d" % k].tobytes(), R.encode(photo(w, h), q, s), "file %d (%dx%d Q%d %s)" % (k, w, h, q, s))


def _img(a, opaque=True):
    return {"width": a.shape[1], "height": a.shape[0], "data": a, "opaque": opaque}


def _requests(seed):
    """seeded random requests, all under 300 px a side but one of three images about 4000 px wide; requests without images; quality and
    subsampling vary per request (and are left to their defaults in some)"""
    rng = np.random.default_rng(seed)
    reqs = [([_img(U.rand_image(seed, 1, 1))], "vertical", {"quality": 100, "subsampling": "444"}),
            ([_img(U.smooth_image(seed + k, 40, 1300 + 40 * k)) for k in range(3)], "horizontal", {"quality": 50}),
            ([], "horizontal", {"quality": 30}),
            ([_img(U.rand_image(seed + 4, 40, 50, opaque=False), False), _img(U.rand_image(seed + 5, 30, 70, opaque=False), False)],
             "horizontal", {"gap": 3, "subsampling": "444"}),
            ([], "vertical"),
            ([_img(U.smooth_image(seed + 6, 150, 60)), _img(U.smooth_image(seed + 7, 140, 60))], "vertical")]
    for k in range(int(rng.integers(4, 8))):
        n = int(rng.integers(1, 4))
        px = [U.smooth_image(seed * 100 + 10 * k + i, int(rng.integers(5, 100)), int(rng.integers(5, 290)), opaque=bool(rng.random() < 0.7))
              for i in range(n)]
        reqs.append(([_img(a, bool(a[..., 3].min() == 255)) for a in px], str(rng.choice(["vertical", "horizontal"])),
                     {"filter": str(rng.choice(["nearest", "bilinear", "area"])), "mode": str(rng.choice(["min", "max", "original"])),
                      "gap": int(rng.choice([0, 4])), "quality": int(rng.choice([1, 35, 75, 90, 100])), "subsampling": str(rng.choice(LAYOUTS))}))
    order = rng.permutation(len(reqs))
    return [reqs[i] for i in order]


def _jpeg_opts(r):
    o = dict(r[2]) if len(r) == 3 else {}
    return o.pop("quality", 90), o.pop("subsampling", "420"), o


def _check_requests(ist, reqs, files):
    """files[k]: the batch's file of request k (bytes) or None"""
    assert len(files) == len(reqs)
    for k, r in enumerate(reqs):
        if not r[0]:
            assert files[k] is None, k
            continue
        q, s, o = _jpeg_opts(r)
        canvas = ist.stitch(r[0], r[1], o)
        _same(files[k], R.encode(canvas["data"], q, s), "request %d against the reference" % k)
        _same(files[k], ist.stitch_jpeg(*r)["jpeg"], "request %d against stitch_jpeg" % k)


def test_stitch_jpeg_batch_equals_the_loop(ist):
    reqs = _requests(7)
    assert any(r[0] and sum(im["width"] for im in r[0]) > 3900 for r in reqs) and any(not r[0] for r in reqs)
    batch, single = _counters()
    got = ist.stitch_jpeg_batch(reqs)
    assert _counters() == (batch + 1, single)               # one sub-batch, one round
    for k, (r, g) in enumerate(zip(reqs, got)):
        if g is not None:
            canvas = ist.stitch(r[0], r[1], _jpeg_opts(r)[2])
            assert (g["width"], g["height"]) == (canvas["width"], canvas["height"]), k
    _check_requests(ist, reqs, [None if g is None else g["jpeg"] for g in got])


SUB_BATCH_BYTES = 600000


def _sub_batches(ist, reqs, budget):
    """the rule of ist_batch.cpp: consecutive live requests while sources + canvas + file bound fit the budget"""
    L = _lib()
    count, held = 0, 0
    for r in reqs:
        if not r[0]:
            continue
        q, s, o = _jpeg_opts(r)
        p = ist.plan([{k: v for k, v in im.items() if k != "data"} for im in r[0]], r[1], o)
        need = p.canvas_w * p.canvas_h * 4 + sum(im["width"] * im["height"] * 4 for im in r[0]) + L.lib.ist_jpeg_bound(p.canvas_w, p.canvas_h, J[s])
        if count == 0 or held + need > budget:
            count, held = count + 1, 0
        held += need
    return count


def test_sub_batches_reuse_both_halves(ist, tmp_path):
    """IST_BATCH_BYTES is read once, in tuning mode: the batch runs in a process of its own"""
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests.test_gpu_jpeg_batch import _requests
reqs = _requests(19)
before = L.lib.ist_debug_jpeg_batch_launches()
got = ist.stitch_jpeg_batch(reqs)
print("launches", L.lib.ist_debug_jpeg_batch_launches() - before)
np.savez(sys.argv[1], **{"f%%d" %% k: np.frombuffer(g["jpeg"], np.uint8) for k, g in enumerate(got) if g is not None})
""" % (ROOT,)
    reqs = _requests(19)
    subs = _sub_batches(ist, reqs, SUB_BATCH_BYTES)
    assert subs >= 4, subs                                  # half 0, half 1, and each of them again
    env = dict(os.environ, IST_TUNING="1", IST_BATCH_BYTES=str(SUB_BATCH_BYTES))
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    launches = int(r.stdout.split("launches")[1].split()[0])
    assert launches >= subs, (launches, subs)
    got = np.load(tmp_path / "out.npz")
    _check_requests(ist, reqs, [got["f%d" % k].tobytes() if ("f%d" % k) in got.files else None for k in range(len(reqs))])


def test_a_failing_request_fails_the_whole_batch_and_the_next_one_succeeds(ist):
    from imagestitching_amd.stitch import _batch_requests, _ctx
    L = _lib()
    reqs = _requests(41)
    live = [k for k, r in enumerate(reqs) if r[0]]
    creqs, keep = _batch_requests([(r[0], r[1], _jpeg_opts(r)[2]) for r in reqs], "")
    bad = live[len(live) // 2]
    creqs[bad].src[0] = None                                # request `bad`: its first image has no buffer
    n = len(reqs)
    plans, outs, lens = (L.Plan * n)(), (C.POINTER(C.c_uint8) * n)(), (C.c_int64 * n)()
    qs, ss = (C.c_int * n)(*[_jpeg_opts(r)[0] for r in reqs]), (C.c_int * n)(*[J[_jpeg_opts(r)[1]] for r in reqs])
    rc = L.lib.ist_stitch_jpeg_batch(_ctx(0), creqs, n, qs, ss, plans, outs, lens)
    assert rc == -6 and ("request %d" % bad) in L.last_error(), (rc, L.last_error())
    assert all(not outs[k] for k in range(n)) and all(lens[k] == 0 for k in range(n))
    assert all(plans[k].canvas_w == 0 and not plans[k].rects for k in range(n))
    got = ist.stitch_jpeg_batch(reqs)
    _check_requests(ist, reqs, [None if g is None else g["jpeg"] for g in got])


def test_a_second_identical_call_allocates_nothing(ist):
    import torch
    L = _lib()
    reqs = _requests(53)
    cans = [torch.from_numpy(photo(w, h)).cuda() for w, h in ((64, 48), (7, 9), (100, 30))]
    outs = [torch.empty(int(L.lib.ist_jpeg_bound(int(c.shape[1]), int(c.shape[0]), 1)) + 16, dtype=torch.uint8, device="cuda") for c in cans]
    ist.stitch_jpeg_batch(reqs)
    ist.encode_jpeg_batch_device(cans, outs=outs)
    before = L.lib.ist_debug_device_allocs()
    got = ist.stitch_jpeg_batch(reqs)
    files = ist.encode_jpeg_batch_device(cans, outs=outs)
    assert L.lib.ist_debug_device_allocs() == before
    assert all((g is None) == (not r[0]) for g, r in zip(got, reqs))
    torch.cuda.synchronize()
    for (t, n), (w, h) in zip(files, ((64, 48), (7, 9), (100, 30))):
        _same(t.cpu().numpy().tobytes(), R.encode(photo(w, h), 90, "420"), "%dx%d" % (w, h))
