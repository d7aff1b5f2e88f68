"""Batched stitching on the GPU (ist_jobs_launch / launch_jobs, ist_stitch_rgba8_batch / stitch_batch, the Node stitchBatch): every
entry of a batch is one unchanged onStitch (pages/index/index.js:1186-1633), so every entry must be byte-identical to the same job
launched alone - which the single-job tests pin to the oracle - and every entry is checked against the oracle here as well."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from imagestitching_amd.stitch import _filter_of, _merge
from tests import cubic_reference as R
from tests import util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON_A, POISON_B, GUARD = 0xAB, 0x5C, 0xCD


def _batch_launches():
    return L.lib.ist_debug_batch_launches()


def _rand_entry(rng, k):
    """one random stitch: (pixels, orientations, direction, opts, clip or None)"""
    n = int(rng.integers(1, 5))
    opaque = bool(rng.random() < 0.6)
    px = [U.rand_image(1000 * k + i, int(rng.integers(6, 180)), int(rng.integers(6, 180)), opaque=opaque) for i in range(n)]
    ori = [int(v) for v in rng.integers(1, 9, n)] if rng.random() < 0.4 else [1] * n
    opts = {"mode": str(rng.choice(["min", "max", "original"])), "gap": int(rng.choice([0, 0, 3, 8])),
            "filter": str(rng.choice(["nearest", "bilinear", "area", "cubic"]))}
    if rng.random() < 0.25:
        opts["edgeAA"] = True
    if rng.random() < 0.5:
        opts["superSample"] = 2.2                             # (a canvas 2.2x as large: most draws are enlarged, which under 'cubic' is the streamed Catmull-Rom path)
    direction = str(rng.choice(["vertical", "horizontal"]))
    clip = None
    if rng.random() < 0.25:
        p = ist.plan(U.hip_images(px, ori), direction, opts)
        x0, y0 = int(rng.integers(0, p.canvas_w)), int(rng.integers(0, p.canvas_h))
        clip = (x0, y0, int(rng.integers(1, p.canvas_w - x0 + 1)), int(rng.integers(1, p.canvas_h - y0 + 1)))
    return px, ori, direction, opts, clip


def _compile(st, px, ori, direction, opts, clip=None):
    o = _merge(opts)
    p = ist.plan(U.hip_images(px, ori), direction, o)
    ops, n = p.ops()
    return p, st.compile_ops(p.canvas_w, p.canvas_h, ops, n, p._descs, len(px), _filter_of(o), clip=clip)


def _canvases(shapes, pads, poison):
    """canvases cut from ONE allocation: guard gaps of GUARD bytes between them, row pitch = width * 4 + pad"""
    gap = 4096
    offs, at = [], gap
    for (h, w), pad in zip(shapes, pads):
        offs.append(at)
        at += h * (w * 4 + pad)
        at = (at + 255) // 256 * 256 + gap
    raw = torch.full((at,), GUARD, dtype=torch.uint8, device=DEV)
    views = []
    for (h, w), pad, off in zip(shapes, pads, offs):
        pitch = w * 4 + pad
        views.append(raw[off:off + h * pitch].view(h, pitch)[:, :w * 4].view(h, w, 4))
        raw[off:off + h * pitch].fill_(poison)
    mask = torch.ones(at, dtype=torch.bool, device=DEV)
    for (h, w), pad, off in zip(shapes, pads, offs):
        mask[off:off + h * (w * 4 + pad)] = False
    return raw, views, mask


def _single(job, srcs, shape, pad, poison):
    _, (out,), _ = _canvases([shape], [pad], poison)
    job.launch(srcs, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _entries(seed, count, st):
    rng = np.random.default_rng(seed)
    es = []
    for k in range(count):
        px, ori, direction, opts, clip = _rand_entry(rng, seed * 100 + k)
        p, job = _compile(st, px, ori, direction, opts, clip)
        srcs = [torch.from_numpy(a).to(DEV) for a in px]
        pad = int(rng.choice([0, 0, 4, 64, 4096]))
        es.append({"px": px, "ori": ori, "direction": direction, "opts": opts, "clip": clip, "plan": p, "job": job, "srcs": srcs,
                   "shape": (p.canvas_h, p.canvas_w), "pad": pad})
    return es


@pytest.mark.parametrize("seed,count", [(1, 1), (2, 7), (3, 23), (4, 64)])
def test_random_batches_match_single_launches_write_every_clip_pixel_and_keep_the_guards(seed, count):
    st = ist.Stitcher(0)
    es = _entries(seed, count, st)
    shapes, pads = [e["shape"] for e in es], [e["pad"] for e in es]
    results = []
    for poison in (POISON_A, POISON_B):
        raw, outs, guard = _canvases(shapes, pads, poison)
        before = _batch_launches()
        ist.launch_jobs([e["job"] for e in es], [e["srcs"] for e in es], outs)
        torch.cuda.synchronize()
        assert 1 <= _batch_launches() - before <= 7           # one launch per kernel kind: five, and the two of cubic jobs (5: streamed cubic, 6: + the per-pixel stack)
        assert bool((raw[guard] == GUARD).all()), "a byte outside every canvas changed"
        results.append([o.cpu().numpy() for o in outs])
    for k, e in enumerate(es):
        want = _single(e["job"], e["srcs"], e["shape"], e["pad"], POISON_A)
        assert np.array_equal(results[0][k], want), "entry %d differs from its single launch" % k
        inside = np.zeros(e["shape"], bool)
        x0, y0, w, h = e["clip"] if e["clip"] else (0, 0, e["shape"][1], e["shape"][0])
        inside[y0:y0 + h, x0:x0 + w] = True
        assert np.array_equal(results[0][k][inside], results[1][k][inside]), "entry %d: a clip pixel was not written" % k
        assert (results[1][k][~inside] == POISON_B).all() and (results[0][k][~inside] == POISON_A).all(), "entry %d: wrote outside its clip" % k
    # every entry against the oracle (area, cubic, edge AA and clipped entries included: the reference cropped to the clip): nearest
    # without AA exact, otherwise the op-list rule, and differences rare
    stats = U.RareDiff()
    for k, e in enumerate(es):
        if e["opts"]["filter"] == "cubic":         # (the oracle does not know the filter: the fp64 reference of tests/cubic_reference.py on the plan's ops)
            p = e["plan"]
            ref = R.render_ops(p.canvas_w, p.canvas_h, R.plan_ops(p), None, e["px"], "cubic", edge_aa=U.edge_aa_of(e["opts"]))
        else:
            ref, _, _ = U.oracle_stitch(e["px"], e["direction"], e["opts"], e["ori"])
        assert ref.shape[:2] == e["shape"] and (ref[..., 3] == 255).all()          # a strip is filled white first: every pixel is solid (within 1 LSB, or exact)
        x0, y0, w, h = e["clip"] if e["clip"] else (0, 0, e["shape"][1], e["shape"][0])
        exact = e["opts"]["filter"] == "nearest" and not e["opts"].get("edgeAA")
        try:
            stats.add(U.oracle_tolerance(results[0][k][y0:y0 + h, x0:x0 + w], ref[y0:y0 + h, x0:x0 + w], exact))
        except AssertionError as err:
            raise AssertionError("entry %d vs the oracle (%s, %r, clip %r): %s" % (k, e["direction"], e["opts"], e["clip"], err))
    stats.check()


def test_entries_may_share_sources():
    st = ist.Stitcher(0)
    px = [U.smooth_image(300 + i, 90 + 13 * i, 120 - 7 * i, opaque=(i != 1)) for i in range(3)]
    srcs = [torch.from_numpy(a).to(DEV) for a in px]
    cases = [("vertical", {"filter": "bilinear"}), ("horizontal", {"filter": "nearest", "gap": 4}), ("vertical", {"filter": "area", "mode": "max"}),
             ("horizontal", {"filter": "bilinear", "mode": "original", "gap": 2}), ("vertical", {"filter": "bilinear", "edgeAA": True, "gap": 5})]
    jobs, plans = [], []
    for d, o in cases:
        p, j = _compile(st, px, [1, 6, 3], d, o)
        jobs.append(j); plans.append(p)
    shapes = [(p.canvas_h, p.canvas_w) for p in plans]
    raw, outs, guard = _canvases(shapes, [0] * len(shapes), POISON_A)
    ist.launch_jobs(jobs, [srcs] * len(jobs), outs)          # the same device pointers in every entry
    torch.cuda.synchronize()
    assert bool((raw[guard] == GUARD).all())
    for k, (j, s) in enumerate(zip(jobs, shapes)):
        assert np.array_equal(outs[k].cpu().numpy(), _single(j, srcs, s, 0, POISON_A)), k


RING = 4          # ist_ctx::kBatchRing: per-launch job tables in flight per context


def test_relaunch_without_sync_never_reads_a_refilled_table():
    """ONE batch relaunched back to back, without a host synchronisation, onto RING + 2 distinct destination sets: every refill of a
    ring slot writes a table with other destination pointers than the launch that used the slot before, so a slot refilled while
    its launch is still queued would send that launch's canvases to the wrong set (or leave its own set poisoned).  A long first
    launch keeps the queue deep while the host refills the slots."""
    st = ist.Stitcher(0)
    es = _entries(11, 12, st)
    big = [U.rand_image(1100 + i, 1500, 1400) for i in range(6)]                   # ~0.1 GB of copy work in front of the queue
    pb, jb = _compile(st, big, [1] * 6, "vertical", {"filter": "bilinear"})
    es.insert(0, {"job": jb, "srcs": [torch.from_numpy(a).to(DEV) for a in big], "shape": (pb.canvas_h, pb.canvas_w), "pad": 0})
    shapes = [e["shape"] for e in es]
    sets = [_canvases(shapes, [0] * len(es), POISON_A) for _ in range(RING + 2)]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    for raw, outs, _ in sets:
        ist.launch_jobs([e["job"] for e in es], [e["srcs"] for e in es], outs, stream)
    torch.cuda.synchronize()
    wants = [_single(e["job"], e["srcs"], e["shape"], 0, POISON_A) for e in es]
    for n, (raw, outs, guard) in enumerate(sets):
        assert bool((raw[guard] == GUARD).all()), "set %d: a guard byte changed" % n
        for k, want in enumerate(wants):
            assert np.array_equal(outs[k].cpu().numpy(), want), "set %d, entry %d" % (n, k)


def test_one_launch_per_kernel_form():
    st = ist.Stitcher(0)
    same = [U.rand_image(500 + i, 64 + 8 * i, 256) for i in range(3)]
    copy_jobs = [_compile(st, same, [1, 1, 1], "vertical", {"filter": "bilinear", "gap": g}) for g in (0, 2, 5, 9)]
    srcs = [torch.from_numpy(a).to(DEV) for a in same]
    shapes = [(p.canvas_h, p.canvas_w) for p, _ in copy_jobs]
    raw, outs, _ = _canvases(shapes, [0] * len(shapes), POISON_A)
    before = _batch_launches()
    ist.launch_jobs([j for _, j in copy_jobs], [srcs] * len(copy_jobs), outs)
    torch.cuda.synchronize()
    assert _batch_launches() - before == 1                   # homogeneous: one launch
    for k, (p, j) in enumerate(copy_jobs):
        assert np.array_equal(outs[k].cpu().numpy(), _single(j, srcs, shapes[k], 0, POISON_A))
    # a copy-only job, a box-filter job and a quarter-turn job: three kernel forms, three launches
    mixed_px = [U.rand_image(600 + i, 300 - 40 * i, 200 + 30 * i) for i in range(3)]
    msrcs = [torch.from_numpy(a).to(DEV) for a in mixed_px]
    mixed = [_compile(st, same, [1, 1, 1], "vertical", {"filter": "bilinear"}),
             _compile(st, mixed_px, [1, 1, 1], "vertical", {"filter": "area", "mode": "min"}),
             _compile(st, mixed_px, [6, 6, 6], "horizontal", {"filter": "bilinear"})]
    msrc = [srcs, msrcs, msrcs]
    shapes = [(p.canvas_h, p.canvas_w) for p, _ in mixed]
    raw, outs, _ = _canvases(shapes, [0] * 3, POISON_A)
    before = _batch_launches()
    ist.launch_jobs([j for _, j in mixed], msrc, outs)
    torch.cuda.synchronize()
    assert _batch_launches() - before == 3
    for k, (p, j) in enumerate(mixed):
        assert np.array_equal(outs[k].cpu().numpy(), _single(j, msrc[k], shapes[k], 0, POISON_A)), k


def test_a_bad_entry_fails_the_whole_batch_and_nothing_is_written():
    st = ist.Stitcher(0)
    es = _entries(21, 6, st)
    px = [U.rand_image(2100 + i, 40 + i, 50) for i in range(2)]
    p3, j3 = _compile(st, px, [1, 1], "vertical", {"filter": "bilinear"})
    es[3] = {"job": j3, "srcs": [torch.from_numpy(a).to(DEV) for a in px], "shape": (p3.canvas_h, p3.canvas_w), "plan": p3}
    srcs = [list(e["srcs"]) for e in es]
    srcs[3][0] = None                                        # entry 3 lacks a source its job samples
    shapes = [e["shape"] for e in es]
    raw, outs, guard = _canvases(shapes, [0] * len(es), POISON_A)
    before = _batch_launches()
    with pytest.raises(ist.StitchError) as e:
        ist.launch_jobs([x["job"] for x in es], srcs, outs)
    torch.cuda.synchronize()
    assert e.value.code == -6 and "job 3" in e.value.reason
    assert _batch_launches() == before
    assert all(bool((o == POISON_A).all()) for o in outs) and bool((raw[guard] == GUARD).all())
    # jobs of two contexts
    other = L.lib.ist_ctx_create(0)
    assert other
    try:
        p = es[0]["plan"]
        ops, n = p.ops()
        h = L.lib.ist_job_create(other, p.canvas_w, p.canvas_h, (C.c_uint8 * 4)(), ops, n, p._descs, p.n_images, 1, None)
        assert h
        foreign = ist.StitchJob(other, h, p.n_images)
        with pytest.raises(ist.StitchError) as e:
            ist.launch_jobs([es[0]["job"], foreign], [es[0]["srcs"], es[0]["srcs"]], outs[:2])
        assert e.value.code == -1 and "job 1" in e.value.reason
        foreign.close()
    finally:
        L.lib.ist_ctx_destroy(other)


def _host_requests(seed, count):
    rng = np.random.default_rng(seed)
    reqs = []
    for k in range(count):
        px, ori, direction, opts, _ = _rand_entry(rng, 7000 + seed * 100 + k)
        imgs = U.hip_images(px, ori)
        reqs.append((imgs, direction, opts) if rng.random() < 0.8 else (imgs, direction))
    return reqs


def test_stitch_batch_equals_a_loop_of_stitch():
    reqs = _host_requests(31, 17)
    reqs.insert(5, ([], "vertical"))                          # an empty request: None, like stitch()
    got = ist.stitch_batch(reqs)
    assert len(got) == len(reqs) and got[5] is None
    for k, r in enumerate(reqs):
        want = ist.stitch(*r)
        if want is None:
            assert got[k] is None
        else:
            assert got[k] is not None and np.array_equal(got[k], want["data"]), k


SUB_BATCH_BYTES = 512 << 20      # ist_batch.cpp kSubBatchBytes: sources + canvases of one sub-batch


def test_stitch_batch_splits_a_large_batch_into_sub_batches():
    """more than two sub-batches, so both halves of the double buffer are reused while the other one's canvases come down; a
    75 MB canvas (the 9-photo request) is batched like the rest"""
    mid = [U.rand_image(900 + i, 960, 540) for i in range(9)]               # 9 x 540x960: 18.7 MB of sources + 18.7 MB of canvas per request
    reqs = [(mid[k % 9:] + mid[:k % 9], "vertical", {"gap": k % 3}) for k in range(24)]
    photos = [U.rand_image(950 + i, 1920, 1080) for i in range(9)]          # 75 MB of sources, a 75 MB canvas
    reqs.insert(4, (photos, "vertical"))
    reqs.insert(17, (photos[::-1], "vertical", {"gap": 5}))
    subs, held = 1, 0
    for r in reqs:                                                           # the library's greedy cut, all requests copy-only
        p = ist.plan(r[0], r[1], r[2] if len(r) == 3 else None)
        b = p.canvas_w * 4 * p.canvas_h + sum(a.size for a in r[0])
        if held and held + b > SUB_BATCH_BYTES:
            subs, held = subs + 1, 0
        held += b
    assert subs >= 3
    before = _batch_launches()
    got = ist.stitch_batch(reqs)
    assert _batch_launches() - before == subs
    for k, r in enumerate(reqs):
        assert np.array_equal(got[k], ist.stitch(*r)["data"]), k


NODE = shutil.which("node")
ADDON = os.path.join(U.ROOT, "node", "imagestitch.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
def test_node_stitch_batch_equals_stitch_sync(tmp_path):
    reqs = _host_requests(51, 5)
    reqs.insert(2, ([], "horizontal"))
    jreqs = []
    for k, r in enumerate(reqs):
        imgs = []
        for i, im in enumerate(r[0]):
            f = tmp_path / ("r%d_%d.rgba" % (k, i))
            np.ascontiguousarray(im["data"]).tofile(f)
            imgs.append({"width": im["width"], "height": im["height"], "orientation": im["orientation"], "file": str(f)})
        opts = dict(r[2]) if len(r) == 3 else {}
        jreqs.append({"images": imgs, "direction": r[1], "opts": opts})
    script = tmp_path / "batch.js"
    script.write_text("""
const fs = require('fs'); const crypto = require('crypto');
const api = require(%s);
const reqs = JSON.parse(fs.readFileSync(process.argv[2])).map((r) => ({direction: r.direction, opts: r.opts,
  images: r.images.map((m) => ({width: m.width, height: m.height, orientation: m.orientation, data: fs.readFileSync(m.file)}))}));
const digest = (x) => x === null ? null : [x.width, x.height, crypto.createHash('sha256').update(x.data).digest('hex')];
(async () => {
  const sync = api.stitchBatchSync(reqs).map(digest);
  const prom = (await api.stitchBatch(reqs)).map(digest);
  const each = reqs.map((r) => digest(api.stitchSync(r.images, r.direction, r.opts)));
  console.log(JSON.stringify({sync, prom, each}));
})().catch((e) => { console.error(e); process.exit(1); });
""" % json.dumps(os.path.join(U.ROOT, "node", "index.js")))
    jp = tmp_path / "reqs.json"
    jp.write_text(json.dumps(jreqs))
    r = subprocess.run([NODE, str(script), str(jp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["each"][2] is None
    assert out["sync"] == out["each"] and out["prom"] == out["each"]
    import hashlib
    for k, rq in enumerate(reqs):                            # and the same bytes as the Python host path
        want = ist.stitch(*rq)
        if want is None:
            assert out["sync"][k] is None
        else:
            assert out["sync"][k][2] == hashlib.sha256(np.ascontiguousarray(want["data"]).tobytes()).hexdigest(), k
