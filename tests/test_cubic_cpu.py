"""filter 'cubic' (IST_FILTER_CUBIC) where no GPU is needed: the source rows a shard holds, the hosts' option parsing, the planner's
cell classification and the gfx950 code that ships.  Reference anchor: index.js:1363 (the small-job plan super-samples 2.2-2.6x:
every draw of it is an enlargement), index.js:1416-1421 (imageSmoothingQuality 'high')."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from imagestitching_amd import _lib as L
from imagestitching_amd import dist as D
from imagestitching_amd.stitch import FILTER_EDGE_AA, _FILTERS, _filter_of, _merge
from tests import cubic_reference as R
from tests import test_shard_holdings as H
from tests import util as U

SPLITS = ["image", "band", "rows", "auto"]
SLOTS = [1, 2, 3, 5, 8]


def _random_job(rng):
    """strips under 'cubic' in which some draws are enlarged (mode 'max', superSample > 1), some shrink on both axes (mode 'min'
    with a narrow image) and some straddle 1 (mixed sizes close to each other)"""
    n = int(rng.integers(1, 5))
    kind = int(rng.integers(0, 3))
    sizes = []
    for _ in range(n):
        if kind == 0:                                     # close sizes: scales on both sides of 1
            sizes.append((int(rng.integers(60, 90)), int(rng.integers(20, 80))))
        elif rng.random() < 0.4:
            sizes.append((int(rng.integers(6, 30)), int(rng.integers(10, 60))))         # narrow
        else:
            sizes.append((int(rng.integers(40, 260)), int(rng.integers(20, 160))))
    direction = "vertical" if rng.random() < 0.5 else "horizontal"
    if direction == "horizontal":
        sizes = [(h, w) for w, h in sizes]
    ori = [int(v) for v in rng.integers(1, 9, n)] if rng.random() < 0.4 else [1] * n
    opts = {"mode": ["min", "max", "max", "original"][int(rng.integers(0, 4))], "gap": int(rng.choice([0, 3])), "filter": "cubic",
            "edgeAA": bool(rng.random() < 0.3)}
    if rng.random() < 0.4:
        opts["superSample"] = float(rng.choice([1.5, 2.2, 2.6]))
    return sizes, ori, direction, opts


def test_every_shard_renders_from_its_holding_alone_under_cubic():
    """the property of tests/test_shard_holdings.py under filter 3, with the numpy reference as renderer: each part, rendered from
    sources poisoned outside the rows [sy0, sy1) its owner holds, equals the clean render inside its clip byte for byte"""
    rng = np.random.default_rng(1717)
    seen, regimes = set(), set()
    for trial in range(60):
        sizes, ori, direction, opts = _random_job(rng)
        split, world = SPLITS[trial % 4], SLOTS[trial % 5]
        descs = [{"width": w, "height": h, "orientation": o} for (w, h), o in zip(sizes, ori)]
        try:
            sh = D.ShardedStitch(descs, direction, opts, 0, world, 0, split=split)
        except L.StitchError as e:
            assert split in ("image", "band") and "rows" in e.reason, (trial, e)
            continue
        pixels = [U.rand_image(9500 + 10 * trial + i, h, w) for i, (w, h) in enumerate(sizes)]
        cw, ch = sh.plan.canvas_w, sh.plan.canvas_h
        aa = U.edge_aa_of(sh.opts)
        ss = sh.plan.super_sample
        for r in sh.plan.rects:
            w, h = sizes[r["image"]]
            if r["orientation"] > 4:
                w, h = h, w
            kx, ky = w / (r["dw"] * ss), h / (r["dh"] * ss)
            regimes.add("grow" if max(kx, ky) < 1 else "shrink" if min(kx, ky) > 1 else "unit" if kx == ky == 1 else "mixed")
        for part in sh.parts:
            ops, n, clip = sh.band_ops(part)
            lst = H._ops(ops, n)
            clean = R.render_ops(cw, ch, lst, descs, pixels, "cubic", edge_aa=aa)
            poisoned = []
            for i, a in enumerate(pixels):
                p = np.full_like(a, 0xEE)
                p[..., 1] = 0x11
                a0, a1 = H._held(part).get(i, (0, 0))
                p[a0:a1] = a[a0:a1]
                poisoned.append(p)
            got = R.render_ops(cw, ch, lst, descs, poisoned, "cubic", edge_aa=aa)
            x, y, w, h = clip
            assert np.array_equal(got[y:y + h, x:x + w], clean[y:y + h, x:x + w]), (trial, split, world, opts, ori, part.index)
        seen.add((sh.split, world, aa))
    assert {s for s, _, _ in seen} == {"image", "band", "rows"}
    assert {w for _, w, _ in seen} == set(SLOTS)
    assert {a for _, _, a in seen} == {False, True}
    assert regimes >= {"grow", "shrink", "mixed"}, regimes


def test_cubic_holdings_of_an_enlargement_cover_the_four_taps():
    """one 2.6x draw cut into thin bands: band [Y0, Y1) holds rows floor(k (Y0 + .5) - .5) - 1 .. floor(k (Y1 - .5) - .5) + 2,
    clamped, and at most one more at either end"""
    w, h = 120, 400
    descs = [{"width": w, "height": h}]
    sh = D.ShardedStitch(descs, "vertical", {"filter": "cubic", "superSample": 2.6}, 0, 8, 0, split="band")
    assert sh.plan.super_sample == 2.6 and len(sh.parts) == 8
    k = h / sh.plan.canvas_h
    assert abs(k - 1 / 2.6) < 1e-3
    for p in sh.parts:
        lo = max(0, math.floor(k * (p.Y0 + 0.5) - 0.5) - 1)
        hi = min(h - 1, math.floor(k * (p.Y1 - 0.5) - 0.5) + 2)
        assert lo - 1 <= p.sy0 <= lo and hi + 1 <= p.sy1 <= hi + 2, (p.Y0, p.Y1, p.sy0, p.sy1, lo, hi)
    # the bilinear holding of the same cut is one row shorter at either end wherever it is not clamped
    bl = D.ShardedStitch(descs, "vertical", {"filter": "bilinear", "superSample": 2.6}, 0, 8, 0, split="band")
    inner = [(a, b) for a, b in zip(sh.parts, bl.parts)][1:-1]
    assert all(a.sy0 == b.sy0 - 1 and a.sy1 == b.sy1 + 1 for a, b in inner)


def test_the_hosts_accept_cubic_and_still_refuse_unknown_names():
    assert L.FILTER_CUBIC == 3 and _FILTERS["cubic"] == 3
    assert _filter_of(_merge({"filter": "cubic", "edgeAA": True})) == 3 | FILTER_EDGE_AA
    with pytest.raises(KeyError):
        _filter_of(_merge({"filter": "lanczos"}))
    src = open(os.path.join(U.ROOT, "node", "index.js")).read()
    assert re.search(r"const FILTER = \{[^}]*cubic: 3", src)
    assert "'cubic'" in open(os.path.join(U.ROOT, "node", "index.d.ts")).read()
    node = shutil.which("node")
    if node is None or not os.path.exists(os.path.join(U.ROOT, "node", "imagestitch.node")):
        return                                            # (the addon is built only where Node's headers are: plan() needs it)
    js = ("const ist = require(%s); const im = [{width: 64, height: 48}, {width: 32, height: 24}];"
          "const p = ist.plan(im, 'vertical', {filter: 'cubic', mode: 'max'});"
          "let refused = false; try { ist.plan(im, 'vertical', {filter: 'lanczos'}); } catch (e) { refused = /unknown filter/.test(e.message); }"
          "console.log(JSON.stringify({n: p.rects.length, f: ist.FILTER.cubic, refused}));") % json.dumps(os.path.join(U.ROOT, "node"))
    out = subprocess.run([node, "-e", js], capture_output=True, text=True, check=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    assert got["f"] == 3 and got["n"] == 2 and got["refused"], got


def _compile(cw, ch, ops_o, px, filt, opaque=True):
    """ist_job_create needs a device context; ist_debug_flat_form compiles the same op list on the CPU alone and returns what
    compile_ops returns"""
    ops = (L.Op * len(ops_o))()
    for i, o in enumerate(ops_o):
        ops[i].m[:] = o["m"]
        if o["kind"] == "fill":
            ops[i].kind = 0; ops[i].image = -1; ops[i].d[:] = o["rect"]; ops[i].rgba[:] = o["rgba"]
        else:
            ops[i].kind = 1; ops[i].image = o["image"]; ops[i].s[:] = o["s"]; ops[i].d[:] = o["d"]
    descs = (L.ImageDesc * len(px))(*[L.ImageDesc(w, h, 1, 0, 0, int(opaque), 0) for w, h in px])
    n = C.c_int(0)
    return L.lib.ist_debug_flat_form(cw, ch, None, ops, len(ops_o), descs, len(px), filt, None, None, None, None, 0, C.byref(n))


def test_the_planner_accepts_filter_3_and_refuses_filter_4():
    ops = [{"kind": "draw", "image": 0, "m": [1, 0, 0, 1, 0, 0], "s": [0, 0, 40, 30], "d": [0, 0, 104, 78]}]
    assert _compile(104, 78, ops, [(40, 30)], 3) == 0
    assert _compile(104, 78, ops, [(40, 30)], 3 | 0x100) == 0
    assert _compile(104, 78, ops, [(40, 30)], 4) == -1 and "unknown filter" in L.last_error()


READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


@pytest.mark.skipif(not os.path.exists(READELF) or shutil.which("objcopy") is None, reason="needs llvm-readelf and objcopy")
def test_the_cubic_kernels_ship_for_gfx950_and_the_batch_twins_cost_the_same(tmp_path):
    """kinds 5 (fill / copy / box / cubic: paths 99) and 6 (+ the per-pixel stack: 107), single-job and batch: the same VGPR count, no
    private segment (no spill); and the five older forms are what tests/test_batch_device_code.py pins"""
    from tests import test_batch_device_code as B
    ks = B._kernels(str(tmp_path))
    for paths in (99, 107):
        single = "_ZN3ist16ist_cubic_kernelILi%dELi0ELb0EEEvNS_10LaunchArgsEl" % paths
        twin = "_ZN3ist22ist_cubic_batch_kernelILi%dELi0EEEvNS_9BatchArgsE" % paths
        assert single in ks and twin in ks, sorted(k for k in ks if "cubic" in k)
        assert ks[single][".vgpr_count"] == ks[twin][".vgpr_count"], (ks[single], ks[twin])
        assert ks[single][".private_segment_fixed_size"] == 0 and ks[twin][".private_segment_fixed_size"] == 0, (ks[single], ks[twin])
        assert ks[single][".vgpr_count"] <= 128, ks[single]          # 4 waves per SIMD: the streamed path is latency-bound, and 3 measured 20 % slower
    assert len([k for k in ks if "ist_cubic_batch" in k]) == 2
