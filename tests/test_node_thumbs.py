"""Thumbnails through the Node host (node/index.js: thumbnails(bitmaps, {width, height, mode, orient})) on the GPU: the grid of chosen
images (pages/index/index.wxml:4-22).  The bytes are the Python host's thumbnails of the same files - both run ist_bitmaps_thumbs,
whose pixels tests/test_gpu_thumbs.py holds against the oracle."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import imagestitching_amd as ist
from tests.test_gpu_bitmaps import _jpeg, _photo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "node", "imagestitch.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")]

JS = r"""
const api = require(process.argv[1]);
const fs = require('fs');
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = {};
const name = async (p) => { try { await p; return 'resolved'; } catch (e) { return e.code || e.constructor.name; } };
(async () => {
  const bms = await api.decodeBitmaps(job.paths);
  for (const [tag, cell] of Object.entries(job.cells)) {
    const r = await api.thumbnails(bms, cell);
    out[tag] = r.map((t) => [t.width, t.height, t.data.length]);
    fs.writeFileSync(job.out + '.' + tag + '.rgba', Buffer.concat(r.map((t) => t.data)));
  }
  out.empty = (await api.thumbnails([], { width: 4, height: 4 })).length;
  out.noCell = await name(api.thumbnails(bms, { width: 4 }));
  out.badMode = await name(api.thumbnails(bms, { width: 4, height: 4, mode: 'cover' }));
  out.notBitmaps = await name(api.thumbnails([{ width: 4, height: 4 }], { width: 4, height: 4 }));
  out.zeroCell = await name(api.thumbnails(bms, { width: 0, height: 4 }));
  out.missing = await name(api.thumbnails([bms[0], null], { width: 4, height: 4 }));
  bms[1].release();
  out.released = await name(api.thumbnails(bms, { width: 4, height: 4 }));
  bms.forEach((b) => b.release());
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(String(e && e.stack || e)); process.exit(3); });
"""

CELLS = {"fill": {"width": 96, "height": 96}, "fit": {"width": 100, "height": 60, "mode": "fit"},
         "stored": {"width": 80, "height": 50, "mode": "fill", "orient": False}}


def test_node_thumbnails_are_the_python_hosts(tmp_path):
    blobs = [_jpeg(_photo(160 + k, h, w), orientation=o, quality=90) for k, (w, h, o) in enumerate([(400, 300, 1), (420, 280, 6), (300, 380, 8), (64, 48, 3)])]
    paths = []
    for k, f in enumerate(blobs):
        paths.append(str(tmp_path / ("f%d.jpg" % k)))
        open(paths[-1], "wb").write(f)
    job = {"paths": paths, "out": str(tmp_path / "r"), "cells": CELLS}
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, "-e", JS, os.path.join(ROOT, "node", "index.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    bms = ist.decode_bitmaps(blobs)
    for tag, cell in CELLS.items():
        want = ist.thumbnails(bms, (cell["width"], cell["height"]), mode=cell.get("mode", "fill"), orient=cell.get("orient", True))
        assert out[tag] == [[w.shape[1], w.shape[0], w.size] for w in want], tag
        got = np.frombuffer(open(str(tmp_path / ("r.%s.rgba" % tag)), "rb").read(), np.uint8)
        assert np.array_equal(got, np.concatenate([w.reshape(-1) for w in want])), tag
    for b in bms:
        b.close()
    assert out["empty"] == 0
    assert out["noCell"] == "TypeError" and out["badMode"] == "TypeError" and out["notBitmaps"] == "TypeError"
    assert out["zeroCell"] == "-1" and out["missing"] == "-6" and out["released"] == "Error"
