"""Colour profiles through the Node host (node/index.js decodeBitmaps(files, {colorProfile}), imageColor, stitchFiles opts.colorProfile)
on the GPU: the downloads and the file equal the Python host's, the kinds agree, a call without the option is untouched by the calls
around it, and a bad value is a TypeError before anything is decoded."""
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import icc_writer as W
import imagestitching_amd as ist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "node", "imagestitch.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")]

JS = r"""
const api = require(process.argv[1]);
const fs = require('fs');
const job = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = {};
(async () => {
  out.kinds = job.paths.map((p) => api.imageColor(p));
  out.kindOfBuffer = api.imageColor(fs.readFileSync(job.paths[2]));
  // the three calls are queued together: each one's setting travels with it
  const [plain, conv, again] = await Promise.all([api.decodeBitmaps(job.paths), api.decodeBitmaps(job.paths, { colorProfile: 'srgb', scale: job.scales }),
                                                  api.decodeBitmaps(job.paths, { colorProfile: 'ignore' })]);
  plain.forEach((b, k) => fs.writeFileSync(job.out + '.plain.' + k, b.download()));
  conv.forEach((b, k) => fs.writeFileSync(job.out + '.conv.' + k, b.download()));
  out.againSame = again.every((b, k) => b.download().equals(plain[k].download()));
  out.decodeImageSame = api.decodeImage(fs.readFileSync(job.paths[2])).data.equals(plain[2].download());
  const res = await api.stitchFiles(job.strip, 'vertical', { colorProfile: 'srgb' });
  fs.writeFileSync(job.out + '.png', res.png);
  const res0 = await api.stitchFiles(job.strip, 'vertical');
  fs.writeFileSync(job.out + '.plain.png', res0.png);
  out.bad = await api.decodeBitmaps(job.paths, { colorProfile: 'p3' }).then(() => 'resolved', (e) => e.constructor.name);
  out.badFiles = await api.stitchFiles(job.strip, 'vertical', { colorProfile: 1 }).then(() => 'resolved', (e) => e.constructor.name);
  out.refused = await api.stitchPng(plain.slice(0, 1), 'vertical', { colorProfile: 'srgb' }).then(() => 'resolved', (e) => e.constructor.name + ': ' + e.message);
  [...plain, ...conv, ...again].forEach((b) => b.release());
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(String(e && e.stack || e)); process.exit(3); });
"""


def _file(fmt, w, h, icc, seed, **kw):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(xx * 255) // (w - 1), (yy * 255) // (h - 1), ((xx + yy) * 7) % 256], -1)
    a = (a + rng.integers(-10, 10, a.shape)).clip(0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(a).save(b, fmt, **({"icc_profile": icc} if icc else {}), **kw)
    return b.getvalue()


def test_node_colour_profiles_equal_the_python_hosts(tmp_path):
    fx = W.fixtures()
    p3, adobe = fx["p3_para3"], fx["adobe_gamma"]
    gray = W.profile(W.P3, W.para(0, 2.2), space=b"GRAY")
    files = [_file("JPEG", 48, 32, None, 1), _file("JPEG", 48, 32, fx["srgb_para3"], 2), _file("JPEG", 65, 17, p3, 3), _file("JPEG", 40, 24, gray, 4),
             _file("PNG", 33, 9, adobe, 5), _file("WEBP", 30, 20, p3, 6, lossless=True), _file("JPEG", 64, 48, p3, 7, progressive=True)]
    scales = [1, 1, 1, 1, 1, 1, 2]
    strip = [_file("JPEG", 64, 24, p3, 8), _file("JPEG", 64, 40, adobe, 9), _file("JPEG", 64, 16, None, 10)]
    paths, spaths = [], []
    for k, f in enumerate(files):
        paths.append(str(tmp_path / ("f%d" % k)))
        open(paths[-1], "wb").write(f)
    for k, f in enumerate(strip):
        spaths.append(str(tmp_path / ("s%d.jpg" % k)))
        open(spaths[-1], "wb").write(f)
    job = {"paths": paths, "scales": scales, "strip": spaths, "out": str(tmp_path / "r")}
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, "-e", JS, os.path.join(ROOT, "node", "index.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["kinds"] == [ist.image_color(f) for f in files] == ["none", "identity", "convert", "unsupported", "convert", "convert", "convert"]
    assert out["kindOfBuffer"] == "convert"
    plain, conv = ist.decode_bitmaps(files), ist.decode_bitmaps(files, scale=scales, profile="srgb")
    for k, (p, c) in enumerate(zip(plain, conv)):
        assert np.array_equal(np.fromfile(str(tmp_path / ("r.plain.%d" % k)), np.uint8).reshape(p.shape), p.download()), k
        assert np.array_equal(np.fromfile(str(tmp_path / ("r.conv.%d" % k)), np.uint8).reshape(c.shape), c.download()), k
        p.close()
        c.close()
    assert out["againSame"] and out["decodeImageSame"]
    want = ist.stitch_files(spaths, "vertical", {"colorProfile": "srgb"})["png"]
    assert np.array_equal(ist.decode_png(open(str(tmp_path / "r.png"), "rb").read()), ist.decode_png(want))
    want0 = ist.stitch_files(spaths, "vertical")["png"]
    assert np.array_equal(ist.decode_png(open(str(tmp_path / "r.plain.png"), "rb").read()), ist.decode_png(want0))
    assert not np.array_equal(ist.decode_png(want), ist.decode_png(want0))
    assert out["bad"] == "TypeError" and out["badFiles"] == "TypeError"
    assert out["refused"].startswith("TypeError") and "colorProfile" in out["refused"], out["refused"]
