"""The Node host's lossless JPEG join (joinJpegCheck, joinJpeg): the same bytes as the Python host for two cases - and so the numpy
reference, which tests/test_gpu_jpeg_join.py holds the Python host to - and the check's record for one refusal."""
import json
import os
import shutil
import subprocess

import pytest

from tests import jpeg_join_reference as JR
from tests import util as U
from tests.jpeg_writer import write_jpeg

pytestmark = pytest.mark.gpu
NODE = shutil.which("node")
ADDON = os.path.join(U.ROOT, "node", "imagestitch.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
def test_node_join_equals_the_python_host(tmp_path):
    import imagestitching_amd as ist
    cases = {"v": ("partial column and row 420", "vertical", True), "h": ("horizontal 444", "horizontal", False)}
    sets = {}
    for key, (name, direction, optimize) in cases.items():
        frames = JR.case_frames(name)
        sets[key] = [write_jpeg(f, restart=2) if k == 1 else write_jpeg(f) for k, f in enumerate(frames)]
        for k, blob in enumerate(sets[key]):
            (tmp_path / ("%s%d.jpg" % (key, k))).write_bytes(blob)
    script = tmp_path / "jpeg_join.js"
    script.write_text("""
const fs = require('fs'); const path = require('path');
const api = require(%s);
const dir = process.argv[2];
const read = (key, n) => Array.from({length: n}, (_, k) => fs.readFileSync(path.join(dir, key + k + '.jpg')));
(async () => {
  const v = read('v', 3), h = read('h', 3);
  fs.writeFileSync(path.join(dir, 'v.out.jpg'), await api.joinJpeg(v, 'vertical', {optimize: true}));
  fs.writeFileSync(path.join(dir, 'h.out.jpg'), await api.joinJpeg([0, 1, 2].map((k) => path.join(dir, 'h' + k + '.jpg')), 'horizontal'));
  const ok = api.joinJpegCheck(v, 'vertical');
  const refused = api.joinJpegCheck([v[0], v[2], v[1]], 'vertical');
  let rejected = null;
  try { await api.joinJpeg([v[0], v[2], v[1]], 'vertical'); } catch (e) { rejected = {code: e.code, message: e.message}; }
  let typed = null;
  try { await api.joinJpeg(v, 'vertical', {optimize: 1}); } catch (e) { typed = e instanceof TypeError; }
  console.log(JSON.stringify({ok, refused, rejected, typed}));
})().catch((e) => { console.error(e); process.exit(1); });
""" % json.dumps(os.path.join(U.ROOT, "node", "index.js")))
    r = subprocess.run([NODE, str(script), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for key, (name, direction, optimize) in cases.items():
        want = ist.join_jpeg(sets[key], direction, optimize=optimize)
        assert (tmp_path / (key + ".out.jpg")).read_bytes() == want == JR.expected_file(JR.case_frames(name), direction, optimize), name
    assert got["ok"] == ist.jpeg_join_check(sets["v"], "vertical") == {"ok": True, "reason": "ok", "image": -1, "width": 40, "height": 57, "subsampling": "420"}
    v = sets["v"]
    assert got["refused"] == ist.jpeg_join_check([v[0], v[2], v[1]], "vertical") == {"ok": False, "reason": "align", "image": 1, "width": 0, "height": 0, "subsampling": "420"}
    assert got["rejected"] is not None and "image 1" in got["rejected"]["message"], got["rejected"]
    assert got["typed"] is True
