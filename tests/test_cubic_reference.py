"""What makes tests/cubic_reference.py a reference (pure CPU): run with bilinear and box weights it reproduces the project's
fp64 oracle on random op lists - that pins its coverage, clamping, premultiplication and compositing - and with cubic weights
it agrees with an independent Catmull-Rom, torch's antialiased bicubic (a = -0.5; plain 4 taps when enlarging), away from the
border, where torch renormalises instead of clamping.  Reference anchor: utils/canvas.js:153-202 (drawImage under a CTM)."""
import math

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import cubic_reference as R
from tests import util as U


@pytest.mark.parametrize("mode,k_lo,k_hi", [("bilinear", 0.1, 8.0), ("area", 0.3, 40.0)])
def test_with_bilinear_and_box_weights_it_is_the_oracle(mode, k_lo, k_hi):
    """both are fp64 and differ in the order of summation only: the op-list tolerance rule, differences rare and unbiased"""
    rng = np.random.default_rng(77 if mode == "area" else 78)
    stats = U.RareDiff()
    exact = 0
    for case in range(60):
        cw, ch, ops, px, clear, aa = R.random_op_list(rng, case, k_lo, k_hi, max_src=2.0e5)
        descs = [{"width": a.shape[1], "height": a.shape[0]} for a in px]
        want = O.render_ops(cw, ch, ops, descs, px, mode, clear=clear, edge_aa=aa)
        got = R.render_ops(cw, ch, ops, descs, px, mode, clear=clear, edge_aa=aa)
        try:
            stats.add(U.oracle_tolerance(got, want))
        except AssertionError as e:
            raise AssertionError("case %d (aa %s): %s; ops %r" % (case, aa, e, ops))
        exact += int(np.array_equal(got, want))
    print("reference with %s weights against the oracle: %r, %d of 60 cases byte-identical" % (mode, stats, exact))
    stats.check(fraction=1e-3)               # (two fp64 sums: far rarer than the 1 % the fp32 kernels are allowed)


@pytest.mark.parametrize("size,out", [((29, 37), (75, 96)), ((40, 31), (52, 31)), ((17, 23), (17, 60)), ((33, 20), (86, 52))])
def test_with_cubic_weights_it_is_torchs_antialiased_bicubic_in_the_interior(size, out):
    """one opaque enlarging draw; the margin ceil(2 / k) + 1 output pixels is where a tap leaves the image and torch renormalises"""
    (h, w), (H, W) = size, out
    img = U.rand_image(5, h, w)
    ops = [{"kind": "draw", "image": 0, "m": [1, 0, 0, 1, 0, 0], "s": [0, 0, w, h], "d": [0, 0, W, H]}]
    Rv = R.resolve(ops[0]["m"], W, H, w, h, ops[0]["s"], ops[0]["d"], False)
    v = R.sample_draw(Rv, img, "cubic")
    assert np.abs(v[..., 3] - 255.0).max() < 1e-9                     # the weights sum to 1
    mine = v[..., :3] / 255.0                                         # unclamped, unrounded
    t = torch.from_numpy(img[..., :3].astype(np.float64)).permute(2, 0, 1)[None]
    ref = torch.nn.functional.interpolate(t, size=(H, W), mode="bicubic", antialias=True, align_corners=False)[0].permute(1, 2, 0).numpy()
    my, mx = math.ceil(2 / (h / H)) + 1, math.ceil(2 / (w / W)) + 1
    inner = (slice(my, H - my), slice(mx, W - mx))
    assert mine[inner].size > 0
    assert np.abs(mine[inner] - ref[inner]).max() < 1e-9, np.abs(mine[inner] - ref[inner]).max()
    assert mine.min() < -1.0 and mine.max() > 256.0                   # noise overshoots: the clamp of the contract is needed
    # ... and the rendered bytes are that, clamped and rounded once
    got = R.render_ops(W, H, ops, None, [img], "cubic")
    assert np.array_equal(got[inner][..., :3], np.clip(np.floor(ref[inner] + 0.5), 0, 255).astype(np.uint8)) or \
        U.max_abs_diff(got[inner][..., :3], np.clip(np.floor(ref[inner] + 0.5), 0, 255).astype(np.uint8)) <= 1
    assert (got[..., 3] == 255).all()


def test_the_weights_sum_to_one_and_interpolate():
    t = np.linspace(0.0, 1.0, 1001)[:-1]
    w = np.array(R.cubic_weights(t))
    assert np.abs(w.sum(axis=0) - 1.0).max() < 1e-15
    assert [float(v[0]) for v in w] == [0.0, 1.0, 0.0, 0.0]
    assert w[0].min() < -0.07 and w[3].min() < -0.07                  # negative lobes (-2/27 at t = 1/3 and 2/3)


@pytest.mark.parametrize("opaque", [True, False])
def test_an_integer_offset_unit_draw_is_the_identity(opaque):
    img = U.rand_image(11, 40, 50, opaque=opaque)
    ops = [{"kind": "fill", "m": [1, 0, 0, 1, 0, 0], "rect": [0, 0, 64, 48], "rgba": (9, 99, 199, 255)},
           {"kind": "draw", "image": 0, "m": [1, 0, 0, 1, 0, 0], "s": [3, 2, 44, 30], "d": [7, 5, 44, 30]}]
    descs = [{"width": 50, "height": 40}]
    got = R.render_ops(64, 48, ops, descs, [img], "cubic")
    assert np.array_equal(got, O.render_ops(64, 48, ops, descs, [img], "bilinear"))
    if opaque:
        assert np.array_equal(got[5:35, 7:51], img[2:32, 3:47])
    # mirrored at 1:1 (EXIF 2): every weight is still (0, 1, 0, 0)
    ops[1]["m"] = [-1, 0, 0, 1, 64, 0]
    assert np.array_equal(R.render_ops(64, 48, ops, descs, [img], "cubic"), O.render_ops(64, 48, ops, descs, [img], "bilinear"))
