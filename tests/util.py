"""Shared helpers for the parity tests (test infrastructure; may use the oracle)."""
import os

import numpy as np

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rand_image(seed, h, w, opaque=True):
    a = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    if opaque:
        a[..., 3] = 255
    return a


def smooth_image(seed, h, w, opaque=True):
    """Low-frequency content (gradients + a few blobs): closer to photos than noise, exercises the lerp weights."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((h, w, 4), np.float64)
    for c in range(4):
        fx, fy, ph = rng.uniform(0.5, 3.0), rng.uniform(0.5, 3.0), rng.uniform(0, 6.28)
        out[..., c] = 127.5 + 127.5 * np.sin(fx * xx / max(w, 1) * 6.28 + fy * yy / max(h, 1) * 6.28 + ph)
    out = np.clip(np.round(out), 0, 255).astype(np.uint8)
    if opaque:
        out[..., 3] = 255
    return out


def oracle_limits(opts):
    """Same meaning as imagestitching_amd.stitch._limits, built for the oracle."""
    opts = opts or {}
    plat = opts.get("platform")
    if plat is None:
        lim = O.lifted_limits(1.0)
    else:
        lim = O.default_limits(plat)
    if opts.get("maxSide") is not None:
        lim.max_side = float(opts["maxSide"])
    if opts.get("maxPixels") is not None:
        lim.max_pixels = float(opts["maxPixels"])
    if opts.get("superSample") is not None:
        lim.max_super_sample = float(opts["superSample"])
    return lim


def edge_aa_of(opts):
    """the hosts' default (imagestitching_amd.stitch.edge_aa_of, node/index.js edgeAA): on iff a reference platform's plan
    is requested, unless the caller says otherwise"""
    v = (opts or {}).get("edgeAA")
    return ((opts or {}).get("platform") is not None) if v is None else bool(v)


def oracle_stitch(pixels, direction, opts=None, orientations=None, threads=4):
    opts = opts or {}
    descs = [{"width": a.shape[1], "height": a.shape[0], "orientation": (orientations[i] if orientations else 1)}
             for i, a in enumerate(pixels)]
    rc, pd, rl = O.plan(descs, direction, opts.get("mode", "min"), opts.get("gap", 0), oracle_limits(opts))
    assert rc == 0, rc
    img = O.render(pd, rl, descs, pixels, opts.get("filter", "bilinear"), threads, edge_aa=edge_aa_of(opts))
    return img, pd, rl


def hip_images(pixels, orientations=None):
    return [{"width": a.shape[1], "height": a.shape[0], "data": a, "orientation": (orientations[i] if orientations else 1)}
            for i, a in enumerate(pixels)]


def max_abs_diff(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max()) if a.size else 0


def mismatch_fraction(a, b):
    return float((a != b).any(axis=-1).mean()) if a.size else 0.0


def oracle_tolerance(got, ref, exact=False):
    """The op-list tolerance rule against the fp64 oracle: solid pixels within 1 LSB; a translucent pixel of a transparent canvas
    reads back un-premultiplied (c * 255 / a), so one LSB of the premultiplied value may become up to 1 + ceil(255 / a) LSBs of its
    colour; `exact` (nearest without edge AA) allows no difference at all.  Returns (differing, total, signed sum) over the channel
    bytes of the solid pixels: the "rarely different" statistics."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got.astype(np.int16) - ref.astype(np.int16)
    if exact:
        assert not d.any(), "max diff %d" % int(np.abs(d).max())
        return 0, int((ref[..., 3] == 255).sum()) * 4, 0
    a = np.abs(d)
    assert int(a[..., 3].max(initial=0)) <= 1, "alpha off by %d" % int(a[..., 3].max())
    solid = ref[..., 3] == 255
    ds = d[solid]
    assert int(np.abs(ds).max(initial=0)) <= 1, "solid pixel off by %d" % int(np.abs(ds).max())
    soft = ~solid & (ref[..., 3] > 0)
    if soft.any():
        lim = 1 + np.ceil(255.0 / ref[..., 3][soft].astype(np.float64))
        assert (a[..., :3][soft].max(axis=-1) <= lim).all(), "translucent readback beyond 1 + ceil(255 / a)"
    return int((ds != 0).sum()), int(ds.size), int(ds.sum())


class RareDiff:
    """accumulates oracle_tolerance's statistics over many cases and checks that differences are rare and unbiased"""

    def __init__(self):
        self.diff = self.total = self.signed = 0

    def add(self, stats):
        self.diff += stats[0]
        self.total += stats[1]
        self.signed += stats[2]

    @property
    def fraction(self):
        return self.diff / max(1, self.total)

    @property
    def mean(self):
        return self.signed / max(1, self.total)

    def check(self, fraction=0.01, mean=0.001):
        """fewer than `fraction` of the bytes differ, and their signed sum stays within `mean` LSB per byte plus three standard
        deviations of a sum of that many unbiased +-1 differences (a systematic error - a weight dropped or counted twice - is
        one-sided)"""
        assert self.total > 0
        assert self.fraction < fraction, "%.5f of the solid channel bytes differ from the oracle" % self.fraction
        assert abs(self.signed) <= mean * self.total + 3.0 * self.diff ** 0.5, "mean signed difference %.6f LSB (%r)" % (self.mean, self)

    def __repr__(self):
        return "%d of %d solid channel bytes differ (%.2e), mean signed difference %+.2e LSB" % (self.diff, self.total, self.fraction, self.mean)
