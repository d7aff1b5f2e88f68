"""The render harness the cubic GPU tests share (test infrastructure): op lists as the reference renderer takes them, compiled and
launched on device tensors that are embedded in poison."""
import numpy as np
import torch

import imagestitching_amd as ist
from imagestitching_amd import _lib as L

CUBIC, AA = 3, 0x100
GUARD = 3          # poisoned rows above and below the canvas, and poisoned columns to its right (the row pitch is wider than the canvas)


def c_ops(ops_o):
    ops = (L.Op * len(ops_o))()
    for i, o in enumerate(ops_o):
        ops[i].m[:] = o["m"]
        if o["kind"] == "fill":
            ops[i].kind = 0; ops[i].image = -1; ops[i].d[:] = o["rect"]; ops[i].rgba[:] = o["rgba"]
        else:
            ops[i].kind = 1; ops[i].image = o["image"]; ops[i].s[:] = o["s"]; ops[i].d[:] = o["d"]
    return ops


def descs(px, opaque=None):
    return (L.ImageDesc * len(px))(*[L.ImageDesc(a.shape[1], a.shape[0], 1, 0, 0, int(bool(opaque and opaque[k])), 0) for k, a in enumerate(px)])


def embed(a):
    """the bitmap as a view into a larger device tensor of 0xC3 with its true pitch (8 rows above and below, 7 and 8 pixels beside it:
    an odd offset, so rows do not start on 16 bytes): a tap that misses its clamp reads poison instead of a neighbour's valid bytes,
    and stays inside the allocation"""
    h, w = a.shape[:2]
    host = np.full((h + 16, w + 15, 4), 0xC3, np.uint8)
    host[8:8 + h, 7:7 + w] = a
    return torch.from_numpy(host).cuda()[8:8 + h, 7:7 + w]


def render_job(cw, ch, clear, ops_o, px, opaque, filt=CUBIC, clip=None, poison=0x5A, srcs=None):
    """A compiled job on device tensors.  The canvas sits inside a larger tensor of poison (guard rows above and below, a pitch 5
    pixels wider than the canvas); every source sits inside a larger tensor of poison with its true pitch (embed; srcs: tensors made
    that way before).  Returns (canvas, job.info) after checking the guards; with a clip, what lies outside it is still poison."""
    job = ist.Stitcher(0).compile_ops(cw, ch, c_ops(ops_o), len(ops_o), descs(px, opaque), len(px), filt, clear=clear, clip=clip)
    big = torch.full((ch + 2 * GUARD, cw + 5, 4), poison, dtype=torch.uint8, device="cuda")
    out = big[GUARD:GUARD + ch, :cw]
    job.launch(srcs if srcs is not None else [embed(a) for a in px], out)
    torch.cuda.synchronize()
    info = dict(job.info)
    job.close()
    whole = big.cpu().numpy()
    assert (whole[:GUARD] == poison).all() and (whole[GUARD + ch:] == poison).all() and (whole[:, cw:] == poison).all(), "a write left the canvas"
    return whole[GUARD:GUARD + ch, :cw].copy(), info
