"""The compressing PNG export (ist_png_deflate.hip, pngLevel 1) byte for byte against its CPU statement
(tests/png_deflate_reference.py).  The round-trip tests (test_gpu_png.py) accept any valid deflate stream; the encoder is
deterministic by design, so here every byte is predicted: the chunk grid, the tokens of every span, the stored / Huffman choice and
its tie, the order in which the code rule hands its slack back, the alignment pads, the framing, and the layout of the IDAT chunks.
The inputs (tests/png_stream_cases.py) are judged on the CPU first (tests/test_png_deflate_reference.py): each group reaches its
regime and can tell the design from a near miss."""
import struct
import zlib

import numpy as np
import pytest
import torch

import imagestitching_amd as ist
from tests import png_deflate_reference as R
from tests import png_stream_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def walk(png, w, h):
    """every chunk's CRC, the fixed head (signature, IHDR, the tEXt chunk that puts the IDAT data at offset 64) and the chunk
    order; returns the IDAT data of each IDAT chunk"""
    png = bytes(png)
    head = R.file_head(w, h)
    assert len(head) == 56 and png[:56] == head, "signature / IHDR / tEXt: %r" % png[:56]
    at, kinds, idat = 8, [], []
    while at < len(png):
        n, kind = struct.unpack(">I4s", png[at:at + 8])
        data = png[at + 8:at + 8 + n]
        assert len(data) == n and struct.unpack(">I", png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF, (kind, at)
        kinds.append(kind)
        if kind == b"IDAT":
            idat.append(data)
        at += 12 + n
    assert at == len(png) and kinds == [b"IHDR", b"tEXt"] + [b"IDAT"] * len(idat) + [b"IEND"] and idat, kinds
    assert png.index(b"IDAT") + 4 == 64
    return idat


def stream_difference(got, rep):
    """None, or where the stream leaves the reference's: the first differing byte with the chunk and the bit of the chunk it is in"""
    if got == rep.stream:
        return None
    n = min(len(got), len(rep.stream))
    at = next((i for i in range(n) if got[i] != rep.stream[i]), n)
    k = max(i for i, c in enumerate(rep.chunks) if c.offset <= at)
    c = rep.chunks[k]
    if at >= c.offset + c.nbytes:
        where = "the trailer"
    else:
        x = (got[at] ^ rep.stream[at]) if at < n else 1
        bit = 8 * (at - c.offset) + (x & -x).bit_length() - 1
        where = "chunk %d of %d (%s, %d bytes for %d filtered bytes, %d pads, %d rounds), bit %d of the chunk" % (
            k, len(rep.chunks), c.form, c.nbytes, len(c.data), c.pads, c.rounds, bit)
    return "stream of %d bytes, reference %d; first difference at byte %d (%s against %s): %s" % (
        len(got), len(rep.stream), at, got[at:at + 1].hex() or "end", rep.stream[at:at + 1].hex() or "end", where)


def check_host(name, a, limit=None):
    """ist.encode_png (the host path: slabs of chunks, an IDAT per slab) against the reference; returns the IDAT count"""
    rep = C.report(name, a)
    h, w = a.shape[:2]
    idat = walk(ist.encode_png(a, level=1), w, h)
    bad = stream_difference(b"".join(idat), rep)
    assert bad is None, "%s: %s" % (name, bad)
    want = R.idat_lengths([c.nbytes for c in rep.chunks], R.idat_limit(limit), R.host_slabs(len(rep.chunks)))
    assert [len(d) for d in idat] == want, name
    return len(idat)


def check_group(cases):
    failures = []
    for name, a in cases:
        try:
            check_host(name, a)
        except AssertionError as e:
            failures.append(str(e).splitlines()[0])
    assert not failures, "%d of %d inputs:\n%s" % (len(failures), len(cases), "\n".join(failures[:12]))


GRID_NAMES = ["grid photo %dx%d" % s for s in C.GRID_SHAPES] + ["grid noise 64x33", "grid noise 4097x2", "grid flat 257x19",
                                                                 "grid flat 2048x3", "grid flat 4096x2", "grid flat 8191x2"]


@pytest.mark.parametrize("name", GRID_NAMES)
def test_chunk_grid(name):
    """whole rows per chunk (several, two, one), the widest row that is one chunk, and pieces of a row with a 4-byte and an
    8-byte tail piece and three pieces per row"""
    cases = dict(C.grid_cases())
    assert sorted(cases) == sorted(GRID_NAMES)
    C.check_grid_regimes()
    check_host(name, cases[name])


def test_runs_become_the_matches_of_the_design():
    """every run length at every offset of a dword pair, runs through span boundaries, runs of exactly 3 and 4, a run that ends with
    a ragged last span, two runs back to back, every match length (length symbols 257 .. 276, every extra-bit count the encoder
    sends with a nonzero value); every chunk is a Huffman chunk, so its tokens are in the bytes"""
    C.check_runs_regimes()
    check_group(C.runs_cases())


def test_stored_or_huffman_on_either_side_of_the_tie():
    """seeded search with the reference: chunks whose Huffman form is exactly as long as the stored one (stored) and one byte
    shorter (Huffman), as chunk 0 (behind the two zlib header bytes) and as a later chunk"""
    C.check_boundary_regimes()
    check_group(C.boundary_cases())


def test_every_pad_count():
    C.check_pad_regimes()                                     # 0 .. 15 pad blocks over this file's inputs, on the reference side
    check_group(C.pad_cases())


def test_code_rule_in_bytes():
    """the adversarial histograms and the Fibonacci counts of test_gpu_png.py, a histogram of many equal counts (the order inside
    a length class decides which symbols are shortened) and the most rounds a seeded search finds (at least 5)"""
    C.check_code_regimes()
    check_group(C.code_cases())


def test_several_slabs_on_the_host_path():
    """800 chunks: slabs of 768 and 32, each its own IDAT, with stored and Huffman chunks in both"""
    C.check_slab_regimes()
    assert check_host(*C.slab_case()) >= 2


# ---- every entry point writes the same bytes -----------------------------------------------------------------------------------
def _pick(*names):
    cases = dict(C.all_cases())
    return [(n, cases[n]) for n in names]


def _file(t, n):
    got = t.cpu().numpy().tobytes()
    assert len(got) == n
    return got


def _check_file(name, a, got, how=""):
    rep = C.report(name, a)
    h, w = a.shape[:2]
    idat = walk(got, w, h)
    bad = stream_difference(b"".join(idat), rep)
    assert bad is None, "%s%s: %s" % (name, how, bad)
    assert got == R.file_bytes(a, rep.stream), name + how            # one slab, one IDAT: the whole file


def test_encode_png_device_writes_the_reference_file():
    for name, a in _pick("grid photo 257x19", "grid photo 4097x2", "grid flat 2048x3", "every match length", "boundary tie 0, chunk 1"):
        h, w = a.shape[:2]
        dense = torch.from_numpy(a).to(DEV)
        _check_file(name, a, _file(*ist.encode_png_device(dense, level=1)))
        wide = torch.full((h, w + 13, 4), 0xEE, dtype=torch.uint8, device=DEV)
        wide[:, :w] = dense
        view = wide[:, :w]
        assert view.stride(0) == 4 * (w + 13)
        _check_file(name, a, _file(*ist.encode_png_device(view, level=1)), " (pitched)")


def test_encode_png_batch_device_writes_the_reference_files():
    """rows per chunk, one row per chunk, pieces of a row and 1 x 1 in one launch"""
    picked = _pick("grid photo 257x19", "grid photo 2048x3", "grid photo 4097x2", "grid photo 1x1", "runs of 3 and of 4")
    files = ist.encode_png_batch_device([torch.from_numpy(a).to(DEV) for _, a in picked], level=1)
    assert len(files) == len(picked)
    for (name, a), (t, n) in zip(picked, files):
        _check_file(name, a, _file(t, n))


def test_stitch_png_writes_the_stream_of_the_stitched_canvas():
    imgs = [{"width": w, "height": h, "data": C.photo_like(40 + k, h, w)} for k, (w, h) in enumerate(((90, 60), (60, 90), (75, 50)))]
    for direction in ("vertical", "horizontal"):
        opts = {"gap": 3, "mode": "max"}
        canvas = ist.stitch(imgs, direction, opts)
        got = ist.stitch_png(imgs, direction, dict(opts, pngLevel=1))
        assert (got["width"], got["height"]) == (canvas["width"], canvas["height"])
        a = np.ascontiguousarray(canvas["data"])
        rep = C.report("stitch " + direction, a)
        assert zlib.decompress(rep.stream) == rep.filtered and len(rep.chunks) >= 2
        bad = stream_difference(b"".join(walk(got["png"], a.shape[1], a.shape[0])), rep)
        assert bad is None, bad


@pytest.mark.parametrize("limit", ["4096", "65536"])
def test_idat_limit_moves_chunk_boundaries_only(monkeypatch, limit):
    """IST_PNG_IDAT_LIMIT: the concatenated IDAT data is unchanged and every IDAT is what FileLayout::slab's rule gives it, on
    the host path and on the device path"""
    name, a = C.limit_case()
    rep = C.report(name, a)
    assert len(rep.stream) > 65536 and len(rep.chunks) == 17
    monkeypatch.setenv("IST_PNG_IDAT_LIMIT", limit)
    n_idat = check_host(name, a, limit)
    assert n_idat >= 2
    t, n = ist.encode_png_device(torch.from_numpy(a).to(DEV), level=1)
    idat = walk(_file(t, n), 640, 100)
    assert b"".join(idat) == rep.stream
    assert [len(d) for d in idat] == R.idat_lengths([c.nbytes for c in rep.chunks], R.idat_limit(limit))
    if limit == "4096":
        assert min(c.nbytes for c in rep.chunks) > 4096 and len(idat) == len(rep.chunks)      # every chunk is larger than the limit: one each
    else:
        assert all(len(d) <= 65536 for d in idat) and len(idat) < len(rep.chunks)
