"""Builds matrix/TRC RGB ICC profiles (v4 or v2) from colorants and a curve, and splices a profile into JPEG / PNG / WebP files - the
fixtures of the colour tests.  Nothing here is read by the library; the profiles load in littleCMS (PIL.ImageCms)."""
import struct
import zlib

# D50-adapted colorants: columns r, g, b as (X, Y, Z)
SRGB = tuple(tuple(v / 65536.0 for v in col) for col in ((28576, 14581, 912), (25239, 46983, 6361), (9375, 3972, 46787)))      # the sRGB profile's own s15.16 values
P3 = ((0.51512, 0.24120, -0.00105), (0.29198, 0.69225, 0.04189), (0.15710, 0.06657, 0.78407))
ADOBE = ((0.60974, 0.31111, 0.01947), (0.20528, 0.62567, 0.06087), (0.14919, 0.06322, 0.74457))
SRGB_PARA = (2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045)      # g a b c d of 'para' type 3


def s15f16(x):
    return struct.pack(">i", int(round(x * 65536.0)))


def xyz_tag(xyz):
    return b"XYZ \0\0\0\0" + b"".join(s15f16(v) for v in xyz)


def curv_gamma(u8f8):
    """'curv' with one u8Fixed8 entry (563 = Adobe RGB's 563 / 256)"""
    return b"curv\0\0\0\0" + struct.pack(">IH", 1, u8f8)


def curv_table(values):
    return b"curv\0\0\0\0" + struct.pack(">I", len(values)) + b"".join(struct.pack(">H", v) for v in values)


def para(ftype, *params):
    assert len(params) == (1, 3, 4, 5, 7)[ftype]
    return b"para\0\0\0\0" + struct.pack(">HH", ftype, 0) + b"".join(s15f16(p) for p in params)


def srgb_curve_table(n=1024):
    def s(x):
        return x / 12.92 if x <= 0.04045 else ((x + 0.055) / 1.055) ** 2.4
    return curv_table([int(round(65535 * s(i / (n - 1)))) for i in range(n)])


def _text_tag(sig, text, v4):
    if v4:
        u = text.encode("utf-16-be")
        return b"mluc\0\0\0\0" + struct.pack(">II", 1, 12) + b"enUS" + struct.pack(">II", len(u), 28) + u
    if sig == b"desc":
        a = text.encode("ascii") + b"\0"
        return b"desc\0\0\0\0" + struct.pack(">I", len(a)) + a + b"\0" * (4 + 4 + 2 + 1 + 67)
    return b"text\0\0\0\0" + text.encode("ascii") + b"\0"


def profile(colorants, trc, v4=True, space=b"RGB ", pcs=b"XYZ ", extra=()):
    """colorants: ((Xr, Yr, Zr), (Xg, Yg, Zg), (Xb, Yb, Zb)); trc: one curve tag's bytes for all channels, or three.  extra: further
    (signature, bytes) tags, put in FRONT of the table (an 'A2B0' beside the matrix tags, say)."""
    trcs = (trc, trc, trc) if isinstance(trc, bytes) else tuple(trc)
    tags = list(extra) + [(b"desc", _text_tag(b"desc", "test profile", v4)), (b"cprt", _text_tag(b"cprt", "none", v4)),
                          (b"wtpt", xyz_tag((0.9642, 1.0, 0.8249)))]
    tags += [(s, xyz_tag(c)) for s, c in zip((b"rXYZ", b"gXYZ", b"bXYZ"), colorants)]
    tags += [(s, t) for s, t in zip((b"rTRC", b"gTRC", b"bTRC"), trcs)]
    return assemble(tags, v4, space, pcs)


def assemble(tags, v4=True, space=b"RGB ", pcs=b"XYZ "):
    table, body, seen = b"", b"", {}
    at = 128 + 4 + 12 * len(tags)
    for sig, data in tags:
        if data in seen:                                   # shared tag data, as real profiles share their TRC
            off, ln = seen[data]
        else:
            off, ln = at + len(body), len(data)
            seen[data] = (off, ln)
            body += data + b"\0" * (-len(data) % 4)
        table += sig + struct.pack(">II", off, ln)
    head = struct.pack(">I4sI4s4s4s", 0, b"\0\0\0\0", 0x04300000 if v4 else 0x02100000, b"mntr", space, pcs)
    head += struct.pack(">6H", 2024, 1, 1, 0, 0, 0) + b"acsp" + b"\0" * 4 + b"\0" * 4 + b"\0" * 8 + b"\0" * 8 + struct.pack(">I", 0)
    head += b"".join(s15f16(v) for v in (0.9642, 1.0, 0.8249)) + b"\0" * 4 + b"\0" * 16 + b"\0" * 28
    assert len(head) == 128
    out = head + struct.pack(">I", len(tags)) + table + body
    return struct.pack(">I", len(out)) + out[4:]


def fixtures():
    """name -> profile bytes: the profiles the issue names"""
    f = {
        "p3_para3": profile(P3, para(3, *SRGB_PARA)),
        "adobe_gamma": profile(ADOBE, curv_gamma(563), v4=False),
        "p3_gamma18": profile(P3, curv_gamma(461)),
        "srgb_table1024": profile(SRGB, srgb_curve_table(1024), v4=False),
        "srgb_para3": profile(SRGB, para(3, *SRGB_PARA)),
        "p3_para0": profile(P3, para(0, 2.2)),
        "p3_para1": profile(P3, para(1, 2.2, 0.9, 0.1)),
        "p3_para2": profile(P3, para(2, 2.2, 0.95, 0.04, 0.01)),
        "p3_para4": profile(P3, para(4, 2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045, 0.0, 0.0)),
        "p3_curv0": profile(P3, b"curv\0\0\0\0" + struct.pack(">I", 0)),
    }
    return f


# ---- splicing a profile into files (the existing writers stay as they are) --------------------------------------------------

def jpeg_with_icc(jpeg, icc, chunks=1, order=None, drop=None, count=None):
    """the JPEG with `icc` in `chunks` APP2 segments behind SOI (any APP2 ICC segments it had are removed); order: the sequence
    numbers in file order (default 1 .. chunks); drop: a sequence number left out; count: the count byte (default chunks)"""
    assert jpeg[:2] == b"\xff\xd8"
    body, pos = b"", 2
    while pos + 4 <= len(jpeg) and jpeg[pos] == 0xFF and jpeg[pos + 1] not in (0xDA, 0xD9):      # copy the segments in front of the scan
        ln = struct.unpack(">H", jpeg[pos + 2:pos + 4])[0]
        seg = jpeg[pos:pos + 2 + ln]
        if not (jpeg[pos + 1] == 0xE2 and seg[4:16] == b"ICC_PROFILE\0"):
            body += seg
        pos += 2 + ln
    body += jpeg[pos:]
    step = -(-len(icc) // chunks)
    parts = [icc[i * step:(i + 1) * step] for i in range(chunks)]
    segs = b""
    for seq in (order or range(1, chunks + 1)):
        if seq == drop:
            continue
        data = b"ICC_PROFILE\0" + bytes([seq, chunks if count is None else count]) + parts[seq - 1]
        segs += b"\xff\xe2" + struct.pack(">H", len(data) + 2) + data
    return jpeg[:2] + segs + body


def _png_chunk(ctype, data):
    return struct.pack(">I", len(data)) + ctype + data + struct.pack(">I", zlib.crc32(ctype + data) & 0xFFFFFFFF)


def png_with_chunks(png, chunks):
    """the PNG with the given (type, data) chunks right behind IHDR"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    end = 8 + 12 + struct.unpack(">I", png[8:12])[0]
    return png[:end] + b"".join(_png_chunk(t, d) for t, d in chunks) + png[end:]


def png_with_icc(png, icc, corrupt=False):
    z = zlib.compress(icc)
    if corrupt:
        z = z[:10] + bytes(b ^ 0xFF for b in z[10:40]) + z[40:]
    return png_with_chunks(png, [(b"iCCP", b"test\0\0" + z)])


def webp_with_icc(webp, icc):
    """a simple-format (or extended) WebP -> an extended file with an ICCP chunk; the canvas size is read from the bitstream"""
    assert webp[:4] == b"RIFF" and webp[8:12] == b"WEBP"
    chunks, pos = [], 12
    while pos + 8 <= len(webp):
        ln = struct.unpack("<I", webp[pos + 4:pos + 8])[0]
        chunks.append((webp[pos:pos + 4], webp[pos + 8:pos + 8 + ln]))
        pos += 8 + ln + (ln & 1)
    chunks = [c for c in chunks if c[0] not in (b"ICCP",)]
    vp8x = [c for c in chunks if c[0] == b"VP8X"]
    if vp8x:
        flags, rest = vp8x[0][1][0] | 0x20, vp8x[0][1][1:]
    else:
        tag, d = next(c for c in chunks if c[0] in (b"VP8 ", b"VP8L"))
        if tag == b"VP8L":
            bits = struct.unpack("<I", d[1:5])[0]
            w, h, alpha = (bits & 0x3FFF) + 1, ((bits >> 14) & 0x3FFF) + 1, (bits >> 28) & 1
        else:
            w, h, alpha = struct.unpack("<H", d[6:8])[0] & 0x3FFF, struct.unpack("<H", d[8:10])[0] & 0x3FFF, 0
        flags = 0x20 | (0x10 if alpha else 0)
        rest = b"\0\0\0" + struct.pack("<I", w - 1)[:3] + struct.pack("<I", h - 1)[:3]
    out = [(b"VP8X", bytes([flags]) + rest), (b"ICCP", icc)] + [c for c in chunks if c[0] != b"VP8X"]
    body = b"WEBP" + b"".join(t + struct.pack("<I", len(d)) + d + b"\0" * (len(d) & 1) for t, d in out)
    return b"RIFF" + struct.pack("<I", len(body)) + body
