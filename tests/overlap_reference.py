"""The overlap contract of include/imagestitch.h ("overlap removal for scrolled screenshots") restated in numpy, and the synthetic
screenshots the overlap tests share.  Everything is integer: numpy int64 for the sums of one row pair, Python ints for the products of
the selection, so the GPU and the C rules can be compared with == and nothing else."""
import numpy as np

CELLS = 32
DEFAULTS = {"tolerance": 8, "min_rows": 16, "min_informative": 8}


def _opts(opts):
    o = dict(DEFAULTS)
    unknown = set(opts) - set(o)
    assert not unknown, unknown
    o.update(opts)
    return o


def signatures(img):
    """HxWx4 uint8 -> Hx32 int64: S(y, c) = sum of R + 2 G + B over e(c) <= x < e(c + 1), e(c) = floor(c w / 32)"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    v = img[..., 0].astype(np.int64) + 2 * img[..., 1].astype(np.int64) + img[..., 2].astype(np.int64)
    s = np.zeros((h, CELLS), np.int64)
    for c in range(CELLS):
        s[:, c] = v[:, (c * w) // CELLS:((c + 1) * w) // CELLS].sum(axis=1)
    return s


def row_diff(sa, sb):
    """D of rows (any leading shape) of two signature tables"""
    return np.abs(sa - sb).sum(axis=-1)


def edge_rule(d, T):
    """the greatest t in [1, len(d)] with d[t - 1] <= T and #{y < t: d[y] > T} <= t // 4, else 0"""
    best, bad = 0, 0
    for y, v in enumerate(d):
        ok = int(v) <= T
        bad += 0 if ok else 1
        if ok and bad <= (y + 1) // 4:
            best = y + 1
    return best


def select_rule(cost, inf, kmax, T, **opts):
    """K among k in [min_rows, kmax] with cost[k] <= T k and inf[k] >= min_informative: the least cost[k] / k, the smaller k on a tie"""
    o = _opts(opts)
    best = 0
    for k in range(max(o["min_rows"], 1), kmax + 1):
        ck = int(cost[k])
        if ck > T * k or int(inf[k]) < o["min_informative"]:
            continue
        if best == 0 or ck * best < int(cost[best]) * k:
            best = k
    return best


def pair_tables(a, b, **opts):
    """everything the rule computes for one pair of equal width: dict with T, L, dtop, dbot, H, F, kmax, cost[0..kmax], inf[0..kmax]"""
    o = _opts(opts)
    sa, sb = signatures(a), signatures(b)
    ha, hb, w = a.shape[0], b.shape[0], a.shape[1]
    T = o["tolerance"] * w
    L = min(ha, hb) // 2
    dtop = row_diff(sa[:L], sb[:L])
    dbot = row_diff(sa[::-1][:L], sb[::-1][:L])
    H, F = edge_rule(dtop, T), edge_rule(dbot, T)
    body_a, body_b = ha - F - H, hb - F - H
    kmax = min(body_a, body_b - 1)
    cost = [0] * (max(kmax, 0) + 1)
    for k in range(1, kmax + 1):
        cost[k] = int(row_diff(sa[ha - F - k:ha - F], sb[H:H + k]).sum())
    flags = row_diff(sb[H:H + body_b - 1], sb[H + 1:H + body_b]) > T if body_b > 1 else np.zeros(0, bool)
    inf = [0] * (max(kmax, 0) + 1)
    for k in range(1, kmax + 1):
        inf[k] = inf[k - 1] + (int(flags[k - 1]) if k - 1 < body_b - 1 else 0)
    return {"T": T, "L": L, "dtop": dtop, "dbot": dbot, "H": H, "F": F, "kmax": kmax, "cost": cost, "inf": inf}


def pair(a, b, **opts):
    """{'header', 'footer', 'overlap', 'cost'} of A above B"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape[1] != b.shape[1]:
        return {"header": 0, "footer": 0, "overlap": 0, "cost": 0}
    t = pair_tables(a, b, **opts)
    K = select_rule(t["cost"], t["inf"], t["kmax"], t["T"], **opts) if t["kmax"] >= 1 else 0
    return {"header": t["H"], "footer": t["F"], "overlap": K, "cost": t["cost"][K] if K > 0 else 0}


def find_overlaps(images, **opts):
    return [pair(images[i], images[i + 1], **opts) for i in range(len(images) - 1)]


def overlap_rows(pairs, heights):
    """the crop rule: [(top, bot)] per image"""
    n = len(heights)
    top, bot = [0] * n, list(heights)
    for i in range(n - 1):
        if pairs[i]["overlap"] > 0:
            top[i + 1] = pairs[i]["header"] + pairs[i]["overlap"]
            bot[i] = heights[i] - pairs[i]["footer"]
    for i in range(1, n - 1):
        if bot[i] - top[i] < 1:
            bot[i], top[i + 1] = heights[i], 0
    return list(zip(top, bot))


def crop(images, **opts):
    """the images cut by the rule, as contiguous arrays"""
    rows = overlap_rows(find_overlaps(images, **opts), [im.shape[0] for im in images])
    return [np.ascontiguousarray(im[t:b]) for im, (t, b) in zip(images, rows)]


# ---- synthetic screenshots ----------------------------------------------------------------------------------------------------
def synth_shots(w, header, footer, bodies, offsets, seed=0, noise=0, clock=True, indicator=True):
    """Shots of one scrolled page: shot i shows page rows [offsets[i], offsets[i] + bodies[i]) between a header and a footer that are the
    same in every shot - but for a clock patch inside the header that changes from shot to shot (under a quarter of the header's rows)
    and a two-pixel scroll indicator in the body that moves with the offset.  The page is random per pixel, so every body row is
    informative and no two rows match.  noise: + uniform [-noise, noise] per channel and shot (a shot that went through a JPEG).
    Alpha is random: it is not read."""
    rng = np.random.default_rng(seed)
    page_rows = max(o + b for o, b in zip(offsets, bodies))
    page = rng.integers(0, 256, (page_rows, w, 4), dtype=np.uint8)
    head = rng.integers(0, 256, (header, w, 4), dtype=np.uint8)
    foot = rng.integers(0, 256, (footer, w, 4), dtype=np.uint8)
    shots = []
    for i, (off, body) in enumerate(zip(offsets, bodies)):
        hd = head.copy()
        if clock and header >= 8 and w >= 4:
            r0, rows = header // 4, max(1, header // 5)                      # rows < header / 4: inside the rule's allowance
            patch = hd[r0:r0 + rows, w // 4:w // 4 + max(1, w // 3)]
            patch[...] = rng.integers(0, 256, patch.shape, dtype=np.uint8)
        bd = page[off:off + body].copy()
        if indicator and w >= 64:
            bar = max(2, body // 8)
            at = min(body - bar, (off * body) // max(1, page_rows))
            bd[at:at + bar, w - 3:w - 1, :3] = 128
        shot = np.concatenate([hd, bd, foot], axis=0)
        shot[..., 3] = rng.integers(0, 256, shot.shape[:2], dtype=np.uint8)
        if noise:
            d = rng.integers(-noise, noise + 1, shot.shape, dtype=np.int16)
            d[..., 3] = 0
            shot = np.clip(shot.astype(np.int16) + d, 0, 255).astype(np.uint8)
        shots.append(np.ascontiguousarray(shot))
    return shots


def truth(header, footer, bodies, offsets, min_rows=16):
    """the (H, F, K) a pair of synth_shots should give, per neighbouring pair (K = 0 when the page rows overlap by less than min_rows)"""
    out = []
    for i in range(len(bodies) - 1):
        k = offsets[i] + bodies[i] - offsets[i + 1]
        out.append((header, footer, k if max(min_rows, 1) <= k <= min(bodies[i], bodies[i + 1] - 1) else 0))
    return out
