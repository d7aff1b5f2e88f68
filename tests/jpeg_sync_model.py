"""A CPU model of how the GPU Huffman decoder (csrc/ist_jpeg_gpu.hip) cuts a scan up, and the files that put its synchronisation
into each of its regimes (tests/test_jpeg_sync_model.py holds both to their word; tests/test_gpu_jpeg_sync_regimes.py decodes them).

The model works from what the writer coded (write_jpeg(..., trace=...): the _symbols events and the length in bits of every code
and every run of magnitude bits, per restart interval).  It decodes nothing: it only says WHERE things fall - how many 1024-bit
subsequences and workgroups a unit (a scan, or one restart interval) occupies, where its blocks start, which subsequences hold no
block start at all, which boundaries cut a symbol between its code and its magnitude bits, how many codes miss the 9-bit
look-ahead - so that a case can assert it reaches the regime it is named for instead of quietly testing something else.

The constants restate the kernel file's; test_jpeg_sync_model.py reads them back out of the source text.
"""
import functools
import io

import numpy as np

from tests import jpeg_writer as JW

K_SUB_BITS = 1024        # kSubBits (IST_SUB_BITS): bits per subsequence, one lane each
K_SYNC_THREADS = 128     # kSyncThreads (IST_SYNC_THREADS): subsequences per workgroup; a unit is padded to whole workgroups
K_INNER_PASSES = 48      # kInnerPasses: passes a workgroup makes inside one launch
K_MAX_PASSES = 64        # kMaxPasses: launches before the batch is handed to the host decoder
K_CHECK_BITS = 256       # kCheckBits: the checkpoint of a re-decode, in bits behind the subsequence's start
K_MARGIN_WORDS = 64      # kMarginWords: 32-bit words staged behind a workgroup's own bits
K_LOOK_BITS = 9          # kJpegDcLookBits = kJpegAcLookBits (ist_jpeg.h): codes longer than this take the general step


def unit_facts(tr, k):
    """the facts of restart interval k (0: the whole scan when there are no intervals) of one traced scan"""
    a, b = int(tr["bounds"][k]), int(tr["bounds"][k + 1])
    lens, cls, comp = tr["lens"][a:b], tr["cls"][a:b], tr["comp"][a:b]
    start = np.cumsum(lens) - lens
    coded = int(lens.sum())
    bits = -(-coded // 8) * 8                                  # (the writer pads to a byte with 1 bits; the decoder counts bytes)
    n_sub = max(1, -(-bits // K_SUB_BITS))
    block_start = start[(cls == 0) & (comp >= 0)]              # every block opens with its DC code
    length = np.diff(np.append(block_start, coded))
    owners = np.unique(block_start // K_SUB_BITS)
    bounds = np.arange(1, n_sub) * K_SUB_BITS
    raw_start = start[(comp < 0) & (lens > 0)]                 # magnitude bits: they follow their code at once
    return {"bits": bits, "coded_bits": coded, "n_sub": n_sub, "workgroups": -(-n_sub // K_SYNC_THREADS), "blocks": len(block_start),
            "block_start": block_start, "longest_block": int(length.max()) if len(length) else 0,
            "subs_without_block_start": sorted(set(range(n_sub)) - set(owners.tolist())),
            "subs_cut_in_symbol": (bounds[np.isin(bounds, raw_start)] // K_SUB_BITS).tolist(),
            "whole_subsequences": bits % K_SUB_BITS == 0, "tail_bits": bits % K_SUB_BITS, "short": bits < K_CHECK_BITS}


def model(frame, trace):
    """the facts of a file with one interleaved scan (what the GPU decoder takes)"""
    assert len(trace) == 1, "one scan"
    tr = trace[0]
    n_units = len(tr["bounds"]) - 1
    units = [unit_facts(tr, k) for k in range(n_units)]
    slots = sum(frame.eff(frame.comps[ci])[0] * frame.eff(frame.comps[ci])[1] for ci in tr["comps"])
    long_codes = {}                                            # (class, table slot) -> share of its codes behind the look-ahead
    code = tr["comp"] >= 0
    for tc, slot_of in ((0, tr["dc_slots"]), (1, tr["ac_slots"])):
        for slot in sorted({slot_of[ci] for ci in tr["comps"]}):
            m = code & (tr["cls"] == tc) & np.isin(tr["comp"], [ci for ci in tr["comps"] if slot_of[ci] == slot])
            long_codes[(tc, slot)] = float((tr["lens"][m] > K_LOOK_BITS).mean()) if m.any() else 0.0
    shared = slots > 1 and len({tr["dc_slots"][ci] for ci in tr["comps"]}) == 1 and len({tr["ac_slots"][ci] for ci in tr["comps"]}) == 1
    return {"units": units, "slots": slots, "shared_tables": shared, "long_codes": long_codes,
            "n_sub": sum(u["n_sub"] for u in units), "max_unit_sub": max(u["n_sub"] for u in units),
            "workgroups": sum(u["workgroups"] for u in units)}


# ---- the files -------------------------------------------------------------------------------------------------------------------
def _case(name, frame, pixels=True, **opts):
    """pixels: the IDCT stays inside frame_edges' range, so PIL's pixels are a witness too (False: coefficients only)"""
    trace = []
    marker = opts.pop("marker", "jfif" if frame.colour != "rgb" else "adobe0")
    data = JW.write_jpeg(frame, marker=marker, trace=trace, **opts)
    return {"name": name, "data": data, "frame": frame, "model": model(frame, trace), "pixels": pixels,
            "width": frame.width, "height": frame.height}


def _pillow(name, px, **save):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(px).save(b, "JPEG", **save)
    return {"name": name, "data": b.getvalue(), "frame": None, "model": None, "pixels": True, "width": px.shape[1], "height": px.shape[0]}


SHARED = dict(dc_slots=(0, 0, 0), ac_slots=(0, 0, 0), huff="optimal")
ONES = np.ones(64, np.int64)


def _dense_pm1(blocks_x, blocks_y, seed, dc_range=8):
    """grey, quantisation table all 1, every AC coefficient +-1: under 'deep' tables the one AC symbol gets a 16-bit code, a block is
    ~1090 bits - longer than a subsequence - and no end-of-block ever tells a decoder where a block stops.  dc_range: the DC values are
    uniform in +-dc_range.  How far a wrong zig-zag index survives depends on it (CPU replay of the host loop, tools/sim_slot_sync.cpp,
    160 x 160, seeds 0-9 each): with +-3 or +-8 the re-decodes reach the last lane of a workgroup and every seed takes 3 launches;
    with +-40 they die out inside the workgroups and every seed takes 2, although some workgroup still needs more than kInnerPasses
    passes (a third launch follows only when a chain reaches a lane whose exit another workgroup reads).  The slow case wants the
    third launch, hence +-8."""
    rng = np.random.default_rng(seed)
    f = JW._new_frame(8 * blocks_x, 8 * blocks_y, "grey", [ONES])
    co = f.comps[0]["coef"]
    co[...] = rng.choice([-1, 1], co.shape)
    co[..., 0] = rng.integers(-dc_range, dc_range + 1, co.shape[:2])
    return f


@functools.lru_cache(maxsize=None)
def slow_cases():
    """(a) files whose first launch cannot settle: the truth advances one subsequence per inner pass"""
    pic = JW.photo(70, 200, 300)
    out = [_pillow("pillow_keep_rgb_300x200", pic, quality=85, keep_rgb=True, subsampling=0),
           _case("shared_420_300x200", JW.frame_from_pixels(pic, "420", 0.5), **SHARED),
           _case("shared_444_300x200", JW.frame_from_pixels(pic, "444", 0.5), **SHARED),
           _case("dense_pm1_deep_160x160", _dense_pm1(20, 20, 5), pixels=False, huff="deep")]
    # restart intervals longer than kInnerPasses subsequences: each restarts from the truth and still needs a third launch
    noisy = JW.photo(71, 200, 300, noise=90)
    out.append(_case("shared_420_restart40", JW.frame_from_pixels(noisy, "420", 0.06), restart=40, **SHARED))
    return out


@functools.lru_cache(maxsize=None)
def carried_checkpoint_case():
    """(a) grey, 'deep' tables: stretches of 120 dense +-1 blocks (the truth walks them a subsequence per pass, into the second launch)
    between stretches of 60 coarse photo blocks of ~40 bits (any decoder falls into step there within a few symbols).  Where the truth leaves a dense
    stretch in a LATER launch, the next subsequence is re-decoded from a new start and arrives at its checkpoint in the state an
    earlier launch recorded: its tally is the new first leg + the old second leg, from `checks` and `tally` carried across launches.
    (The shared-table files never do that: their re-decodes differ in the slot all the way.)"""
    rng = np.random.default_rng(5)
    dense, photo, reps = 120, 60, 6
    by = (dense + photo) * reps // 16 + 1
    src = JW.frame_from_pixels(JW.photo(5, 8 * by, 128, noise=40)[..., 1], "grey", qtabs=[JW.quant_table(0, 8.0)])
    f = JW._new_frame(128, 8 * by, "grey", [ONES])
    flat = f.comps[0]["coef"].reshape(-1, 64)
    flat[:] = src.comps[0]["coef"].reshape(-1, 64)
    for r in range(reps):
        at = r * (dense + photo) + photo
        flat[at:at + dense] = rng.choice([-1, 1], (dense, 64))
        flat[at:at + dense, 0] = rng.integers(-40, 41, dense)
    return _case("dense_and_photo_stretches", f, huff="deep")


@functools.lru_cache(maxsize=None)
def control_case():
    """(a) the same picture as Pillow writes it in YCbCr: two table sets, falls into step at once"""
    return _pillow("pillow_ycbcr_300x200", JW.photo(70, 200, 300), quality=85, subsampling=0)


@functools.lru_cache(maxsize=None)
def unsettled_case():
    """(b) shared tables, noise, a quarter more subsequences than kMaxPasses launches of kInnerPasses passes can walk"""
    want = (K_MAX_PASSES * K_INNER_PASSES * 5) // 4
    rng = np.random.default_rng(11)
    side = 480
    while True:
        px = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
        c = _case("shared_444_noise_%d" % side, JW.frame_from_pixels(px, "444", 0.1), **SHARED)
        if c["model"]["n_sub"] >= want:
            return c
        side += 16


def _max_block(dc):
    """63 AC values of category 10: with the Annex K tables 20 + 63 * 26 bits after a DC difference of category 11"""
    b = np.full(64, 1023, np.int64)
    b[1::2] = -1023
    b[0] = dc
    return b


@functools.lru_cache(maxsize=None)
def long_block_cases():
    """(c) blocks longer than a subsequence"""
    dense = _case("dense_pm1_deep_160x160", _dense_pm1(20, 20, 5), pixels=False, huff="deep")
    # grey, Annex K tables, 16 blocks a row: [lead] maximal blocks, [fill] all-zero blocks (6 bits each: DC difference 0 + end of
    # block) placed by the model so that the NEXT maximal block starts in the last 64 bits of the first workgroup's 128th
    # subsequence, zero blocks to the end of the row, and a maximal block as the very last block of the scan
    edge = K_SYNC_THREADS * K_SUB_BITS

    def build(lead, fill):
        n = lead + fill + 1
        total = -(-(n + 1) // 16) * 16
        f = JW._new_frame(128, 8 * (total // 16), "grey", [ONES])
        flat = f.comps[0]["coef"].reshape(-1, 64)
        sign = 1
        for k in list(range(lead)) + [lead + fill, total - 1]:
            flat[k] = _max_block(1016 * sign)
            sign = -sign
        for k in range(lead, lead + fill):
            flat[k, 0] = flat[lead - 1, 0]                     # DC difference 0
        for k in range(lead + fill + 1, total - 1):
            flat[k, 0] = flat[lead + fill, 0]
        return _case("max_blocks_margin", f, pixels=False), lead + fill

    lead, fill = edge // 1660 - 1, 0
    for _ in range(4):
        c, target = build(lead, fill)
        at = int(c["model"]["units"][0]["block_start"][target])
        if edge - 64 <= at < edge:
            break
        fill += (edge - 32 - at) // 6
        assert fill >= 0
    c["target_block"] = target
    return [dense, c]


@functools.lru_cache(maxsize=None)
def deep_cases():
    """(d) codes behind the look-ahead in all four tables, over several workgroups, with and without mid-row restarts"""
    out = []
    for layout, seed in (("420", 21), ("440", 22)):
        f = JW.frame_from_pixels(JW.photo(seed, 200, 300), layout, 0.5)
        out.append(_case("deep_%s_300x200" % layout, f, huff="deep"))
        out.append(_case("deep_%s_300x200_restart7" % layout, f, huff="deep", restart=7))
    return out


def _dc_ramp_frame(width, height, seed):
    """4:2:0, quantisation tables all 1: every component's DC plane is a triangle wave between -1016 and +1016 in raster order, every
    fourth block swapped for the +-1016 alternation of frame_edges (DC differences of category 11), a few small AC values everywhere so
    that the scan is long; every IDCT output stays far inside [-512, 511]"""
    rng = np.random.default_rng(seed)
    f = JW._new_frame(width, height, "420", [ONES] * 3)
    for c in f.comps:
        co = c["coef"]
        by, bx = co.shape[:2]
        n = by * bx
        t = np.arange(n)
        period = max(2, n // 3)                                  # up and down one and a half times
        tri = np.abs((t % (2 * period)) - period) * 2032 // period - 1016
        alt = np.where((t // 4) % 2 == 0, 1016, -1016)
        dc = np.where(t % 4 == 3, alt, tri)
        flat = co.reshape(n, 64)
        for z in range(1, 9):
            flat[:, JW.ZIGZAG[z]] = rng.integers(-12, 13, n)
        flat[:, 0] = dc
    return f


@functools.lru_cache(maxsize=None)
def dc_cases():
    """(e) DC integration across workgroups (the scan of the tallies), without and with restart intervals"""
    f = _dc_ramp_frame(640, 480, 31)
    return [_case("dc_ramp_420", f), _case("dc_ramp_420_restart500", f, restart=500)]


def _grey_prefix(source, n_content, zeros, bx=1):
    """grey, bx blocks a row (1: any number of blocks is a frame): the first n_content blocks of `source` in coding order, then `zeros` blocks that repeat the last DC (6
    bits each: DC difference 0, end of block), and as many again as fill the last row"""
    by = -(-(n_content + zeros) // bx)
    f = JW._new_frame(8 * bx, 8 * by, "grey", [source.comps[0]["q"]])
    flat = f.comps[0]["coef"].reshape(-1, 64)
    flat[:n_content] = source.comps[0]["coef"].reshape(-1, 64)[:n_content]
    flat[n_content:, 0] = flat[n_content - 1, 0]
    return f


def _grey_with_bits(name, lo, hi, seed):
    """a grey file whose coded bits fall in (lo, hi]: content blocks up to ~lo, then as many 6-bit zero blocks as it takes (hi - lo >= 6)"""
    source = JW.frame_from_pixels(JW.photo(seed, 8 * (lo // 400 + 8), 32, noise=60)[..., 1], "grey", 0.3)
    starts = _case(name, source)["model"]["units"][0]["block_start"]
    assert starts[-1] > lo, "the source is too short"
    n_content = int(np.searchsorted(starts, lo - 64, side="right")) - 1      # the content ends at most 64 bits before lo
    zeros = 0
    for _ in range(6):
        c = _case(name, _grey_prefix(source, n_content, zeros))
        got = c["model"]["units"][0]["coded_bits"]
        if lo < got <= hi:
            return c
        zeros += max(1, -(-(lo + 1 - got) // 6)) if got <= lo else -max(1, (got - hi + 5) // 6)
        assert zeros >= 0
    raise AssertionError("%s: %d coded bits, wanted (%d, %d]" % (name, got, lo, hi))


@functools.lru_cache(maxsize=None)
def geometry_cases():
    """(f) units that end on, just before and just behind a workgroup; whole subsequences; units shorter than the checkpoint"""
    out = []
    for k, n_sub in enumerate((127, 128, 129, 256, 257)):
        out.append(_grey_with_bits("grey_%d_sub" % n_sub, (n_sub - 1) * K_SUB_BITS + 8, n_sub * K_SUB_BITS - 16, 40 + k))
    out.append(_grey_with_bits("grey_tail_0", 5 * K_SUB_BITS - 8, 5 * K_SUB_BITS, 46))                 # bits % 1024 == 0
    out.append(_grey_with_bits("grey_tail_8", 5 * K_SUB_BITS, 5 * K_SUB_BITS + 8, 47))                 # bits % 1024 == 8
    small = JW.frame_from_pixels(JW.photo(48, 24, 40, noise=6)[..., 0], "grey", 1.5)
    out.append(_case("grey_restart1_short", small, restart=1))
    return out


def batch_cases():
    """(g) everything of (a), (c), (d), (e) and (f) in one call"""
    names, out = set(), []
    for c in slow_cases() + [carried_checkpoint_case(), control_case()] + long_block_cases() + deep_cases() + dc_cases() + geometry_cases():
        if c["name"] not in names:
            names.add(c["name"])
            out.append(c)
    return out
