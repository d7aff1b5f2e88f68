"""The lossless JPEG join (include/imagestitch.h, section 'lossless JPEG joins') restated in numpy: the only oracle of join_jpeg.

THE RULE.  A join of n JPEG files (1 <= n <= 128), vertical or horizontal:
  - the result has image 0's sampling layout (4:4:4 or 4:2:0) and image 0's quantisation tables;
  - vertical: W = w_0, H = sum h_i, and every component's block rows are the sources' block rows of that component, one image after
    the other; horizontal: H = h_0, W = sum w_i, and every block row is the sources' block rows of the same index side by side.  (W, H)
    is ist_plan_compute's canvas for these images with mode 'min', gap 0, unlimited caps;
  - everything else is the export's file: write_jpeg(J, sof=0, marker='jfif', huff='std' | 'optimal', restart = MCUs per MCU row),
    J the Frame whose coefficient arrays are the sources' arrays concatenated along axis 0 (vertical) or axis 1 (horizontal).

ELIGIBILITY (refusal(): the first failing image and its reason; per image the reasons in this order):
  limit     n > 128 (image 128, before any file is looked at)
  not_jpeg  not a JPEG, or one the decoder refuses
  layout    not three YCbCr components, or not sampled 4:4:4 / 4:2:0
  mixed     the layout differs from image 0's
  tables    a component's table differs from image 0's; in image 0 Cb's differs from Cr's, or an entry is 0 or above 255
  size      widths differ (vertical) / heights differ (horizontal)
  align     not the last image, and its height (vertical) / width (horizontal) is no multiple of the MCU size (8 / 16)
  orient    EXIF orientation above 1
  limit     the joined side exceeds 65535 at this image
"""
import numpy as np

from tests.jpeg_encode_reference import mcus_per_row
from tests.jpeg_writer import _new_frame, frame_from_pixels, photo, write_jpeg

MAX_IMAGES = 128


def layout_of(f):
    """'444' / '420' of a Frame, or None for any other layout"""
    if len(f.comps) != 3 or f.colour != "ycc":
        return None
    samp = tuple((c["h"], c["v"]) for c in f.comps)
    return {((1, 1), (1, 1), (1, 1)): "444", ((2, 2), (1, 1), (1, 1)): "420"}.get(samp)


def join(frames, direction):
    """the Frame of the joined file: the sources' coefficient arrays concatenated (the sets are eligible)"""
    axis = 0 if direction == "vertical" else 1
    f0 = frames[0]
    layout = layout_of(f0)
    W = f0.width if axis == 0 else sum(f.width for f in frames)
    H = sum(f.height for f in frames) if axis == 0 else f0.height
    J = _new_frame(W, H, layout, [c["q"] for c in f0.comps])
    for ci, c in enumerate(J.comps):
        coef = np.concatenate([f.comps[ci]["coef"] for f in frames], axis=axis)
        assert coef.shape == c["coef"].shape, (coef.shape, c["coef"].shape)
        c["coef"] = coef
    return J


def expected_file(frames, direction, optimize=False):
    J = join(frames, direction)
    return write_jpeg(J, sof=0, marker="jfif", huff="optimal" if optimize else "std", restart=mcus_per_row(J.width, layout_of(J)))


def describe(f, orientation=0, jpeg=True):
    """what refusal() reads of one file: a Frame (or None: not a JPEG the decoder takes) and its EXIF orientation"""
    return {"frame": f if jpeg else None, "orientation": orientation}


def refusal(files, direction):
    """('ok', -1) or (reason, image) of a list of describe() records"""
    n = len(files)
    if n > MAX_IMAGES:
        return "limit", MAX_IMAGES
    along = 0
    f0 = files[0]["frame"]
    for i, d in enumerate(files):
        f = d["frame"]
        if f is None:
            return "not_jpeg", i
        lay = layout_of(f)
        if lay is None:
            return "layout", i
        if lay != layout_of(f0):
            return "mixed", i
        q = [np.asarray(c["q"]) for c in f.comps]
        if i == 0:
            if not np.array_equal(q[1], q[2]) or min(int(t.min()) for t in q) < 1 or max(int(t.max()) for t in q) > 255:
                return "tables", i
        elif any(not np.array_equal(a, np.asarray(c0["q"])) for a, c0 in zip(q, f0.comps)):
            return "tables", i
        if (f.width != f0.width) if direction == "vertical" else (f.height != f0.height):
            return "size", i
        mcu = 16 if lay == "420" else 8
        if i < n - 1 and (f.height if direction == "vertical" else f.width) % mcu:
            return "align", i
        if d["orientation"] > 1:
            return "orient", i
        along += f.height if direction == "vertical" else f.width
        if along > 65535:
            return "limit", i
    return "ok", -1


# ---- the cases: (name, layout, direction, the side every image shares, the sizes along the join) ----------------------------------
# A workgroup of the join kernel owns 32 consecutive blocks of one MCU row; a row holds 3 (4:4:4) or 6 (4:2:0) blocks per MCU, so it
# is never exactly 32 blocks long: 'whole workgroups' is 96 blocks, 'one block more' 33.
CASES = [
    ("one MCU each 420", "420", "vertical", 16, (16, 16)),
    ("one MCU each 444", "444", "vertical", 8, (8, 8)),
    ("single file 420", "420", "vertical", 40, (25,)),
    ("single file 444", "444", "horizontal", 11, (19,)),
    ("partial column and row 420", "420", "vertical", 40, (16, 32, 9)),
    ("narrow, last row of one pixel 420", "420", "vertical", 17, (48, 16, 1)),
    ("partial column and row 444", "444", "vertical", 33, (8, 24, 3)),
    ("horizontal 420", "420", "horizontal", 24, (16, 32, 9)),
    ("horizontal 444", "444", "horizontal", 9, (8, 8, 5)),
    ("row of 96 blocks: whole workgroups 444", "444", "vertical", 256, (8, 3)),
    ("row of 33 blocks 444", "444", "vertical", 88, (16, 8)),
    ("row of 36 blocks across two images 420", "420", "horizontal", 17, (64, 32)),
    ("row of 96 blocks across three images 420", "420", "horizontal", 16, (96, 144, 16)),
    ("128 images of one MCU, vertical 444", "444", "vertical", 8, (8,) * 128),
    ("128 images of one MCU, horizontal 420", "420", "horizontal", 16, (16,) * 128),
]
CASE_NAMES = [c[0] for c in CASES]


def case_sizes(case):
    """[(height, width)] of a case's sources"""
    _, _, direction, shared, along = case
    return [(a, shared) if direction == "vertical" else (shared, a) for a in along]


_frames = {}


def case_frames(name, scale=0.6):
    """the source Frames of a case (made once per process and left unchanged)"""
    if (name, scale) not in _frames:
        case = next(c for c in CASES if c[0] == name)
        k = CASE_NAMES.index(name)
        _frames[(name, scale)] = [frame_from_pixels(photo(1000 * k + i, h, w), case[1], scale) for i, (h, w) in enumerate(case_sizes(case))]
    return _frames[(name, scale)]


def pillow_file(rgb, subsampling, quality=85, progressive=False):
    """a source as Pillow (libjpeg-turbo) writes it: subsampling 0 (4:4:4) or 2 (4:2:0).  The progressive file of the same pixels
    carries the same quantised coefficients as the baseline one: only the entropy coding differs."""
    import io
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=subsampling, progressive=progressive)
    return b.getvalue()


def pillow_rgb(data):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def witness_mismatch(joined, sources, direction, layout):
    """Pillow's decode of the joined file against Pillow's decodes of the sources laid side by side: the rows (vertical) or columns
    (horizontal) that differ anywhere, and the ones the rule allows to differ: none for 4:4:4; for 4:2:0 the one pixel row or column
    on each side of each seam (libjpeg's triangle chroma filter reaches one chroma sample across the seam)."""
    got = pillow_rgb(joined)
    parts = [pillow_rgb(s) for s in sources]
    axis = 0 if direction == "vertical" else 1
    want = np.concatenate(parts, axis=axis)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = np.any(got != want, axis=(1 - axis, 2))
    seams = np.cumsum([p.shape[axis] for p in parts])[:-1]
    allowed = set()
    if layout == "420":
        for s in seams:
            allowed.update((int(s) - 1, int(s)))
    return sorted(int(i) for i in np.nonzero(diff)[0]), allowed
