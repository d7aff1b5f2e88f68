"""tests/preview_reference.py held against what it restates, CPU only: the fp64 reference against the oracle, geometry() against
ist_debug_preview_geometry, the exact rule against a replay of the kernel's finish, the near-tie cap of the inputs, and - the evidence
that tests/test_gpu_preview_regimes.py can fail - the reference perturbed the way a kernel bug would perturb it, rejected by the rule
of the case that targets the regime.  No wrong kernel is built or run for that."""
import ctypes as C

import numpy as np
import pytest

from imagestitching_amd import _lib as L
from tests import preview_reference as PR
from tests import util as U
from tests.test_gpu_preview import oracle_preview


def _debug_geometry(w, h, pw, ph):
    out = (C.c_int32 * 6)(*([-7] * 6))
    rc = L.lib.ist_debug_preview_geometry(w, h, pw, ph, out)
    return rc, tuple(out)


# ---- the reference against the oracle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,pw,ph", [(13, 8, 5, 3), (40, 30, 7, 4), (64, 48, 9, 5), (50, 37, 12, 9), (33, 21, 2, 2), (300, 7, 1, 2)])
@pytest.mark.parametrize("opaque", [True, False])
def test_the_reference_rounds_to_the_oracle(w, h, pw, ph, opaque):
    img = U.rand_image(w + h, h, w, opaque=opaque)
    v = PR.unrounded(img, pw, ph, opaque)
    clear = (PR.tie_distance(PR.rounded_values(v, opaque)) > 1e-6).all(axis=-1)
    assert clear.mean() > 0.9
    assert np.array_equal(PR.finish(v, opaque)[clear], oracle_preview(img, pw, ph)[clear])
    assert PR.consistent(PR.finish(v, opaque), v, PR.EPS, opaque).all()


def test_the_weights_are_the_boxes_of_the_contract():
    for n_out, n_in in [(1, 2), (3, 7), (5, 632), (257, 258), (7, 21), (2, 16382)]:
        wgt = PR.weights(n_out, n_in)
        k = n_in / n_out
        assert np.allclose(wgt.sum(axis=1), k, rtol=0, atol=1e-9) and np.allclose(wgt.sum(axis=0), 1.0, rtol=0, atol=1e-9)
        assert wgt.min() >= 0.0 and wgt.max() <= 1.0
        for X in range(n_out):
            (nz,) = np.nonzero(wgt[X])
            assert nz[0] == int(np.floor(k * X + 1e-12)) and nz[-1] == int(np.ceil(k * (X + 1) - 1e-12)) - 1
    assert np.array_equal(PR.weights(7, 21), np.kron(np.eye(7), np.ones(3)))      # integer ratios: every weight is exactly 1


# ---- the geometry ---------------------------------------------------------------------------------------------------------------

def _shapes_around(boundaries, n_out):
    """source sizes whose ratio to n_out lies on a boundary and on either side of it"""
    return sorted({max(n_out + 1, int(round(b * n_out)) + d) for b in boundaries for d in (-1, 0, 1)})


def test_geometry_is_the_librarys_on_a_sweep_and_beside_every_boundary():
    grid = [1.001 * (9000.0 / 1.001) ** (i / 59.0) for i in range(60)]
    widths = sorted({max(4, int(round(k * 3))) for k in grid})
    # kx: per_group changes at 253 / j, passes at ceil(kx) + 3 crossing 256 and 512, sub at ceil(kx) + 1 crossing 4 .. 64
    widths10 = _shapes_around([253.0 / j for j in range(1, 253)] + [253.0, 509.0, 510.0, 765.0, 2.0, 3.0, 7.0, 15.0, 31.0, 63.0, 64.0], 10)
    # ky: chunks change with ceil(ky) + 2 crossing multiples of 64, chunk_rows grows once that passes 4096, then every 256 rows
    heights10 = _shapes_around([62.0, 126.0, 190.0, 4030.0, 4094.0, 4095.0, 4350.0, 4606.0, 8190.0, 8191.0], 10)
    shapes = [(w, h, 3, 3) for w in widths for h in widths]
    shapes += [(w, h, 10, 10) for w in widths10 for h in (13, 700, 40950)] + [(w, h, 10, 10) for w in (31, 2531) for h in heights10]
    seen = set()
    for w, h, pw, ph in shapes:
        rc, got = _debug_geometry(w, h, pw, ph)
        assert rc == 0 and got == tuple(PR.geometry(w, h, pw, ph)), (w, h, pw, ph, got)
        seen.add((got[0], got[2], got[3], got[4], got[5]))
    assert len(shapes) > 3000 and len(seen) > 100
    for c in PR.CASES:
        assert _debug_geometry(c.w, c.h, c.pw, c.ph) == (0, tuple(PR.geometry(c.w, c.h, c.pw, c.ph)))
    for k in PR.BATCH_KS:
        rc, got = _debug_geometry(5 * k, 5 * k, 5, 5)
        assert rc == 0 and got == tuple(PR.geometry(5 * k, 5 * k, 5, 5)) and (got[0], got[3], got[2], got[5]) == PR.BATCH_REGIMES[k], k


def test_the_boundaries_fall_where_the_rule_says():
    g = PR.geometry
    assert (g(632, 7, 5, 2).per_group, g(506, 7, 4, 2).per_group, g(633, 7, 5, 2).per_group) == (2, 2, 1)
    assert [g(w, 7, 10, 2).passes for w in (2530, 2531, 5090, 5091)] == [1, 2, 2, 3]
    assert [g(9, h, 3, 10).chunks for h in (610, 620, 621, 1260, 1261)] == [1, 1, 2, 2, 3]
    assert [tuple(g(9, h, 3, 2))[4:] for h in (8186, 8188, 8190)] == [(64, 64), (64, 64), (68, 61)]
    assert [g(w, 7, 10, 2).sub for w in (21, 30, 31, 70, 71, 150, 151, 310, 311, 630, 700)] == [4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 64]


def test_shapes_that_do_not_shrink_on_both_axes_take_the_job_path():
    for w, h, pw, ph in [(10, 10, 10, 5), (10, 10, 5, 10), (10, 10, 11, 5), (10, 10, 5, 12), (1, 1, 1, 1), (10, 10, 0, 5), (10, 10, 5, -1),
                         ((1 << 30) + 1, 10, 5, 5)]:
        assert _debug_geometry(w, h, pw, ph) == (1, (0,) * 6), (w, h, pw, ph)
        assert PR.geometry(w, h, pw, ph) is None
    assert L.lib.ist_debug_preview_geometry(10, 10, 5, 5, None) == -1 and "NULL" in L.last_error()
    assert _debug_geometry(1 << 30, 1 << 30, 5, 5)[0] == 0


def test_every_case_claims_its_regime_and_every_regime_is_claimed():
    for c in PR.CASES:
        g = PR.geometry(c.w, c.h, c.pw, c.ph)
        assert (g.per_group, g.sub, PR.rounds(g, c.pw), g.passes, g.chunks, g.chunk_rows) == tuple(c[4:10]), PR.case_id(c)
    claimed = PR.CASES
    assert {c.rounds for c in claimed} >= {1, 2, 4}
    assert {c.sub for c in claimed} == {4, 8, 16, 32, 64}
    assert any(c.w / c.pw > c.sub for c in claimed)                                   # a box wider than sub
    assert {c.per_group == 1 for c in claimed} == {True, False}
    assert {c.passes for c in claimed} == {1, 2, 3}
    assert {c.chunks for c in claimed} >= {1, 2, 3, 22, 64}
    assert {c.chunk_rows for c in claimed} >= {64, 68, 132}
    assert {c.w % 4 for c in PR.KX_SWEEP} == {0, 1, 2, 3}
    # the passes that are claimed really hold columns: a footprint wider than 256 (512) columns
    assert any(c.passes == 2 and c.w // c.pw > 256 for c in claimed) and any(c.passes == 3 and c.w // c.pw > 512 for c in claimed)
    # on both sides of one row per wave slot: 16 slots (4 waves x 4 rows in flight)
    assert {c.h // c.ph for c in PR.KY_SWEEP} >= {13, 15, 17, 61, 63, 65, 127, 129}


# ---- the exact rule -------------------------------------------------------------------------------------------------------------

def test_the_replay_decides_which_cases_are_exact():
    for n in (9, 765, 1533, 3075, 4095, 4225, 12285, 16129, 65025):
        assert PR.exact_ok(n), n
    assert PR.exact_mismatches(253 * 253) == 127              # so no blanket size limit does: 255 * 255 holds, 253 * 253 does not
    for c in PR.CASES:
        n = PR.integer_n(c)
        if c.rule == "exact":
            assert n is not None and (c.w // c.pw) & 1 and (c.h // c.ph) & 1 and PR.exact_ok(n), PR.case_id(c)
    assert all(c.rule == "exact" for c in PR.INTEGER_CASES) and all(c.rule == "consistent" for c in PR.FRACTIONAL_CASES)
    assert [k for k in PR.BATCH_KS if PR.exact_ok(k * k)] == list(PR.BATCH_EXACT)
    for n in (9, 225, 255, 257):
        assert PR.exact_mismatches_translucent(n) == 0, n


def test_the_integer_rules_are_the_reference_rounded():
    for c in (PR.KX_SWEEP[0], PR.KX_SWEEP[9], PR.KY_SWEEP[5], PR.TALL[1]):
        img = PR.case_image(c)
        assert np.array_equal(PR.exact_bytes(img, c.pw, c.ph), PR.finish(PR.unrounded(img, c.pw, c.ph, True), True))
        assert np.array_equal(PR.exact_bytes_translucent(img, c.pw, c.ph), PR.exact_bytes(img, c.pw, c.ph))
    for c in (PR.KX_SWEEP[0], PR.KX_SWEEP[9]):
        soft = PR.case_image(c, opaque=False)
        assert np.array_equal(PR.exact_bytes_translucent(soft, c.pw, c.ph), PR.finish(PR.unrounded(soft, c.pw, c.ph, False), False))


# ---- the inputs -----------------------------------------------------------------------------------------------------------------

def test_ties_are_rare_in_the_inputs():
    """a condition on the inputs, not a measurement of the kernel: where the reference is within the roundoff bound of a tie, either
    byte is a correct rounding and consistent() cannot tell a right sum from a slightly wrong one"""
    near = total = 0
    for c in PR.CASES:
        if c.rule == "exact":
            continue
        for opaque in (True, False):
            d = PR.tie_distance(PR.rounded_values(PR.unrounded(PR.case_image(c, opaque), c.pw, c.ph, opaque), opaque))
            near += int((d < 2e-3).sum())
            total += d.size
    print("%d of %d reference values within 2e-3 of a tie (%.2f %%)" % (near, total, 100.0 * near / total))
    assert total > 200000 and near <= 0.01 * total


def test_exact_cases_without_the_hint_hold_no_near_tie():
    """hint off, n > 257: the premultiplied sums are no integers in fp32 any more, so equality with the integer rule needs every mean
    farther than EPS from a tie - consistent() then admits exactly the integer rule's bytes"""
    for c in PR.INTEGER_CASES:
        if PR.integer_n(c) <= 257:
            continue
        img = PR.case_image(c)
        v = PR.unrounded(img, c.pw, c.ph, False)
        assert PR.tie_distance(PR.rounded_values(v, False)[..., :3]).min() >= PR.EPS, PR.case_id(c)
        want = PR.exact_bytes(img, c.pw, c.ph)
        assert PR.consistent(want, v, PR.EPS, False).all()
        for d in (-1, 1):
            off = want.copy()
            off[..., 0] = np.clip(off[..., 0].astype(np.int64) + d, 0, 255)
            assert not PR.consistent(off, v, PR.EPS, False).any()


# ---- the tests can fail ---------------------------------------------------------------------------------------------------------

def _with(c, opaque, wx=None, wy=None, img=None):
    """the case's bytes with one axis' weights replaced (what a kernel that summed those would store)"""
    img = PR.case_image(c, opaque) if img is None else img
    wx = PR.weights(c.pw, c.w) if wx is None else wx
    wy = PR.weights(c.ph, c.h) if wy is None else wy
    return PR.finish(PR.reduce_with(PR.planes(img, opaque), wy, wx, (c.w * c.h) / float(c.pw * c.ph)), opaque)


def _rejected_exact(c, **kw):
    assert c.rule == "exact"
    img = PR.case_image(c)
    assert np.array_equal(_with(c, True), PR.exact_bytes(img, c.pw, c.ph))            # unperturbed, the rule accepts
    return not np.array_equal(_with(c, True, **kw), PR.exact_bytes(img, c.pw, c.ph))


def _rejected_consistent(c, opaque, **kw):
    v = PR.unrounded(PR.case_image(c, opaque), c.pw, c.ph, opaque)
    assert PR.consistent(_with(c, opaque), v, PR.EPS, opaque).all()
    return not PR.consistent(_with(c, opaque, **kw), v, PR.EPS, opaque).all()


def _case(w, h, pw, ph):
    (c,) = [c for c in PR.CASES if (c.w, c.h, c.pw, c.ph) == (w, h, pw, ph)]
    return c


def test_a_column_dropped_at_the_end_of_a_group_is_rejected():
    c = _case(507, 15, 169, 5)                               # groups of 84 pixels: the first one's footprint ends at column 251
    wx = PR.weights(c.pw, c.w)
    assert wx[83, 251] == 1.0 and wx[84, 252] == 1.0
    wx[83, 251] = 0.0
    assert _rejected_exact(c, wx=wx)
    c = _case(632, 7, 5, 2)                                  # fractional, two pixels per group: column 252 ends the first group
    wx = PR.weights(c.pw, c.w)
    assert 0.79 < wx[1, 252] < 0.81
    wx[1, 252] = 0.0
    assert _rejected_consistent(c, True, wx=wx)


def test_a_seam_column_given_to_the_wrong_neighbour_is_rejected():
    c = _case(507, 15, 169, 5)
    wx = PR.weights(c.pw, c.w)
    wx[84, 252], wx[83, 252] = 0.0, 1.0                      # the first column of the second group, summed by the first
    assert _rejected_exact(c, wx=wx)
    c = _case(495, 15, 15, 5)                                # two column rounds: pixel 4 opens the second round of its group
    wx = PR.weights(c.pw, c.w)
    wx[4, 4 * 33], wx[3, 4 * 33] = 0.0, 1.0
    assert _rejected_exact(c, wx=wx)


@pytest.mark.parametrize("w,first", [(1527, 256), (1539, 512)])
def test_a_skipped_pass_is_rejected(w, first):
    c = _case(w, 15, 3, 5)
    k = c.w // c.pw
    wx = PR.weights(c.pw, c.w)
    for X in range(c.pw):
        assert wx[X, k * X + first:k * (X + 1)].sum() == k - first
        wx[X, k * X + first:] = 0.0                          # the columns of pass 2 (pass 3) never reach the pixel's sum
    assert _rejected_exact(c, wx=wx)


def test_a_row_chunk_moved_by_one_row_is_rejected():
    c = _case(21, 195, 7, 3)                                 # ky 65: chunk 1 holds the box's row 64
    wy = PR.weights(c.ph, c.h)
    for Y in range(c.ph):
        wy[Y, 65 * Y + 64] = 0.0
        if 65 * Y + 65 < c.h:
            wy[Y, 65 * Y + 65] = 1.0
    assert _rejected_exact(c, wy=wy)
    c = _case(21, 387, 7, 3)                                 # ky 129: chunk 0 read one row late
    wy = PR.weights(c.ph, c.h)
    for Y in range(c.ph):
        wy[Y, 129 * Y], wy[Y, 129 * Y + 64] = 0.0, 2.0
    assert _rejected_exact(c, wy=wy)


@pytest.mark.parametrize("w,h,pw,ph,rows", [(21, 195, 7, 3, 64), (21, 387, 7, 3, 128), (15, 8186, 5, 2, 63 * 64), (15, 8190, 5, 2, 60 * 68),
                                            (15, 16382, 5, 2, 62 * 132)])
def test_a_skipped_last_chunk_is_rejected(w, h, pw, ph, rows):
    c = _case(w, h, pw, ph)
    g = PR.geometry(w, h, pw, ph)
    assert rows == (g.chunks - 1) * g.chunk_rows or (g.chunks - 1) * g.chunk_rows >= h // ph      # the last chunk that holds rows
    wy = PR.weights(c.ph, c.h)
    ky = h // ph
    for Y in range(c.ph):
        assert wy[Y, ky * Y + rows:ky * (Y + 1)].sum() >= 1.0
        wy[Y, ky * Y + rows:ky * (Y + 1)] = 0.0
    assert _rejected_exact(c, wy=wy)


@pytest.mark.parametrize("opaque", [True, False])
def test_a_skipped_fractional_row_in_a_chunk_of_its_own_is_rejected(opaque):
    c = _case(21, 191, 7, 3)
    wy = PR.weights(c.ph, c.h)
    (nz,) = np.nonzero(wy[1])
    assert (nz[0], nz[-1]) == (63, 127) and 0.33 < wy[1, 127] < 0.34      # row 127 is the box's 65th: chunk 1
    wy[1, 127] = 0.0
    assert _rejected_consistent(c, opaque, wy=wy)


@pytest.mark.parametrize("w,h,pw,ph", [(601, 97, 273, 44), (1001, 333, 77, 41), (523, 37, 400, 28), (2531, 7, 10, 2)])
@pytest.mark.parametrize("opaque", [True, False])
def test_an_end_weight_taken_from_the_wrong_side_is_rejected(w, h, pw, ph, opaque):
    c = _case(w, h, pw, ph)
    wx = PR.weights(c.pw, c.w)
    for X in range(c.pw):
        (nz,) = np.nonzero(wx[X])
        wx[X, nz[-1]] = 1.0 - wx[X, nz[-1]]
    assert _rejected_consistent(c, opaque, wx=wx)
    wy = PR.weights(c.ph, c.h)
    for Y in range(c.ph):
        (nz,) = np.nonzero(wy[Y])
        wy[Y, nz[0]] = 1.0 - wy[Y, nz[0]]
    assert _rejected_consistent(c, opaque, wy=wy)


@pytest.mark.parametrize("w,h,pw,ph", [(507, 15, 169, 5), (455, 15, 7, 5), (21, 45, 7, 3)])
def test_a_column_read_past_the_window_is_rejected(w, h, pw, ph):
    """the surround of the GPU tests' windows is 255 and the image at most 127: one surround column in the last box raises its sum"""
    c = _case(w, h, pw, ph)
    img = np.concatenate([PR.case_image(c), np.full((c.h, 1, 4), 255, np.uint8)], axis=1)
    wx = np.concatenate([PR.weights(c.pw, c.w), np.zeros((c.pw, 1))], axis=1)
    wx[c.pw - 1, c.w] = 1.0
    assert _rejected_exact(c, wx=wx, img=img)
    wx[c.pw - 1, c.w - 1] = 0.0                              # ... or read INSTEAD of the window's last column
    assert _rejected_exact(c, wx=wx, img=img)


def test_a_fractional_case_one_column_off_is_rejected():
    """the fractional cases of small ratio, both forms: the whole footprint read one column to the right (a misplaced window base).
    (At kx = 126 one column is a 126th of a box, under half an LSB of noise: what finds a column there are the exact cases.)"""
    small = [c for c in PR.FRACTIONAL_CASES if c.w / c.pw < 16]
    assert len(small) == 5
    for c in small:
        for opaque in (True, False):
            wx = np.roll(PR.weights(c.pw, c.w), 1, axis=1)
            assert _rejected_consistent(c, opaque, wx=wx), PR.case_id(c)
