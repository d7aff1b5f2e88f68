"""The three host rules of the overlap search (ist_overlap_edge, ist_overlap_select, ist_overlap_rows: pure CPU) against the numpy
restatement of the contract (tests/overlap_reference.py), and the argument rules of the calls that need no GPU to refuse."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import imagestitching_amd as ist
from imagestitching_amd import _lib as L
from tests import overlap_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edge(d, T):
    arr = (C.c_int64 * max(1, len(d)))(*[int(v) for v in d])
    t = C.c_int32(-1)
    assert L.lib.ist_overlap_edge(arr, len(d), int(T), C.byref(t)) == 0
    return t.value


def _select(cost, inf, kmax, T, **opts):
    o = dict(R.DEFAULTS, **opts)
    co = L.OverlapOpts(o["tolerance"], o["min_rows"], o["min_informative"], 0)
    n = max(1, kmax + 1)
    k = C.c_int32(-1)
    assert L.lib.ist_overlap_select((C.c_int64 * n)(*[int(v) for v in cost[:n]]), (C.c_int32 * n)(*[int(v) for v in inf[:n]]), kmax, int(T), C.byref(co), C.byref(k)) == 0
    return k.value


def test_the_header_states_the_contract_and_its_defaults():
    text = open(os.path.join(ROOT, "include", "imagestitch.h"), encoding="utf-8").read()
    for must in ("e(c) = floor(c w / 32)", "floor(t / 4)", "kmax = min(bodyA, bodyB - 1)", "SMALLER", "contract defaults", "not measured optima",
                 "two 8-bit levels per pixel"):
        assert must in re.sub(r"\s*\n \*\s*", " ", text), must
    assert C.sizeof(L.OverlapOpts) == 16 and C.sizeof(L.Overlap) == 24


def test_edge_rule_on_random_rows():
    rng = np.random.default_rng(1)
    for trial in range(300):
        n = int(rng.integers(0, 60))
        T = int(rng.integers(0, 50))
        p = rng.choice([0.05, 0.25, 0.5, 0.9])
        d = np.where(rng.random(n) < p, T + 1 + rng.integers(0, 100, n), rng.integers(0, T + 1, n))
        assert _edge(d, T) == R.edge_rule(d, T), (trial, list(d), T)


def test_edge_rule_at_the_allowance_and_at_the_end():
    T, ok, bad = 10, 10, 11                                   # (d == T matches: the rule is <=)
    assert _edge([], T) == 0
    assert _edge([bad] * 8, T) == 0
    assert _edge([ok] * 8, T) == 8                            # a run that ends exactly at L
    assert _edge([ok] * 7 + [bad], T) == 7
    # t = 8 allows two misses: exactly two pass, three do not (the rule then falls back to the last t that held)
    assert _edge([ok, ok, ok, bad, bad, ok, ok, ok], T) == 8
    assert _edge([ok, ok, ok, bad, bad, bad, ok, ok], T) == 3
    assert _edge([ok, ok, ok, bad, bad, bad, ok, ok, ok, ok, ok, ok], T) == 12     # ... until t / 4 has caught up
    assert _edge([bad, ok, ok, ok], T) == 4                   # one miss in front needs t >= 4
    assert _edge([bad, ok, ok], T) == 0
    for d in ([ok, ok, ok, bad, bad, ok, ok, ok], [bad, ok, ok, ok], [bad, ok, ok], [ok] * 7 + [bad]):
        assert _edge(d, T) == R.edge_rule(d, T)


def test_selection_on_random_tables():
    rng = np.random.default_rng(2)
    for trial in range(300):
        kmax = int(rng.integers(-1, 80))
        T = int(rng.integers(1, 40))
        n = max(1, kmax + 1)
        cost = np.concatenate([[0], np.cumsum(rng.integers(0, 2 * T + 1, n - 1) * (rng.random(n - 1) < 0.6))]) if n > 1 else np.zeros(1, np.int64)
        inf = np.concatenate([[0], np.cumsum(rng.random(n - 1) < 0.5)]).astype(np.int64) if n > 1 else np.zeros(1, np.int64)
        opts = {"min_rows": int(rng.integers(0, 20)), "min_informative": int(rng.integers(0, 12))}
        assert _select(cost, inf, kmax, T, **opts) == R.select_rule(cost, inf, kmax, T, **opts), trial


def test_selection_ties_go_to_the_smaller_k_and_each_condition_counts():
    T = 10
    n = 41
    inf = list(range(n))
    # cost(k) = 3 k everywhere: every mean is equal, the smallest candidate wins
    assert _select([3 * k for k in range(n)], inf, n - 1, T) == 16
    # 20 and 40 tie exactly below the rest (mean 1): 20
    cost = [3 * k for k in range(n)]
    cost[20], cost[40] = 20, 40
    assert _select(cost, inf, n - 1, T) == 20
    cost[40] = 39                                             # 39 / 40 < 20 / 20
    assert _select(cost, inf, n - 1, T) == 40
    # the best mean fails only the informative count: the next one is taken
    few = list(inf)
    few[40] = 7
    assert _select(cost, few, n - 1, T) == 20
    # ... or only the cost bound (cost <= T k is inclusive)
    dear = [T * k + 1 for k in range(n)]
    assert _select(dear, inf, n - 1, T) == 0
    dear[30] = T * 30
    assert _select(dear, inf, n - 1, T) == 30
    assert _select(dear, [0] * n, n - 1, T) == 0
    # below min_rows nothing is looked at; kmax below min_rows gives 0
    assert _select([0] * n, inf, 15, T) == 0
    assert _select([0] * n, inf, 16, T) == 16
    # products beyond 64 bits compare exactly
    big = [0] * n
    for k in range(n):
        big[k] = (2 ** 56) * k
    big[33] -= 1
    assert _select(big, inf, n - 1, 2 ** 57) == 33 == R.select_rule(big, inf, n - 1, 2 ** 57)


def test_crop_rule_against_the_reference():
    rng = np.random.default_rng(3)
    rec = lambda h, f, k: {"header": h, "footer": f, "overlap": k, "cost": 5}
    assert ist.overlap_rows([rec(44, 50, 100)], [640, 640]) == [(0, 590), (144, 640)]          # n = 2
    assert ist.overlap_rows([rec(44, 50, 0)], [640, 700]) == [(0, 640), (0, 700)]              # K = 0: the bars stay too
    assert ist.overlap_rows([rec(10, 10, 40), rec(10, 10, 30)], [60, 60, 60]) == [(0, 50), (50, 60), (0, 60)]      # the void rule
    assert ist.overlap_rows([], [9]) == [(0, 9)]
    for trial in range(200):
        n = int(rng.integers(1, 7))
        heights = [int(h) for h in rng.integers(20, 90, n)]
        pairs = []
        for i in range(n - 1):
            hm = min(heights[i], heights[i + 1])
            h, f = int(rng.integers(0, hm // 2 + 1)), int(rng.integers(0, hm // 2 + 1))
            kmax = min(heights[i] - h - f, heights[i + 1] - h - f - 1)
            pairs.append(rec(h, f, int(rng.integers(0, kmax + 1)) if kmax > 0 and rng.random() < 0.7 else 0))
        got = ist.overlap_rows(pairs, heights)
        assert got == R.overlap_rows(pairs, heights), (trial, pairs, heights)
        assert got[0][0] == 0 and got[-1][1] == heights[-1] and all(b - t >= 1 for t, b in got[1:-1])


def test_argument_errors():
    t = C.c_int32(0)
    d = (C.c_int64 * 2)(1, 2)
    i32 = (C.c_int32 * 2)(0, 1)
    assert L.lib.ist_overlap_edge(None, 2, 1, C.byref(t)) == -1
    assert L.lib.ist_overlap_edge(d, -1, 1, C.byref(t)) == -1
    assert L.lib.ist_overlap_edge(d, 2, 1, None) == -1
    assert L.lib.ist_overlap_select(None, i32, 1, 1, None, C.byref(t)) == -1
    assert L.lib.ist_overlap_select(d, None, 1, 1, None, C.byref(t)) == -1
    assert L.lib.ist_overlap_select(d, i32, 1, 1, None, None) == -1
    assert L.lib.ist_overlap_select(d, i32, 1, 1, C.byref(L.OverlapOpts(-1, 16, 8, 0)), C.byref(t)) == -1 and "negative" in L.last_error()
    assert L.lib.ist_overlap_select(d, i32, 1, 1, None, C.byref(t)) == 0 and t.value == 0     # NULL opts: the defaults (min_rows 16)
    one = (L.Overlap * 1)()
    h = (C.c_int32 * 2)(5, 5)
    assert L.lib.ist_overlap_rows(one, h, 0, i32, i32) == -1
    assert L.lib.ist_overlap_rows(None, h, 2, i32, i32) == -1
    assert L.lib.ist_overlap_rows(one, None, 2, i32, i32) == -1
    assert L.lib.ist_overlap_rows(one, h, 2, None, i32) == -1
    with pytest.raises(ValueError):
        ist.overlap_rows([], [5, 5])
    # the calls that run on a GPU refuse these before they ask for one
    out = (L.Overlap * 1)()
    p = (C.c_void_p * 2)()
    assert L.lib.ist_bitmaps_overlap(None, p, 2, None, out) == -4
    assert L.lib.ist_overlap_device(None, p, None, None, 2, None, out) == -4
    assert L.lib.ist_bitmap_rows(None, 0, 1) is None and "NULL" in L.last_error()
    assert L.lib.ist_debug_overlap_launches() == 0 or L.lib.ist_debug_overlap_launches() % 3 == 0


def test_the_option_is_refused_where_it_does_not_apply():
    a = np.zeros((4, 4, 4), np.uint8)
    assert ist.DEFAULT_OPTS["overlap"] is None
    for call in (lambda: ist.stitch([a, a], "vertical", {"overlap": "auto"}),
                 lambda: ist.stitch_png([a, a], "vertical", {"overlap": "auto"}),
                 lambda: ist.stitch_jpeg([a, a], "vertical", {"overlap": {"tolerance": 4}}),
                 lambda: ist.plan([a, a], "vertical", {"overlap": "auto"}),
                 lambda: ist.stitch_batch([([a, a], "vertical", {"overlap": "auto"})])):
        with pytest.raises(TypeError) as e:
            call()
        assert "overlap" in str(e.value)
    with pytest.raises(TypeError) as e:
        ist.stitch([a, a], "vertical", {"overlap": "auto"})
    assert "upload_bitmap" in str(e.value) and "decode_bitmaps" in str(e.value)
    with pytest.raises(TypeError):
        ist.stitch([a, a], "vertical", {"overlap": "always"})
    with pytest.raises(TypeError):
        ist.stitch([a, a], "vertical", {"overlap": {"rows": 3}})
    with pytest.raises(TypeError):
        ist.find_overlaps([a, a])
