"""CPU suite for text lines (ttr_config.lines; DESIGN.md "Text lines"): the host rule (ttr_lines_from_quads) against the numpy restatement
tests/lines_ref.py - exact, so every comparison is np.array_equal -, its invariants, the hand-made layouts with their stated lines, the
outputs derived from line / word (reading order, line bbox, text joins) and the config checks.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import lines_ref as L

SIZES = (0, 1, 2, 37, 1000)


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


def _rule(quads):
    from tuatara_amd.engine import lines_from_quads
    return lines_from_quads(quads)


def _groups(quads):
    """the engine's lines as lists of item indices: lines in line order, members in word order (checked against numpy first)"""
    line, word, nl = _rule(quads)
    want = L.lines_from_quads(quads)
    assert np.array_equal(line, want[0]) and np.array_equal(word, want[1]) and nl == want[2], (line, word, nl, want)
    order, first = L.reading_order(line, word, nl)
    return [order[first[l]:first[l + 1]].tolist() for l in range(nl)]


@pytest.mark.parametrize("n", SIZES)
def test_random_equals_numpy(built, n):
    for seed in range(3 if n < 1000 else 1):
        q = L.random_quads(n, 100 * n + seed)
        line, word, nl = _rule(q)
        want = L.lines_from_quads(q)
        assert line.dtype == np.int32 and word.dtype == np.int32
        assert np.array_equal(line, want[0]) and np.array_equal(word, want[1]) and nl == want[2]
        if n >= 37:
            assert 1 < nl < n                      # the sets hold both links and loners


@pytest.mark.parametrize("n", SIZES)
def test_invariants(built, n):
    q = L.random_quads(n, 7 + n)
    line, word, nl = _rule(q)
    order, first = L.reading_order(line, word, nl)
    assert np.array_equal(np.sort(order), np.arange(n))                                  # a permutation
    assert len(first) == nl + 1 and first[0] == 0 and first[-1] == n and (np.diff(first) > 0).all()
    for l in range(nl):
        m = order[first[l]:first[l + 1]]
        assert (line[m] == l).all() and np.array_equal(word[m], np.arange(len(m)))       # line / word agree with order / line_first
    # a shuffle of the items changes nothing but the indices (inputs without exact key ties: the tie-breaks are by index)
    c, u, _ = L.cuv(q)
    groups = [order[first[l]:first[l + 1]] for l in range(nl)]
    tie = False
    for m in groups:
        U = u[m].sum(axis=0)
        keys = c[m, 0] * U[0] + c[m, 1] * U[1]
        tie |= len(np.unique(keys)) != len(keys)
    heads = np.array([c[m[0]] for m in groups]).reshape(-1, 2)
    tie |= len(np.unique(heads, axis=0)) != len(heads)
    if n == 1000:
        assert not tie                                                                   # (the large set is one of those)
    if not tie:
        perm = np.random.default_rng(n).permutation(n)
        line2, word2, nl2 = _rule(q[perm])
        assert nl2 == nl and np.array_equal(line2, line[perm]) and np.array_equal(word2, word[perm])


def test_bad_arguments(built):
    from tuatara_amd.engine import EngineError
    q = L.rect_quad(100, 100, 50, 20)[None].copy()
    for bad in (np.nan, np.inf, 32768.0, -40000.0):
        b = q.copy()
        b[0, 3] = bad
        with pytest.raises(EngineError):
            _rule(b)
        with pytest.raises(ValueError):
            L.lines_from_quads(b)
    b = q.copy()
    b[0, 2] = 32767.9                                                                    # the largest coordinates pass
    assert _rule(b)[2] == 1


# ---- hand-made layouts: word widths, a height h and a gap; each must give exactly the stated lines and word order
def test_paragraph_of_three_lines(built):
    h = 20.0
    rows = [[60, 35, 80, 20, 55], [45, 90, 30, 70], [25, 65, 40]]
    q = np.concatenate([L.row_quads(40, 100 + 1.3 * h * r, w, h, 0.4 * h) for r, w in enumerate(rows)])
    assert _groups(q) == [[0, 1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11]]
    perm = np.array([7, 2, 11, 0, 9, 4, 5, 1, 10, 3, 8, 6])                              # any item order: the same lines, in the new indices
    inv = np.argsort(perm)
    assert _groups(q[perm]) == [[int(inv[i]) for i in g] for g in ([0, 1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11])]


def test_two_columns_interleave_by_y(built):
    h = 20.0
    left = [L.row_quads(40, 100 + 2.5 * h * r, [50, 60, 40], h, 0.4 * h) for r in range(3)]                      # ends at x = 206
    right = [L.row_quads(206 + 3 * h, 100 + 2.5 * h * r + 0.5 * h, [70, 30], h, 0.4 * h) for r in range(3)]    # 3 h further right, half a line lower
    q = np.concatenate(left + right)
    assert _groups(q) == [[0, 1, 2], [9, 10], [3, 4, 5], [11, 12], [6, 7, 8], [13, 14]]


@pytest.mark.parametrize("deg", (20.0, -30.0, 44.0))
def test_tilted_parallel_lines(built, deg):
    h = 24.0
    a = np.deg2rad(deg)
    rows = [[70, 40, 90, 50], [55, 85, 35], [60, 60, 60, 60]]
    # the rows' origins step down the page along the lines' normal, 1.5 h apart
    q = np.concatenate([L.row_quads(500 - np.sin(a) * 1.5 * h * r, 300 + np.cos(a) * 1.5 * h * r, w, h, 0.5 * h, deg) for r, w in enumerate(rows)])
    got = _groups(q)
    assert sorted(got) == [[0, 1, 2, 3], [4, 5, 6], [7, 8, 9, 10]]                       # the words of each line in baseline order
    # line order is by the first word's (c.y, c.x)
    c = L.cuv(q)[0]
    assert [g[0] for g in got] == sorted((g[0] for g in got), key=lambda f: (int(c[f, 1]), int(c[f, 0]), f))


def test_heading_beside_body_text(built):
    head = L.row_quads(40, 100, [200], 60.0, 0.0)
    body = L.row_quads(40 + 200 + 10, 100, [50, 70], 20.0, 8.0)                          # same centre line, 10 px away, a third of the height
    assert _groups(np.concatenate([head, body])) == [[0], [1, 2]]


def test_height_ratio_one_and_a_half_links(built):
    q = np.concatenate([L.row_quads(40, 100, [80], 20.0, 0.0), L.row_quads(40 + 80 + 8, 100, [60], 30.0, 0.0)])
    assert _groups(q) == [[0, 1]]


def test_gap_threshold(built):
    h = 30.0
    linked = L.row_quads(40, 100, [90, 60], h, 29.0)                                     # a gap of 29/30 h
    apart = L.row_quads(40, 100, [90, 60], h, 31.0)                                      # 31/30 h
    assert _groups(linked) == [[0, 1]]
    assert _groups(apart) == [[0], [1]]


def test_quarter_turned_neighbour_does_not_link(built):
    a = L.rect_quad(100, 100, 80, 20, 0.0)
    b = L.rect_quad(100 + 40 + 6 + 10, 100, 80, 20, 90.0)                                # upright beside it, 6 px away: 20 wide, 80 tall
    assert _groups(np.stack([a, b])) == [[0], [1]]
    c = L.rect_quad(100 + 40 + 6 + 40, 100, 80, 20, 180.0)                               # upside down: the baselines point opposite ways
    assert _groups(np.stack([a, c])) == [[0], [1]]


def test_degenerate_words_stand_alone(built):
    q = np.concatenate([L.row_quads(40, 100, [50, 60], 20.0, 8.0), np.float32([[70, 100] * 4]), np.float32([[60, 100, 90, 100, 90, 100, 60, 100]])])
    assert _groups(q) == [[0, 1], [2], [3]]                                              # (all on y = 100: line order by c.x - the row's first word at 65, the point at 70, the segment at 75)


def test_line_bbox_and_text_joins(built):
    """The outputs derived from line / word on a small hand-made result: the ABI's ttr_results_gather_lines layout is checked on the GPU;
    here the numpy restatement of the derivation against the stated values, and ttr_lines_from_quads feeding it."""
    h = 20.0
    q = np.concatenate([L.row_quads(40, 140, [60, 30], h, 8.0), L.row_quads(40, 100, [50, 40, 70], h, 8.0)])
    texts = ["world", "again", "hello", "big", "round"]
    bbox = np.float32([[q[i, 0::2].min(), q[i, 1::2].min(), q[i, 0::2].max(), q[i, 1::2].max()] for i in range(5)])
    bbox[3, 1] -= 3                                                                      # one word a little taller
    line, word, nl = _rule(q)
    assert line.tolist() == [1, 1, 0, 0, 0] and word.tolist() == [0, 1, 0, 1, 2] and nl == 2
    order, first = L.reading_order(line, word, nl)
    assert order.tolist() == [2, 3, 4, 0, 1] and first.tolist() == [0, 3, 5]
    assert L.line_texts(texts, order, first) == ["hello big round", "world again"]
    assert L.page_text(texts, order, first) == "hello big round\nworld again"
    assert np.array_equal(L.line_bboxes(bbox, order, first), np.float32([[40, 87, 40 + 50 + 8 + 40 + 8 + 70, 110], [40, 130, 138, 150]]))
    from tuatara_amd.engine import PageResult
    pr = PageResult(texts, bbox, np.zeros((5, 26), np.int32), line=line, word=word, order=order, line_first=first, line_bbox=L.line_bboxes(bbox, order, first))
    assert pr.text == "hello big round\nworld again"
    assert [ln["items"] for ln in pr.lines] == [[2, 3, 4], [0, 1]] and pr.lines[1]["bbox"] == [40.0, 130.0, 138.0, 150.0]
    assert (pr[4]["line"], pr[4]["word"]) == (0, 2)
    off = PageResult(texts, bbox, np.zeros((5, 26), np.int32))
    assert off.lines == [] and off.text == "" and "line" not in off[0]


def test_config_field_and_checks(built, tmp_path):
    from tuatara_amd import engine
    cfg = engine.Config()
    engine.load().ttr_config_default(ctypes.byref(cfg))
    assert cfg.lines == 0
    assert engine.Config.lines.offset == engine.Config.orient_page.offset + 4            # appended: the earlier fields keep their offsets
    for kw, msg in (({"lines": 2}, "lines must be"), ({"lines": -1}, "lines must be"), ({"lines": 1, "max_components": 5000}, "max_components")):
        with pytest.raises(engine.EngineError, match=msg):
            engine.Engine(str(tmp_path), **kw)


def test_run_ocr_annotate_by_lines():
    """bindings/run_ocr.py: annotate keeps its output unless by_lines=True, which lays the third panel out by (line, word) with a row per line."""
    import os
    import sys
    from tests.conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "bindings"))
    import run_ocr
    img = np.full((200, 320, 3), 255, np.uint8)
    plain = [{"text": "right", "bbox": [200, 40, 260, 60]}, {"text": "left", "bbox": [20, 42, 80, 62]}, {"text": "below", "bbox": [20, 100, 90, 120]}]
    lined = [dict(d, line=l, word=w) for d, (l, w) in zip(plain, ((0, 1), (0, 0), (1, 0)))]
    base = np.array(run_ocr.annotate(img, plain))
    assert np.array_equal(np.array(run_ocr.annotate(img, lined)), base)                    # the extra keys alone change nothing
    assert np.array_equal(np.array(run_ocr.annotate(img, plain, by_lines=True)), base)     # no lines in the items: the default layout
    by = np.array(run_ocr.annotate(img, lined, by_lines=True))
    assert by.shape == base.shape and np.array_equal(by[:, :640], base[:, :640])           # the first two panels are the same
    rows = lambda a: np.flatnonzero(a[:, 640:].any(axis=(1, 2)))                           # noqa: E731
    assert rows(by).max() > rows(base).max()                                               # "below" starts a row of its own
