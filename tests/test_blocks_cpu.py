"""CPU suite for text blocks (ttr_config.blocks; DESIGN.md "Text blocks"): the host rule (ttr_blocks_from_quads) against the numpy restatement
tests/blocks_ref.py - exact, so every comparison is np.array_equal -, the hand-made layouts with their stated blocks and reading order, the
cap, a precedence cycle, the invariance under word permutation, the outputs derived from block / pos and the config checks.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import blocks_ref as B
from tests import lines_ref as L


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


def _rule(quads):
    from tuatara_amd.engine import blocks_from_quads
    return blocks_from_quads(quads)


def _same(got, want):
    assert len(got) == len(want) == 7
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (k, g, w)


def _checked(quads):
    """the engine's rule on the quads, checked against numpy -> (line, word, n_lines, block, pos, n_blocks, mode)"""
    got = _rule(quads)
    _same(got, B.blocks_from_quads(quads))
    assert got[3].dtype == np.int32 and got[4].dtype == np.int32
    return got


def _partition(quads):
    """the blocks as a set of frozensets of word indices, and the blocks in reading order as lists of word-index lists (line after line)"""
    line, word, nl, block, pos, nb, _ = _checked(quads)
    order, first = B.block_order(block, pos, nb)
    worder, wfirst = L.reading_order(line, word, nl)
    seq = [[worder[wfirst[l]:wfirst[l + 1]].tolist() for l in order[first[b]:first[b + 1]]] for b in range(nb)]
    return {frozenset(i for ln in blk for i in ln) for blk in seq}, seq


@pytest.mark.parametrize("n", (0, 1, 2, 37, 1000))
def test_random_equals_numpy(built, n):
    for seed in range(3 if n < 1000 else 1):
        line, word, nl, block, pos, nb, mode = _checked(L.random_quads(n, 300 * n + seed))
        assert len(block) == len(pos) == nl and mode == 1 and (nb >= 1) == (n >= 1) and nb <= nl
        if n == 0:
            assert nb == 0


@pytest.mark.parametrize("seed", range(12))
def test_generated_pages_equal_numpy(built, seed):
    q = B.random_page(seed)
    line, word, nl, block, pos, nb, mode = _checked(q)
    order, first = B.block_order(block, pos, nb)
    assert np.array_equal(np.sort(order), np.arange(nl)) and (np.diff(first) > 0).all() and mode == 1
    assert 1 <= nb <= nl


def test_null_outputs_and_refused_inputs(built):
    from tuatara_amd import engine
    lib = engine.load()
    q = np.ascontiguousarray(L.random_quads(37, 5))
    nb, mode = ctypes.c_int32(-7), ctypes.c_int32(-7)
    assert lib.ttr_blocks_from_quads(engine._f(q), 37, None, None, None, None, None, ctypes.byref(nb), ctypes.byref(mode)) == 0
    assert (nb.value, mode.value) == _rule(q)[5:]
    assert lib.ttr_blocks_from_quads(engine._f(q), 37, None, None, None, None, None, None, None) == 0
    block = np.full(37, 99, np.int32)
    assert lib.ttr_blocks_from_quads(engine._f(q), 37, None, None, None, engine._i(block), None, None, None) == 0
    nl = _rule(q)[2]
    assert np.array_equal(block[:nl], _rule(q)[3]) and (block[nl:] == -1).all()          # per line; -1 behind the lines
    assert lib.ttr_blocks_from_quads(None, 0, None, None, None, None, None, ctypes.byref(nb), ctypes.byref(mode)) == 0
    assert (nb.value, mode.value) == (0, 1)                                              # an empty page: no blocks, mode 1
    assert lib.ttr_blocks_from_quads(None, 3, None, None, None, None, None, None, None) == -1
    assert lib.ttr_blocks_from_quads(engine._f(q), -1, None, None, None, None, None, None, None) == -1
    for bad in (np.inf, np.nan, 32768.0, -40000.0):
        b = q.copy()
        b[11, 3] = bad
        with pytest.raises(engine.EngineError, match="finite"):
            _rule(b)


# ------------------------------------------------------------------------------------------------- the hand-made layouts
def _two_paragraphs(leading, deg=0.0, h=20.0):
    """a four-line and a three-line paragraph of 20 px words, one blank line between them"""
    a = np.deg2rad(deg)
    d = (4 + 1) * leading * h
    p1, _ = B.paragraph(300, 200, 600, 4, h, leading, deg, seed=11)
    p2, _ = B.paragraph(300 - np.sin(a) * d, 200 + np.cos(a) * d, 600, 3, h, leading, deg, seed=12)
    return np.concatenate([p1, p2]), len(p1)


@pytest.mark.parametrize("leading", (1.2, 1.33, 1.6, 2.0, 2.2))
def test_paragraphs_split_at_the_blank_line(built, leading):
    q, n1 = _two_paragraphs(leading)
    line, word, nl, block, pos, nb, mode = _checked(q)
    assert nl == 7 and nb == 2 and mode == 1
    parts, seq = _partition(q)
    assert parts == {frozenset(range(n1)), frozenset(range(n1, len(q)))}
    assert [len(b) for b in seq] == [4, 3]                                               # the upper paragraph first, its lines top to bottom
    assert block.tolist() == [0, 0, 0, 0, 1, 1, 1] and pos.tolist() == [0, 1, 2, 3, 0, 1, 2]


def test_a_leading_of_2_3_heights_gives_single_lines(built):
    q, _ = _two_paragraphs(2.3)
    line, word, nl, block, pos, nb, mode = _checked(q)
    assert nl == 7 and nb == 7 and pos.tolist() == [0] * 7 and block.tolist() == list(range(7))


def test_tilted_column_gives_the_same_two_blocks(built):
    q, n1 = _two_paragraphs(1.33, deg=15.0)
    parts, seq = _partition(q)
    assert parts == {frozenset(range(n1)), frozenset(range(n1, len(q)))} and [len(b) for b in seq] == [4, 3]
    assert set(seq[0][0]) < set(range(n1))                                               # the upper paragraph is read first


def test_two_section_page_reads_columns_in_order(built):
    q, names, rows, counts = B.two_section_page()
    line, word, nl, block, pos, nb, mode = _checked(q)
    assert nl == 25 and nb == 9 and mode == 1
    start = np.cumsum([0] + counts)
    parts, seq = _partition(q)
    assert parts == {frozenset(range(start[k], start[k + 1])) for k in range(9)}         # one block per part
    got = [names[int(np.searchsorted(start, blk[0][0], side="right")) - 1] for blk in seq]
    assert got == ["heading", "L1", "L2", "R1", "R2", "heading2", "L3", "R3", "footer"] == names
    assert [len(blk) for blk in seq] == rows
    # the line order (c.y, c.x) interleaves the columns: the second line of the page's line order is not in L1
    worder, wfirst = L.reading_order(line, word, nl)
    by_line = [names[int(np.searchsorted(start, worder[wfirst[l]], side="right")) - 1] for l in range(nl)]
    assert by_line[:4] == ["heading", "L1", "R1", "L1"]


def test_joined_rows_of_two_columns_stay_one_block_per_paragraph(built):
    """two columns closer than one text height: the line rule joins their rows, and the joined paragraphs are one block each"""
    h, ld = 20.0, 1.4
    rows = []
    for r in range(7):
        if r == 3:
            continue                                                                     # the blank line
        rows.append(np.concatenate([L.row_quads(100, 100 + ld * h * r, [80, 60, 90], h, 8.0), L.row_quads(100 + 246 + 15, 100 + ld * h * r, [70, 85, 60], h, 8.0)]))
    q = np.concatenate(rows)
    line, word, nl, block, pos, nb, mode = _checked(q)
    assert nl == 6 and nb == 2
    assert block.tolist() == [0, 0, 0, 1, 1, 1] and pos.tolist() == [0, 1, 2, 0, 1, 2]


def test_the_cap(built):
    q = B.isolated_words(513)
    line, word, nl, block, pos, nb, mode = _checked(q)
    assert nl == 513 and nb == 513 and mode == 0 and (pos == 0).all()
    c, u, v = L.cuv(q)
    ext = np.abs(u) + np.abs(v)
    keys = sorted((int(c[i, 1] - ext[i, 1]), int(c[i, 0] - ext[i, 0]), int(line[i])) for i in range(513))   # (y0, x0, root): every word its own line
    want = np.zeros(513, np.int32)
    for rank, (_, _, l) in enumerate(keys):
        want[l] = rank
    assert np.array_equal(block, want)
    line, word, nl, block, pos, nb, mode = _checked(q[:512])
    assert nb == 512 and mode == 1
    assert np.array_equal(np.sort(block), np.arange(512))


def test_a_precedence_cycle_ends(built):
    """four blocks: A is left of B and nothing between them spans both; B is above C, C above D and D above A, each pair overlapping in x:
    A < B < C < D < A.  (C also lies left of ... no: A left of C and D left of B are barred by D and C, which span those pairs.)  Nothing is
    free, so the smallest key goes first - B, the topmost; that frees C, then D, then A."""
    A = L.rect_quad(50, 400, 100, 20)                   # x 0..100
    Bq = L.rect_quad(250, 100, 100, 20)                 # x 200..300
    Cq = L.rect_quad(200, 200, 100, 20)                 # x 150..250: overlaps B and D
    D = L.rect_quad(105, 300, 110, 20)                  # x 50..160: overlaps C and A
    q = np.stack([A, Bq, Cq, D])
    c, u, v = L.cuv(q)
    ext = np.abs(u) + np.abs(v)
    x0, x1, y0, y1 = (c - ext)[:, 0], (c + ext)[:, 0], (c - ext)[:, 1], (c + ext)[:, 1]
    P = B.precedence(x0.tolist(), x1.tolist(), [(int(y0[i] + y1[i]), i) for i in range(4)])
    assert P.tolist() == [[False, True, False, False], [False, False, True, False], [False, False, False, True], [True, False, False, False]]
    line, word, nl, block, pos, nb, mode = _checked(q)
    assert nl == 4 and nb == 4 and mode == 1 and line.tolist() == [3, 0, 1, 2]
    assert block[line].tolist() == [3, 0, 1, 2]                                          # read B, C, D, A


def test_partition_is_invariant_under_word_permutation(built):
    for k, q in enumerate([B.two_section_page()[0], B.random_page(3), B.random_page(8), _two_paragraphs(1.6, 7.0)[0]]):
        parts, seq = _partition(q)
        perm = np.random.default_rng(40 + k).permutation(len(q))
        parts2, seq2 = _partition(q[perm])
        assert {frozenset(int(perm[i]) for i in p) for p in parts2} == parts
        flat = lambda s: [[perm[i] for i in ln] for blk in s for ln in blk]               # noqa: E731
        assert [[int(i) for i in ln] for ln in flat(seq2)] == [ln for blk in seq for ln in blk]   # and the reading order (no key ties on these pages)


# ------------------------------------------------------------------------------------------------- derived outputs, surface
def test_block_order_bboxes_and_text_joins(built):
    h = 20.0
    left = np.concatenate([L.row_quads(40, 100, [50, 40], h, 8.0), L.row_quads(40, 128, [60, 30], h, 8.0)])
    right = np.concatenate([L.row_quads(300, 100, [45, 45], h, 8.0), L.row_quads(300, 128, [70], h, 8.0)])
    q = np.concatenate([right, left])
    texts = ["c1", "c2", "d1", "a1", "a2", "b1", "b2"]
    bbox = np.float32([[q[i, 0::2].min(), q[i, 1::2].min(), q[i, 0::2].max(), q[i, 1::2].max()] for i in range(7)])
    line, word, nl, block, pos, nb, mode = _checked(q)
    assert nl == 4 and line.tolist() == [1, 1, 3, 0, 0, 2, 2]                            # (c.y, c.x): the columns interleave
    assert nb == 2 and block.tolist() == [0, 1, 0, 1] and pos.tolist() == [0, 0, 1, 1]
    order, first = B.block_order(block, pos, nb)
    assert order.tolist() == [0, 2, 1, 3] and first.tolist() == [0, 2, 4]
    worder, wfirst = L.reading_order(line, word, nl)
    ltexts = L.line_texts(texts, worder, wfirst)
    lbox = L.line_bboxes(bbox, worder, wfirst)
    assert L.page_text(texts, worder, wfirst) == "a1 a2\nc1 c2\nb1 b2\nd1"
    assert B.block_texts(ltexts, order, first) == ["a1 a2\nb1 b2", "c1 c2\nd1"]
    assert B.page_text_blocks(ltexts, order, first) == "a1 a2\nb1 b2\n\nc1 c2\nd1"
    bbx = B.block_bboxes(lbox, order, first)
    assert np.array_equal(bbx, np.float32([[40, 90, 138, 138], [300, 90, 398, 138]]))
    assert B.item_blocks(line, block).tolist() == [1, 1, 1, 0, 0, 0, 0]
    from tuatara_amd.engine import PageResult
    pr = PageResult(texts, bbox, np.zeros((7, 26), np.int32), line=line, word=word, order=worder, line_first=wfirst, line_bbox=lbox,
                    block=B.item_blocks(line, block), line_block=block, line_pos=pos, block_order=order, block_first=first, block_bbox=bbx, block_mode=mode)
    assert pr.text == "a1 a2\nc1 c2\nb1 b2\nd1" and pr.text_blocks == "a1 a2\nb1 b2\n\nc1 c2\nd1"
    assert [b["lines"] for b in pr.blocks] == [[0, 2], [1, 3]] and pr.blocks[1]["bbox"] == [300.0, 90.0, 398.0, 138.0]
    assert pr.blocks[0]["text"] == "a1 a2\nb1 b2" and pr[0]["block"] == 1 and pr[3]["block"] == 0 and pr.block_mode == 1
    off = PageResult(texts, bbox, np.zeros((7, 26), np.int32), line=line, word=word, order=worder, line_first=wfirst, line_bbox=lbox)
    assert off.blocks == [] and off.text_blocks == "" and "block" not in off[0] and off.text == pr.text


def test_config_field_and_checks(built, tmp_path):
    from tuatara_amd import engine
    cfg = engine.Config()
    engine.load().ttr_config_default(ctypes.byref(cfg))
    assert cfg.blocks == 0
    assert engine.Config.blocks.offset == engine.Config.chars.offset + 4                 # appended: the earlier fields keep their offsets
    for kw, msg in (({"blocks": 2, "lines": 1}, "blocks must be 0 or 1"), ({"blocks": -1, "lines": 1}, "blocks must be 0 or 1"),
                    ({"blocks": 1}, "blocks needs lines = 1"), ({"blocks": 1, "lines": 0}, "blocks needs lines = 1")):
        with pytest.raises(engine.EngineError, match=msg):
            engine.Engine(str(tmp_path), **kw)


def test_run_ocr_annotate_by_blocks():
    """bindings/run_ocr.py: by_blocks=True lays the third panel out by (block, line, word), a row per line and an empty row between blocks."""
    import os
    import sys
    from tests.conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "bindings"))
    import run_ocr
    img = np.full((200, 320, 3), 255, np.uint8)
    plain = [{"text": "right", "bbox": [200, 40, 260, 60]}, {"text": "left", "bbox": [20, 42, 80, 62]}, {"text": "below", "bbox": [20, 100, 90, 120]}]
    lined = [dict(d, line=l, word=0, block=b) for d, (l, b) in zip(plain, ((1, 1), (0, 0), (2, 0)))]
    base = np.array(run_ocr.annotate(img, plain))
    assert np.array_equal(np.array(run_ocr.annotate(img, lined)), base)                    # the extra keys alone change nothing
    assert np.array_equal(np.array(run_ocr.annotate(img, plain, by_blocks=True)), base)    # no blocks in the items: the default layout
    by = np.array(run_ocr.annotate(img, lined, by_blocks=True))
    assert by.shape == base.shape and np.array_equal(by[:, :640], base[:, :640])           # the first two panels are the same
    rows = lambda a: np.flatnonzero(a[:, 640:].any(axis=(1, 2)))                           # noqa: E731
    assert rows(by).max() > rows(np.array(run_ocr.annotate(img, lined, by_lines=True))).max()   # the blank row between the blocks
