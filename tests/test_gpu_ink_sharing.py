"""GPU suite for the one decision the ink readers share (DESIGN.md "Adding a page layer"): which of tables, selection marks and barcodes enqueues a batch's ink
pass.  The bitmaps in place are reused exactly when the LAST pass of the batch ran under the rule the next reader wants - the local rule, or the fixed one with
the same `ink` - so the counts below follow from the order tables, marks, barcodes alone; no measurement is involved.  One small page (a table of two cells, one
checkbox, two words, one Code 128 barcode), a one-page batch per case through one engine; every case also holds the three layers' views to the host rules on the
same image and the returned quads, so a pass that was wrongly shared shows as wrong bits too, not only as a wrong count."""
import numpy as np
import pytest

from tests import barcodes_ref as B
from tests import marks_ref as M
from tests import tables_ref as T

pytestmark = pytest.mark.gpu

A_, B_, C_ = 128, 96, 160            # three thresholds under which a black-on-white page has the same ink (checked below, on the CPU)
MIN_LEN, MARKS, BARCODES = 48, (10, 64, 24), (8, 3)   # the layers' other parameters: (min_side, max_side, fill), (min_lines, symbologies)
LOCAL = (16, 38, 0)                  # radius, drop, dark ink


@pytest.fixture(scope="module")
def eng(weights):
    """a rectified engine (its results carry the quads); every layer OFF at rest"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    build_lib()
    e = Engine(weights["dir"], crop_mode=CROP_RECTIFIED, mixed_batches=1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def page():
    """256 x 320: a table of one row and two cells, a word in its second cell and one beside it, a ticked checkbox, a Code 128 label - pure black on white"""
    img = M.blank(256, 320)
    for y in (60, 110):
        T.hline(img, y, 40, 240)
    for x in (40, 140, 240):
        T.vline(img, x, 60, 110)
    rng = np.random.default_rng(5)
    for x, y in ((160, 78), (60, 20)):                                                # the "words": bars of seeded noise, what the test detector boxes
        img[y:y + 14, x:x + 64] = np.where(rng.random((14, 64, 1)) < 0.7, 0, 255)
    M.frame(img, 270, 20, 16, 1)
    M.cross(img, 274, 24, 8)
    B.draw(img, B.text128(b"INK-42"), 2, 30, 170, 24)
    for t in (B_, C_):                                                                # the same set of pixels under A, B and C
        assert np.array_equal(T.ink_mask(img, A_), T.ink_mask(img, t))
    return img


def _host(E, page, quads, ink):
    """the three host rules on the page under one ink rule: ink an int (the fixed rule) or a tuple (the local one)"""
    if isinstance(ink, tuple):
        return (E.tables_from_page_ink(page, quads, MIN_LEN, local_ink=ink), E.marks_from_page_ink(page, quads, *MARKS, local_ink=ink),
                E.barcodes_from_page_ink(page, quads, *BARCODES, local_ink=ink))
    return (E.tables_from_page(page, quads, MIN_LEN, ink), E.marks_from_page(page, quads, *MARKS, ink), E.barcodes_from_page(page, quads, BARCODES[0], ink, BARCODES[1]))


def _same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), (what, got, want)


def _views_equal_host(E, res, page, tables, marks, barcodes, local):
    """every layer that ran: its views equal its host rule's on the same image and quads, under the rule the batch ran it with; the others' stay empty"""
    quads = res.quad if len(res) else None
    n = len(res)
    if tables and n:
        want = _host(E, page, quads, local or tables)[0]
        assert res.table_mode == want["mode"]
        for k, w in (("rulings", "rulings"), ("table_rects", "tables"), ("table_lines", "lines"), ("cells", "cells"), ("item_table", "item_table"), ("item_cell", "item_cell")):
            _same(getattr(res, k), want[w], k)
        assert [c["items"] for t in res.tables for c in t["cells"]] == [np.nonzero(want["item_cell"] == c)[0].tolist() for c in range(len(want["cells"]))]
        assert [res[j]["cell"] for j in range(n)] == want["item_cell"].tolist()
    else:
        assert res.table_rects is None and res.tables == []
    if marks:
        want = _host(E, page, quads, local or marks)[1]
        assert res.mark_mode == want["mode"] == 1
        _same(res.mark_recs, want["marks"], "marks")
        _same(res.item_mark, want["item_mark"], "item_mark")
        assert res.marks == E.mark_dicts(want["marks"], res.texts) and [res[j]["mark"] for j in range(n)] == want["item_mark"].tolist()
    else:
        assert res.mark_recs is None and res.marks == []
    if barcodes:
        want = _host(E, page, quads, local or barcodes)[2]
        assert res.barcode_mode == want["mode"] == 1
        _same(res.barcode_recs, want["records"], "barcodes")
        _same(res.item_barcode, want["item_barcode"], "item_barcode")
        assert res.barcodes == want["barcodes"] and [res[j]["barcode"] for j in range(n)] == want["item_barcode"].tolist()
    else:
        assert res.barcode_recs is None and res.barcodes == []


def _run(eng, page, tables, marks, barcodes, local):
    """one one-page batch with the layers on under their thresholds (0 = off) -> the result and the ink passes it enqueued"""
    eng.set_tables((MIN_LEN, tables) if tables else False)
    eng.set_marks(MARKS + (marks,) if marks else False)
    eng.set_barcodes((BARCODES[0], barcodes, BARCODES[1]) if barcodes else False)
    eng.set_local_ink(local if local else False)
    try:
        n0 = eng.page_ink_passes()
        res = eng.images_to_data([page])[0]
        return res, eng.page_ink_passes() - n0
    finally:
        eng.set_tables(False)
        eng.set_marks(False)
        eng.set_barcodes(False)
        eng.set_local_ink(False)


CASES = [  # tables, marks, barcodes (their `ink`, 0 = off), local ink, passes
    (A_, A_, A_, None, 1),
    (A_, B_, A_, None, 3),        # barcodes compare with the last pass, the marks' one
    (A_, A_, B_, None, 2),
    (0, A_, A_, None, 1),
    (0, A_, B_, None, 2),
    (A_, 0, A_, None, 1),
    (A_, B_, C_, LOCAL, 1),       # the local rule: one pass whatever the thresholds
]


@pytest.mark.parametrize("tables,marks,barcodes,local,passes", CASES)
def test_who_forms_the_bits(eng, page, tables, marks, barcodes, local, passes):
    from tuatara_amd import engine as E
    res, got = _run(eng, page, tables, marks, barcodes, local)
    assert got == passes
    assert len(res) >= 2                                                              # the batch has words: tables run
    _views_equal_host(E, res, page, tables, marks, barcodes, local)
    if marks:
        assert len(res.mark_recs) == 1 and res.marks[0]["selected"]
    if barcodes:
        assert [b["text"] for b in res.barcodes] == ["INK-42"]
    if tables:
        assert len(res.table_rects) == 1 and (res.item_cell >= 0).sum() >= 1
    assert (res.ink is not None) == bool(local)


@pytest.mark.parametrize("drawn", [False, True])
def test_a_batch_without_words(eng, page, drawn):
    """N = 0: tables do not run, marks form the bits and barcodes share them - one pass - and the zero offsets go up once for both; on a blank page, and on the
    drawn one with the detector's boxes dropped (the engine's own knob, as in the marks suite)"""
    from tuatara_amd import engine as E
    img = page if drawn else M.blank(256, 320)
    assert eng.set_tuning("detector_only", 1) == 0
    try:
        res, got = _run(eng, img, A_, A_, A_, None)
    finally:
        assert eng.set_tuning("detector_only", 0) == 0
    assert got == 1 and len(res) == 0
    assert res.mark_mode == 1 and res.barcode_mode == 1 and res.item_mark.shape == (0,) and res.item_barcode.shape == (0,)
    _views_equal_host(E, res, img, A_, A_, A_, None)
    assert (len(res.mark_recs), len(res.barcode_recs)) == ((1, 1) if drawn else (0, 0))
