"""Selection marks (DESIGN.md "Selection marks") without a GPU: the host rule (ttr_marks_from_page) against tests/marks_ref.py bit for bit in every output, on
small hand-made pages, the rule's properties on them against hand-written values, the refusals that need no device, and the FUNSD page.  Every test here
fails on the parent commit: ttr_marks_from_page and engine.marks_from_page are absent."""
import os

import numpy as np
import pytest

from tests import marks_ref as M
from tests.conftest import ROOT

NEW_SYMBOLS = ("ttr_engine_set_marks", "ttr_engine_marks", "ttr_result_mark_mode", "ttr_result_mark_count", "ttr_result_marks", "ttr_result_item_mark",
               "ttr_results_gather_marks", "ttr_marks_from_page", "ttr_marks_from_page_ink", "ttr_marks_page", "ttr_dbg_marks")


@pytest.fixture(scope="module")
def E():
    from tuatara_amd import build
    build.build_all()
    from tuatara_amd import engine
    return engine


def both(E, img, quads=None, min_side=10, max_side=64, fill=24, ink=128, **kw):
    """the host rule's result, after holding it to the reference in every output"""
    got, want = E.marks_from_page(img, quads, min_side, max_side, fill, ink, **kw), M.marks_ref(img, quads, min_side, max_side, fill, ink)
    for k in ("marks", "item_mark"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, got[k], want[k])
    for k in ("mode", "corners", "kept"):
        assert got[k] == want[k], (k, got[k], want[k])
    return got


def boxes(r):
    return r["marks"][:, :4].tolist()


def test_symbols_are_exported(E):
    lib = E.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in E.SYMBOLS), name


def test_hand_page(E):
    """four frames with t = 1, 2, 3, 1; the crossed one reads 16 of 144 and is selected; the solid square is no mark; 18 corners"""
    r = both(E, M.hand_page())
    assert r["mode"] == 1 and r["corners"] == 18
    assert r["marks"].tolist() == M.HAND_MARKS
    t = (r["marks"][:, 4] - r["marks"][:, 0] - 1).tolist()
    assert t == [1, 2, 3, 1]


@pytest.mark.parametrize("side,found", [(10, True), (9, False), (64, True), (65, False)])
def test_side_bounds(E, side, found):
    r = both(E, M.frame(M.blank(100, 100), 5, 5, side, 1))
    assert (len(r["marks"]) == 1) == found


@pytest.mark.parametrize("a,b,found", [(20, 25, True), (20, 26, False), (25, 20, True), (26, 20, False), (16, 20, True), (16, 21, False)])
def test_aspect_bound(E, a, b, found):
    """4 |a - b| <= min(a, b) on both sides of equality"""
    r = both(E, M.frame(M.blank(60, 60), 5, 5, a, 1, side_y=b))
    assert (len(r["marks"]) == 1) == found


@pytest.mark.parametrize("t,found", [(4, True), (5, False)])
def test_thickness_bound(E, t, found):
    """side 20: q = 5; a frame of thickness q - 1 is a mark, one of thickness q is a bar"""
    r = both(E, M.frame(M.blank(60, 60), 5, 5, 20, t))
    assert (len(r["marks"]) == 1) == found
    if found:
        assert r["marks"][0, 4:8].tolist() == [10, 10, 19, 19]


@pytest.mark.parametrize("inked,state", [(13, 0), (14, 1)])
def test_fill_bound(E, inked, state):
    """a 16-px frame: area 144; 256 inked >= 24 x 144 = 3456 from 14 px on (3584 against 3328)"""
    img = M.frame(M.blank(40, 40), 5, 5, 16, 1)
    img[12, 7:19] = 0                                          # 12 px, and 1 or 2 more
    img[10, 8:8 + inked - 12] = 0
    r = both(E, img)
    assert r["marks"][0, 8:11].tolist() == [inked, 144, state]


def test_word_boundaries(E):
    """a run across one word boundary (x = 58..74) and one through three words at side 128"""
    pages = M.shared_pages()
    assert boxes(both(E, pages["straddle"][0])) == [[58, 10, 74, 26]]
    r = both(E, pages["wide"][0], max_side=128)
    assert boxes(r) == [[30, 10, 157, 137]] and r["marks"][0, 4:8].tolist() == [33, 13, 154, 134]
    assert boxes(both(E, pages["wide"][0], max_side=127)) == []


def test_page_edges(E):
    assert boxes(both(E, M.shared_pages()["edges"][0])) == [[0, 0, 11, 11], [88, 52, 99, 63]]


@pytest.mark.parametrize("w", list(range(1, 131)))
def test_every_width(E, w):
    """widths 1..130 at height 20: a frame flush with the right edge wherever one fits, noise elsewhere"""
    img = M.blank(20, w)
    if w >= 12:
        M.frame(img, w - 12, 4, 12, 1)
    img[np.random.RandomState(w).rand(20, w) < 0.03] = 0
    both(E, img)


def test_padded_stride_and_channel_orders(E):
    img = M.hand_page()
    want = both(E, img)
    wide = np.full((300, 200 * 3 + 40), 7, np.uint8)
    wide[:, :600] = img.reshape(300, 600)
    buf = np.ascontiguousarray(wide)
    view = np.lib.stride_tricks.as_strided(buf, (300, 200, 3), (640, 3, 1))
    got = E.marks_from_page(view, row_stride=640)
    assert np.array_equal(got["marks"], want["marks"]) and got["corners"] == want["corners"]
    tinted = img.copy()
    tinted[..., 0] = np.where(img[..., 0] == 0, 90, 255)      # ink that is dark in two channels only: s = 90 < 384
    a, b = both(E, tinted), both(E, np.ascontiguousarray(tinted[..., ::-1]))
    assert np.array_equal(a["marks"], b["marks"]) and np.array_equal(a["marks"], want["marks"])


def test_box_inside_a_grid(E):
    img, box = M.grid_with_box()
    r = both(E, img)
    assert boxes(r) == [box]


def test_items_and_labels(E):
    """the `x` inside the ticked box is that box's item; every box's label is the word beside it - the nearer of two on the first line"""
    img, quads = M.form_page()
    r = both(E, img, quads)
    assert r["marks"][:, 10].tolist() == [0, 1, 0]
    assert r["item_mark"].tolist() == [-1, -1, -1, 1, -1]
    assert r["marks"][:, 11].tolist() == [0, 1, 2]


def test_label_beyond_eight_sides_is_not_taken(E):
    img = M.frame(M.blank(60, 400), 10, 10, 16, 1)
    # the frame's right edge is x = 26: 64 (cx - 26) <= 64 * 8 * 16 holds up to cx = 154
    near, far = M.quad_box(144, 12, 164, 24), M.quad_box(145, 12, 165, 24)            # centres 154 and 155
    assert both(E, img, np.asarray([near], np.float32))["marks"][0, 11] == 0
    assert both(E, img, np.asarray([far], np.float32))["marks"][0, 11] == -1
    above = M.quad_box(40, 0, 60, 8)                                                   # cy = 4: not level with the box
    assert both(E, img, np.asarray([above], np.float32))["marks"][0, 11] == -1


def test_cap(E):
    pages = M.shared_pages()
    r = both(E, pages["boxes512"][0], min_side=8)
    assert r["mode"] == 1 and len(r["marks"]) == 512
    q = np.asarray([M.quad_box(3, 3, 8, 8)], np.float32)                               # inside the first box
    r = both(E, pages["boxes513"][0], q, min_side=8)
    assert r["mode"] == -6 and len(r["marks"]) == 0 and r["kept"] == 513 and r["item_mark"].tolist() == [-1]
    assert both(E, pages["boxes512"][0], q, min_side=8)["item_mark"].tolist() == [0]


@pytest.mark.parametrize("seed", range(8))
def test_random_pages(E, seed):
    img, quads = M.random_page(seed)
    both(E, img, quads, min_side=8)
    both(E, img, quads, min_side=12, max_side=30, fill=60, ink=100)


def test_many_bands_page(E):
    img, quads = M.many_bands_page()
    r = both(E, img, quads)
    assert len(r["marks"]) > 100 and [1280, 1080, 1299, 1099] in boxes(r)


def test_local_ink_rule(E):
    """under local ink's bitmap the rule is the same: the host rule against the restatement on local ink's mask, and a shaded copy of the form gives the clean
    form's marks in box, state, label and item"""
    from tests import ink_ref as I
    img, quads = M.form_page()
    shaded = I.shade(img)
    for li in ((16, 38, 2), (8, 60, 0)):
        got, want = E.marks_from_page_ink(shaded, quads, local_ink=li), M.marks_of_mask(I.ink_mask(shaded, *li)[0], quads)
        assert np.array_equal(got["marks"], want["marks"]) and np.array_equal(got["item_mark"], want["item_mark"])
        assert (got["mode"], got["corners"], got["kept"]) == (want["mode"], want["corners"], want["kept"])
    clean, got = both(E, img, quads), E.marks_from_page_ink(shaded, quads)
    assert np.array_equal(got["marks"][:, :4], clean["marks"][:, :4]) and np.array_equal(got["marks"][:, 10:], clean["marks"][:, 10:])
    assert np.array_equal(got["item_mark"], clean["item_mark"])


def test_refusals(E):
    img = M.blank(40, 40)
    for bad in [(7, 64, 24, 128), (65, 128, 24, 128), (10, 9, 24, 128), (10, 129, 24, 128), (10, 64, 0, 128), (10, 64, 256, 128), (10, 64, 24, 0), (10, 64, 24, 256)]:
        with pytest.raises(Exception, match="min_side must lie in 8..64"):
            E.marks_from_page(img, None, *bad)
    for v in (np.nan, np.inf, 32768.0, -32768.0):
        q = np.asarray([M.quad_box(1, 1, 5, 5)], np.float32)
        q[0, 3] = v
        with pytest.raises(Exception, match="not finite or has"):
            E.marks_from_page(img, q)
    lib = E.load()
    buf = np.zeros(8, np.uint8)
    assert lib.ttr_marks_from_page(E._u8(buf), 32768, 1, 0, 10, 64, 24, 128, None, 0, None, None, None, None) == -1
    assert b"32768" in lib.ttr_last_error()
    assert lib.ttr_marks_from_page(E._u8(buf), 1, 32768, 0, 10, 64, 24, 128, None, 0, None, None, None, None) == -1
    assert lib.ttr_marks_from_page(None, 4, 4, 0, 10, 64, 24, 128, None, 0, None, None, None, None) == -1
    assert lib.ttr_marks_from_page(E._u8(buf), 2, 2, 5, 10, 64, 24, 128, None, 0, None, None, None, None) == -1       # a stride below 3 w
    with pytest.raises(Exception, match="radius"):
        E.marks_from_page_ink(img, None, local_ink=(0, 38, 2))


def test_funsd_page(E):
    """the one real document in the tree: its bullets, letters and table corners all fail the rule"""
    from PIL import Image
    img = np.array(Image.open(os.path.join(ROOT, "tests", "data", "funsd_0001129658.png")).convert("RGB"))
    assert img.shape[:2] == (1000, 754)
    r = both(E, img)
    assert r["mode"] == 1 and len(r["marks"]) == 0 and r["corners"] == 3323
