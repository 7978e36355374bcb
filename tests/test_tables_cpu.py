"""Tables (DESIGN.md "Tables") without a GPU: the host rule (ttr_tables_from_page) against tests/tables_ref.py bit for bit in every output, on small hand-made
pages (about 200 x 160, min_len = 16), the rule's properties on them against hand-written values, the refusals that need no device, and the FUNSD page.  Every
test here fails on the parent commit: ttr_tables_from_page and engine.tables_from_page are absent."""
import os

import numpy as np
import pytest

from tests import tables_ref as T
from tests.conftest import ROOT

NEW_SYMBOLS = ("ttr_engine_set_tables", "ttr_engine_tables", "ttr_result_table_mode", "ttr_result_ruling_count", "ttr_result_rulings", "ttr_result_table_count",
               "ttr_result_tables", "ttr_result_table_lines", "ttr_result_cell_count", "ttr_result_cells", "ttr_result_item_table", "ttr_result_item_cell",
               "ttr_result_cell_text", "ttr_results_gather_tables", "ttr_tables_from_page", "ttr_tables_page", "ttr_dbg_tables")


@pytest.fixture(scope="module")
def E():
    from tuatara_amd import build
    build.build_all()
    from tuatara_amd import engine
    return engine


def both(E, img, quads=None, min_len=16, ink=128, **kw):
    """the host rule's result, after holding it to the reference in every output"""
    got, want = E.tables_from_page(img, quads, min_len, ink, **kw), T.tables_ref(img, quads, min_len, ink)
    for k in ("rulings", "tables", "lines", "cells", "item_table", "item_cell"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert got["mode"] == want["mode"]
    return got


def test_symbols_are_exported(E):
    lib = E.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in E.SYMBOLS), name


def test_grid_3x4(E):
    """2-px lines at y = 20, 60, 100, 140 and x = 10, 50, 100, 150, 190: doubled centres 2 y + 1, cells between the truncated halves"""
    r = both(E, T.grid_page(), T.grid_words())
    assert r["mode"] == 1 and len(r["rulings"]) == 9 and (r["rulings"][:, 5] == 0).all()
    assert r["tables"].tolist() == [[10, 20, 191, 141, 3, 4, 0, 12]]
    (Y, X), = E.table_line_lists(r["tables"], r["lines"])
    assert Y.tolist() == [41, 121, 201, 281] and X.tolist() == [21, 101, 201, 301, 381]
    ys, xs = [20, 60, 100, 140], [10, 50, 100, 150, 190]
    want = [[0, i, j, 1, 1, xs[j], ys[i], xs[j + 1], ys[i + 1]] for i in range(3) for j in range(4)]
    assert r["cells"].tolist() == want
    assert r["item_table"].tolist() == [0] * 12 and r["item_cell"].tolist() == list(range(12))


def test_merged_cells(E):
    r = both(E, T.grid_page(colspan=True, rowspan=True), T.grid_words())
    assert len(r["cells"]) == 10
    assert r["cells"][1].tolist() == [0, 0, 1, 1, 2, 50, 20, 150, 60]          # colspan = 2
    assert r["cells"][3].tolist() == [0, 1, 0, 2, 1, 10, 60, 50, 140]          # rowspan = 2
    assert r["item_cell"].tolist() == [0, 1, 1, 2, 3, 4, 5, 6, 3, 7, 8, 9]
    only = both(E, T.grid_page(colspan=True), T.grid_words())
    assert len(only["cells"]) == 11 and only["cells"][1, 4] == 2


def test_an_l_shaped_merge_becomes_its_box(E):
    """removing the borders (0,0)-(0,1) and (0,0)-(1,0) leaves an L of three base cells: the cell takes in (1,1), so cells still tile the grid"""
    img = T.grid_page()
    img[22:60, 50:52] = 255
    img[60:62, 12:50] = 255
    r = both(E, img, T.grid_words())
    assert r["cells"][0].tolist() == [0, 0, 0, 2, 2, 10, 20, 100, 100] and len(r["cells"]) == 9


def test_two_tables_and_a_loose_underline(E):
    r = both(E, T.two_tables_page())
    assert r["tables"][:, :6].tolist() == [[10, 10, 91, 71, 2, 2], [110, 90, 191, 151, 2, 2]]
    loose = r["rulings"][r["rulings"][:, 5] == -1]
    assert loose.tolist() == [[0, 10, 84, 80, 84, -1]]
    assert len(r["cells"]) == 8 and r["tables"][1, 6] == 4


@pytest.mark.parametrize("deg", [1, 2, -1, -2])
def test_rotated_grid_keeps_its_structure(E, deg):
    img, quads = T.rotated_grid(deg)
    r = both(E, img, quads)
    assert len(r["tables"]) == 1 and r["tables"][0, 4:6].tolist() == [3, 4] and len(r["cells"]) == 12
    assert r["item_cell"].tolist() == list(range(12))


def test_a_black_bar_is_no_ruling(E):
    img = T.blank()
    img[40:70, 30:130] = 0
    r = both(E, img)
    assert r["mode"] == 1 and len(r["rulings"]) == 0
    T.hline(img, 100, 30, 129, t=12)           # 8 T <= L holds at 12 x 100, and so does A <= 16 L
    assert len(both(E, img)["rulings"]) == 1
    T.hline(img, 100, 30, 129, t=13)
    assert len(both(E, img)["rulings"]) == 0


def test_rulings_at_the_page_edge(E):
    img = T.blank(64, 128)
    T.hline(img, 0, 0, 127)
    T.hline(img, 62, 0, 127)
    T.vline(img, 0, 0, 63)
    T.vline(img, 126, 0, 63)
    r = both(E, img, np.array([[60, 30, 70, 30, 70, 36, 60, 36]], np.float32))
    assert r["tables"].tolist() == [[0, 0, 127, 63, 1, 1, 0, 1]] and r["item_cell"].tolist() == [0]


@pytest.mark.parametrize("w", [1, 63, 64, 65, 129, 193])
def test_widths_about_the_word_size(E, w):
    """a run up to the row's last pixel, a run across every word boundary, vertical lines in the last column"""
    img = T.blank(40, w)
    T.hline(img, 5, 0, w - 1)
    T.hline(img, 30, max(w - 20, 0), w - 1)
    T.vline(img, w - 1, 0, 39, t=1)
    T.vline(img, 0, 0, 39, t=1)
    r = both(E, img)
    if w >= 16:
        assert [0, 0, 5, w - 1, 6, 0] in r["rulings"].tolist()


def test_padded_row_stride(E):
    img = T.grid_page()
    buf = np.full((160, 200 * 3 + 37), 7, np.uint8)
    buf[:, :600] = img.reshape(160, 600)
    view = buf[:, :600].reshape(160, 200, 3)
    got = E.tables_from_page(view, T.grid_words(), 16, 128, row_stride=buf.strides[0])
    assert T.same(got, both(E, img, T.grid_words()))


def test_channel_order_does_not_matter(E):
    rng = np.random.default_rng(3)
    img = T.two_tables_page()
    img = np.where(img == 0, rng.integers(0, 120, img.shape, dtype=np.uint8), rng.integers(140, 256, img.shape, dtype=np.uint8)).astype(np.uint8)
    assert T.same(both(E, img), both(E, np.ascontiguousarray(img[:, :, ::-1])))


def test_the_ink_threshold_is_exact(E):
    """s = 3 ink - 1 is ink, s = 3 ink is not"""
    ink = 100
    img = T.blank(40, 100)
    img[10, 10:60] = (99, 100, 100)    # s = 299
    img[20, 10:60] = (100, 100, 100)   # s = 300
    r = both(E, img, ink=ink)
    assert r["rulings"][:, :5].tolist() == [[0, 10, 10, 59, 10]]


@pytest.mark.parametrize("seed", range(12))
def test_random_pages_agree(E, seed):
    img = T.random_page(seed, h=80 + 7 * seed, w=120 + 11 * seed, p=0.5 + 0.04 * seed)
    both(E, img, T.random_quads(seed, 40, img.shape[0], img.shape[1]), min_len=16 + seed)


def test_random_pages_hold_tables(E):
    """the seeded pages of test_random_pages_agree are not empty of tables: the host rule finds some"""
    assert sum(len(E.tables_from_page(T.random_page(s, h=80 + 7 * s, w=120 + 11 * s, p=0.5 + 0.04 * s), None, 16 + s)["tables"]) for s in range(12)) >= 3


def test_run_cap_overflow(E):
    r = both(E, T.dashes_page())
    assert r["mode"] == -2 and len(r["rulings"]) == len(r["tables"]) == len(r["cells"]) == 0
    q = both(E, T.dashes_page(), T.random_quads(0, 5, 400, 400))
    assert (q["item_table"] == -1).all() and (q["item_cell"] == -1).all()


def test_ruling_cap_overflow(E):
    img = T.blank(600, 40)
    for y in range(0, 600, 2):
        img[y, 4:36] = 0
    assert both(E, img)["mode"] == -4


def test_two_caps_at_once_report_the_earlier_step(E):
    """more than 256 horizontal rulings AND more than 8192 vertical runs: the runs of both directions are counted first, so -2"""
    img = T.two_caps_page()
    m = T.ink_mask(img, 128)
    assert len(T.runs_of(m)) <= T.RUN_CAP < len(T.runs_of(m.T)) and T.rulings_of(T.runs_of(m), 16, 0) is None
    r = both(E, img, T.random_quads(1, 5, 600, 700))
    assert r["mode"] == -2 and r["runs"] == (0, 0) and (r["item_cell"] == -1).all()


@pytest.mark.parametrize("page,mode", [("many_lines_page", -6), ("many_tables_page", -6), ("many_cells_page", -7)])
def test_line_table_and_cell_caps_overflow(E, page, mode):
    """steps 6 and 7 give up half way through the block: it then holds the mode alone"""
    img = getattr(T, page)()
    r = both(E, img, T.random_quads(2, 8, img.shape[0], img.shape[1]))
    assert r["mode"] == mode and len(r["rulings"]) == len(r["tables"]) == len(r["cells"]) == len(r["lines"]) == 0 and (r["item_table"] == -1).all()


def test_just_inside_the_line_table_and_cell_caps(E):
    lines = T.many_lines_page()
    lines[4 + 8 * 64:4 + 8 * 65 + 1] = 255                                 # 64 row lines are allowed
    r = both(E, lines)
    assert r["mode"] == 1 and r["tables"][0, 4:6].tolist() == [63, 1]
    tabs = T.many_tables_page()
    tabs[:, 165:] = 255                                                    # 6 x 4 = 24 tables ... and 32 x 32 = 1024 cells
    assert len(both(E, tabs)["tables"]) == 24
    cells = T.many_cells_page()
    cells[5 + 8 * 32 + 1:, :] = 255
    cells[:, 5 + 8 * 32 + 1:] = 255
    r = both(E, cells)
    assert r["mode"] == 1 and len(r["cells"]) == 1024


def test_words_on_a_grid_line_go_to_the_cell_that_starts_there(E):
    """centres exactly at X = 101 / 2 and Y = 121 / 2 (doubled lines 101 and 121): cx = 64 * 50.5 = 32 * 101"""
    def word(cx, cy):
        return [cx - 4, cy - 2, cx + 4, cy - 2, cx + 4, cy + 2, cx - 4, cy + 2]
    quads = np.array([word(50.5, 40), word(50.4375, 40), word(30, 60.5), word(30, 60.4375), word(10.5, 40), word(10.4375, 40), word(190.5, 40)], np.float32)
    r = both(E, T.grid_page(), quads)
    assert r["item_cell"].tolist() == [1, 0, 4, 0, 0, -1, -1]


def test_refusals(E):
    img, q = T.grid_page(), T.grid_words()
    for min_len, ink in ((15, 128), (4097, 128), (16, 0), (16, 256)):
        with pytest.raises(Exception, match="min_len must lie in 16..4096 and ink in 1..255"):
            E.tables_from_page(img, q, min_len, ink)
    E.tables_from_page(img, q, 4096, 255)
    E.tables_from_page(img, q, 16, 1)
    bad = q.copy()
    bad[3, 2] = 32768.0
    with pytest.raises(Exception, match="quad 3 has a coordinate"):
        E.tables_from_page(img, bad, 16, 128)
    bad[3, 2] = np.nan
    with pytest.raises(Exception, match="quad 3 has a coordinate"):
        E.tables_from_page(img, bad, 16, 128)


def test_funsd_page(E):
    """the one real document in the tree: three tables, the first a grid of 3 rows x 5 columns; the lines to +-1 doubled pixel of the issue's prototype"""
    from PIL import Image
    img = np.array(Image.open(os.path.join(ROOT, "tests", "data", "funsd_0001129658.png")).convert("RGB"))
    r = both(E, img, None, min_len=48, ink=128)
    assert r["mode"] == 1 and len(r["tables"]) == 3 and r["tables"][0, 4:6].tolist() == [3, 5]
    assert (r["rulings"][:, 0] == 0).sum() == 20 and (r["rulings"][:, 0] == 1).sum() == 12
    m = T.ink_mask(img, 128)
    assert r["runs"] == (175, 105) == (len(T.runs_of(m)), len(T.runs_of(m.T)))
    Y, X = E.table_line_lists(r["tables"], r["lines"])[0]
    assert np.abs(Y - np.array([800, 848, 908, 966])).max() <= 1 and np.abs(X - np.array([140, 205, 461, 786, 1017, 1272])).max() <= 1
