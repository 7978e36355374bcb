"""Local ink (DESIGN.md "Local ink") without a GPU: the host rule (ttr_ink_from_page) against tests/ink_ref.py bit for bit - bits, bitsT and the record -, the
rule's stated consequences, every refusal that needs no device, and what the layer is for: the tables and deskew rules on shaded pages before and after it.
Every test here but the last group fails on the parent commit, where the symbols are absent."""
import numpy as np
import pytest

from tests import deskew_ref as D
from tests import ink_ref as R
from tests import tables_ref as T

NEW_SYMBOLS = ("ttr_engine_set_ink", "ttr_engine_ink", "ttr_result_ink", "ttr_results_gather_ink", "ttr_ink_from_page", "ttr_ink_page", "ttr_dbg_ink_page",
               "ttr_tables_from_page_ink", "ttr_deskew_from_page_ink")
TABLE_KEYS = ("rulings", "tables", "lines", "cells", "item_table", "item_cell")


@pytest.fixture(scope="module")
def E():
    from tuatara_amd import build
    build.build_all()
    from tuatara_amd import engine
    return engine


def both(E, img, radius, drop, polarity, **kw):
    """the host rule's result, after holding it to the restatement in every output"""
    got, want = E.ink_from_page(img, radius, drop, polarity, **kw), R.ink_ref(img, radius, drop, polarity)
    assert R.same(got, want), (np.asarray(img).shape, radius, drop, polarity, got["ink"], want["ink"])
    return got


def test_symbols_are_exported(E):
    lib = E.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in E.SYMBOLS), name
    assert (E.LOCAL_INK_RADIUS, E.LOCAL_INK_DROP, E.LOCAL_INK_POLARITY) == (16, 38, 2)


@pytest.mark.parametrize("radius", [1, 64])
def test_every_width_at_the_heights_around_the_window(E, radius):
    """widths 1..193 at heights 1, 2, 2 R and 2 R + 1: pages narrower and lower than the window, and the first sizes at which a window is whole"""
    for hi, h in enumerate((1, 2, 2 * radius, 2 * radius + 1)):
        page = R.random_page(radius + hi, h, 193)
        for w in range(1, 194):
            both(E, page[:, :w], radius, (1, 255, 38)[w % 3], w % 3)


@pytest.mark.parametrize("radius,drop", [(1, 1), (1, 255), (64, 1), (64, 255), (16, 38), (7, 100)])
def test_seeded_random_pages(E, radius, drop):
    for seed, (h, w) in enumerate(((37, 53), (70, 129), (150, 200))):
        for pol in (0, 1, 2):
            both(E, R.random_page(seed, h, w), radius, drop, pol)


def test_pages_smaller_than_the_window_in_both_axes(E):
    for h, w in ((1, 1), (3, 5), (9, 9), (31, 17)):
        both(E, R.random_page(h, h, w), 16, 38, 0)
        both(E, R.random_page(w, h, w), 64, 200, 2)


def test_a_padded_stride(E):
    wide = R.random_page(5, 40, 100)
    view = wide[:, :77]                              # rows 300 bytes apart, 231 used
    got = E.ink_from_page(view, 16, 38, 0, row_stride=300)
    assert R.same(got, R.ink_ref(np.ascontiguousarray(view), 16, 38, 0))


@pytest.mark.parametrize("value", [0, 255, 97])
def test_uniform_pages_carry_no_ink(E, value):
    """a blank page, an all-black page and a grey one: s n 256 < s n (256 - drop) never holds"""
    img = np.full((50, 90, 3), value, np.uint8)
    for pol in (0, 1, 2):
        r = both(E, img, 16, 38, pol)
        assert not r["bits"].any() and not r["bitsT"].any()


def test_a_solid_region_thicker_than_the_window_loses_its_interior(E):
    img = np.full((120, 120, 3), 255, np.uint8)
    img[20:100, 20:100] = 0
    r = both(E, img, 8, 38, 0)
    m = R.ink_mask(img, 8, 38, 0)[0]
    assert m[20, 20] and m[20:100, 20].all() and not m[40:80, 40:80].any()
    assert np.array_equal(r["bits"], R.pack_bits(m))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_inverse_page_under_light_ink_is_the_page_under_dark_ink(E, seed):
    img = R.random_page(seed, 61, 131)
    a, b = both(E, img, 16, 38, R.DARK), both(E, 255 - img, 16, 38, R.LIGHT)
    assert np.array_equal(a["bits"], b["bits"]) and np.array_equal(a["bitsT"], b["bitsT"])
    assert (a["ink"]["inverted"], b["ink"]["inverted"]) == (0, 1)


def test_auto_polarity_on_a_page_its_inverse_and_an_exact_tie(E):
    page = T.grid_page()
    a, b = both(E, page, 16, 38, R.AUTO), both(E, 255 - page, 16, 38, R.AUTO)
    assert (a["ink"]["inverted"], b["ink"]["inverted"]) == (0, 1)
    assert np.array_equal(a["bits"], b["bits"]) and a["bits"].any()
    tie = R.tie_page()
    r = both(E, tie, 1, 38, R.AUTO)
    assert 2 * r["ink"]["sum"] == 765 * 2 * 2 and r["ink"]["inverted"] == 0       # a tie stays dark
    tie[0, 0, 0] = 254                                                            # one step darker: light ink
    assert both(E, tie, 1, 38, R.AUTO)["ink"]["inverted"] == 1


def test_refusals(E):
    img = np.full((8, 8, 3), 255, np.uint8)
    for bad in ((0, 38, 0), (65, 38, 0), (-1, 38, 0), (16, 0, 0), (16, 256, 0), (16, 38, 3), (16, 38, -1)):
        with pytest.raises(RuntimeError, match="radius must lie in 1..64"):
            E.ink_from_page(img, *bad)
        with pytest.raises(RuntimeError, match="radius must lie in 1..64"):
            E.tables_from_page_ink(img, None, 48, bad)
        with pytest.raises(RuntimeError, match="radius must lie in 1..64"):
            E.deskew_from_page_ink(img, 64, 288, bad)
    with pytest.raises(RuntimeError, match="bad image size"):
        E.ink_from_page(img, 16, 38, 0, row_stride=23)
    with pytest.raises(RuntimeError, match="min_len must lie"):
        E.tables_from_page_ink(img, None, 15, True)
    with pytest.raises(RuntimeError, match="max_slope must lie"):
        E.deskew_from_page_ink(img, 129, 288, True)
    with pytest.raises(E.EngineError, match="local_ink must be"):
        E._local_ink_arg("yes")
    lib = E.load()
    assert lib.ttr_ink_from_page(None, 8, 8, 0, 16, 38, 0, None, None, None) == -1
    assert lib.ttr_result_ink(None, None) == 0 and lib.ttr_engine_ink(None, None, None) == 0 and lib.ttr_results_gather_ink(None, 0, None) == -1


# ---- what the layer is for
def same_tables(a, b):
    return all(np.array_equal(a[k], b[k]) for k in TABLE_KEYS) and a["mode"] == b["mode"]


def test_the_shaded_grid_page_loses_its_table_under_the_fixed_rule_and_keeps_it_under_the_local_one(E):
    page, words = T.grid_page(), T.grid_words()
    clean = E.tables_from_page(page, words, 16, 128)
    assert len(clean["tables"]) == 1 and len(clean["cells"]) == 12 and (clean["item_cell"] >= 0).all()
    shaded = R.shade(page, 0.35)
    fixed = E.tables_from_page(shaded, words, 16, 128)
    assert len(fixed["tables"]) == 0 and len(fixed["cells"]) == 0
    local = E.tables_from_page_ink(shaded, words, 16, (16, 38, 0))
    assert same_tables(local, clean)
    assert same_tables(E.tables_from_page_ink(page, words, 16, (16, 38, 0)), clean)       # the unshaded page is unchanged by the local rule
    assert same_tables(local, R.tables_ref_ink(shaded, words, 16, (16, 38, 0)))
    for radius in (4, 9, 32):
        assert same_tables(E.tables_from_page_ink(shaded, words, 16, (radius, 38, 0)), clean), radius


def test_the_inverted_grid_page_gives_its_table_under_light_ink(E):
    page, words = 255 - T.grid_page(), T.grid_words()
    assert len(E.tables_from_page(page, words, 16, 128)["tables"]) == 0
    clean = E.tables_from_page(T.grid_page(), words, 16, 128)
    assert same_tables(E.tables_from_page_ink(page, words, 16, (16, 38, 1)), clean)
    assert same_tables(E.tables_from_page_ink(page, words, 16, (16, 38, 2)), clean)


@pytest.mark.parametrize("name,tilt,want", [("columns", 27, 27), ("columns", -45, -45), ("columns", 5, 5), ("funsd", 5, 6)])
def test_shaded_tilted_pages_stand_still_under_the_fixed_rule_and_turn_under_the_local_one(E, name, tilt, want):
    page = D.tilt(D.columns_page() if name == "columns" else D.funsd_page(), tilt)
    assert E.deskew_from_page(page, 64, 288, 128)["skew"]["slope"] == want        # the clean page
    shaded = R.shade(page, 0.35)
    fixed = E.deskew_from_page(shaded, 64, 288, 128)["skew"]
    assert fixed["slope"] == 0 and fixed["found"] == want                         # found, but the gain gate holds the page still
    local = E.deskew_from_page_ink(shaded, 64, 288, (16, 38, 0))
    assert local["skew"]["slope"] == want
    assert D.same(local, R.deskew_ref_ink(shaded, 64, 288, (16, 38, 0)))


@pytest.mark.parametrize("local_ink", [(16, 38, 0), (3, 120, 2), (64, 10, 1)])
def test_the_ink_forms_of_the_host_rules_against_the_restatements_fed_the_local_mask(E, local_ink):
    for img, quads in ((T.grid_page(), T.grid_words()), (R.shade(T.two_tables_page(), 0.5), None), (R.random_page(3, 96, 150), T.random_quads(3, 12, 96, 150))):
        assert same_tables(E.tables_from_page_ink(img, quads, 16, local_ink), R.tables_ref_ink(img, quads, 16, local_ink))
    for img in (R.shade(D.tilt(D.form_page(), 18), 0.5), R.random_page(4, 80, 131)):
        assert D.same(E.deskew_from_page_ink(img, 64, 288, local_ink), R.deskew_ref_ink(img, 64, 288, local_ink))


# ---- the existing entry points keep their bits (these pass on the parent commit too)
def test_the_fixed_rule_entry_points_are_unchanged(E):
    for img, quads in ((T.grid_page(), T.grid_words()), (T.grid_page(colspan=True, rowspan=True), T.grid_words()), (T.two_tables_page(), None), (T.dashes_page(), None),
                       (T.random_page(2), T.random_quads(2, 10, 96, 150))):
        assert same_tables(E.tables_from_page(img, quads, 16, 128), T.tables_ref(img, quads, 16, 128))
    for img in (D.form_page(), D.tilt(D.form_page(), 18), D.corner_page(), D.random_page(3)):
        assert D.same(E.deskew_from_page(img, 64, 288, 128), D.deskew_ref(img, 64, 288, 128))
