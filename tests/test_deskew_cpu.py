"""Deskew (DESIGN.md "Deskew") without a GPU: the host rule (ttr_deskew_from_page) against tests/deskew_ref.py bit for bit in every output - the upright page,
the record and all 2 M + 1 scores -, the rule's properties on the shared pages, the refusals that need no device, and what the layer is for: the tables rule on
a tilted form before and after it.  Every test here fails on the parent commit: ttr_deskew_from_page and engine.deskew_from_page are absent."""
import numpy as np
import pytest

from tests import deskew_ref as R
from tests import tables_ref as T

NEW_SYMBOLS = ("ttr_engine_set_deskew", "ttr_engine_deskew", "ttr_result_skew", "ttr_result_to_page", "ttr_skew_to_page", "ttr_results_gather_skew", "ttr_deskew_from_page",
               "ttr_deskew_page", "ttr_dbg_deskew_page")


@pytest.fixture(scope="module")
def E():
    from tuatara_amd import build
    build.build_all()
    from tuatara_amd import engine
    return engine


def both(E, img, max_slope=128, gain=256, ink=128, **kw):
    """the host rule's result, after holding it to the restatement in every output"""
    got, want = E.deskew_from_page(img, max_slope, gain, ink, **kw), R.deskew_ref(img, max_slope, gain, ink)
    assert got["image"].shape == want["image"].shape and np.array_equal(got["image"], want["image"])
    assert [int(s) for s in got["scores"]] == [int(s) for s in want["scores"]]
    assert got["skew"] == want["skew"], (got["skew"], want["skew"])
    return got


def test_symbols_are_exported(E):
    lib = E.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in E.SYMBOLS), name


@pytest.fixture(scope="module")
def pages():
    return {"columns": R.columns_page(), "funsd": R.funsd_page(), "form": R.form_page(), "grid": T.grid_page()}


# (page, the tilts it is tried at, how far `found` may lie from the tilt)
ESTIMATES = [("columns", R.TILTS, 0), ("funsd", R.TILTS, 1), ("form", (27, 45, -45), 0), ("grid", (5, 18), 2)]


@pytest.mark.parametrize("name,tilts,slack", ESTIMATES)
def test_upright_pages_stay_and_tilted_pages_are_found(E, pages, name, tilts, slack):
    """gain 256 (no gate): `found` is what is measured.  The upright page gives 0 and keeps every byte; a page tilted by the rule's own resampler gives its
    tilt, and estimating the upright result again gives 0."""
    img = pages[name]
    r = both(E, img)
    assert r["skew"]["found"] == 0 and r["skew"]["slope"] == 0 and r["skew"]["mode"] == 0 and np.array_equal(r["image"], img)
    for s in tilts:
        r = both(E, R.tilt(img, s))
        assert abs(r["skew"]["found"] - s) <= slack, (name, s, r["skew"])
        assert r["skew"]["slope"] == r["skew"]["found"] and r["skew"]["mode"] == 1
        again = E.deskew_from_page(r["image"], 128, 256, 128)["skew"]
        assert again["found"] == 0 and again["slope"] == 0, (name, s, again)


@pytest.mark.parametrize("seed", R.RANDOM_SEEDS)
def test_random_pages(E, seed):
    """seeded noise with a few long lines, as it is and tilted: every output against the restatement, under the largest range, the defaults and max_slope 1"""
    img = R.random_page(seed)
    for page in (img, R.tilt(img, 5 * seed - 12)):
        for m, g in ((128, 256), (R.MAX_SLOPE, R.GAIN), (1, 256)):
            both(E, page, m, g)


def test_the_gate_holds_a_page_without_baselines(E):
    img = R.no_baseline_page()
    held, free = both(E, img, 64, R.GAIN), both(E, img, 64, 256)
    assert held["skew"]["slope"] == 0 and held["skew"]["mode"] == 0 and np.array_equal(held["image"], img)
    assert held["skew"]["found"] == free["skew"]["found"] != 0 and free["skew"]["slope"] == free["skew"]["found"] and free["skew"]["mode"] == 1
    assert free["skew"]["score_found"] * 256 < free["skew"]["score0"] * R.GAIN          # the gate is what holds it


def test_blank_and_all_ink_pages(E):
    for v in (255, 0):
        img = np.full((37, 91, 3), v, np.uint8)
        r = both(E, img)
        assert r["skew"]["found"] == 0 and r["skew"]["slope"] == 0 and np.array_equal(r["image"], img)
    assert both(E, np.full((37, 91, 3), 255, np.uint8))["skew"]["score0"] == 0
    assert both(E, np.zeros((37, 91, 3), np.uint8))["skew"]["score0"] == 37 * 91 * 91


def dots(h, w, pts):
    img = np.full((h, w, 3), 255, np.uint8)
    for x, y in pts:
        img[y, x] = 0
    return img


def test_ties(E):
    """one pixel: every slope scores 1, the tie goes to 0.  Two pairs, one level under slope 1, one under slope -1: both score 6 against 4, the negative wins."""
    assert both(E, dots(5, 9, [(4, 2)]))["skew"]["found"] == 0
    r = both(E, dots(12, 520, [(0, 0), (512, 1), (0, 10), (512, 9)]))
    assert [int(r["scores"][128 + k]) for k in (-1, 0, 1)] == [6, 4, 6] and r["skew"]["found"] == -1 and r["skew"]["slope"] == -1


def test_constants_against_hand_written_values(E):
    """k = 0: (65536, 0).  k = 1: d = 512.000977, 65536 * 512 / d = 65535.875 -> 65536, 65536 / d = 127.99976 -> 128.  k = 128: cos = 1 / sqrt(1.0625) =
    0.9701425, sin = cos / 4: 63579.26 -> 63579, 15894.81 -> 15895.  Pages of two pixels that only that slope levels."""
    assert (R.consts(0), R.consts(1), R.consts(128), R.consts(-128)) == ((65536, 0), (65536, 128), (63579, 15895), (63579, -15895))
    for k, (C, S) in ((0, (65536, 0)), (1, (65536, 128)), (128, (63579, 15895)), (-128, (63579, -15895))):
        s = both(E, dots(abs(k) + 2, 520, [(0, max(-k, 0)), (512, max(k, 0))]))["skew"]
        assert (s["slope"], s["C"], s["S"]) == (k, C, S), s


def test_max_slope_1_and_128(E):
    img = R.tilt(R.columns_page(), 1)
    assert both(E, img, 1)["skew"]["found"] == 1 and len(both(E, img, 1)["scores"]) == 3
    assert both(E, R.tilt(R.columns_page(), 128), 128)["skew"]["found"] == 128


def test_refusals(E):
    img = np.full((8, 8, 3), 255, np.uint8)
    for bad in ((0, 288, 128), (129, 288, 128), (-1, 288, 128), (64, 255, 128), (64, 65536, 128), (64, 288, 0), (64, 288, 256)):
        with pytest.raises(RuntimeError, match="max_slope must lie in 1..128"):
            E.deskew_from_page(img, *bad)
    for shape in ((1, 8192, 3), (8192, 1, 3)):
        with pytest.raises(RuntimeError, match="8192 px or more"):
            E.deskew_from_page(np.full(shape, 255, np.uint8))
    with pytest.raises(RuntimeError, match="bad image size"):
        E.deskew_from_page(img, row_stride=23)
    with pytest.raises(RuntimeError):
        E.deskew_from_page(np.zeros((8, 8), np.uint8))
    with pytest.raises(E.EngineError):
        E._deskew_arg("yes")
    assert E._deskew_arg(True) == (64, 288, 128) and E._deskew_arg(None)[0] == 0 and E._deskew_arg((5, 300, 90)) == (5, 300, 90)


def test_slope_0_is_the_identity_on_every_byte(E):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (33, 47, 3)).astype(np.uint8)
    assert np.array_equal(R.resample(img, *R.consts(0)), img)
    r = both(E, img, 64, 65535)                    # (no page passes this gate)
    assert r["skew"]["slope"] == 0 and np.array_equal(r["image"], img)


def test_widths_1_to_193_at_height_1_and_3(E):
    rng = np.random.default_rng(11)
    for w in range(1, 194):
        for h in ((1, 3) if w % 16 == 1 else (1,)):
            both(E, np.where(rng.random((h, w, 1)) < 0.3, rng.integers(0, 100, (h, w, 3)), rng.integers(150, 256, (h, w, 3))).astype(np.uint8), 128, 256)


def test_padded_stride_and_both_channel_orders(E):
    img = R.tilt(T.grid_page(), 18)
    h, w = img.shape[:2]
    want = both(E, img)
    wide = np.full((h, w + 5, 3), 7, np.uint8)
    wide[:, :w] = img
    assert R.same(E.deskew_from_page(wide[:, :w], 128, 256, 128, row_stride=(w + 5) * 3), want)
    flipped = both(E, np.ascontiguousarray(img[:, :, ::-1]))
    assert flipped["skew"] == want["skew"] and np.array_equal(flipped["image"][:, :, ::-1], want["image"])


@pytest.mark.parametrize("h,w", [(40, 70), (9, 1030)])
def test_ink_at_the_first_and_last_bin(E, h, w):
    for M in (1, 128):
        r = both(E, R.corner_page(h, w), M)
        assert int(r["scores"][0]) >= 4 and int(r["scores"][-1]) >= 4            # (four pixels, each in some bin, under slopes -M and +M)


def test_map_back_composed_with_the_forward_geometry(E):
    """the resampler reads output pixel (x, y) at (U, V) / 131072; the map back of (x, y) is that point, to 1e-6 px - and the convenience layer's float32 map
    is the double map rounded once"""
    h, w = 480, 1000
    for k in (-128, -45, 3, 27, 128):
        C, S = R.consts(k)
        skew = {"C": C, "S": S, "w": w, "h": h}
        U, V = R.source_coords(C, S, h, w)
        yy, xx = np.mgrid[0:h:37, 0:w:41]
        back = R.to_page(skew, np.stack([xx, yy], axis=-1))
        assert np.abs(back[..., 0] - U[yy, xx] / 131072.0).max() < 1e-6 and np.abs(back[..., 1] - V[yy, xx] / 131072.0).max() < 1e-6
        assert np.array_equal(E.skew_to_page(skew, np.stack([xx, yy], axis=-1)), back.astype(np.float32))
        assert np.abs(R.from_page(skew, back) - np.stack([xx, yy], axis=-1)).max() < 1e-6


@pytest.mark.parametrize("slope", [45, -45])
def test_a_tilted_form_loses_its_cells_and_the_rule_gives_them_back(E, slope):
    """the 480 x 1000 form, one word at every cell's centre (word k belongs in cell k).  Tilted, the tables rule still finds the grid but puts words into wrong
    cells (12 of 30 measured); on the page the rule makes upright - the words taken along by the inverse of the map back - it puts none wrong."""
    img, words = R.form_page(), R.form_words().reshape(-1, 4, 2)
    tilted = R.tilt(img, slope)
    on_tilted = R.tilt_points(words, slope, R.FORM_H, R.FORM_W).reshape(-1, 8).astype(np.float32)
    before = T.tables_ref(tilted, on_tilted, 48, 128)
    wrong = int((before["item_cell"] != np.arange(30)).sum())
    print("wrong cells on the tilted form:", wrong)
    assert before["mode"] == 1 and len(before["cells"]) == 30 and wrong >= 1
    r = both(E, tilted, R.MAX_SLOPE, R.GAIN)
    assert r["skew"]["found"] == slope and r["skew"]["slope"] == slope
    upright = R.from_page(r["skew"], on_tilted.reshape(-1, 4, 2)).reshape(-1, 8).astype(np.float32)
    after = T.tables_ref(r["image"], upright, 48, 128)
    assert after["mode"] == 1 and len(after["cells"]) == 30 and after["item_cell"].tolist() == list(range(30))
