"""Curved words (DESIGN.md "Curved words") without a GPU: the host rule (ttr_curve_frame, ttr_curve_columns, ttr_curve_knots, ttr_curve_crop,
ttr_curve_outline) against tests/curve_ref.py bit for bit, the rule's properties, its function on hand-made words of bars set on circular arcs, the arched
synthetic page under the CPU oracle's detector, the refusals that need no device, the exported symbols and the callers' switches as far as they go without a
device.  Every test here fails on the parent commit: the symbols are absent."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import curve_ref as CV
from tests import rectify_ref as RR
from tests import regions_ref as GR
from tests.conftest import ROOT

NEW_SYMBOLS = ("ttr_engine_set_curved", "ttr_engine_curved", "ttr_result_curved", "ttr_result_outlines", "ttr_result_spine_knots", "ttr_results_gather_curved",
               "ttr_curve_frame", "ttr_curve_columns", "ttr_curve_knots", "ttr_curve_crop", "ttr_curve_outline", "ttr_curve_crops")


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


def test_symbols_are_exported(built):
    """Fails on the parent commit: none of these symbols exists there."""
    from tuatara_amd import engine
    lib = engine.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in engine.SYMBOLS), name


# ---------------------------------------------------------------- 1. the rule, bit for bit
def _images():
    rng = np.random.default_rng(5)
    H, W = 200, 256
    out = {"random": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "flat": np.full((H, W, 3), 200, np.uint8)}
    row = np.full((H, W, 3), 255, np.uint8)
    row[97] = 0
    out["one dark row"] = row
    out["saturated noise"] = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    out["arc"] = CV.arc_word(11, 9.0, 27.0, 150.0, 17.0, True, True)[0][28:228]
    out["arc, light on dark"] = CV.arc_word(8, 12.0, 14.0, 160.0, -10.0, False, False)[0][28:228]
    return out


def _quads():
    return {"upright": CV.quad_of(128, 100, 160, 50), "tilted 17": CV.quad_of(128, 100, 164, 48, 17.0), "tilted -30": CV.quad_of(120, 96, 150, 44, -30.0),
            "small": CV.quad_of(60, 40, 30, 9, 4.0), "thin": CV.quad_of(128, 97, 200, 3), "upside down": CV.quad_of(128, 100, 160, 50, 180.0),
            "partly outside left/top": CV.quad_of(10, 8, 160, 50, 5.0), "partly outside right/bottom": CV.quad_of(240, 190, 150, 44, -8.0),
            "wholly outside": CV.quad_of(400, -90, 100, 30), "degenerate": np.full(8, 50.0, np.float32)}


def _same_word(got, ref, name):
    assert got["flag"] == ref["flag"], name
    assert np.array_equal(got["hb"], ref["hb"]) and np.array_equal(got["spine"], ref["spine"]), (name, got["hb"], ref["hb"])
    assert np.array_equal(got["knots"], ref["table"]) and np.array_equal(got["knots1"], ref["table1"]), name


@pytest.mark.parametrize("image_name", ["random", "flat", "one dark row", "saturated noise", "arc", "arc, light on dark"])
def test_host_rule_bit_for_bit(built, image_name):
    """Host rule == numpy reference on every integer output of both passes, the crop and the outline; both channel orders give the same statistics.
    (Fails on the parent commit: engine.curve_frame is absent.)"""
    from tuatara_amd import engine
    image = _images()[image_name]
    swapped = np.ascontiguousarray(image[:, :, ::-1])
    for name, quad in _quads().items():
        frame = engine.curve_frame(quad)
        assert np.array_equal(frame, CV.frame(quad)), name
        ref = CV.word(image, quad)
        stats = engine.curve_columns(image, frame)
        assert stats.dtype == np.int32 and all(np.array_equal(stats[i], ref["stats1"][i]) for i in range(4)), name
        assert np.array_equal(engine.curve_columns(swapped, frame), stats), name
        got = engine.curve_knots(image, frame)
        _same_word(got, ref, (image_name, name))
        _same_word(engine.curve_knots(swapped, frame), ref, (image_name, name, "swapped"))
        if ref["stats2"] is not None:
            stats2 = engine.curve_columns(image, frame, ref["table1"])
            assert all(np.array_equal(stats2[i], ref["stats2"][i]) for i in range(4)), name
        if ref["table"].any():
            assert np.array_equal(engine.curve_crop(image, got["knots"]), CV.crop(image, ref["table"])), name
        assert engine.curve_outline(quad, got["flag"], got["knots"]).tobytes() == CV.outline(quad, ref["flag"], ref["table"]).tobytes(), name
        if image_name == "flat":                               # no ink edge anywhere: neither pass finds a column
            assert got["flag"] == 0 and not got["hb"].any() and not got["spine"].any() and not got["knots"].any(), name


def test_refused_quads_and_bad_arguments(built):
    from tuatara_amd import engine
    lib = engine.load()
    bad = CV.quad_of(100, 100, 100, 20)
    bad[3] = np.inf
    with pytest.raises(engine.EngineError, match="not finite"):
        engine.curve_frame(bad)
    far = CV.quad_of(100, 100, 100, 20)
    far[0] = 40000.0
    with pytest.raises(engine.EngineError, match="32768"):
        engine.curve_frame(far)
    img = np.zeros((8, 30, 3), np.uint8)
    frame = np.zeros(6, np.int64)
    assert lib.ttr_curve_columns(None, 8, 30, 0, engine._i64(frame), None, engine._i(np.zeros(512, np.int32))) == -1 and b"null argument" in lib.ttr_last_error()
    assert lib.ttr_curve_columns(engine._u8(img), 8, 30, 10, engine._i64(frame), None, engine._i(np.zeros(512, np.int32))) == -1 and b"bad image size" in lib.ttr_last_error()
    assert lib.ttr_curve_knots(engine._u8(img), 0, 30, 0, engine._i64(frame), None, None, None, None, None) == -1
    assert lib.ttr_curve_crop(engine._u8(img), 8, 30, 0, None, engine._u8(np.zeros((32, 128, 3), np.uint8))) == -1
    assert engine.curve_knots(img, frame)["flag"] == 0        # a frame of zeros samples one pixel: nothing to find, nothing read outside the page


def test_null_engine_and_null_results(built):
    from tuatara_amd import engine
    lib = engine.load()
    assert lib.ttr_engine_set_curved(None, 1) == -1 and b"null argument" in lib.ttr_last_error()
    assert lib.ttr_engine_curved(None) == 0
    for name in ("ttr_result_curved", "ttr_result_outlines", "ttr_result_spine_knots"):
        assert not getattr(lib, name)(None), name
    assert lib.ttr_results_gather_curved(None, 0, None, None, None) == -1
    assert lib.ttr_curve_crops(None, None, 0, 0, 0, None, 0, 0, None, None, None, None, None) == -1 and b"null argument" in lib.ttr_last_error()


# ---------------------------------------------------------------- 2. properties
def _bar_word(n_bars, bar_h, length, degrees, dark=True, size=256):
    """a straight word of n_bars bars on a `size` page -> (image, its tight quad)"""
    import math
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    a = math.radians(degrees)
    c0 = size / 2.0
    lx, ly = (xx - c0) * math.cos(a) + (yy - c0) * math.sin(a), -(xx - c0) * math.sin(a) + (yy - c0) * math.cos(a)
    pitch = length / (n_bars - 0.4)
    inside = (np.abs(ly) <= bar_h / 2.0) & (np.abs(lx) <= length / 2.0) & (((lx + length / 2.0) % pitch) <= 0.6 * pitch)
    fg, bg = (20, 235) if dark else (235, 20)
    img = np.where(inside[..., None], fg, bg).astype(np.uint8).repeat(3, 2)
    return np.ascontiguousarray(img), CV.quad_of(c0 - 0.5, c0 - 0.5, length + 1.0, bar_h + 1.0, degrees)


def test_a_straight_word_is_never_curved(built):
    """Straight words of 6 to 20 bars at tilts up to 30 degrees, in tight and in loose quads (the loose one half again as tall, off centre): flag 0 - so the
    engine leaves the row alone and the crop stays the kind-1 crop."""
    from tuatara_amd import engine
    for n_bars in (6, 11, 20):
        for degrees in (0.0, 7.0, -30.0):
            for dark in (True, False):
                img, quad = _bar_word(n_bars, 16.0, 150.0, degrees, dark)
                loose = CV.quad_of(127.5, 130.0, 156.0, 30.0, degrees)
                for q in (quad, loose):
                    got = engine.curve_knots(img, engine.curve_frame(q))
                    assert got["flag"] == 0 and got["hb"][0] > 0, (n_bars, degrees, dark, got["hb"])


def test_knot_tables_are_monotone_along_the_baseline(built):
    """the centres of a curved word advance along the quad's baseline from knot to knot, and every half-band vector points to the quad's bottom side"""
    from tuatara_amd import engine
    for degrees in (0.0, 17.0, -30.0, 180.0):
        for up in (True, False):
            img, quad = CV.arc_word(11, 10.0, 20.0, 150.0, degrees, up, True)
            got = engine.curve_knots(img, engine.curve_frame(quad))
            assert got["flag"] == 1
            q = quad.astype(np.float64).reshape(4, 2)
            base, down = q[1] - q[0], q[3] - q[0]
            for tab in (got["knots1"], got["knots"]):
                t = tab.astype(np.float64) / 65536.0
                along = t[:, 0:2] @ base
                assert (np.diff(along) > 0).all(), (degrees, up)
                assert (t[:, 2:4] @ down > 0).all(), (degrees, up)


# ---------------------------------------------------------------- 3. function
ARC_CASES = [(n, sr, up, deg, dark) for n in (6, 11, 20) for sr in (1.0, 2.0, 3.0) for up in (True, False) for deg, dark in ((0.0, True), (17.0, False), (-30.0, True))]


@pytest.mark.parametrize("n_bars,sr,up,degrees,dark", ARC_CASES)
def test_arc_words_are_straightened(built, n_bars, sr, up, degrees, dark):
    """Hand-made words of 6, 11 and 20 equal bars on circular arcs, chord 150 px, word 4:1, sagitta 1, 2 and 3 bar heights, arched up and down, tilted by 0,
    17 and -30 degrees, dark on light and light on dark.  Every word is flagged; the ink centroid of every column inside a bar of the straightened crop stays
    within `bound` crop rows of the mid-line; in today's kind-1 crop of the same quad it wanders over at least 12 rows (32 s / (s + h) >= 16 at s >= h, less
    the quantisation of the bars' ends).

    The bound, in page pixels, then in crop rows of r = 2 hb / 32 px (hb the final half band in pixels): eight chords leave s / 64 of the sagitta between
    the knots; a window of 32 columns sees pass 1's residual, which is those chords' own (s / 64 again); every ink edge is read at the nearest pixel of a
    drawing that includes whole pixels (1/2 px for the read, 1/2 px for the drawing); spine rows are carried in frame rows in pass 1 and in band rows in pass
    2 (half of each); and the centroid itself is measured on whole crop rows (1/2 row).  The sum is capped at 4 crop rows."""
    from tuatara_amd import engine
    chord = 150.0
    bar_h = chord / 4.0 / (1.0 + sr)
    s = sr * bar_h
    img, quad = CV.arc_word(n_bars, bar_h, s, chord, degrees, up, dark)
    got = engine.curve_knots(img, engine.curve_frame(quad))
    ref = CV.word(img, quad)
    _same_word(got, ref, "arc")
    assert got["flag"] == 1
    crop = engine.curve_crop(img, got["knots"])
    cen = CV.ink_centroid(crop, dark)
    assert np.isfinite(cen).sum() >= n_bars
    q = quad.astype(np.float64).reshape(4, 2)
    frame_row = float(np.hypot(*(q[3] - q[0]))) / CV.V                       # px per frame row
    hb_px = float(np.hypot(*(got["knots"][4, 2:4].astype(np.float64) / 65536.0)))                 # the final half band, in px
    r = 2.0 * hb_px / 32.0
    band_row = float(got["hb"][0]) * frame_row / 32.0
    bound = min(4.0, (2.0 * s / 64.0 + 0.5 + 0.5 + 0.5 * frame_row + 0.5 * band_row) / r + 0.5)
    dev = float(np.nanmax(np.abs(cen - 16.0)))
    today = CV.ink_centroid(GR.region_crop(img, quad), dark)
    wander = float(np.nanmax(today) - np.nanmin(today))
    print(f"bars {n_bars} sagitta {sr} h up {up} tilt {degrees} dark {dark}: deviation {dev:.2f} rows, bound {bound:.2f}, today's wander {wander:.2f}")
    assert dev <= bound, (dev, bound)
    assert wander >= 12.0, wander


# ---------------------------------------------------------------- 4. the arched page under the CPU oracle's detector
def test_the_arched_page_yields_flagged_words_under_the_oracle(built, oracle_models):
    """tuatara_amd.synth.synthetic_arched_page(1), the page tests/test_gpu_curve.py reads: the CPU oracle's detector boxes its six words, and the rule flags
    at least two of them (the arched ones) and leaves the straight ones"""
    from oracle import pipeline
    from tuatara_amd import engine, synth
    img, words = synth.synthetic_arched_page(1)
    det = pipeline.detect(oracle_models[0], img)
    assert len(det["boxes"]) == len(words) == 6
    flags = []
    for b in det["boxes"]:
        quad = np.asarray(RR.deskew(b)[1], np.float32).ravel()
        flags.append(engine.curve_knots(img, engine.curve_frame(quad))["flag"])
    assert 2 <= sum(flags) == sum(w["sagitta"] > 0 for w in words), flags


# ---------------------------------------------------------------- 5. callers
def test_pytuatara_keyword_without_a_device(built, capfd):
    """curved is keyword-only and a bool; it does not combine with what the engine refuses (checked before the engine is created: no device needed)."""
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(TypeError):
        pytuatara.image_to_data(img, "w", "o", curved="yes")
    for kw in (dict(orient="flip"), dict(chars=True), dict(wide=True)):
        with pytest.raises(ValueError, match="curved"):
            pytuatara.image_to_data(img, "w", "o", curved=True, **kw)
    assert pytuatara.image_to_data(img, "/nonexistent/weights", "o", curved=True) == []      # (passes the check; the engine then fails as it does without it)
    assert "error loading" in capfd.readouterr().err


def test_ocr_cli_knows_curved(built, tmp_path):
    """`ocr_cli --curved` is an option, not an image path: with too few arguments left the usage line names it."""
    cli = os.path.join(ROOT, "build", "examples", "ocr_cli")
    r = subprocess.run([cli, "--curved", str(tmp_path / "none.png")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--curved" in r.stderr, r.stderr
