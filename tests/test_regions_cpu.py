"""Regions and per-row character sets (DESIGN.md "Regions and per-row character sets") without a GPU: the host rules (the pixel-edge quad of a rectangle,
the sampler's coefficients of a caller's quad, the bbox rule, the strict test) against tests/regions_ref.py, the refusals that need no device by name,
the exported symbols, the row-by-row reference decode, pytuatara's regions= keyword and ocr_cli --regions on a malformed file."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import charset_ref as CR
from tests import regions_ref as GR
from tests.conftest import ROOT

DIGITS = "0123456789"
NEW_SYMBOLS = ("ttr_region_from_rect", "ttr_region_geometry", "ttr_regions_to_data_dev", "ttr_image_regions_to_data", "ttr_result_sets", "ttr_pack_regions",
               "ttr_parseq_logits_sets", "ttr_logits_confidence_sets")


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


def test_symbols_are_exported(built):
    from tuatara_amd import engine
    lib = engine.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in engine.SYMBOLS), name
    header = open(os.path.join(ROOT, "include", "tuatara_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
    assert C.sizeof(engine.Region) == 40                                         # float quad[8]; int32 page, set


def test_region_from_rect_is_the_pixel_edge_quad(built):
    from tuatara_amd.engine import EngineError, region_from_rect, region_quad
    for rect in ((0, 0, 1, 1), (3, 4, 10, 9), (-5, -7, 2, 3), (100, 200, 1124, 968), (0, 0, 32767, 32767)):
        q = region_from_rect(*rect)
        assert q.dtype == np.float32 and q.tobytes() == GR.region_from_rect(*rect).tobytes(), rect
        assert region_quad(rect).tobytes() == q.tobytes()
        assert region_quad(q).tobytes() == q.tobytes() and region_quad(q.reshape(4, 2)).tobytes() == q.tobytes()
    for rect in ((3, 4, 3, 9), (3, 4, 10, 4), (5, 5, 1, 9)):
        with pytest.raises(EngineError, match="empty"):
            region_from_rect(*rect)
    with pytest.raises(ValueError):
        region_quad((1.5, 2, 3, 4))
    with pytest.raises(ValueError):
        region_quad((1, 2, 3))


def test_region_geometry_against_the_reference(built):
    from tuatara_amd.engine import region_geometry
    rng = np.random.default_rng(5)
    quads = [GR.region_from_rect(10, 20, 138, 52), GR.tilted_quad(300, 200, 180, 40, 7), GR.tilted_quad(300, 200, 180, 40, -30), GR.tilted_quad(50, 60, 90, 30, 45),
             GR.tilted_quad(5, 5, 120, 40, 0), np.array([7, 7, 7, 7, 9, 20, 5, 20], np.float32)]             # the last: degenerate, tl == tr
    quads += [rng.uniform(-2000, 3000, 8).astype(np.float32) for _ in range(40)]
    quads += [np.array([32767.996] * 8, np.float32), np.array([-32767.996, 0, 32767.996, 0, 32767.996, 1, -32767.996, 1], np.float32)]
    for q in quads:
        assert GR.quad_ok(q)
        fixed, bbox, inside = region_geometry(q, 768, 1024)
        assert np.array_equal(fixed, GR.region_fixed(q)), q
        assert bbox.tobytes() == GR.region_bbox(q).tobytes(), q
        assert inside == GR.inside(q, 768, 1024), q
    # the strict test's edges are inclusive: the whole page as a region is inside, half a pixel more is not
    page = GR.region_from_rect(0, 0, 1024, 768)
    assert region_geometry(page, 768, 1024)[2] and not region_geometry(page, 768, 1023)[2] and not region_geometry(page, 767, 1024)[2]
    assert not region_geometry(page + np.float32(0.5), 768, 1024)[2] and not region_geometry(page - np.float32(0.5), 768, 1024)[2]
    # the upright quad of a 128 x 32 rectangle samples pixel centres: X0 = x0, A = one pixel
    fixed, _, _ = region_geometry(GR.region_from_rect(10, 20, 138, 52))
    assert fixed.tolist() == [10 << 16, 1 << 16, 0, 20 << 16, 0, 1 << 16]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, 32768.0, -32768.0, 1e9])
def test_a_bad_coordinate_is_refused_by_name(built, bad):
    from tuatara_amd.engine import EngineError, region_geometry
    for k in (0, 5, 7):
        q = GR.region_from_rect(3, 4, 10, 9)
        q[k] = bad
        assert not GR.quad_ok(q)
        with pytest.raises(EngineError, match="not finite or has .x. >= 32768"):
            region_geometry(q, 100, 100)


def test_row_by_row_reference_decode():
    x = np.random.default_rng(3).normal(0, 3, (9, 26, 95)).astype(np.float32)
    digits = np.array([0x7FF, 0, 0], np.uint32)
    one = np.array([1 | (1 << 20), 0, 0], np.uint32)
    masks = [digits, one, CR.FULL]
    set_of = [0, 1, 2, -1, 0, 1, 2, -1, 0]
    ids, prob, conf, rows = GR.masked_decode_rows(x, masks, set_of, own=digits)
    assert ids.shape == (9, 26) and prob.shape == (9, 26) and conf.shape == (9,) and rows.shape == (9, 3)
    for i, s in enumerate(set_of):
        m = digits if s < 0 else masks[s]
        a = CR.allowed(m)
        assert a[ids[i]].all()
        ri, rp, rc = CR.masked_decode(x[i:i + 1], m)
        assert np.array_equal(ri[0], ids[i]) and np.array_equal(rp[0], prob[i]) and rc[0] == conf[i]
    assert np.array_equal(ids[2], x[2].argmax(-1))                                # the full mask: the plain decode
    assert set(np.unique(ids[1])) <= {0, 20}


def test_region_crop_reference_on_an_upright_rectangle():
    """a 128 x 32 upright rectangle samples the pixels themselves; outside the image the border pixel is replicated"""
    img = np.random.default_rng(1).integers(0, 256, (60, 200, 3), dtype=np.uint8)
    assert np.array_equal(GR.region_crop(img, GR.region_from_rect(10, 20, 138, 52)), img[20:52, 10:138])
    out = GR.region_crop(img, GR.region_from_rect(-20, -8, 108, 24))
    assert np.array_equal(out[8:, 20:], img[:24, :108]) and (out[:8, :20] == img[0, 0]).all()
    assert np.array_equal(out[:8, 20:], np.broadcast_to(img[0, :108], (8, 108, 3)))


def test_pytuatara_regions_keyword_without_a_gpu(built, capfd):
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    img = np.zeros((8, 8, 3), np.uint8)
    w = "/nonexistent/weights"
    good = [{"rect": (0, 0, 4, 4), "allowlist": DIGITS}, {"quad": [0, 0, 4, 0, 4, 4, 0, 4]}, {"quad": [[0, 0], [4, 0], [4, 4], [0, 4]], "blocklist": "|"}]
    with pytest.raises(TypeError):
        pytuatara.image_to_data(img, w, "o", False, False, None, False, False, False, False, None, None, good)   # keyword-only
    # every bad list raises ValueError before anything runs (the weights directory does not exist: nothing else is reached)
    for bad, what in (([{"rect": (0, 0, 4, 4), "allowlist": "12~"}], "'~'"), ([{"quad": [0, 0, 4, 0], "allowlist": DIGITS}], "8 floats"),
                      ([{"rect": (0, 0, 4)}], "four integers"), ([{"rect": (0, 0, 0, 4)}], "empty"), ([{"quad": [0] * 8, "rect": (0, 0, 4, 4)}], "one of them"),
                      ([{}], "one of them"), ([{"rect": (0, 0, 4, 4), "charset": DIGITS}], "unknown key"), ([(0, 0, 4, 4)], "dict"), ("quad", "list of dicts"),
                      ([{"quad": [0, 0, float("nan"), 0, 4, 4, 0, 4]}], "not finite"), ([{"quad": [0, 0, 4e4, 0, 4, 4, 0, 4]}], "32768"),
                      (good + [{"rect": (0, 0, 4, 4), "blocklist": " "}], r"regions\[3\]")):
        with pytest.raises(ValueError, match=what):
            pytuatara.image_to_data(img, w, "o", regions=bad)
    with pytest.raises(ValueError, match="do not combine"):
        pytuatara.image_to_data(img, w, "o", regions=good, lines=True)
    with pytest.raises(ValueError, match="'~'"):                                               # the call's own lists are still checked first
        pytuatara.image_to_data(img, w, "o", regions=good, allowlist="~")
    capfd.readouterr()
    assert pytuatara.image_to_data(img, "", "o", regions=good) == []                           # the reference's conventions, as on every call
    assert "Please provide a value for weights_dir" in capfd.readouterr().err
    assert pytuatara.image_to_data(img, w, "o", regions=good) == []
    assert "error loading" in capfd.readouterr().err


def test_ocr_cli_regions_parser_on_a_malformed_file(built, tmp_path):
    cli = os.path.join(ROOT, "build", "examples", "ocr_cli")
    png = os.path.join(ROOT, "tests", "data", "funsd_0001129658.png")
    cases = [("10 20 138\n", ":1:"), ("# fields\n10 20 138 52 0123456789\n\n10 x 138 52\n", ":4:"), ("10 20 138.5 52\n", "integers"), ("10 20 10 52\n", "empty"),
             ("1 2 3 4 5 6 7 8 a b c\n", ":1:"), ("1 2 3 4 5 6 7 nan\n", "not a coordinate"), ("1 2 3 4 ab cd ef\n", ":1:")]
    for text, what in cases:
        f = tmp_path / "regions.txt"
        f.write_text(text)
        out = subprocess.run([cli, "--regions", str(f), png, "/nonexistent/weights", str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 1 and what in out.stderr and out.stdout == "", (text, out.stderr)
    out = subprocess.run([cli, "--regions", str(tmp_path / "missing.txt"), png, "/nonexistent/weights", str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "cannot read regions file" in out.stderr
    # a well-formed file gets as far as the engine (which this machine cannot create): the parser accepted it
    f = tmp_path / "ok.txt"
    f.write_text("# a date, an amount, a name\n10 20 138 52 0123456789/\n10.5 20 138 22.25 137 54 9.5 52 0123456789. ,   # a tilted field\n10 60 138 92\n")
    out = subprocess.run([cli, "--regions", str(f), png, "/nonexistent/weights", str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "error loading" in out.stderr and "regions" not in out.stderr, out.stderr
