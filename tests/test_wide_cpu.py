"""Wide words (DESIGN.md "Wide words") without a GPU: the host rule (ttr_wide_plan, ttr_wide_profile, ttr_wide_cuts_from_profile, ttr_wide_piece_coef,
ttr_wide_piece_quads) against tests/wide_ref.py bit for bit, the rule's properties, its function on hand-made pages of bars and gaps, the refusals that need no
device, the exported symbols and the callers' switches as far as they go without a device.  Every test here fails on the parent commit: the symbols are absent."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import regions_ref as GR
from tests import wide_ref as WR
from tests.conftest import ROOT

NEW_SYMBOLS = ("ttr_engine_set_wide", "ttr_engine_wide", "ttr_result_piece_first", "ttr_result_piece_ids", "ttr_result_piece_probs", "ttr_result_piece_confs",
               "ttr_result_piece_quads", "ttr_result_piece_cuts", "ttr_results_gather_pieces", "ttr_wide_plan", "ttr_wide_profile", "ttr_wide_cuts_from_profile",
               "ttr_wide_piece_coef", "ttr_wide_piece_quads", "ttr_wide_cuts")


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


# ---------------------------------------------------------------- 1. the plan
@pytest.mark.parametrize("max_aspect", [2.0, 8.0, 64.0])
def test_plan_counts_and_frame(built, max_aspect):
    """n at aspects just below and just above max_aspect, 2 max_aspect, 16 max_aspect and beyond, and with b2 = 0; the frame against the reference; n = 1 is
    region_coef's frame.  (Fails on the parent commit: engine.wide_plan is absent.)"""
    from tuatara_amd import engine
    h = 8.0 if max_aspect == 64.0 else 16.0                   # (the quad rules stop at |x| < 32768: 40 x 64 x 8 = 20480)
    cases = [(0.5, 1), (0.999, 1), (1.001, 2), (1.999, 2), (2.001, 3), (15.999, 16), (16.001, 16), (40.0, 16)]
    for degrees in (0.0, 7.0, -30.0):
        for f, want in cases:
            quad = WR.quad_of(11.25, 40.5, f * max_aspect * h, h, degrees)
            n, frame = engine.wide_plan(quad, max_aspect)
            rn, rframe = WR.plan(quad, max_aspect)
            assert n == rn == want, (degrees, f, n, rn, want)
            assert np.array_equal(frame, rframe), (degrees, f)
            if n == 1:
                assert np.array_equal(frame, GR.region_fixed(quad))
    flat = np.array([3, 5, 90, 5, 90, 5, 3, 5], np.float32)   # b2 = 0
    n, frame = engine.wide_plan(flat, max_aspect)
    assert n == 1 and np.array_equal(frame, WR.plan(flat, max_aspect)[1]) and np.array_equal(frame, GR.region_fixed(flat))


def test_plan_refuses_bad_arguments(built):
    from tuatara_amd import engine
    quad = WR.quad_of(0, 0, 100, 10)
    for a in (0.0, 1.5, 65.0, float("nan"), float("inf"), -8.0):
        with pytest.raises(engine.EngineError, match="max_aspect"):
            engine.wide_plan(quad, a)
    bad = quad.copy()
    bad[3] = np.inf
    with pytest.raises(engine.EngineError, match="not finite"):
        engine.wide_plan(bad, 8.0)


# ---------------------------------------------------------------- 2. profile and cuts, bit for bit
def _images():
    rng = np.random.default_rng(5)
    H, W = 72, 900
    out = {"random": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "flat": np.full((H, W, 3), 200, np.uint8)}
    col = np.full((H, W, 3), 255, np.uint8)
    col[:, 417] = 0
    out["one dark column"] = col
    out["saturated noise"] = (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    smooth = rng.integers(0, 256, (H, W // 6 + 1, 3), dtype=np.uint8).repeat(6, 1)[:, :W]
    out["blocky"] = np.ascontiguousarray(smooth)
    return out


def _quads():
    return {"upright n=4": (WR.quad_of(20.0, 20.0, 800.0, 25.0), 8.0),
            "upright n=2": (WR.quad_of(100.5, 10.25, 390.0, 30.0), 8.0),
            "tilted 7": (WR.quad_of(30.0, 5.0, 700.0, 20.0, 3.0), 8.0),
            "tilted -30": (WR.quad_of(200.0, 71.0, 130.0, 12.0, -30.0), 2.0),
            "n=16": (WR.quad_of(2.0, 30.0, 890.0, 9.0), 2.0),
            "partly outside left/top": (WR.quad_of(-150.0, -8.0, 600.0, 24.0), 8.0),
            "partly outside right/bottom": (WR.quad_of(500.0, 60.0, 700.0, 30.0, 2.0), 8.0),
            "n=1": (WR.quad_of(40.0, 12.0, 120.0, 31.0), 8.0)}


@pytest.mark.parametrize("image_name", ["random", "flat", "one dark column", "saturated noise", "blocky"])
def test_profile_cuts_and_coefficients_bit_for_bit(built, image_name):
    """Host rule == numpy reference on every integer output.  (Fails on the parent commit: engine.wide_profile is absent.)"""
    from tuatara_amd import engine
    image = _images()[image_name]
    for name, (quad, aspect) in _quads().items():
        n, frame = engine.wide_plan(quad, aspect)
        rn, rframe, rq, rcuts, rcoef = WR.word(image, quad, aspect)
        assert n == rn and np.array_equal(frame, rframe), name
        q = engine.wide_profile(image, frame, n)
        assert q.dtype == np.uint16 and np.array_equal(q, rq), name
        cuts = engine.wide_cuts_from_profile(q, n)
        assert np.array_equal(cuts, rcuts), (name, cuts, rcuts)
        coef = np.stack([engine.wide_piece_coef(frame, cuts[j], cuts[j + 1]) for j in range(n)])
        assert np.array_equal(coef, rcoef), name
        assert np.array_equal(engine.wide_piece_quads(quad, cuts, n), WR.piece_quads(quad, cuts, n)), name
        widths = np.diff(cuts[:n + 1])
        assert cuts[0] == 0 and cuts[n] == 128 * n and (cuts[n + 1:] == -1).all() and widths.min() >= 64 and widths.max() <= 192, name
        if image_name == "flat":                               # every cost ties: the tie rule decides and every width is 128
            assert (q == 0).all() and (widths == 128).all(), name


def test_random_profiles_bit_for_bit(built):
    """The DP alone on synthetic profiles of every n, the extremes of u16 included."""
    from tuatara_amd import engine
    rng = np.random.default_rng(6)
    for n in range(1, 17):
        for kind in range(3):
            q = rng.integers(0, 1021, 128 * n).astype(np.uint16)
            if kind == 1:
                q = (rng.integers(0, 2, 128 * n) * 1020).astype(np.uint16)
            if kind == 2:
                q[rng.integers(0, 128 * n, 3 * n)] = 0
            cuts = engine.wide_cuts_from_profile(q, n)
            assert np.array_equal(cuts, WR.cuts_from_profile(q, n)), (n, kind)


# ---------------------------------------------------------------- 3. properties
def test_pieces_tile_the_frame(built):
    """n = 1 coefficients equal region_coef's; the pieces' sampled frame positions tile the frame: piece j's column k (of 128) lands on frame column
    c0 + (k + 0.5) w / 128 - 0.5 to within one unit of 2^-16 px per column, so neighbouring pieces meet with no gap or overlap beyond that."""
    from tuatara_amd import engine
    rng = np.random.default_rng(7)
    for trial in range(40):
        n = int(rng.integers(1, 17))
        aspect = 4.0
        height = float(rng.uniform(8, 20))
        length = (n - 0.5) * aspect * height
        quad = WR.quad_of(float(rng.uniform(0, 50)), float(rng.uniform(0, 50)), length, height, float(rng.uniform(-30, 30)))
        pn, frame = engine.wide_plan(quad, aspect)
        assert pn == n
        if n == 1:
            row = engine.wide_piece_coef(frame, 0, 128)
            assert np.array_equal(row, np.concatenate([[1], GR.region_fixed(quad), [0]]))
            continue
        q = rng.integers(0, 1021, 128 * n).astype(np.uint16)
        cuts = engine.wide_cuts_from_profile(q, n)
        X0, Ax, Bx, Y0, Ay, By = (int(v) for v in frame)
        for j in range(n):
            c0, c1 = int(cuts[j]), int(cuts[j + 1])
            w = c1 - c0
            row = [int(v) for v in engine.wide_piece_coef(frame, c0, c1)]
            assert row[0] == 1 and row[7] == 0 and row[3] == Bx and row[6] == By
            for (P0, Ap), (F0, A) in (((row[1], row[2]), (X0, Ax)), ((row[4], row[5]), (Y0, Ay))):
                for k in (0, 1, 63, 64, 127):
                    got = P0 + k * Ap                                              # piece column k, row 0, in 2^-16 px
                    want = F0 + A * c0 + (A * w * (2 * k + 1) - 128 * A) / 256.0    # frame column c0 + (k + 0.5) w / 128 - 0.5
                    assert abs(got - want) <= 1.0 + k, (trial, j, k, got, want)    # one unit per column at the most
            if j + 1 < n:                                                          # the seam: the next piece starts where this one ends
                nxt = [int(v) for v in engine.wide_piece_coef(frame, c1, int(cuts[j + 2]))]
                end_x = row[1] + 127 * row[2] + row[2] / 2.0                        # this piece's right edge
                start_x = nxt[1] - nxt[2] / 2.0                                    # the next piece's left edge
                assert abs(end_x - start_x) <= 130.0, (trial, j)                   # < 2 / 1000 px


# ---------------------------------------------------------------- 4. function
def bars_page(rng, n_chars, height=24, margin=6):
    """A white page holding one word of n_chars dark bars of random widths with blank gaps between them, drawn so that at the word's own scale (one frame
    column per page pixel) every window of 64..192 columns holds a blank column: bars are 4..40 px wide (narrower for the longest words), gaps 3..8 px.  Returns (image, quad, bars)."""
    widths = rng.integers(4, 41 if n_chars <= 60 else 23 if n_chars <= 90 else 15, n_chars)   # (120 bars still fit the 2048 columns of 16 pieces)
    gaps = rng.integers(3, 9, n_chars + 1)
    total = int(widths.sum() + gaps.sum())
    img = np.full((height + 2 * margin, total + 2 * margin, 3), 255, np.uint8)
    x = margin + int(gaps[0])
    bars = []
    for k in range(n_chars):
        img[margin + 2:margin + height - 2, x:x + int(widths[k])] = rng.integers(0, 90, 3).astype(np.uint8)
        bars.append((x, x + int(widths[k])))
        x += int(widths[k] + gaps[k + 1])
    quad = GR.region_from_rect(margin, margin, margin + total, margin + height)
    return img, quad, bars


def test_cuts_fall_into_the_gaps(built):
    """Words of 30 to 120 bars: every interior cut of the rule lies in a blank gap (q[c - 1] + q[c] == 0), and an even split of the same word does not manage
    that on at least one word of the set."""
    from tuatara_amd import engine
    rng = np.random.default_rng(8)
    even_fails = 0
    for n_chars in (30, 45, 60, 90, 120):
        img, quad, bars = bars_page(rng, n_chars)
        length = float(quad[2] - quad[0])
        aspect = max(2.0, min(64.0, length / 24.0 / (length / 128.0) * 1.0001))   # about one frame column per page pixel: n = ceil(length / 128)
        n, frame = engine.wide_plan(quad, aspect)
        assert n >= 2
        q = engine.wide_profile(img, frame, n)
        U = 128 * n
        blank = q == 0
        for c in range(0, U - 192):                          # the set's premise: a blank column inside every window [64, 192]
            assert blank[c + 64:c + 193].any(), (n_chars, c)
        cuts = engine.wide_cuts_from_profile(q, n)
        assert np.array_equal(cuts, WR.cuts_from_profile(q, n))
        for c in cuts[1:n]:
            assert int(q[c - 1]) + int(q[c]) == 0, (n_chars, int(c))
        even = [128 * j for j in range(1, n)]
        even_fails += any(int(q[c - 1]) + int(q[c]) != 0 for c in even)
    assert even_fails >= 1


# ---------------------------------------------------------------- 5. refusals without a device, callers
def test_null_engine_and_null_results(built):
    from tuatara_amd import engine
    lib = engine.load()
    assert lib.ttr_engine_set_wide(None, 8.0) == -1 and b"null argument" in lib.ttr_last_error()
    assert lib.ttr_engine_wide(None) == 0.0
    for name in ("ttr_result_piece_first", "ttr_result_piece_ids", "ttr_result_piece_probs", "ttr_result_piece_confs", "ttr_result_piece_quads", "ttr_result_piece_cuts"):
        assert not getattr(lib, name)(None), name
    assert lib.ttr_results_gather_pieces(None, 0, None, None, None, None, None, None) == -1


def test_host_rule_refuses_bad_arguments(built):
    from tuatara_amd import engine
    img = np.zeros((8, 300, 3), np.uint8)
    frame = np.zeros(6, np.int64)
    for n in (0, 17, -1):
        with pytest.raises(engine.EngineError, match="1..16"):
            engine.wide_profile(img, frame, n)
        with pytest.raises(engine.EngineError, match="1..16"):
            engine.wide_cuts_from_profile(np.zeros(2048, np.uint16), n)
        with pytest.raises(engine.EngineError, match="1..16"):
            engine.wide_piece_quads(np.zeros(8, np.float32), np.zeros(17, np.int32), n)
    for c0, c1 in ((-1, 5), (5, 5), (0, 2049)):
        with pytest.raises(engine.EngineError, match="columns"):
            engine.wide_piece_coef(frame, c0, c1)


def test_wide_argument_of_the_python_layers(built):
    from tuatara_amd import engine
    assert engine.WIDE_DEFAULT == 8.0
    assert engine._wide_arg(True) == 8.0 and engine._wide_arg(False) == 0.0 and engine._wide_arg(None) == 0.0 and engine._wide_arg(3) == 3.0


def test_pytuatara_keyword_without_a_device(built, capfd):
    """wide is keyword-only; a bad value is refused before the engine is created (no device needed)."""
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    img = np.zeros((8, 8, 3), np.uint8)
    for bad in (1.0, 65.0, -2.0, float("nan")):
        with pytest.raises(RuntimeError, match="wide"):
            pytuatara.image_to_data(img, "w", "o", wide=bad)
    with pytest.raises(TypeError):
        pytuatara.image_to_data(img, "w", "o", wide="yes")
    assert pytuatara.image_to_data(img, "/nonexistent/weights", "o", wide=True) == []      # (passes the check; the engine then fails as it does without it)
    assert "error loading" in capfd.readouterr().err


def test_ocr_cli_refuses_a_bad_wide_value(built, tmp_path):
    cli = os.path.join(ROOT, "build", "examples", "ocr_cli")
    """`ocr_cli --wide x img weights out` fails, naming the option, before the image is read (the image does not exist)."""
    for bad in ("x", "1.5", "65", "nan"):
        r = subprocess.run([cli, "--wide", bad, str(tmp_path / "none.png"), str(tmp_path), str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--wide takes an aspect" in r.stderr, (bad, r.stderr)
