"""GPU suite for deskew (DESIGN.md "Deskew"; tuatara_amd/csrc/deskew.hip): the pixel pass, deskew_score_kernel and deskew_rotate_kernel through the stage call
against the host rule bit for bit - the upright page's bytes, the record and all 2 M + 1 scores - on the pages of tests/test_deskew_cpu.py, widths 1 to 193, a
window that is not dword-aligned, a padded stride, the corner-pixel pages and a 1300 x 1100 page; and the layer's contract: a page call with the layer on
returns, in every field the result carries, what the same call returns with the layer off for tests/deskew_ref.py's upright page - through the list,
mixed-size, device and streamed entry points with text lines, text blocks and tables on (the columns page and the form, slopes 27 and -45), and tiled.  Every test here fails on the parent commit: Engine.set_deskew /
Engine.deskew_page and their symbols are absent."""
import numpy as np
import pytest

from tests import deskew_ref as R
from tests import tables_ref as T

pytestmark = pytest.mark.gpu

M, G, INK = R.MAX_SLOPE, R.GAIN, R.INK


@pytest.fixture(scope="module")
def eng(weights):
    """a rectified engine (its results carry the quads) with text lines and blocks on, batching mixed sizes; deskew and tables OFF at rest"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import CROP_RECTIFIED, Engine
    build_lib()
    e = Engine(weights["dir"], crop_mode=CROP_RECTIFIED, mixed_batches=1, lines=1, blocks=1)
    yield e
    e.close()


class deskew_on:
    def __init__(self, eng, arg=True, tables=False):
        self.eng, self.arg, self.tables = eng, arg, tables

    def __enter__(self):
        self.eng.set_deskew(self.arg)
        self.eng.set_tables(self.tables)
        return self.eng

    def __exit__(self, *a):
        self.eng.set_deskew(False)
        self.eng.set_tables(False)


FIELDS = ("ids", "conf", "prob", "bbox", "quad", "line", "word", "order", "line_first", "line_bbox", "block", "line_block", "line_pos", "block_order", "block_first",
          "block_bbox", "rulings", "table_rects", "table_lines", "cells", "item_table", "item_cell")


def assert_same_result(a, b, what=""):
    """every field the result carries, bit for bit (a field may be None in both)"""
    assert list(a.texts) == list(b.texts), what
    assert a.block_mode == b.block_mode and a.table_mode == b.table_mode and a.cell_texts == b.cell_texts, what
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert np.asarray(x).shape == np.asarray(y).shape and np.array_equal(x, y), (what, k)


@pytest.fixture(scope="module")
def pairs():
    """the main test's pages, once: name -> (tilted page, the restatement's upright page, its record) under the defaults"""
    out = {}
    for name, page in (("columns", R.columns_page()), ("form", R.form_page(words=True))):
        for s in (27, -45):
            tilted = R.tilt(page, s)
            ref = R.deskew_ref(tilted, M, G, INK)
            assert ref["skew"]["slope"] == s
            out[f"{name} {s}"] = (tilted, ref["image"], ref["skew"])
    return out


def _dev(arr):
    from tuatara_amd.engine import DeviceBuffer
    arr = np.ascontiguousarray(arr)
    b = DeviceBuffer(arr.nbytes)
    b.upload(arr)
    return b


# ------------------------------------------------------------------------------------------------- 1. the kernels against the host rule
def _stage_cases():
    out = [("columns", R.columns_page()), ("columns 37", R.tilt(R.columns_page(), 37)), ("form -45", R.tilt(R.form_page(True), -45)), ("grid 18", R.tilt(T.grid_page(), 18)),
           ("no baselines", R.no_baseline_page()), ("blank", np.full((37, 91, 3), 255, np.uint8)), ("all ink", np.zeros((37, 91, 3), np.uint8)),
           ("corners", R.corner_page(40, 70)), ("wide corners", R.corner_page(9, 1030))]
    for s in range(4):
        out.append((f"random {s}", T.random_page(s, h=80 + 7 * s, w=120 + 11 * s, p=0.1 + 0.1 * s)))
    return out


def test_stage_call_equals_the_host_rule(eng):
    from tuatara_amd import engine as E
    for name, img in _stage_cases():
        for m, g in ((128, 256), (M, G), (1, 256)):
            assert R.same(eng.deskew_page(img, m, g, INK), E.deskew_from_page(img, m, g, INK)), (name, m, g)


def test_funsd_page_and_its_tilts(eng, funsd):
    from tuatara_amd import engine as E
    for s in (0, -9, 64):
        img = R.tilt(funsd, s) if s else funsd
        got = eng.deskew_page(img, 128, 256, INK)
        assert R.same(got, E.deskew_from_page(img, 128, 256, INK)) and abs(got["skew"]["found"] - s) <= 1


def test_widths_1_to_193(eng):
    """widths below 64 and widths that are no multiples of 64; heights 1 to 5 - every row end of the rotate kernel's four-pixel stores and the score kernel's words"""
    from tuatara_amd import engine as E
    rng = np.random.default_rng(11)
    for w in range(1, 194):
        h = 1 + w % 5
        img = np.where(rng.random((h, w, 1)) < 0.3, rng.integers(0, 100, (h, w, 3)), rng.integers(150, 256, (h, w, 3))).astype(np.uint8)
        assert R.same(eng.deskew_page(img, 128, 256, INK), E.deskew_from_page(img, 128, 256, INK)), w


@pytest.mark.parametrize("offset,pad", [(3, 7), (1, 0), (0, 5), (2, 2)])
def test_a_window_that_is_not_dword_aligned(eng, offset, pad):
    from tuatara_amd import engine as E
    img = R.tilt(T.grid_page(), -18)[:, :197]
    got = eng.deskew_page(img, 128, 256, INK, dev_offset=offset, dev_stride=197 * 3 + pad)
    assert R.same(got, E.deskew_from_page(np.ascontiguousarray(img), 128, 256, INK)) and got["skew"]["mode"] == 1


def test_a_page_of_many_tiles(eng):
    from tuatara_amd import engine as E, synth
    img = R.tilt(synth.synthetic_page(7, 1300, 1100, n_words=60), 9)
    got = eng.deskew_page(img, 128, 256, INK)
    assert R.same(got, E.deskew_from_page(img, 128, 256, INK)) and got["skew"]["slope"] != 0


# ------------------------------------------------------------------------------------------------- 2. page calls
def test_layer_on_equals_layer_off_on_the_upright_page(eng, pairs):
    """the main test, through the list entry point (one call of four pages of two sizes: two mixed batches), with lines, blocks and tables on"""
    names = list(pairs)
    eng.set_tables(True)
    try:
        off = eng.images_to_data([pairs[n][1] for n in names], conf=True)
        assert all(r.skew is None and "quad_page" not in r[0] for r in off)
        with deskew_on(eng, True, tables=True):
            on = eng.images_to_data([pairs[n][0] for n in names], conf=True)
    finally:
        eng.set_tables(False)
    for n, a, b in zip(names, on, off):
        assert len(a) >= 8, n
        assert_same_result(a, b, n)
        want = pairs[n][2]
        assert a.skew == want, (n, a.skew)
        assert a.line is not None and a.block is not None and a.item_cell is not None


# (family, a window of its page that shares the page's canvas: the second size of the mixed batch)
WINDOWS = [("columns", 500, 760), ("form", 470, 996)]


@pytest.mark.parametrize("family,wh,ww", WINDOWS)
def test_device_mixed_and_streamed_entry_points(eng, pairs, family, wh, ww):
    """both pages of a family (slopes 27 and -45) as a uniform device batch, as a mixed batch of two sizes (page 1 a window with an odd row stride) and streamed,
    with lines, blocks and TABLES on: the tables' pixel pass of batch N reads the slot's upright pages while the detector of batch N + 1 runs"""
    from tuatara_amd import engine as E
    from tuatara_amd.engine import EngineError
    names = [n for n in pairs if n.startswith(family)]
    tilted, upright = [pairs[n][0] for n in names], [pairs[n][1] for n in names]
    h, w = tilted[0].shape[:2]
    assert E.canvas_geometry(wh, ww)[:2] == E.canvas_geometry(h, w)[:2]
    bufs = []
    eng.set_tables(True)
    try:
        ut, uu = _dev(np.stack(tilted)), _dev(np.stack(upright))                      # a uniform device batch
        bufs += [ut, uu]

        def rows(pages):                                                              # two sizes on one canvas; page 1 a window with an odd row stride
            out = []
            for k, p in enumerate([pages[0], pages[1][:wh, :ww]]):
                ph, pw = p.shape[:2]
                stride = pw * 3 + (7 if k == 1 else 0)
                host = np.full((ph, stride), 0xAB, np.uint8)
                host[:, :pw * 3] = np.ascontiguousarray(p).reshape(ph, pw * 3)
                b = _dev(host)
                bufs.append(b)
                out.append((b, ph, pw, stride if k == 1 else 0))
            return out
        # (the window of the tilted page is not the tilt of the window: its own upright page comes from the restatement)
        win = np.ascontiguousarray(tilted[1][:wh, :ww])
        win_ref = R.deskew_ref(win, M, G, INK)
        rt, ru = rows(tilted), rows([upright[0], np.pad(win_ref["image"], ((0, h - wh), (0, w - ww), (0, 0)))])
        want_uni, want_mix = eng.pages_to_data_dev(uu, 2, h, w, conf=True), eng.pages_to_data_dev_v(ru, conf=True)
        with deskew_on(eng, True, tables=True):
            got_uni, got_mix = eng.pages_to_data_dev(ut, 2, h, w, conf=True), eng.pages_to_data_dev_v(rt, conf=True)
            streamed = []
            for push in (lambda: eng.stream_push_v(rt, conf=True), lambda: eng.stream_push(ut, 2, h, w, conf=True), lambda: eng.stream_push_v(rt[::-1], conf=True),
                         lambda: eng.stream_push(ut, 2, h, w, conf=True), lambda: eng.stream_push_v(rt, conf=True)):
                r = push()
                if r:
                    streamed.append(r)
            with pytest.raises(EngineError, match="streamed batches are in flight"):  # the setter and the stage call refuse while batches stream
                eng.set_deskew(False)
            with pytest.raises(EngineError, match="streamed batches are in flight"):
                eng.deskew_page(tilted[0])
            while True:
                r = eng.stream_flush(conf=True)
                if not r:
                    break
                streamed.append(r)
        for a, b, n in zip(got_uni, want_uni, names):
            assert len(a) >= 8 and a.item_cell is not None and a.line is not None and a.block is not None, n
            assert_same_result(a, b, n)
            assert a.skew == pairs[n][2]
        assert_same_result(got_mix[0], want_mix[0], "mixed 0")
        assert_same_result(got_mix[1], want_mix[1], "mixed 1: a window")
        assert got_mix[1].item_cell is not None and got_mix[1].skew == win_ref["skew"] and (got_mix[1].skew["w"], got_mix[1].skew["h"]) == (ww, wh)
        if family == "form":
            assert all(len(r.cells) >= 1 and (r.item_cell >= 0).any() for r in got_uni)       # tables were found, and words lie in their cells
        assert len(streamed) == 5
        for a, b in zip(streamed, [got_mix, got_uni, got_mix[::-1], got_uni, got_mix]):
            for x, y in zip(a, b):
                assert x.item_cell is not None
                assert_same_result(x, y, "streamed")
                assert x.skew == y.skew
    finally:
        eng.set_tables(False)
        for b in bufs:
            b.free()


def test_sixteen_pages_sixteen_slopes(eng):
    """one uniform device batch of 16 pages, each with its own slope (one of them straight): every page is read as its own upright page"""
    page = R.columns_page()
    slopes = (-60, -45, -31, -25, -18, -9, -5, 0, 5, 7, 12, 18, 27, 37, 50, 64)
    tilted = [R.tilt(page, s) if s else page for s in slopes]
    refs = [R.deskew_ref(t, M, G, INK) for t in tilted]
    assert [r["skew"]["slope"] for r in refs] == list(slopes)
    h, w = page.shape[:2]
    bt, bu = _dev(np.stack(tilted)), _dev(np.stack([r["image"] for r in refs]))
    try:
        want = eng.pages_to_data_dev(bu, 16, h, w, conf=True)
        with deskew_on(eng):
            got = eng.pages_to_data_dev(bt, 16, h, w, conf=True)
    finally:
        bt.free()
        bu.free()
    for a, b, r in zip(got, want, refs):
        assert_same_result(a, b, r["skew"]["slope"])
        assert a.skew == r["skew"]


def test_an_upright_page_keeps_every_bit(eng, funsd):
    off = eng.images_to_data([funsd], conf=True)[0]
    with deskew_on(eng):
        on = eng.images_to_data([funsd], conf=True)[0]
    assert_same_result(on, off)
    assert on.skew["slope"] == 0 and on.skew["mode"] == 0 and (on.skew["C"], on.skew["S"]) == (65536, 0) and on.skew["degrees"] == 0.0
    assert on[0]["quad_page"] == on[0]["quad"]


def test_tables_give_every_word_its_cell_again(eng):
    """the form tilted by slope 45, tables on: with the layer on item_cell is the upright page's assignment; with it off it is another"""
    tilted = R.tilt(R.form_page(words=True), 45)
    ref = R.deskew_ref(tilted, M, G, INK)
    eng.set_tables(True)
    try:
        want = eng.images_to_data([ref["image"]])[0]
        off = eng.images_to_data([tilted])[0]
        with deskew_on(eng, True, tables=True):
            on = eng.images_to_data([tilted])[0]
    finally:
        eng.set_tables(False)
    assert len(want.cells) >= 1 and (want.item_cell >= 0).any()
    assert np.array_equal(on.item_cell, want.item_cell) and np.array_equal(on.item_table, want.item_table)
    # layer off: the tilted page's words, taken to the upright frame by the inverse of the map back and matched to the upright page's words by their centres
    assert off.item_cell is not None and len(off.cells) >= 1
    c_off = R.from_page(ref["skew"], off.quad.reshape(-1, 4, 2).mean(axis=1))
    c_want = want.quad.reshape(-1, 4, 2).mean(axis=1)
    moved = matched = 0
    for k, c in enumerate(c_off):
        d = np.abs(c_want - c).max(axis=1)
        j = int(d.argmin())
        if d[j] <= 4.0 and want.item_cell[j] >= 0:
            matched += 1
            moved += int(off.item_cell[k] != want.item_cell[j])
    print("words matched", matched, "in another cell with the layer off", moved)
    assert matched >= 20 and moved >= 1


def test_skew_to_page_and_quad_page_against_the_restatement(eng, pairs):
    import math
    tilted, _, want = pairs["form -45"]
    with deskew_on(eng):
        on = eng.images_to_data([tilted])[0]
    assert on.skew == want and on.skew["degrees"] == math.degrees(math.atan(-45 / 512.0))
    back = R.to_page(want, on.quad.reshape(-1, 4, 2))                                 # float64
    assert np.array_equal(on.to_page(on.quad.reshape(-1, 4, 2)), back.astype(np.float32))
    assert on.quad_page.shape == on.quad.shape and np.array_equal(on.quad_page.reshape(-1, 4, 2), back.astype(np.float32))   # (ttr_result_to_page; skew: ttr_results_gather_skew)
    for j in (0, len(on) - 1):
        assert np.array_equal(np.array(on[j]["quad_page"], np.float32), back[j].astype(np.float32))
    assert np.abs(back - on.quad.reshape(-1, 4, 2)).max() > 5.0                       # (the map moves points: no identity passes here)


def test_views_with_the_layer_off(eng, funsd):
    r = eng.images_to_data([funsd])[0]
    assert eng.deskew is None and r.skew is None and "quad_page" not in r[0]
    pts = np.array([[1.5, 2.5], [100.0, 7.0]], np.float32)
    assert np.array_equal(r.to_page(pts), pts)


def test_tiled_pages_read_the_upright_page(eng):
    from tuatara_amd import synth
    tilted = R.tilt(synth.synthetic_page(7, 1300, 1100, n_words=60), 18)
    ref = R.deskew_ref(tilted, M, G, INK)
    assert ref["skew"]["slope"] != 0
    eng.set_tiled(128)
    try:
        want = eng.images_to_data([ref["image"]], conf=True)[0]
        with deskew_on(eng):
            got = eng.images_to_data([tilted], conf=True)[0]
    finally:
        eng.set_tiled(0)
    assert got.tiles == want.tiles == 4
    assert_same_result(got, want)
    assert got.skew == ref["skew"]


# ------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals(eng, eng_x4, pairs):
    from tuatara_amd.engine import Comm, EngineError
    page = pairs["columns 27"][0]
    for bad in ((129, 288, 128), (-1, 288, 128), (64, 255, 128), (64, 65536, 128), (64, 288, 0), (64, 288, 256)):
        with pytest.raises(EngineError, match="ttr_engine_set_deskew: max_slope must be 0 .off. or lie in 1..128"):
            eng.set_deskew(bad)
        assert eng.deskew is None
        with pytest.raises(EngineError, match="max_slope must lie in 1..128"):
            eng.deskew_page(page, *bad)
    with pytest.raises(EngineError, match="8192 px or more"):
        eng.deskew_page(np.full((2, 8192, 3), 255, np.uint8))
    wide = _dev(np.full((40, 8192, 3), 255, np.uint8))
    buf = _dev(page)
    h, w = page.shape[:2]
    try:
        with deskew_on(eng, (5, 300, 90)):
            assert eng.deskew == (5, 300, 90)
            with pytest.raises(EngineError, match="deskew: a page side of 8192 px or more"):
                eng.pages_to_data_dev(wide, 1, 40, 8192)
        assert eng.deskew is None
        eng_x4.set_deskew(True)                                                       # region calls run as before (an engine without lines: regions refuse those)
        try:
            plain = eng_x4.read_regions(page, [{"rect": (20, 24, 160, 60)}])
        finally:
            eng_x4.set_deskew(False)
        again = eng_x4.read_regions(page, [{"rect": (20, 24, 160, 60)}])
        assert len(plain) == 1 and plain[0]["text"] == again[0]["text"] and plain[0]["quad"] == again[0]["quad"] and "quad_page" not in plain[0]
        comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
        try:
            comm.attach(True)
            try:
                with pytest.raises(EngineError, match="ttr_engine_set_deskew: pages are straightened by one engine alone, and a communicator is attached"):
                    eng.set_deskew(True)
                assert eng.deskew is None
            finally:
                comm.attach(False)
            with deskew_on(eng):
                with pytest.raises(EngineError, match="ttr_engine_attach_comm: pages are straightened by one engine alone"):
                    comm.attach(True)
                with pytest.raises(EngineError, match="latency mode does not support deskew"):
                    comm.pages_to_data_sharded(buf, 1, h, w)
        finally:
            comm.close()
    finally:
        wide.free()
        buf.free()


# ------------------------------------------------------------------------------------------------- 4. callers
def test_pytuatara_ocr_cli_and_the_environment(eng_x4, weights, pairs, monkeypatch, tmp_path):
    import math
    import os
    import subprocess
    import sys
    from PIL import Image
    from tests.conftest import ROOT
    from tuatara_amd import build as B
    B.build_pytuatara()
    B.build_examples()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in [k for k in os.environ if k.startswith("TUATARA_")]:
        monkeypatch.delenv(k, raising=False)
    tilted, upright, skew = pairs["columns 27"]
    want = eng_x4.images_to_data([upright])[0]                                        # the callers' engine: plain crops
    want_bgr = eng_x4.images_to_data([np.ascontiguousarray(upright[:, :, ::-1])])[0]  # (the CLI feeds BGR; the rule treats the channels alike)
    off = pytuatara.image_to_data(tilted, weights["dir"], "o")
    on = pytuatara.image_to_data(tilted, weights["dir"], "o", deskew=True)
    assert [(d["text"], d["bbox"]) for d in on] == [(t, b.tolist()) for t, b in zip(want.texts, want.bbox)]
    assert [(d["text"], d["bbox"]) for d in on] != [(d["text"], d["bbox"]) for d in off]
    assert [d["bbox"] for d in pytuatara.image_to_data(tilted, weights["dir"], "o", deskew=(64, 288, 128))] == [d["bbox"] for d in on]
    got_skew = pytuatara.last_call_skew()                                             # the call's own record, and its map back
    assert {k: got_skew[k] for k in ("slope", "found", "C", "S", "w", "h", "mode")} == {k: skew[k] for k in ("slope", "found", "C", "S", "w", "h", "mode")}
    assert got_skew["degrees"] == pytest.approx(skew["degrees"], abs=1e-12)
    corners = [(float(d["bbox"][0]), float(d["bbox"][1])) for d in on]
    assert np.array_equal(np.array(pytuatara.last_call_to_page(corners), np.float32), R.to_page(skew, np.array(corners, np.float32)).astype(np.float32))
    assert [d["bbox"] for d in pytuatara.image_to_data(tilted, weights["dir"], "o")] == [d["bbox"] for d in off]   # the call's setting is gone afterwards
    assert pytuatara.last_call_skew() is None and pytuatara.last_call_to_page([(3.0, 4.0)]) == [(3.0, 4.0)]
    with pytest.raises(RuntimeError, match="max_slope must be 0 .off. or lie in 1..128"):
        pytuatara.image_to_data(tilted, weights["dir"], "o", deskew=(129, 288, 128))
    monkeypatch.setenv("TUATARA_DESKEW", "1")                                         # the C++ switch
    assert [d["bbox"] for d in pytuatara.image_to_data(tilted, weights["dir"], "o")] == [d["bbox"] for d in on]
    monkeypatch.delenv("TUATARA_DESKEW")
    png = str(tmp_path / "page.png")
    Image.fromarray(tilted).save(png)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    cli = os.path.join(B.ROOT, "build", "examples", "ocr_cli")
    out = subprocess.run([cli, "--deskew", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    assert lines[0] == "# page 0 slope %d degrees %.4f found %d" % (skew["slope"], math.degrees(math.atan(skew["slope"] / 512.0)), skew["found"])
    assert [ln.split("\t")[1] for ln in lines[1:] if ln] == list(want_bgr.texts)
    mapped = np.array([[float(v) for v in ln.split("\t")[2].split()] for ln in lines[1:] if ln], np.float32)   # PageSkew::to_page on every box's first corner
    assert np.array_equal(mapped, R.to_page(skew, want_bgr.bbox[:, :2].astype(np.float32)).astype(np.float32))
    bad = subprocess.run([cli, "--deskew", "129", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert bad.returncode != 0 and "1..128" in bad.stderr
