"""GPU suite: tiled pages (ttr_engine_set_tiled; tuatara_amd/csrc/tiles.hip, engine_pages.cpp: detect_enqueue; DESIGN.md "Tiled pages").

An engine of its own with canvas_size = 256 and overlap 64 reads pages larger than its canvas as tiles: 448 x 640 (2 x 3 tiles), 500 x 700 (3 x 4, ragged on
both axes: last origins 256 and 448), 256 x 700 (1 x 4) and 200 x 256 (one tile) - FUNSD windows and a synthetic page; one synthetic page of 1300 x 1100 runs
at the default canvas under overlap 128 (2 x 2 tiles).  Held here: the stitch kernel against the host rule bit for bit; every tile's canvas; the page map
against the numpy stitch of the tiles' own maps; image_to_data against the composition of the existing stage calls on that map and against the CPU oracle;
the other entry points, lines + chars, and every refusal.  Fails on the parent commit, which has no ttr_engine_set_tiled."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tiles_ref as R
from tests.conftest import ROOT
from tests.test_gpu_images import _same
from tests.test_gpu_mixed import _conf_close, _equal

pytestmark = pytest.mark.gpu

S, O = 256, 64


def make_pages(funsd):
    """name -> (page, tiles ny x nx).  The FUNSD windows and the synthetic seed were chosen on the CPU with the oracle path alone (oracle_tiled below): every
    multi-tile page yields at least 8 words, at least one of them across a seam centre - both asserted again in test_end_to_end."""
    from tuatara_amd import synth
    return {
        "funsd 448 x 640": (np.ascontiguousarray(funsd[80:528, 60:700]), (2, 3)),
        "funsd 500 x 700": (np.ascontiguousarray(funsd[300:800, 30:730]), (3, 4)),
        "synth 256 x 700": (synth.synthetic_page(5, 256, 700, n_words=12), (1, 4)),
        "funsd 200 x 256": (np.ascontiguousarray(funsd[100:300, 100:356]), (1, 1)),
    }


def tile_windows(page, p):
    return [page[p.oy[ty]:p.oy[ty] + p.ey[ty], p.ox[tx]:p.ox[tx] + p.ex[tx]] for ty in range(p.ny) for tx in range(p.nx)]


def tile_canvases_ref(page, p):
    """the detector's canvas of every tile: the window's bytes in the detector's channel order (tuatara.cpp:349), zeros behind"""
    out = np.zeros((p.ny * p.nx, p.Hc, p.Wc, 3), np.uint8)
    for k, win in enumerate(tile_windows(page, p)):
        out[k, :win.shape[0], :win.shape[1]] = win[:, :, ::-1]
    return out


def seam_centres(p):
    """seam centres in image pixels: (ys, xs)"""
    return [2 * c for c in R.seams(p.oy, p.Hc // 2)], [2 * c for c in R.seams(p.ox, p.Wc // 2)]


def crossing(boxes, p):
    """how many boxes [n, 5] (image units) have a bounding rect that crosses a seam centre"""
    from oracle import post
    ys, xs = seam_centres(p)
    n = 0
    for b in boxes:
        x, y, w, h = post.bounding_rect(b)
        n += any(x < c < x + w for c in xs) or any(y < c < y + h for c in ys)
    return n


def oracle_tiled(craft, parseq, page, p):
    """the CPU oracle of a tiled page: oracle.pipeline.craft_heatmap per tile canvas, the numpy stitch, oracle.post.get_detected_boxes on the page map, then
    the reference's crop / recognise / decode steps at ratio 1 -> (boxes [n, 5], result dicts)"""
    from oracle import pipeline, post
    maps = np.stack([pipeline.craft_heatmap(craft, c) for c in tile_canvases_ref(page, p)])
    heat = R.stitch(maps, p.oy, p.ox, p.Hc, p.Wc, p.H2, p.W2)
    det, _, _ = post.get_detected_boxes(heat[:, :, 0], heat[:, :, 1])
    boxes = post.adjust_result_coordinates(det, 1.0, 1.0)
    swapped = np.ascontiguousarray(page[:, :, ::-1])
    crops, keep = [], []
    for i, b in enumerate(boxes):
        c = post.crop_resize(swapped, b, True)
        if c is not None:
            crops.append(c)
            keep.append(i)
    crops = np.stack(crops) if crops else np.zeros((0, 32, 128, 3), np.uint8)
    texts, _ = post.decode_logits(pipeline.parseq_logits(parseq, crops))
    return boxes[keep], [{"text": t, "bbox": post.tesseract_bbox(boxes[i])} for t, i in zip(texts, keep)]


def _engine(weights, **kw):
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine

    build_lib()
    return Engine(weights["dir"], **kw)


@pytest.fixture(scope="module")
def eng(weights):
    """canvas_size 256, tiling OFF at rest: every test that turns it on turns it off again"""
    return _engine(weights, canvas_size=S, mixed_batches=1)


@pytest.fixture(scope="module")
def pages(funsd):
    return make_pages(funsd)


@pytest.fixture(scope="module")
def ref_maps(eng, pages):
    """name -> (plan, page map): the numpy stitch of eng.craft_heatmap on every tile canvas alone.  Computed once, shared, never written to."""
    out = {}
    for name, (page, _) in pages.items():
        p = eng.tile_plan(page.shape[0], page.shape[1], O)
        maps = np.stack([eng.craft_heatmap(c) for c in tile_canvases_ref(page, p)])
        m = R.stitch(maps, p.oy, p.ox, p.Hc, p.Wc, p.H2, p.W2)
        m.setflags(write=False)
        out[name] = (p, m)
    return out


class tiled:
    def __init__(self, eng, overlap=O):
        self.eng, self.overlap = eng, overlap

    def __enter__(self):
        self.eng.set_tiled(self.overlap)
        return self.eng

    def __exit__(self, *a):
        self.eng.set_tiled(0)


# ---------------------------------------------------------------- 1: the stitch kernel alone
@pytest.mark.parametrize("h,w,shape", [(448, 640, (2, 3)), (500, 700, (3, 4)), (256, 700, (1, 4))])
def test_stitch_kernel_equals_the_host_rule_bit_for_bit(eng, h, w, shape):
    from tuatara_amd import engine as E
    p = eng.tile_plan(h, w, O)
    assert (p.ny, p.nx) == shape
    t = R.seeded_tiles(11 + h, p.tiles, p.Hc // 2, p.Wc // 2, pages=2)               # (the maps tests/test_tiles_cpu.py holds the host rule to numpy on)
    ref = E.stitch_tiles(t, p.oy, p.ox, p.Hc, p.Wc, p.H2, p.W2)
    got = eng.stitch_heat(t, p.oy, p.ox, p.Hc, p.Wc, p.H2, p.W2)
    diff = got.view(np.uint32) != ref.view(np.uint32)
    print(f"stitch {h} x {w}: {int(diff.sum())} of {diff.size} words differ; NaN in {int(np.isnan(ref).sum())}")
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], ref[diff][:4])


# ---------------------------------------------------------------- 2: the tiles' canvases
def test_every_tile_canvas_is_its_windows_bytes(eng, pages):
    for name, (page, shape) in pages.items():
        p = eng.tile_plan(page.shape[0], page.shape[1], O)
        assert (p.ny, p.nx) == shape, name
        got = eng.tile_canvases(page, O)
        assert np.array_equal(got, tile_canvases_ref(page, p)), name
        if p.tiles == 1:                                                             # one tile: the canvas of the engine with tiling off
            assert np.array_equal(got[0], eng.resize_canvas(page)[0]), name


# ---------------------------------------------------------------- 3: the page map
def test_page_map_is_the_stitch_of_the_tiles_own_maps(eng, pages, ref_maps):
    for name, (page, _) in pages.items():
        p, ref = ref_maps[name]
        got = eng.craft_heatmap_tiled(page, O)
        assert got.shape == (p.H2, p.W2, 2) and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), name


# ---------------------------------------------------------------- 4: end to end
def _stage_reference(eng, page, heat):
    """the existing stage calls on a page map: ccl_boxes -> pack_crops at ratio 1 -> parseq_logits (+ the final decode for conf)"""
    from oracle import post
    rects = eng.ccl_boxes(np.array(heat))
    crops, boxes = eng.pack_crops(page, rects, 1.0)
    logits, ids = eng.parseq_logits(crops)
    _, _, conf = eng.logits_confidence(logits)
    ref = [{"text": None, "bbox": post.tesseract_bbox(b), "ids": np.asarray(ids).reshape(-1, 26)[i].tolist(), "conf": float(conf[i])} for i, b in enumerate(boxes)]
    return boxes, ref


def _same_boxes_and_ids(got, ref):
    return [g["bbox"] for g in got] == [r["bbox"] for r in ref] and [g["ids"] for g in got] == [r["ids"] for r in ref]


def test_end_to_end_equals_the_stage_calls_and_the_oracle(eng, pages, ref_maps, oracle_models):
    craft, parseq = oracle_models
    for name, (page, _) in pages.items():
        p, heat = ref_maps[name]
        boxes, ref = _stage_reference(eng, page, heat)
        with tiled(eng):
            got = eng.image_to_data(page, conf=True)
            raw = eng.images_to_data([page])[0]
        assert raw.tiles == p.tiles, name
        assert len(got) == len(ref) and _same_boxes_and_ids(got, ref) and _conf_close(got, ref), name
        obox, oref = oracle_tiled(craft, parseq, page, p)
        print(f"{name}: {len(got)} words, {crossing(boxes, p)} across a seam centre; oracle {len(oref)} words")
        assert np.array_equal(np.array([g["bbox"] for g in got]), np.array([r["bbox"] for r in oref])), name
        assert [g["text"] for g in got] == [r["text"] for r in oref], name
        if p.tiles > 1:                                                              # the seeds: enough words, and a seam that matters
            assert len(got) >= 8 and crossing(boxes, p) >= 1, (name, len(got), crossing(boxes, p))
            assert len(oref) >= 8 and crossing(obox, p) >= 1, name


def test_default_canvas_page_of_2_x_2_tiles(eng_x4):
    """1300 x 1100 at canvas_size 1024 under overlap 128: origins 0 / 288 and 0 / 96"""
    from tuatara_amd import synth
    page = synth.synthetic_page(7, 1300, 1100, n_words=60)
    p = eng_x4.tile_plan(1300, 1100, 128)
    assert (p.ny, p.nx, p.oy, p.ox, p.Hc, p.Wc) == (2, 2, [0, 288], [0, 96], 1024, 1024)
    maps = np.stack([eng_x4.craft_heatmap(c) for c in tile_canvases_ref(page, p)])
    heat = R.stitch(maps, p.oy, p.ox, p.Hc, p.Wc, p.H2, p.W2)
    assert np.array_equal(eng_x4.craft_heatmap_tiled(page, 128).view(np.uint32), heat.view(np.uint32))
    boxes, ref = _stage_reference(eng_x4, page, heat)
    off = eng_x4.image_to_data(page, conf=True)                                      # tiling off: the page shrunk onto the canvas
    with tiled(eng_x4, 128):
        got = eng_x4.image_to_data(page, conf=True)
        assert eng_x4.canvas_geometry(1300, 1100) == (1312, 1120, 1.0)
    assert eng_x4.tiled == 0 and eng_x4.canvas_geometry(1300, 1100)[:2] == (1024, 896)
    assert len(got) >= 8 and crossing(boxes, p) >= 1
    assert _same_boxes_and_ids(got, ref) and _conf_close(got, ref)
    assert [list(m) for m in [eng_x4.image_to_data(page, conf=True)]] == [list(m) for m in [off]]   # off again: the bits of before


# ---------------------------------------------------------------- 5: the other entry points and modes
def test_one_tile_page_and_tiling_off_keep_their_bits(eng, pages):
    small, big = pages["funsd 200 x 256"][0], pages["funsd 448 x 640"][0]
    off_small, off_big = eng.image_to_data(small, conf=True), eng.image_to_data(big, conf=True)
    with tiled(eng):
        on_small = eng.image_to_data(small, conf=True)
        assert eng.images_to_data([small])[0].tiles == 1
        assert eng.canvas_geometry(200, 256) == (224, 256, 1.0) and eng.canvas_geometry(448, 640) == (448, 640, 1.0)
    assert len(off_small) > 0 and on_small == off_small                               # every field, conf included: the same launches
    assert eng.image_to_data(big, conf=True) == off_big and eng.images_to_data([big])[0].tiles == 0
    assert eng.canvas_geometry(448, 640)[:2] == (192, 256)


def test_batches_streams_and_lists_equal_the_single_calls(eng, pages, funsd):
    from tuatara_amd.engine import DeviceBuffer, EngineError
    trio = [np.ascontiguousarray(funsd[y:y + h, x:x + w]) for (y, x, h, w) in [(80, 60, 448, 640), (200, 40, 440, 630), (400, 100, 425, 615)]]   # one page canvas 448 x 640
    with tiled(eng):
        singles = [eng.image_to_data(p, conf=True) for p in trio]
        assert all(len(s) >= 8 for s in singles)
        bufs, rows = [], []
        for k, p in enumerate(trio):
            h, w = p.shape[:2]
            stride = w * 3 + (7 if k == 1 else 0)                                   # page 1: a padded row stride
            host = np.full((h, stride), 0xAB, np.uint8)
            host[:, :w * 3] = p.reshape(h, w * 3)
            b = DeviceBuffer(host.nbytes)
            b.upload(host)
            bufs.append(b)
            rows.append((b, h, w, stride if k == 1 else 0))
        got = eng.pages_to_data_dev_v(rows, conf=True)
        for g, s in zip(got, singles):
            assert _equal(g, s) and _conf_close(g, s)
        same = np.stack([trio[0]] * 3)                                               # the uniform entry point: three equal pages
        ub = DeviceBuffer(same.nbytes)
        ub.upload(same)
        uni = eng.pages_to_data_dev(ub, 3, 448, 640, conf=True)
        for g in uni:
            assert _equal(g, singles[0]) and _conf_close(g, singles[0])
        streamed = []
        for push in (lambda: eng.stream_push_v(rows, conf=True), lambda: eng.stream_push(ub, 3, 448, 640, conf=True), lambda: eng.stream_push_v(rows[::-1], conf=True)):
            r = push()
            if r:
                streamed.append(r)
        with pytest.raises(EngineError, match="streamed batches are in flight"):     # the setter and the stage twin refuse while batches stream
            eng.set_tiled(0)
        with pytest.raises(EngineError, match="streamed batches are in flight"):
            eng.stitch_heat(np.zeros((1, 128, 128, 2), np.float32), [0], [0], 256, 256, 128, 128)
        while True:
            r = eng.stream_flush(conf=True)
            if not r:
                break
            streamed.append(r)
        assert len(streamed) == 3
        for a, b in zip(streamed, [got, uni, got[::-1]]):
            assert [list(m) for m in a] == [list(m) for m in b]
        lst = eng.images_to_data(trio + [pages["funsd 200 x 256"][0]], conf=True)    # the list form buckets by page canvas: 448 x 640 three times, 224 x 256 once
        assert eng.last_images_batches() == [3, 1]
        for g, s in zip(lst[:3], singles):
            assert _equal(g, s) and _conf_close(g, s)
        assert [r.tiles for r in lst] == [6, 6, 6, 1]
        with pytest.raises(EngineError, match=r"page 1 \(200 x 256\) has canvas 224 x 256, page 0 \(448 x 640\) has canvas 448 x 640"):
            small = DeviceBuffer(200 * 256 * 3)
            bufs.append(small)
            eng.pages_to_data_dev_v([rows[0], (small, 200, 256, 0)])
    for b in bufs + [ub]:
        b.free()


def test_lines_and_chars_ride_along(weights, pages):
    from tuatara_amd import engine as E
    page = pages["funsd 500 x 700"][0]
    e = _engine(weights, canvas_size=S, crop_mode=1, lines=1, chars=1, tiled=O)
    assert e.tiled == O
    res = e.images_to_data([page], conf=True)[0]
    assert res.tiles == 12 and len(res) >= 8
    line, word, n_lines = E.lines_from_quads(res.quad)
    assert np.array_equal(res.line, line) and np.array_equal(res.word, word) and len(res.line_first) == n_lines + 1
    assert res.char_first is not None and len(res.char_first) == len(res) + 1 and int(res.char_first[-1]) > 0 and len(res.char_quad) == int(res.char_first[-1])
    w, h = page.shape[1], page.shape[0]
    assert res.char_bbox[:, 0].min() >= -1 and res.char_bbox[:, 2].max() <= w + 1 and res.char_bbox[:, 3].max() <= h + 1


def test_refusals(eng, weights, pages):
    from tuatara_amd.engine import Comm, DeviceBuffer, EngineError
    for bad, msg in [(48, "got 48"), (32, "got 32"), (96, r"canvas_size / 4 = 64\], got 96"), (-64, "got -64")]:
        with pytest.raises(EngineError, match="ttr_engine_set_tiled: tiled pages: the overlap must be a multiple of 32.*" + msg):
            eng.set_tiled(bad)
        assert eng.tiled == 0
    with pytest.raises(EngineError, match="mag_ratio must be 1.0"):
        _engine(weights, canvas_size=S, mag_ratio=1.5, tiled=O)
    with pytest.raises(EngineError, match="canvas_size must be a positive multiple of 32, got 250"):
        _engine(weights, canvas_size=250, tiled=O)
    with tiled(eng):
        with pytest.raises(EngineError, match="at most 16 tiles per axis, the width 3400 needs 18"):
            eng.image_to_data(np.full((64, 3400, 3), 255, np.uint8))
        with pytest.raises(EngineError, match="at most 64 tiles per page, 1800 x 1800 needs 10 x 10 = 100"):
            eng.image_to_data(np.full((1800, 1800, 3), 255, np.uint8))
        assert len(eng.image_to_data(pages["funsd 448 x 640"][0])) >= 8             # the engine works afterwards
    # a communicator: the setter refuses with one attached; with tiling on, attaching and the sharded call refuse
    buf = DeviceBuffer(448 * 640 * 3)
    buf.upload(pages["funsd 448 x 640"][0])
    comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
    try:
        comm.attach(True)
        try:
            with pytest.raises(EngineError, match="ttr_engine_set_tiled: tiled pages are read by one engine alone, and a communicator is attached"):
                eng.set_tiled(O)
            assert eng.tiled == 0
        finally:
            comm.attach(False)
        with tiled(eng):
            with pytest.raises(EngineError, match="ttr_engine_attach_comm: tiled pages are read by one engine alone"):
                comm.attach(True)
            with pytest.raises(EngineError, match="latency mode does not support tiled pages"):
                comm.pages_to_data_sharded(buf, 1, 448, 640)
    finally:
        comm.close()
        buf.free()


# ---------------------------------------------------------------- 6: callers
def test_pytuatara_ocr_cli_and_the_environment(eng_x4, weights, monkeypatch, tmp_path):
    from PIL import Image
    from tuatara_amd import build as B, synth
    B.build_pytuatara()
    B.build_examples()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in [k for k in os.environ if k.startswith("TUATARA_")]:
        monkeypatch.delenv(k, raising=False)
    page = synth.synthetic_page(7, 1300, 1100, n_words=60)
    off = eng_x4.image_to_data(page)
    with tiled(eng_x4, 128):
        want = eng_x4.image_to_data(page)
        want_bgr = eng_x4.image_to_data(np.ascontiguousarray(page[:, :, ::-1]))       # (the CLI feeds BGR)
    assert len(want) >= 8 and not _same(want, off)                                    # the page at full size is not the page shrunk onto the canvas
    assert _same(pytuatara.image_to_data(page, weights["dir"], "o", tiled=True), want)
    assert _same(pytuatara.image_to_data(page, weights["dir"], "o", tiled=128), want)
    assert _same(pytuatara.image_to_data(page, weights["dir"], "o"), off)             # the call's setting is gone afterwards
    monkeypatch.setenv("TUATARA_TILED", "1")
    assert _same(pytuatara.image_to_data(page, weights["dir"], "o"), want)
    monkeypatch.delenv("TUATARA_TILED")
    with pytest.raises(RuntimeError, match="multiple of 32"):
        pytuatara.image_to_data(page, weights["dir"], "o", tiled=48)
    with pytest.raises(ValueError, match="regions"):
        pytuatara.image_to_data(page, weights["dir"], "o", tiled=True, regions=[{"rect": (5, 5, 200, 25)}])
    with pytest.raises(RuntimeError, match="at most 8192 pixels, got 8200"):
        pytuatara.image_to_data(np.full((40, 8200, 3), 255, np.uint8), weights["dir"], "o", tiled=True)
    png = str(tmp_path / "page.png")
    Image.fromarray(page).save(png)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    cli = os.path.join(B.ROOT, "build", "examples", "ocr_cli")
    out = subprocess.run([cli, "--tiled", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    items = [ln.split("\t") for ln in out.stdout.splitlines()]
    assert len(items) == len(want_bgr)
    for (bb, text), w in zip(items, want_bgr):
        assert [float(v) for v in bb.split()] == list(w["bbox"]) and text == w["text"]
    bad = subprocess.run([cli, "--tiled", "48", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert bad.returncode == 1 and "multiple of 32 in [64, 256]" in bad.stderr
