"""GPU suite for word orientation (ttr_config.orient; DESIGN.md "Word orientation"): the oriented crops (pack_crops_rect_kernel on turned
quads) against the numpy restatement tests/orient_ref.py bit for bit, the orient engines against the orient = 0 engine (same items, turn 0
bit for bit), the twins' confidences against the recogniser run on exactly the twin batch, the choice (orient_select_kernel) against the
host rule, every entry point against the single-page call, the page mode, the sharded mode's refusal and the callers (pytuatara, ocr_cli)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import orient_ref as O
from tests.conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

MODES = [(o, m) for o in (1, 2) for m in (0, 1)]      # (orient: FLIP / QUARTER) x crop_mode


@pytest.fixture(scope="module")
def engines(weights):
    """engines by (orient, crop_mode, orient_page), made on first use (default precision, f16x4)"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine
    build_lib()
    cache = {}

    def get(orient, crop_mode, orient_page=0):
        key = (orient, crop_mode, orient_page)
        if key not in cache:
            cache[key] = Engine(weights["dir"], crop_mode=crop_mode, orient=orient, orient_page=orient_page)
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


@pytest.fixture(scope="module")
def pages():
    """an upright synthetic page, the same page upside down and turned by a quarter, and a page of tilted words"""
    from tuatara_amd import synth
    up = synth.synthetic_page(90, 512, 384, n_words=10)
    tilted = synth.synthetic_rotated_page(91, 512, 384, n_words=8, max_deg=30.0)[0]
    return [up, np.ascontiguousarray(np.rot90(up, 2)), np.ascontiguousarray(np.rot90(up, -1)), tilted]


def _batch(eng, imgs):
    """one synchronous batch of same-sized pages (run_pages) as PageResults"""
    from tuatara_amd.engine import DeviceBuffer
    a = np.ascontiguousarray(np.stack(imgs))
    buf = DeviceBuffer(a.nbytes)
    buf.upload(a)
    r = eng.pages_to_data_dev(buf, len(imgs), a.shape[1], a.shape[2])
    buf.free()
    return r


def _one(eng, img):
    """the single-page call (run_pages) as a PageResult"""
    return _batch(eng, [img])[0]


# ------------------------------------------------------------------------------------------------- the packer
def _check_oriented(eng, img, rects, ratio):
    from oracle import post
    boxes = post.adjust_result_coordinates(rects, 1.0 / ratio, 1.0 / ratio)
    for mode in (0, 1):
        for t in range(4):
            crops, quads = eng.pack_crops_oriented(img, rects, ratio, mode, t)
            for i, b in enumerate(boxes):
                ref, q = O.oriented_crop(img, b, mode, t)
                assert np.array_equal(crops[i], ref), (mode, t, i, b)
                assert np.array_equal(quads[i], q), (mode, t, i, b)
            if t == 0:                                                      # turn 0 is the crop mode's own stage entry point
                if mode == 0:
                    assert np.array_equal(crops, eng.pack_crops(img, rects, ratio)[0])
                else:
                    c1, q1 = eng.pack_crops_rectified(img, rects, ratio)
                    assert np.array_equal(crops, c1) and np.array_equal(quads, q1)


def test_pack_crops_oriented_equals_numpy(eng_x4, oracle_models, pages):
    from oracle import pipeline
    for page in pages:                                                     # detected boxes of upright, turned and tilted pages
        d = pipeline.detect(oracle_models[0], page)
        assert len(d["det"]) >= 4
        _check_oriented(eng_x4, page, d["det"], d["ratio"])
    # boxes touching every image edge (clamp), 1-px-thin boxes, on a colour page (heat-map units: x2 -> image pixels)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (300, 420, 3), dtype=np.uint8)
    rects = np.array([[0, 40, 40, 12, 20], [210, 75, 30, 10, -35], [100, 0, 50, 8, 12.5], [100, 150, 50, 8, -7], [0, 0, 30, 30, 45],
                      [210, 150, 25, 6, 60], [105, 75, 60, 0.5, 17], [105, 75, 0.5, 40, 3], [50, 100, 40, 0.5, 0], [80, 30, 20, 10, 90],
                      [150, 120, 70, 14, -80], [60, 60, 3, 2, 33], [0, 75, 12, 40, 0], [209, 149, 8, 8, 0]], np.float32)
    _check_oriented(eng_x4, img, rects, 1.0)


# ------------------------------------------------------------------------------------------------- the engine against orient = 0
def test_same_items_and_turn_zero_bits(engines, funsd, pages):
    off = {m: engines(0, m) for m in (0, 1)}
    for img in [funsd] + pages:
        base = {m: _one(off[m], img) for m in (0, 1)}
        for orient, mode in MODES:
            eng = engines(orient, mode)
            K = eng.orient_candidates
            r, b = _one(eng, img), base[mode]
            assert len(r) == len(b) > 0
            assert np.array_equal(r.bbox, b.bbox)
            if mode == 1:
                assert np.array_equal(r.quad, b.quad)
            assert r.orient_conf.shape == (len(r), K)
            assert r.orient_conf[:, 0].tobytes() == b.conf.tobytes()           # candidate column 0 = the orient = 0 reading, bit for bit
            z = r.orient == 0
            assert np.array_equal(r.ids[z], b.ids[z]) and r.prob[z].tobytes() == b.prob[z].tobytes() and r.conf[z].tobytes() == b.conf[z].tobytes()
            col = r.orient // (2 if K == 2 else 1)
            assert r.conf.tobytes() == r.orient_conf[np.arange(len(r)), col].tobytes()
            assert (r.conf[~z] > b.conf[~z]).all()                              # a turned reading wins only when it is strictly surer
            assert set(r.orient.tolist()) <= set(O.TURNS[K]) and r.page_orient in O.TURNS[K]
            assert [d["orient"] for d in r] == (90 * r.orient).tolist()
            print(f"orient={orient} crop_mode={mode} {img.shape}: {len(r)} words, turns {np.bincount(r.orient, minlength=4).tolist()}, page {r.page_orient}")


def test_twins_are_real_readings(engines, pages):
    """The engine's candidate confs for turns >= 1 are the recogniser's confs on exactly the twin batch, in the engine's row order
    (candidate-major over every word of the batch), for single pages and for a batch of two pages."""
    from oracle import post
    from tuatara_amd.engine import orient_select
    for orient, mode in MODES:
        eng = engines(orient, mode)
        K = eng.orient_candidates
        for batch in ([pages[1]], [pages[2]], [pages[1], pages[3]]):
            res = _batch(eng, batch)
            t0 = _batch(engines(0, mode), batch)
            keep, first = [], [0]
            for img, r in zip(batch, res):      # the engine's own boxes, through its stage entry points (the same kernels as the batch)
                canvas, ratio = eng.resize_canvas(img)
                rects = eng.ccl_boxes(eng.craft_heatmap(canvas))
                boxes = post.adjust_result_coordinates(rects, 1.0 / ratio, 1.0 / ratio)
                kept = [b for b in boxes if (lambda c: c[2] > c[0] and c[3] > c[1])(O.clamped_rect(b, *img.shape[:2]))]
                assert len(kept) == len(r) > 0
                assert [post.tesseract_bbox(b) for b in kept] == r.bbox.tolist()
                keep += [(img, b) for b in kept]
                first.append(len(keep))
            N = len(keep)
            twins = np.stack([O.twin(img, b, mode, t)[0] for t in O.TURNS[K][1:] for img, b in keep])     # row (j - 1) N + c
            logits, _ = eng.parseq_logits(twins)
            ids, prob, conf = eng.logits_confidence(logits)
            cand = np.concatenate([r.orient_conf for r in res])
            got = cand[:, 1:].T.reshape(-1)                                 # (j - 1) N + c order
            assert got.tobytes() == conf.tobytes(), (orient, mode, len(batch), np.abs(got - conf).max())
            tids = ids.reshape(K - 1, N, 26).transpose(1, 0, 2)
            for pg, (r, r0) in enumerate(zip(res, t0)):
                c0, c1 = first[pg], first[pg + 1]
                # the choice: the host rule on the engine's own candidates (column 0 = the turn-0 reading of the orient = 0 engine)
                cand_ids = np.concatenate([r0.ids[:, None], tids[c0:c1]], 1)
                turns, pt = orient_select(r.orient_conf, cand_ids, False)
                assert np.array_equal(turns, r.orient) and pt == r.page_orient
                # the chosen ids and prob are the winning candidate's
                for c in range(c1 - c0):
                    j = O.TURNS[K].index(int(r.orient[c]))
                    if j:
                        assert np.array_equal(r.ids[c], ids[(j - 1) * N + c0 + c]) and r.prob[c].tobytes() == prob[(j - 1) * N + c0 + c].tobytes()


def test_every_entry_point_equals_the_single_page_call(engines, pages):
    """Every entry point that forms the same batch gives the same dicts.  (The twin pass holds the twins of every page of a batch, and the
    recogniser's logits can move in their last bits between batch compositions - DESIGN.md "Recognition confidence" -, so a multi-page
    batch is compared with the same batch through the other paths.)"""
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    small = np.ascontiguousarray(np.rot90(synth.synthetic_page(93, 384, 448, n_words=6), 2))
    for orient, mode in ((2, 0), (1, 1)):
        eng = engines(orient, mode)
        distinct = [pages[1], pages[2], small]                                 # three sizes: one page per batch
        single = [eng.image_to_data(p, conf=True) for p in distinct]
        assert all(len(s) > 0 and all("orient" in d for d in s) for s in single)
        many = eng.images_to_data(distinct, conf=True)                         # mixed sizes
        assert [list(m) for m in many] == single
        assert [list(_one(eng, p)) for p in distinct] == [[{k: v for k, v in d.items() if k not in ("conf", "char_conf")} for d in s] for s in single]
        two = [pages[0], pages[1]]
        buf = DeviceBuffer(2 * 512 * 384 * 3)
        buf.upload(np.stack(two))
        streamed = []
        for k in range(2):                                                      # one page per batch: the streamed pipeline's two slots
            streamed += eng.stream_push(buf.ptr + k * 512 * 384 * 3, 1, 512, 384, conf=True)
        while True:
            r = eng.stream_flush(conf=True)
            if not r:
                break
            streamed += r
        assert [list(m) for m in streamed] == [eng.image_to_data(p, conf=True) for p in two]
        assert [m.page_orient for m in streamed] == [_one(eng, p).page_orient for p in two]
        # a batch of two pages: the synchronous call, the list call and the streamed call form the same batch
        dev = eng.pages_to_data_dev(buf, 2, 512, 384, conf=True)
        assert [list(m) for m in eng.images_to_data(two, conf=True)] == [list(m) for m in dev]
        streamed = eng.stream_push(buf, 2, 512, 384, conf=True) + eng.stream_flush(conf=True) + eng.stream_flush(conf=True)
        assert [list(m) for m in streamed] == [list(m) for m in dev]
        assert [m.orient_conf.tobytes() for m in streamed] == [m.orient_conf.tobytes() for m in dev]
        assert eng.stream_flush() == []
        buf.free()


def test_page_mode_reports_the_page_turn(engines, pages):
    for img in pages:
        per_word, per_page = _one(engines(2, 0), img), _one(engines(2, 0, 1), img)
        assert len(per_page) == len(per_word) > 0
        assert (per_page.orient == per_page.page_orient).all()
        assert per_page.page_orient == per_word.page_orient                   # the same vote in both modes
        assert per_page.orient_conf.tobytes() == per_word.orient_conf.tobytes()
        assert per_page.conf.tobytes() == per_page.orient_conf[:, per_page.page_orient].tobytes()


def test_sharded_refuses_and_the_gather_carries_the_choice(engines, pages):
    from tuatara_amd.engine import Comm, DeviceBuffer, EngineError
    eng = engines(2, 0)
    buf = DeviceBuffer(2 * 512 * 384 * 3)
    buf.upload(np.stack(pages[:2]))
    single = eng.pages_to_data_dev(buf, 2, 512, 384)
    comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
    try:
        with pytest.raises(EngineError, match="word orientation"):
            comm.pages_to_data_sharded(buf, 2, 512, 384)
        comm.attach(True)
        res = eng.pages_to_data_dev(buf, 2, 512, 384)
        assert [list(r) for r in res] == [list(r) for r in single]
        _, ids = comm.last_gathered()
        conf, prob = comm.last_gathered_conf()
        assert np.array_equal(ids, np.concatenate([r.ids for r in res]))         # the gathered rows are the chosen readings
        assert conf.tobytes() == np.concatenate([r.conf for r in res]).tobytes()
        comm.attach(False)
    finally:
        comm.close()
        buf.free()


# ------------------------------------------------------------------------------------------------- callers
def test_pytuatara_orient_keyword(weights, engines, pages, monkeypatch):
    from tuatara_amd import build
    build.build_pytuatara()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ORIENT"):
        monkeypatch.delenv(k, raising=False)
    page = pages[1]
    plain = pytuatara.image_to_data(page, weights["dir"], "o")
    assert set(plain[0]) == {"text", "bbox"}
    for kw, key in (({"orient": "quarter"}, (2, 0, 0)), ({"orient": "flip", "rectify": True, "conf": True}, (1, 1, 0)),
                    ({"orient": "quarter", "orient_page": True}, (2, 0, 1))):
        got = pytuatara.image_to_data(page, weights["dir"], "o", **kw)
        want = engines(*key).image_to_data(page, conf=True)
        assert len(got) == len(want) > 0
        assert [(g["text"], list(g["bbox"]), g["orient"]) for g in got] == [(w["text"], w["bbox"], w["orient"]) for w in want]
        if kw.get("conf"):
            assert [g["conf"] for g in got] == [w["conf"] for w in want] and "quad" in got[0]
        assert pytuatara.images_to_data([page], weights["dir"], "o", **kw) == [got]
    with pytest.raises(Exception):
        pytuatara.image_to_data(page, weights["dir"], "o", orient="sideways")


def test_ocr_cli_orient_lines_match_the_python_dicts(weights, engines, tmp_path):
    from PIL import Image
    from tuatara_amd import build as B
    B.build_examples()
    env = {k: v for k, v in os.environ.items() if k not in ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ORIENT")}
    png = os.path.join(DATA, "funsd_0001129658.png")
    out = subprocess.run([os.path.join(B.ROOT, "build", "examples", "ocr_cli"), "--orient", png, weights["dir"], str(tmp_path)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = [ln.split("\t") for ln in out.stdout.splitlines()]
    rgb = np.array(Image.open(png).convert("RGB"))
    want = engines(2, 0).image_to_data(np.ascontiguousarray(rgb[:, :, ::-1]), conf=True)    # the CLI feeds BGR
    assert len(lines) == len(want) > 20
    for (bb, deg, conf, text), g in zip(lines, want):
        assert [float(v) for v in bb.split()] == g["bbox"] and text == g["text"]
        assert int(deg) == g["orient"] and conf == f"{g['conf']:.6f}"
