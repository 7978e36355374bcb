"""GPU suite for text lines (ttr_config.lines; DESIGN.md "Text lines"): line_group_kernel (ttr_group_lines) against the host rule
(ttr_lines_from_quads) bit for bit - several pages of different word counts in one launch, empty pages included, and 4096 words on a page -,
the lines = 1 engine against the lines = 0 engine (same items, every other output bit for bit), the returned lines against the host rule on
the result's own quads, every entry point against the single-page call, the sharded mode's refusal and the callers (pytuatara, ocr_cli).
Every test runs under a time limit of its own: a step that hangs ends the process instead of holding the GPU."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lines_ref as L
from tests.conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 600


@pytest.fixture(autouse=True)
def step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def engines(weights):
    """engines by (lines, crop_mode, orient), made on first use (default precision, f16x4)"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine
    build_lib()
    cache = {}

    def get(lines, crop_mode=0, orient=0):
        key = (lines, crop_mode, orient)
        if key not in cache:
            cache[key] = Engine(weights["dir"], crop_mode=crop_mode, orient=orient, lines=lines)
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


@pytest.fixture(scope="module")
def pages():
    """synthetic pages of one size: upright words in rows, a second one, and a page of tilted words"""
    from tuatara_amd import synth
    return [synth.synthetic_page(90, 512, 384, n_words=10), synth.synthetic_page(94, 512, 384, n_words=14),
            synth.synthetic_rotated_page(91, 512, 384, n_words=8, max_deg=30.0)[0]]


def _batch(eng, imgs, conf=False):
    from tuatara_amd.engine import DeviceBuffer
    a = np.ascontiguousarray(np.stack(imgs))
    buf = DeviceBuffer(a.nbytes)
    buf.upload(a)
    r = eng.pages_to_data_dev(buf, len(imgs), a.shape[1], a.shape[2], conf=conf)
    buf.free()
    return r


def _raw(eng, img):
    """one image through ttr_image_to_data, read with the per-result calls of the C ABI -> dict of arrays (and the texts)"""
    lib = eng.lib
    img = np.ascontiguousarray(img, np.uint8)
    arr = (C.c_void_p * 1)()
    assert lib.ttr_image_to_data(eng.h, img.ctypes.data_as(C.POINTER(C.c_uint8)), img.shape[0], img.shape[1], img.shape[1] * 3, arr) == 0
    r = arr[0]
    n, nl = lib.ttr_result_count(r), lib.ttr_result_line_count(r)

    def take(p, shape, dt):
        return np.ctypeslib.as_array(p, shape).astype(dt).copy() if p else None

    def text(fn, *a):
        need = fn(r, *a, None, 0)
        buf = C.create_string_buffer(max(need, 1))
        assert fn(r, *a, buf, need) == need
        return buf.raw[:need].decode("latin1")
    out = {"n": n, "n_lines": nl, "texts": [lib.ttr_result_text(r, i).decode("latin1") for i in range(n)],
           "bbox": take(lib.ttr_result_bboxes(r), (n, 4), np.float32), "quad": take(lib.ttr_result_quads(r), (n, 8), np.float32),
           "ids": take(lib.ttr_result_ids_all(r), (n, 26), np.int32), "prob": take(lib.ttr_result_probs_all(r), (n, 26), np.float32),
           "conf": take(lib.ttr_result_confs(r), (n,), np.float32),
           "line": take(lib.ttr_result_lines(r), (n,), np.int32), "word": take(lib.ttr_result_words(r), (n,), np.int32),
           "order": take(lib.ttr_result_reading_order(r), (n,), np.int32), "line_first": take(lib.ttr_result_line_first(r), (nl + 1,), np.int32),
           "line_bbox": take(lib.ttr_result_line_bboxes(r), (nl, 4), np.float32),
           "line_text": [text(lib.ttr_result_line_text, l) for l in range(nl)], "page_text": text(lib.ttr_result_page_text)}
    lib.ttr_result_free(r)
    return out


# ------------------------------------------------------------------------------------------------- the kernel against the host rule
def _check_group(eng, sets):
    from tuatara_amd.engine import lines_from_quads
    first = np.cumsum([0] + [len(q) for q in sets]).astype(np.int32)
    quads = np.concatenate([q.reshape(-1, 8) for q in sets]) if sets else np.zeros((0, 8), np.float32)
    line, word, nl = eng.group_lines(quads, first)
    assert len(line) == len(word) == first[-1] and len(nl) == len(sets)
    for p, q in enumerate(sets):
        want = lines_from_quads(q)
        got = (line[first[p]:first[p + 1]], word[first[p]:first[p + 1]], int(nl[p]))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], (p, len(q))
    return nl


def test_group_lines_equals_the_host_rule(engines):
    eng = engines(0)                                                         # the stage entry point runs whatever the engine's `lines`
    sets = [L.random_quads(n, 500 + k) for k, n in enumerate((0, 1, 2, 37, 0, 1000, 300, 64, 65, 0))]
    nl = _check_group(eng, sets)
    assert nl[0] == nl[4] == nl[9] == 0 and nl[1] == 1 and 1 < nl[5] < 1000
    _check_group(eng, [np.zeros((0, 8), np.float32)])                       # one empty page
    _check_group(eng, [])                                                    # no pages
    _check_group(engines(1), sets[:4])
    # the hand-made layouts of the CPU suite in one launch
    h = 20.0
    para = np.concatenate([L.row_quads(40, 100 + 1.3 * h * r, w, h, 0.4 * h) for r, w in enumerate([[60, 35, 80, 20, 55], [45, 90, 30, 70], [25, 65, 40]])])
    tilted = np.concatenate([L.row_quads(500 - np.sin(np.deg2rad(d)) * 36 * r, 300 + np.cos(np.deg2rad(d)) * 36 * r, [70, 40, 90, 50], 24.0, 12.0, d)
                             for d in (20.0, -30.0, 44.0) for r in range(3)])
    gaps = np.concatenate([L.row_quads(40, 100, [90, 60], 30.0, 29.0), L.row_quads(40, 300, [90, 60], 30.0, 31.0)])
    assert _check_group(eng, [para, tilted, gaps]).tolist() == [3, 9, 3]


def test_group_lines_4096_words_on_a_page(engines):
    from tuatara_amd.engine import EngineError
    eng = engines(0)
    loose = L.random_quads(4096, 77)
    # 64 rows of 64 linked words: long lines, many unions per word
    dense = np.concatenate([L.row_quads(20, 30 + 26.0 * r, [14.0 + (r + k) % 5 for k in range(64)], 16.0, 5.0) for r in range(64)])
    assert len(dense) == 4096
    nl = _check_group(eng, [loose, dense, L.random_quads(3, 1)])
    assert nl[1] == 64
    one_line = L.row_quads(10, 100, [6.0] * 4096, 8.0, 1.0)                 # every word on one line (x up to 28 682 px)
    assert _check_group(eng, [one_line]).tolist() == [1]
    with pytest.raises(EngineError, match="4096"):
        eng.group_lines(L.row_quads(10, 100, [6.0] * 4097, 8.0, 1.0), [0, 4097])
    bad = L.random_quads(5, 2)
    bad[3, 4] = np.inf
    with pytest.raises(EngineError, match="finite"):
        eng.group_lines(bad, [0, 5])


# ------------------------------------------------------------------------------------------------- the engine
def test_lines_on_changes_nothing_else_and_equals_the_host_rule(engines, funsd, pages):
    from tuatara_amd.engine import lines_from_quads
    for mode in (0, 1):
        off, on = engines(0, mode), engines(1, mode)
        for img in [funsd] + pages:
            a, b = _raw(off, img), _raw(on, img)
            assert a["n"] == b["n"] > 0 and a["texts"] == b["texts"]
            for k in ("bbox", "quad", "ids", "prob", "conf"):
                assert a[k].tobytes() == b[k].tobytes(), k                     # bit for bit
            # lines off: NULL pointers, zero counts
            assert a["n_lines"] == 0 and all(a[k] is None for k in ("line", "word", "order", "line_first", "line_bbox")) and a["page_text"] == ""
            # lines on: the host rule on the result's own quads
            line, word, nl = lines_from_quads(b["quad"])
            assert np.array_equal(b["line"], line) and np.array_equal(b["word"], word) and b["n_lines"] == nl
            order, first = L.reading_order(line, word, nl)
            assert np.array_equal(b["order"], order) and np.array_equal(b["line_first"], first)
            assert b["line_bbox"].tobytes() == L.line_bboxes(b["bbox"], order, first).tobytes()
            assert b["line_text"] == L.line_texts(b["texts"], order, first) and b["page_text"] == L.page_text(b["texts"], order, first)
            assert 1 <= nl <= b["n"]
            print(f"crop_mode={mode} {img.shape}: {b['n']} words in {nl} lines, longest {int(np.diff(first).max())}")
    on = engines(1)
    for flat in (np.full((256, 320, 3), 255, np.uint8), np.zeros((64, 64, 3), np.uint8)):   # flat pages: whatever the detector gives, an empty result has no lines
        e = _raw(on, flat)
        if e["n"] == 0:
            assert e["n_lines"] == 0 and e["line"] is None and e["line_first"] is None and e["line_bbox"] is None and e["page_text"] == ""
        else:
            line, word, nl = lines_from_quads(e["quad"])
            assert np.array_equal(e["line"], line) and np.array_equal(e["word"], word) and e["n_lines"] == nl


def test_python_results_carry_the_lines(engines, funsd):
    on, off = engines(1), engines(0)
    r, r0 = on.image_to_data(funsd, conf=True), off.image_to_data(funsd, conf=True)
    assert [{k: v for k, v in d.items() if k not in ("line", "word")} for d in r] == r0 and all("line" not in d for d in r0)
    pr = _batch(on, [funsd])[0]
    raw = _raw(on, funsd)
    assert [(d["line"], d["word"]) for d in r] == list(zip(raw["line"].tolist(), raw["word"].tolist())) == list(zip(pr.line.tolist(), pr.word.tolist()))
    assert [ln["text"] for ln in pr.lines] == raw["line_text"] and pr.text == raw["page_text"]
    assert [ln["items"] for ln in pr.lines] == [raw["order"][raw["line_first"][l]:raw["line_first"][l + 1]].tolist() for l in range(raw["n_lines"])]
    assert np.array_equal(np.float32([ln["bbox"] for ln in pr.lines]), raw["line_bbox"])
    p0 = _batch(off, [funsd])[0]
    assert p0.line is None and p0.lines == [] and p0.text == ""


def test_every_entry_point_gives_the_same_lines(engines, pages):
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    on = engines(1)
    small = synth.synthetic_page(93, 384, 448, n_words=6)
    alone = [_batch(on, [p])[0] for p in pages]
    assert all(len(a) > 0 and len(a.lines) > 0 for a in alone)

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert np.array_equal(g.bbox, w.bbox)
            assert np.array_equal(g.line, w.line) and np.array_equal(g.word, w.word) and np.array_equal(g.order, w.order)
            assert np.array_equal(g.line_first, w.line_first) and g.line_bbox.tobytes() == w.line_bbox.tobytes()
            assert [ln["items"] for ln in g.lines] == [ln["items"] for ln in w.lines]
    same(_batch(on, pages), alone)                                             # in a batch
    mixed = on.images_to_data([pages[0], small, pages[2], pages[1]])         # the list form, mixed sizes
    same(mixed, [alone[0], _batch(on, [small])[0], alone[2], alone[1]])
    assert mixed[1].text == _batch(on, [small])[0].text
    buf = DeviceBuffer(3 * 512 * 384 * 3)
    buf.upload(np.stack(pages))
    streamed = []
    for k in range(3):                                                         # streamed, one page per batch: both slots, twice
        streamed += on.stream_push(buf.ptr + k * 512 * 384 * 3, 1, 512, 384)
    while True:
        r = on.stream_flush()
        if not r:
            break
        streamed += r
    same(streamed, alone)
    streamed = on.stream_push(buf, 3, 512, 384) + on.stream_flush() + on.stream_flush()   # streamed, one batch of three
    same(streamed, alone)
    buf.free()
    same([_batch(engines(1, 1), [p])[0] for p in pages], alone)                # crop_mode = 1
    flip = _batch(engines(1, 0, 1), pages)                                     # orient = "flip"
    same(flip, alone)
    assert all(f.orient is not None for f in flip)
    # a single page's dicts through image_to_data
    assert [(d["line"], d["word"]) for d in on.image_to_data(pages[0])] == list(zip(alone[0].line.tolist(), alone[0].word.tolist()))


def test_sharded_refuses_and_a_communicator_keeps_lines_local(engines, pages):
    from tuatara_amd.engine import Comm, DeviceBuffer, EngineError
    eng = engines(1)
    buf = DeviceBuffer(2 * 512 * 384 * 3)
    buf.upload(np.stack(pages[:2]))
    single = eng.pages_to_data_dev(buf, 2, 512, 384)
    comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
    try:
        with pytest.raises(EngineError, match="text lines"):
            comm.pages_to_data_sharded(buf, 2, 512, 384)
        comm.attach(True)
        res = eng.pages_to_data_dev(buf, 2, 512, 384)
        assert [list(r) for r in res] == [list(r) for r in single]
        assert [r.text for r in res] == [r.text for r in single] and all(r.text for r in res)
        comm.attach(False)
    finally:
        comm.close()
        buf.free()


# ------------------------------------------------------------------------------------------------- callers
def test_pytuatara_lines_keyword(weights, engines, pages, monkeypatch):
    from tuatara_amd import build
    build.build_pytuatara()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ORIENT", "TUATARA_LINES"):
        monkeypatch.delenv(k, raising=False)
    page = pages[1]
    plain = pytuatara.image_to_data(page, weights["dir"], "o")
    assert set(plain[0]) == {"text", "bbox"}
    for kw, key in (({"lines": True}, (1, 0, 0)), ({"lines": True, "rectify": True, "conf": True}, (1, 1, 0)), ({"lines": True, "orient": "flip"}, (1, 0, 1))):
        got = pytuatara.image_to_data(page, weights["dir"], "o", **kw)
        want = engines(*key).image_to_data(page, conf=True)
        assert len(got) == len(want) > 0
        assert [(g["text"], list(g["bbox"]), g["line"], g["word"]) for g in got] == [(w["text"], w["bbox"], w["line"], w["word"]) for w in want]
        assert ("orient" in got[0]) == ("orient" in kw) and ("quad" in got[0]) == bool(kw.get("rectify"))
        assert pytuatara.images_to_data([page], weights["dir"], "o", **kw) == [got]


def test_ocr_cli_lines_prints_the_page_text(weights, engines, tmp_path):
    from PIL import Image
    from tuatara_amd import build as B
    B.build_examples()
    env = {k: v for k, v in os.environ.items() if k not in ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ORIENT", "TUATARA_LINES")}
    png = os.path.join(DATA, "funsd_0001129658.png")
    out = subprocess.run([os.path.join(B.ROOT, "build", "examples", "ocr_cli"), "--lines", png, weights["dir"], str(tmp_path)],
                         capture_output=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    rgb = np.array(Image.open(png).convert("RGB"))
    want = _batch(engines(1), [np.ascontiguousarray(rgb[:, :, ::-1])])[0]     # the CLI feeds BGR
    assert len(want.lines) > 5
    assert out.stdout.decode("latin1") == want.text + "\n"
