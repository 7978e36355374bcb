"""GPU suite for text blocks (ttr_config.blocks; DESIGN.md "Text blocks"): block_group_kernel (ttr_group_blocks) against the host rule
(ttr_blocks_from_quads) bit for bit - ten pages of different sizes in one launch, empty pages included, 4096 words on a page, the 512- and
513-block pages -, the blocks = 1 engine against the lines = 1 engine (every other output bit for bit), the returned blocks against the host
rule on the result's own quads, every entry point against the single-page call, the sharded mode's refusal, the callers (pytuatara,
ocr_cli) and a rendered two-column page read column after column.  Every test runs under a time limit of its own: a step that hangs ends
the process instead of holding the GPU."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import blocks_ref as B
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
    """engines by (blocks, crop_mode, orient, chars), all with lines = 1, made on first use (default precision, f16x4)"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine
    build_lib()
    cache = {}

    def get(blocks, crop_mode=0, orient=0, chars=0):
        key = (blocks, crop_mode, orient, chars)
        if key not in cache:
            cache[key] = Engine(weights["dir"], crop_mode=crop_mode, orient=orient, lines=1, chars=chars, blocks=blocks)
        return cache[key]
    yield get
    for e in cache.values():
        e.close()


@pytest.fixture(scope="module")
def pages():
    """synthetic pages of one size: upright words in rows, a two-column page, and a page of tilted words"""
    from tuatara_amd import synth
    return [synth.synthetic_page(90, 512, 384, n_words=10), synth.synthetic_columns_page(3, 512, 384, rows=5, gutter=60)[0],
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
    n, nl, nb = lib.ttr_result_count(r), lib.ttr_result_line_count(r), lib.ttr_result_block_count(r)

    def take(p, shape, dt):
        return np.ctypeslib.as_array(p, shape).astype(dt).copy() if p else None

    def text(fn, *a):
        need = fn(r, *a, None, 0)
        buf = C.create_string_buffer(max(need, 1))
        assert fn(r, *a, buf, need) == need
        return buf.raw[:need].decode("latin1")
    out = {"n": n, "n_lines": nl, "n_blocks": nb, "block_mode": lib.ttr_result_block_mode(r),
           "texts": [lib.ttr_result_text(r, i).decode("latin1") for i in range(n)],
           "bbox": take(lib.ttr_result_bboxes(r), (n, 4), np.float32), "quad": take(lib.ttr_result_quads(r), (n, 8), np.float32),
           "ids": take(lib.ttr_result_ids_all(r), (n, 26), np.int32), "prob": take(lib.ttr_result_probs_all(r), (n, 26), np.float32),
           "conf": take(lib.ttr_result_confs(r), (n,), np.float32),
           "line": take(lib.ttr_result_lines(r), (n,), np.int32), "word": take(lib.ttr_result_words(r), (n,), np.int32),
           "order": take(lib.ttr_result_reading_order(r), (n,), np.int32), "line_first": take(lib.ttr_result_line_first(r), (nl + 1,), np.int32),
           "line_bbox": take(lib.ttr_result_line_bboxes(r), (nl, 4), np.float32),
           "line_text": [text(lib.ttr_result_line_text, l) for l in range(nl)], "page_text": text(lib.ttr_result_page_text),
           "block": take(lib.ttr_result_blocks(r), (n,), np.int32), "line_block": take(lib.ttr_result_line_blocks(r), (nl,), np.int32),
           "line_pos": take(lib.ttr_result_line_pos(r), (nl,), np.int32), "block_order": take(lib.ttr_result_block_order(r), (nl,), np.int32),
           "block_first": take(lib.ttr_result_block_first(r), (nb + 1,), np.int32), "block_bbox": take(lib.ttr_result_block_bboxes(r), (nb, 4), np.float32),
           "block_text": [text(lib.ttr_result_block_text, b) for b in range(nb)], "page_text_blocks": text(lib.ttr_result_page_text_blocks)}
    assert lib.ttr_result_block_text(r, nb, None, 0) == 0 and lib.ttr_result_block_text(r, -1, None, 0) == 0
    lib.ttr_result_free(r)
    return out


BLOCK_KEYS = ("block", "line_block", "line_pos", "block_order", "block_first", "block_bbox")


# ------------------------------------------------------------------------------------------------- the kernels against the host rule
def _check_group(eng, sets):
    from tuatara_amd.engine import blocks_from_quads
    first = np.cumsum([0] + [len(q) for q in sets]).astype(np.int32)
    quads = np.concatenate([q.reshape(-1, 8) for q in sets]) if sets else np.zeros((0, 8), np.float32)
    line, word, nl, block, pos, nb, mode = eng.group_blocks(quads, first)
    assert len(line) == len(word) == len(block) == len(pos) == first[-1] and len(nl) == len(nb) == len(mode) == len(sets)
    for p, q in enumerate(sets):
        want = blocks_from_quads(q)
        a, m = int(first[p]), int(nl[p])
        got = (line[a:first[p + 1]], word[a:first[p + 1]], m, block[a:a + m], pos[a:a + m], int(nb[p]), int(mode[p]))
        for k in range(7):
            assert np.array_equal(got[k], want[k]), (p, len(q), k)
        assert (block[a + m:first[p + 1]] == -1).all() and (pos[a + m:first[p + 1]] == -1).all()      # behind the page's lines
    return nb, mode


def test_group_blocks_equals_the_host_rule(engines):
    eng = engines(0)                                                         # the stage entry point runs whatever the engine's config
    sets = [L.random_quads(n, 700 + k) for k, n in enumerate((0, 1, 2, 37, 0, 1000, 300, 64, 65, 0))]
    nb, mode = _check_group(eng, sets)
    assert nb[0] == nb[4] == nb[9] == 0 and nb[1] == 1 and 1 < nb[5] < 1000 and (mode[[0, 1, 2, 3, 4, 9]] == 1).all()
    _check_group(eng, [np.zeros((0, 8), np.float32)])                       # one empty page
    _check_group(eng, [])                                                    # no pages
    _check_group(engines(1), sets[:4])
    # generated paragraph pages and the hand-made layouts of the CPU suite in one launch
    two = B.two_section_page()[0]
    para = np.concatenate([B.paragraph(300, 200, 600, 4, 20.0, 1.33, 15.0, seed=11)[0], B.paragraph(300 - np.sin(np.deg2rad(15.0)) * 133, 200 + np.cos(np.deg2rad(15.0)) * 133, 600, 3, 20.0, 1.33, 15.0, seed=12)[0]])
    nb, mode = _check_group(eng, [two, para] + [B.random_page(s) for s in range(8)])
    assert nb[0] == 9 and nb[1] == 2 and (mode == 1).all()


def test_group_blocks_4096_words_on_a_page(engines):
    from tuatara_amd.engine import EngineError
    eng = engines(0)
    loose = L.random_quads(4096, 78)
    # 64 rows of 64 linked words, 1.6 heights apart: one block of 64 lines
    dense = np.concatenate([L.row_quads(20, 30 + 26.0 * r, [14.0 + (r + k) % 5 for k in range(64)], 16.0, 5.0) for r in range(64)])
    assert len(dense) == 4096
    nb, mode = _check_group(eng, [loose, dense, L.random_quads(3, 1)])
    assert nb[1] == 1 and mode[1] == 1
    apart = B.isolated_words(4096, per_row=64)                               # 4096 lines, 4096 blocks: beyond the cap
    nb, mode = _check_group(eng, [apart])
    assert nb[0] == 4096 and mode[0] == 0
    with pytest.raises(EngineError, match="4096"):
        eng.group_blocks(L.row_quads(10, 100, [6.0] * 4097, 8.0, 1.0), [0, 4097])
    bad = L.random_quads(5, 2)
    bad[3, 4] = np.inf
    with pytest.raises(EngineError, match="finite"):
        eng.group_blocks(bad, [0, 5])


def test_group_blocks_at_the_cap(engines):
    eng = engines(0)
    q = B.isolated_words(513)
    nb, mode = _check_group(eng, [q, q[:512], q[:511]])
    assert nb.tolist() == [513, 512, 511] and mode.tolist() == [0, 1, 1]
    # 512 blocks that hold each other in long chains: 16 columns of 32 single-line blocks
    nb, mode = _check_group(eng, [B.isolated_words(512, per_row=16)])
    assert nb[0] == 512 and mode[0] == 1


# ------------------------------------------------------------------------------------------------- the engine
def test_blocks_on_changes_nothing_else_and_equals_the_host_rule(engines, funsd, pages):
    from tuatara_amd.engine import blocks_from_quads
    for crop in (0, 1):
        off, on = engines(0, crop), engines(1, crop)
        for img in [funsd] + pages:
            a, b = _raw(off, img), _raw(on, img)
            assert a["n"] == b["n"] > 0 and a["texts"] == b["texts"] and a["line_text"] == b["line_text"] and a["page_text"] == b["page_text"]
            for k in ("bbox", "quad", "ids", "prob", "conf", "line", "word", "order", "line_first", "line_bbox"):
                assert a[k].tobytes() == b[k].tobytes(), k                     # bit for bit
            assert a["n_lines"] == b["n_lines"]
            # blocks off: NULL pointers, zero counts
            assert a["n_blocks"] == 0 and a["block_mode"] == 0 and all(a[k] is None for k in BLOCK_KEYS) and a["page_text_blocks"] == ""
            # blocks on: the host rule on the result's own quads
            line, word, nl, block, pos, nb, mode = blocks_from_quads(b["quad"])
            assert np.array_equal(b["line"], line) and np.array_equal(b["word"], word) and b["n_lines"] == nl
            assert np.array_equal(b["line_block"], block) and np.array_equal(b["line_pos"], pos) and b["n_blocks"] == nb and b["block_mode"] == mode == 1
            order, first = B.block_order(block, pos, nb)
            assert np.array_equal(b["block_order"], order) and np.array_equal(b["block_first"], first)
            assert np.array_equal(b["block"], B.item_blocks(line, block))
            assert b["block_bbox"].tobytes() == B.block_bboxes(b["line_bbox"], order, first).tobytes()
            assert b["block_text"] == B.block_texts(b["line_text"], order, first) and b["page_text_blocks"] == B.page_text_blocks(b["line_text"], order, first)
            assert 1 <= nb <= nl
            print(f"crop_mode={crop} {img.shape}: {b['n']} words in {nl} lines in {nb} blocks, largest {int(np.diff(first).max())} lines")
    on = engines(1)
    for flat in (np.full((256, 320, 3), 255, np.uint8), np.zeros((64, 64, 3), np.uint8)):   # flat pages: whatever the detector gives, an empty result has no blocks
        e = _raw(on, flat)
        if e["n"] == 0:
            assert e["n_blocks"] == 0 and all(e[k] is None for k in BLOCK_KEYS) and e["page_text_blocks"] == ""
        else:
            want = blocks_from_quads(e["quad"])
            assert np.array_equal(e["line_block"], want[3]) and np.array_equal(e["line_pos"], want[4]) and e["n_blocks"] == want[5]


def test_python_results_carry_the_blocks(engines, funsd):
    on, off = engines(1), engines(0)
    r, r0 = on.image_to_data(funsd, conf=True), off.image_to_data(funsd, conf=True)
    assert [{k: v for k, v in d.items() if k != "block"} for d in r] == r0 and all("block" not in d for d in r0)
    pr = _batch(on, [funsd])[0]
    raw = _raw(on, funsd)
    assert [d["block"] for d in r] == raw["block"].tolist() == pr.block.tolist()
    for k in ("line_block", "line_pos", "block_order", "block_first"):
        assert np.array_equal(getattr(pr, k), raw[k]), k
    assert pr.block_bbox.tobytes() == raw["block_bbox"].tobytes() and pr.block_mode == raw["block_mode"] == 1
    assert [b["text"] for b in pr.blocks] == raw["block_text"] and pr.text_blocks == raw["page_text_blocks"] and pr.text == raw["page_text"]
    assert [b["lines"] for b in pr.blocks] == [raw["block_order"][raw["block_first"][b]:raw["block_first"][b + 1]].tolist() for b in range(raw["n_blocks"])]
    p0 = _batch(off, [funsd])[0]
    assert p0.block is None and p0.blocks == [] and p0.text_blocks == "" and p0.text == pr.text


def test_every_entry_point_gives_the_same_blocks(engines, pages):
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    on = engines(1)
    small = synth.synthetic_page(93, 384, 448, n_words=6)
    alone = [_batch(on, [p])[0] for p in pages]
    assert all(len(a) > 0 and len(a.blocks) > 0 for a in alone)

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert np.array_equal(g.bbox, w.bbox) and np.array_equal(g.line, w.line) and np.array_equal(g.word, w.word)
            for k in ("block", "line_block", "line_pos", "block_order", "block_first"):
                assert np.array_equal(getattr(g, k), getattr(w, k)), k
            assert g.block_bbox.tobytes() == w.block_bbox.tobytes() and g.block_mode == w.block_mode
            assert [b["lines"] for b in g.blocks] == [b["lines"] for b in w.blocks]
    same(_batch(on, pages), alone)                                             # in a batch
    mixed = on.images_to_data([pages[0], small, pages[2], pages[1]])         # the list form, mixed sizes
    same(mixed, [alone[0], _batch(on, [small])[0], alone[2], alone[1]])
    assert mixed[3].text_blocks == alone[1].text_blocks
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
    chars = _batch(engines(1, 0, 0, 1), pages)                                 # chars = 1
    same(chars, alone)
    assert all(c.char_first is not None for c in chars)
    # a single page's dicts through image_to_data
    assert [d["block"] for d in on.image_to_data(pages[1])] == alone[1].block.tolist()


def test_sharded_refuses_and_a_communicator_keeps_blocks_local(engines, pages):
    from tuatara_amd.engine import Comm, DeviceBuffer, EngineError
    eng = engines(1)
    buf = DeviceBuffer(2 * 512 * 384 * 3)
    buf.upload(np.stack(pages[:2]))
    single = eng.pages_to_data_dev(buf, 2, 512, 384)
    comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
    try:
        with pytest.raises(EngineError, match="text blocks"):
            comm.pages_to_data_sharded(buf, 2, 512, 384)
        comm.attach(True)
        res = eng.pages_to_data_dev(buf, 2, 512, 384)
        assert [list(r) for r in res] == [list(r) for r in single]
        assert [r.text_blocks for r in res] == [r.text_blocks for r in single] and all(r.text_blocks for r in res)
        comm.attach(False)
    finally:
        comm.close()
        buf.free()


def test_two_column_page_is_read_column_after_column(engines):
    """a rendered two-column page, six rows per column on shared baselines: by blocks the left column's words all come before the right
    column's; by lines they interleave.  The words are drawn as bars of noise (synth: ink="bars"): the synthetic detector follows ink density,
    gives one box per bar and shatters glyph strokes into fragments, which is no column layout any more."""
    from tuatara_amd import synth
    for seed in (5, 6):
        page, words = synth.synthetic_columns_page(seed, ink="bars")
        r = _batch(engines(1), [page])[0]
        assert len(r) == len(words)                                                      # one box per drawn word
        side = (0.5 * (r.bbox[:, 0] + r.bbox[:, 2]) > page.shape[1] / 2).astype(int)    # 0: the left column, 1: the right
        assert side.sum() == sum(w["column"] for w in words)
        by_blocks = [int(side[i]) for b in r.blocks for l in b["lines"] for i in r.lines[l]["items"]]
        by_lines = [int(side[i]) for ln in r.lines for i in ln["items"]]
        print(f"seed {seed}: {len(r)} words, {len(r.lines)} lines, {len(r.blocks)} blocks; by lines {by_lines}")
        assert len(by_blocks) == len(by_lines) == len(r)
        assert len(r.lines) == 12 and [len(b["lines"]) for b in r.blocks] == [6, 6]      # each column one block of six lines
        assert by_blocks == sorted(by_blocks), by_blocks                                 # every left word before every right word
        assert by_lines != sorted(by_lines), by_lines                                    # the line order interleaves the columns
        assert r.text_blocks.count("\n\n") == 1 and r.text_blocks.replace("\n\n", "\n").count("\n") == r.text.count("\n") == 11
        # the same words in both texts, the left column's first in text_blocks only
        left_texts = [r.texts[i] for i in range(len(r)) if side[i] == 0]
        assert r.text_blocks.split("\n\n")[0].replace("\n", " ").split(" ") == [r.texts[i] for b in r.blocks[:1] for l in b["lines"] for i in r.lines[l]["items"]]
        assert sorted(left_texts) == sorted(r.text_blocks.split("\n\n")[0].replace("\n", " ").split(" "))


# ------------------------------------------------------------------------------------------------- callers
def test_pytuatara_blocks_keyword(weights, engines, pages, monkeypatch):
    from tuatara_amd import build
    build.build_pytuatara()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ORIENT", "TUATARA_LINES", "TUATARA_CHARS", "TUATARA_BLOCKS"):
        monkeypatch.delenv(k, raising=False)
    page = pages[1]
    plain = pytuatara.image_to_data(page, weights["dir"], "o")
    assert set(plain[0]) == {"text", "bbox"}
    assert "block" not in pytuatara.image_to_data(page, weights["dir"], "o", lines=True)[0]
    for kw, key in (({"blocks": True}, (1, 0, 0)), ({"blocks": True, "lines": True, "rectify": True, "conf": True}, (1, 1, 0)), ({"blocks": True, "orient": "flip"}, (1, 0, 1))):
        got = pytuatara.image_to_data(page, weights["dir"], "o", **kw)
        want = engines(*key).image_to_data(page, conf=True)
        assert len(got) == len(want) > 0
        assert [(g["text"], list(g["bbox"]), g["line"], g["word"], g["block"]) for g in got] == [(w["text"], w["bbox"], w["line"], w["word"], w["block"]) for w in want]
        assert ("orient" in got[0]) == ("orient" in kw) and ("quad" in got[0]) == bool(kw.get("rectify"))
        assert pytuatara.images_to_data([page], weights["dir"], "o", **kw) == [got]


def test_ocr_cli_blocks_prints_the_page_text_by_blocks(weights, engines, tmp_path):
    from PIL import Image
    from tuatara_amd import build as Bd
    Bd.build_examples()
    env = {k: v for k, v in os.environ.items() if k not in ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ORIENT", "TUATARA_LINES", "TUATARA_CHARS", "TUATARA_BLOCKS")}
    png = os.path.join(DATA, "funsd_0001129658.png")
    out = subprocess.run([os.path.join(Bd.ROOT, "build", "examples", "ocr_cli"), "--blocks", png, weights["dir"], str(tmp_path)],
                         capture_output=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    rgb = np.array(Image.open(png).convert("RGB"))
    want = _batch(engines(1), [np.ascontiguousarray(rgb[:, :, ::-1])])[0]     # the CLI feeds BGR
    assert len(want.blocks) > 3
    assert out.stdout.decode("latin1") == want.text_blocks + "\n"
