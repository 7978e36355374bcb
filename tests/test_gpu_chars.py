"""GPU suite for character boxes (ttr_config.chars; DESIGN.md "Character boxes"): char_cut_kernel (ttr_char_cuts) against the host rule
(ttr_chars_from_map) bit for bit - the CPU suite's maps and quads, several thousand words in one launch, no words, K = 0 and K = 26, every
turn -, the chars = 1 engine against the chars = 0 engine (same items, every earlier output bit for bit), the returned cuts, cells and
profiles against the host rule, every entry point against the single-page call, the sharded mode's refusal and the callers (pytuatara,
ocr_cli).  Every test runs under a time limit of its own: a step that hangs ends the process instead of holding the GPU."""
import ctypes as C
import faulthandler
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import chars_ref as R
from tests.conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

STEP_LIMIT_S = 600
LOW_TEXT = 0.4                      # ttr_config_default
QLOW = int(np.float32(LOW_TEXT) * np.float32(255.0))


@pytest.fixture(autouse=True)
def step_limit():
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def engines(weights):
    """engines by (chars, crop_mode, orient, lines), made on first use (default precision, f16x4)"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine
    build_lib()
    cache = {}

    def get(chars, crop_mode=0, orient=0, lines=0):
        key = (chars, crop_mode, orient, lines)
        if key not in cache:
            cache[key] = Engine(weights["dir"], crop_mode=crop_mode, orient=orient, lines=lines, chars=chars)
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
    n = lib.ttr_result_count(r)
    counts = [lib.ttr_result_char_count(r, i) for i in range(n)]
    total = sum(counts)

    def take(p, shape, dt):
        return np.ctypeslib.as_array(p, shape).astype(dt).copy() if p else None
    out = {"n": n, "texts": [lib.ttr_result_text(r, i).decode("latin1") for i in range(n)],
           "bbox": take(lib.ttr_result_bboxes(r), (n, 4), np.float32), "quad": take(lib.ttr_result_quads(r), (n, 8), np.float32),
           "ids": take(lib.ttr_result_ids_all(r), (n, 26), np.int32), "prob": take(lib.ttr_result_probs_all(r), (n, 26), np.float32),
           "conf": take(lib.ttr_result_confs(r), (n,), np.float32), "orient": take(lib.ttr_result_orients(r), (n,), np.int32),
           "line": take(lib.ttr_result_lines(r), (n,), np.int32), "word": take(lib.ttr_result_words(r), (n,), np.int32),
           "char_counts": counts, "char_first": take(lib.ttr_result_char_first(r), (n + 1,), np.int32),
           "char_quad": take(lib.ttr_result_char_quads(r), (total, 8), np.float32), "char_bbox": take(lib.ttr_result_char_bboxes(r), (total, 4), np.float32),
           "char_cuts": take(lib.ttr_result_char_cuts(r), (n, 27), np.int32), "char_mode": take(lib.ttr_result_char_modes(r), (n,), np.int32),
           "char_profile": take(lib.ttr_result_char_profiles(r), (n, 128), np.uint8)}
    lib.ttr_result_free(r)
    return out


def _region_plane(eng, img):
    """the page's normalised region plane as binarize_kernel writes it, and its canvas ratio: the stage calls ttr_resize_canvas and
    ttr_craft_heatmap, then (v - min) / (max - min) in numpy float32 (one IEEE subtraction and one IEEE division per pixel, as the kernel)"""
    canvas, ratio = eng.resize_canvas(img)
    t = np.ascontiguousarray(eng.craft_heatmap(canvas)[:, :, 0])
    return (t - t.min()) / (t.max() - t.min()), ratio


def _inside(quad8, pts, tol):
    """every point of pts [m, 2] lies inside the convex quad (either winding) to tol px"""
    q = quad8.reshape(4, 2).astype(np.float64)
    e = np.roll(q, -1, axis=0) - q
    area2 = float(np.sum(q[:, 0] * np.roll(q[:, 1], -1) - np.roll(q[:, 0], -1) * q[:, 1]))
    s = 1.0 if area2 >= 0 else -1.0
    for a, d in zip(q, e):
        dist = s * (d[0] * (pts[:, 1] - a[1]) - d[1] * (pts[:, 0] - a[0])) / max(np.hypot(*d), 1e-9)
        if (dist < -tol).any():
            return False
    return True


def _check_chars(texts, quad, turns, first, cquad, cbbox, cuts, mode, prof, plane=None, ratio=None):
    """the chars = 1 outputs of one page against the host rule on the result's own profile, quad, turn and cuts (and, given the page's region
    plane, the profiles themselves)"""
    from tuatara_amd.engine import char_cuts_from_profile, char_quads_from_cuts, chars_from_map
    n = len(texts)
    K = np.array([len(t) for t in texts], np.int32)
    turns = np.zeros(n, np.int32) if turns is None else turns
    if K.sum() == 0:                     # words without characters: no cells, so the C ABI's cell pointers are NULL
        assert cquad is None or len(cquad) == 0
        cquad, cbbox = np.zeros((0, 8), np.float32), np.zeros((0, 4), np.float32)
    assert np.array_equal(first, np.concatenate([[0], np.cumsum(K)]))
    assert len(cquad) == len(cbbox) == int(K.sum())
    for i in range(n):
        want, wmode = char_cuts_from_profile(prof[i], int(K[i]), QLOW)
        assert np.array_equal(cuts[i], want) and mode[i] == wmode, (i, texts[i])
        wq, wb = char_quads_from_cuts(quad[i], int(turns[i]), cuts[i], int(K[i]))
        a, b = int(first[i]), int(first[i + 1])
        assert cquad[a:b].tobytes() == wq.tobytes() and cbbox[a:b].tobytes() == wb.tobytes(), i
        if K[i]:
            assert _inside(quad[i], cquad[a:b].reshape(-1, 2).astype(np.float64), 2.0 ** -8), (i, texts[i])
    if plane is not None:
        wc, wm, wp = chars_from_map(plane, ratio, LOW_TEXT, quad, turns, K)
        assert np.array_equal(prof, wp), int((prof != wp).sum())
        assert np.array_equal(cuts, wc) and np.array_equal(mode, wm)


def _check_page(pr, plane=None, ratio=None):
    _check_chars(pr.texts, pr.word_quad, pr.orient, pr.char_first, pr.char_quad, pr.char_bbox, pr.char_cuts, pr.char_mode, pr.char_profile, plane, ratio)


# ------------------------------------------------------------------------------------------------- the kernel against the host rule
def _check_stage(eng, T, ratio, quads, turns, nchars, low_text=LOW_TEXT):
    from tuatara_amd.engine import chars_from_map
    got = eng.char_cuts(T, ratio, low_text, quads, turns, nchars)
    want = chars_from_map(T, ratio, low_text, quads, turns, nchars)
    assert np.array_equal(got[2], want[2]), int((got[2] != want[2]).sum())
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


def test_char_cuts_equals_the_host_rule(engines):
    eng = engines(0)                                                         # the stage entry point runs whatever the engine's `chars`
    for H2, W2 in ((64, 96), (200, 333), (512, 384)):                        # the CPU suite's maps and quads
        for ratio in (1.0, 0.8):
            for outside in (False, True):
                T = R.random_map(H2 * 7 + W2, H2, W2)
                quads, turns, nchars = R.random_words(H2 + W2 + int(ratio * 10) + outside, 60, H2, W2, ratio, outside=outside)
                cuts, modes, prof = _check_stage(eng, T, ratio, quads, turns, nchars)
                assert set(modes.tolist()) == {0, 1} and set(turns.tolist()) == {0, 1, 2, 3}
    T = R.random_map(9, 512, 512)
    quads, turns, nchars = R.random_words(10, 5000, 512, 512, 1.0, outside=True)   # several thousand words in one launch
    cuts, modes, _ = _check_stage(eng, T, 1.0, quads, turns, nchars)
    assert (modes == 1).sum() > 1000 and (modes == 0).sum() > 100
    for K in (0, 26):                                                        # the extreme counts, every turn
        _check_stage(eng, T, 1.0, quads[:200], turns[:200], np.full(200, K, np.int32))
    for t in range(4):
        _check_stage(eng, T, 1.0, quads[:100], np.full(100, t, np.int32), nchars[:100])
    for low in (0.0, 0.999):                                                 # qlow = 0 and 254
        _check_stage(eng, T, 1.0, quads[:300], turns[:300], nchars[:300], low_text=low)
    c, m, p = eng.char_cuts(T, 1.0, LOW_TEXT, np.zeros((0, 8), np.float32), [], [])     # n = 0
    assert c.shape == (0, 27) and m.shape == (0,) and p.shape == (0, 128)
    _check_stage(engines(1), T, 1.0, quads[:64], turns[:64], nchars[:64])
    # the hand-made words of the CPU suite's functional test: the kernel places the same cuts
    for Tb, ratio, quad, K, _ in list(R.blob_words(11, 0.5, 20)) + list(R.blob_words(21, 0.4, 20)):
        _check_stage(eng, Tb, ratio, [quad], [0], [K])


def test_char_cuts_refusals(engines):
    from tuatara_amd.engine import EngineError
    eng = engines(0)
    T = np.zeros((32, 32), np.float32)
    good = R.rect_quad(20., 20., 30., 10., 0.)
    bad = good.copy(); bad[5] = np.inf
    with pytest.raises(EngineError, match="finite"):
        eng.char_cuts(T, 1.0, LOW_TEXT, [bad], [0], [3])
    with pytest.raises(EngineError, match="turn"):
        eng.char_cuts(T, 1.0, LOW_TEXT, [good], [4], [3])
    with pytest.raises(EngineError, match="count"):
        eng.char_cuts(T, 1.0, LOW_TEXT, [good], [0], [27])


# ------------------------------------------------------------------------------------------------- the engine
def test_chars_on_changes_nothing_else_and_equals_the_host_rule(engines, funsd, pages):
    """The profiles are checked against ttr_chars_from_map on the page's region plane; the plane's source is the stage calls
    ttr_resize_canvas + ttr_craft_heatmap, normalised in numpy float32 (_region_plane)."""
    modes_seen = set()
    for mode in (0, 1):
        off, on = engines(0, mode), engines(1, mode)
        for img in [funsd] + pages:
            a, b = _raw(off, img), _raw(on, img)
            assert a["n"] == b["n"] > 0 and a["texts"] == b["texts"]
            for k in ("bbox", "quad", "ids", "prob", "conf"):
                assert a[k].tobytes() == b[k].tobytes(), k                     # bit for bit
            assert a["orient"] is None and b["orient"] is None and a["line"] is None and b["line"] is None
            # chars off: NULL pointers, zero counts
            assert all(a[k] is None for k in ("char_first", "char_quad", "char_bbox", "char_cuts", "char_mode", "char_profile")) and sum(a["char_counts"]) == 0
            # chars on: the host rule
            assert b["char_counts"] == [len(t) for t in b["texts"]]
            plane, ratio = _region_plane(on, img)
            _check_chars(b["texts"], b["quad"], None, b["char_first"], b["char_quad"], b["char_bbox"], b["char_cuts"], b["char_mode"], b["char_profile"], plane, ratio)
            modes_seen |= set(b["char_mode"].tolist())
            print(f"crop_mode={mode} {img.shape}: {b['n']} words, {int(b['char_first'][-1])} characters, {int((b['char_mode'] == 1).sum())} words cut at valleys")
    assert 1 in modes_seen
    on = engines(1)
    for flat in (np.full((256, 320, 3), 255, np.uint8), np.zeros((64, 64, 3), np.uint8)):   # flat pages: whatever the detector gives, an empty result has no characters
        e = _raw(on, flat)
        if e["n"] == 0:
            assert e["char_first"] is None and e["char_quad"] is None and e["char_cuts"] is None and e["char_profile"] is None
        else:
            _check_chars(e["texts"], e["quad"], None, e["char_first"], e["char_quad"], e["char_bbox"], e["char_cuts"], e["char_mode"], e["char_profile"])


def test_python_results_carry_the_chars(engines, funsd):
    on, off = engines(1), engines(0)
    r, r0 = on.image_to_data(funsd, conf=True), off.image_to_data(funsd, conf=True)
    assert [{k: v for k, v in d.items() if k != "chars"} for d in r] == r0 and all("chars" not in d for d in r0)
    pr = _batch(on, [funsd])[0]
    raw = _raw(on, funsd)
    for k in ("char_first", "char_quad", "char_bbox", "char_cuts", "char_mode", "char_profile"):
        assert getattr(pr, k).tobytes() == raw[k].tobytes(), k
    assert pr.word_quad.tobytes() == raw["quad"].tobytes()
    for i, d in enumerate(r):
        a, b = int(raw["char_first"][i]), int(raw["char_first"][i + 1])
        assert "".join(c["char"] for c in d["chars"]) == d["text"] and len(d["chars"]) == b - a
        assert np.array_equal(np.float32([c["bbox"] for c in d["chars"]]).reshape(-1, 4), raw["char_bbox"][a:b])
        assert np.array_equal(np.float32([c["quad"] for c in d["chars"]]).reshape(-1, 8), raw["char_quad"][a:b])
    p0 = _batch(off, [funsd])[0]
    assert p0.char_first is None and p0.char_quad is None and p0.char_profile is None and p0.word_quad is None


def test_every_entry_point_gives_the_same_chars(engines, pages):
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer
    on = engines(1)
    small = synth.synthetic_page(93, 384, 448, n_words=6)
    alone = [_batch(on, [p])[0] for p in pages]
    assert all(len(a) > 0 and int(a.char_first[-1]) > 0 for a in alone)
    for a, p in zip(alone, pages):
        _check_page(a, *_region_plane(on, p))

    def same(got, want, profiles=True):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert np.array_equal(g.bbox, w.bbox) and g.texts == w.texts
            assert np.array_equal(g.char_first, w.char_first) and g.char_quad.tobytes() == w.char_quad.tobytes() and g.char_bbox.tobytes() == w.char_bbox.tobytes()
            assert np.array_equal(g.char_cuts, w.char_cuts) and np.array_equal(g.char_mode, w.char_mode)
            if profiles:
                assert np.array_equal(g.char_profile, w.char_profile)
    same(_batch(on, pages), alone)                                             # in a batch
    mixed = on.images_to_data([pages[0], small, pages[2], pages[1]])         # the list form, mixed sizes
    same(mixed, [alone[0], _batch(on, [small])[0], alone[2], alone[1]])
    buf = DeviceBuffer(3 * 512 * 384 * 3)
    buf.upload(np.stack(pages))
    streamed = []
    for k in list(range(3)) + [0]:                                             # streamed, one page per batch: through both slots twice
        streamed += on.stream_push(buf.ptr + k * 512 * 384 * 3, 1, 512, 384)
    while True:
        r = on.stream_flush()
        if not r:
            break
        streamed += r
    same(streamed, alone + alone[:1])
    streamed = on.stream_push(buf, 3, 512, 384) + on.stream_flush() + on.stream_flush()   # streamed, one batch of three
    same(streamed, alone)
    buf.free()
    with_lines = _batch(engines(1, 0, 0, 1), pages)                            # lines = 1
    same(with_lines, alone)
    assert all(w.line is not None for w in with_lines)
    rect = engines(1, 1)                                                       # crop_mode = 1: the recogniser reads other pixels, so the texts (and K) are its own
    rect_alone = [_batch(rect, [p])[0] for p in pages]
    same(_batch(rect, pages), rect_alone)
    for r, p in zip(rect_alone, pages):
        _check_page(r, *_region_plane(rect, p))
    # a single page's dicts through image_to_data
    d = on.image_to_data(pages[0])
    assert [[c["bbox"] for c in w["chars"]] for w in d] == [alone[0].char_bbox[alone[0].char_first[i]:alone[0].char_first[i + 1]].tolist() for i in range(len(alone[0]))]


def test_quarter_turns_set_the_frame(engines, pages):
    """orient = "quarter" on a page of turned words: K, the turn and with them the frame are the chosen reading's"""
    up = pages[0]
    turned = [np.ascontiguousarray(np.rot90(up, -1)), np.ascontiguousarray(np.rot90(up, 2))]
    on = engines(1, 0, 2)
    any_turn = False
    for img in turned + [up]:
        r = _batch(on, [img])[0]
        assert r.orient is not None and len(r) > 0
        _check_page(r, *_region_plane(on, img))
        any_turn |= bool((r.orient != 0).any())
    assert any_turn
    pair = [turned[1], up]                                                     # (one size: they travel as one batch)
    for g, img in zip(_batch(on, pair), pair):
        w = _batch(on, [img])[0]
        assert np.array_equal(g.orient, w.orient) and np.array_equal(g.char_cuts, w.char_cuts) and g.char_quad.tobytes() == w.char_quad.tobytes()


def test_sharded_refuses_and_a_communicator_keeps_chars_local(engines, pages):
    from tuatara_amd.engine import Comm, DeviceBuffer, EngineError
    eng = engines(1)
    buf = DeviceBuffer(2 * 512 * 384 * 3)
    buf.upload(np.stack(pages[:2]))
    single = eng.pages_to_data_dev(buf, 2, 512, 384)
    comm = Comm(eng, 0, 1, unique_id=Comm.unique_id())
    try:
        with pytest.raises(EngineError, match="character boxes"):
            comm.pages_to_data_sharded(buf, 2, 512, 384)
        comm.attach(True)
        res = eng.pages_to_data_dev(buf, 2, 512, 384)
        assert [list(r) for r in res] == [list(r) for r in single]
        for r, s in zip(res, single):
            assert r.char_quad.tobytes() == s.char_quad.tobytes() and np.array_equal(r.char_cuts, s.char_cuts) and int(r.char_first[-1]) > 0
        comm.attach(False)
    finally:
        comm.close()
        buf.free()


# ------------------------------------------------------------------------------------------------- callers
ENV_KEYS = ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ORIENT", "TUATARA_LINES", "TUATARA_CHARS")


def test_pytuatara_chars_keyword(weights, engines, pages, monkeypatch):
    from tuatara_amd import build
    build.build_pytuatara()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    page = pages[1]
    plain = pytuatara.image_to_data(page, weights["dir"], "o")
    assert set(plain[0]) == {"text", "bbox"}
    for kw, key in (({"chars": True}, (1, 0, 0, 0)), ({"chars": True, "rectify": True, "conf": True}, (1, 1, 0, 0)),
                    ({"chars": True, "orient": "quarter"}, (1, 0, 2, 0)), ({"chars": True, "lines": True}, (1, 0, 0, 1))):
        got = pytuatara.image_to_data(page, weights["dir"], "o", **kw)
        want = engines(*key).image_to_data(page, conf=True)
        assert len(got) == len(want) > 0
        assert [(g["text"], list(g["bbox"])) for g in got] == [(w["text"], w["bbox"]) for w in want]
        for g, w in zip(got, want):
            assert [c["char"] for c in g["chars"]] == [c["char"] for c in w["chars"]] and "".join(c["char"] for c in g["chars"]) == g["text"]
            assert [list(c["bbox"]) for c in g["chars"]] == [c["bbox"] for c in w["chars"]]
            assert [[list(p) for p in c["quad"]] for c in g["chars"]] == [[list(p) for p in c["quad"]] for c in w["chars"]]
        assert ("orient" in got[0]) == ("orient" in kw) and ("quad" in got[0]) == bool(kw.get("rectify")) and ("line" in got[0]) == bool(kw.get("lines"))
        assert pytuatara.images_to_data([page], weights["dir"], "o", **kw) == [got]
    assert "chars" not in pytuatara.image_to_data(page, weights["dir"], "o", lines=True)[0]


def test_ocr_cli_chars_prints_one_line_per_character(weights, engines, tmp_path):
    from PIL import Image
    from tuatara_amd import build as B
    B.build_examples()
    env = {k: v for k, v in os.environ.items() if k not in ENV_KEYS}
    png = os.path.join(DATA, "funsd_0001129658.png")
    out = subprocess.run([os.path.join(B.ROOT, "build", "examples", "ocr_cli"), "--chars", png, weights["dir"], str(tmp_path)],
                         capture_output=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    rgb = np.array(Image.open(png).convert("RGB"))
    want = engines(1).image_to_data(np.ascontiguousarray(rgb[:, :, ::-1]))    # the CLI feeds BGR
    lines = []
    for w in want:
        for c in w["chars"]:
            x1, y1, x2, y2 = (int(np.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1) for v in c["bbox"])     # lround: half away from zero
            lines.append(f"{c['char']} {x1} {y1} {x2} {y2}")
    assert len(lines) > 50
    assert out.stdout.decode("latin1") == "\n".join(lines) + "\n"
