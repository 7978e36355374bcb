"""GPU suite for the character alternatives (DESIGN.md "Character alternatives"): decode_alts_kernel against the numpy restatement (tests/alts_ref.py) on
adversarial logits, under one mask and under a table of row masks; the engine's entry points against each other and against the same engine with
alternatives off, bit for bit; regions under their own sets; the refusals; and the callers (pytuatara alts=, ocr_cli --alts / --nbest)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import alts_ref as AR
from tests.conftest import DATA, GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DIGITS = "0123456789"
UPPER = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
LOWER = "abcdefghijklmnopqrstuvwxyz"


@pytest.fixture(scope="module")
def eng(weights):
    """an f16x4 engine of this module's own: the tests switch its alternatives on and off (and leave them off)"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine
    build_lib()
    return Engine(weights["dir"])


@pytest.fixture(scope="module")
def pages():
    from tuatara_amd import synth
    return [synth.synthetic_page(60 + i, 1024, 768, n_words=14 + 6 * i) for i in range(2)]


@pytest.fixture(scope="module")
def itos():
    with open(os.path.join(GOLDEN, "g1_ref_tokenizer.json")) as f:
        return [chr(c) for c in json.load(f)["itos"]]


class _Alts:
    """set_alternatives(k) for a block, off again behind it"""

    def __init__(self, eng, k):
        self.eng, self.k = eng, k

    def __enter__(self):
        self.eng.set_alternatives(self.k)
        return self.eng

    def __exit__(self, *exc):
        self.eng.set_alternatives(0)


def _adversarial_logits(n, seed):
    """test_gpu_conf.py's kind of rows, plus ties below the maximum (the later rounds' ties)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 3.0, (n, 26, 95)).astype(np.float32)
    kind = rng.integers(0, 8, (n, 26))
    for i, p in zip(*np.nonzero(kind == 1)):                  # exact ties at the maximum: the lower class first
        t = rng.choice(95, rng.integers(2, 5), replace=False)
        x[i, p, t] = x[i, p].max() + 1.0
    for i, p in zip(*np.nonzero(kind == 2)):                  # all equal: classes 0, 1, 2, ... each with 1/95
        x[i, p] = np.float32(rng.normal())
    for i, p in zip(*np.nonzero(kind == 3)):                  # near one-hot
        x[i, p, rng.integers(0, 95)] += 40.0
    for i, p in zip(*np.nonzero(kind == 4)):                  # spreads up to +-1e30
        x[i, p] = rng.uniform(-1e30, 1e30, 95).astype(np.float32)
    for i, p in zip(*np.nonzero(kind == 5)):                  # an EOS (id 0) or a dropped id (88) at this position
        x[i, p, 0 if rng.random() < 0.5 else 88] += 12.0
    for i, p in zip(*np.nonzero(kind == 6)):                  # ties below the maximum, across the two halves of the wave's lanes
        t = rng.choice(95, rng.integers(3, 9), replace=False)
        x[i, p, t] = np.sort(x[i, p])[-2] - np.float32(0.5)
        x[i, p, t[:2]] = np.sort(x[i, p])[-1]                 # ... and two on top
    return x


_REF = {}


def _ref(n):
    """the adversarial logits of n crops and their restatement at K = 8 (a smaller K is its prefix), computed once"""
    if n not in _REF:
        x = _adversarial_logits(n, 10 + n)
        _REF[n] = (x,) + AR.topk(x, 8)
    return _REF[n]


def _check_probs(got, p64, d, where):
    """every slot within its own rounding bound of float64 (DESIGN.md "Character alternatives"), non-increasing up to it, inside [0, 1]"""
    got64 = got.astype(np.float64)
    bound = p64 * (2.5e-6 + np.abs(d) * 2.0 ** -23)
    big = p64 >= 1e-30
    err = np.abs(got64 - p64)
    print(f"{where}: max |alt_prob - float64| / bound = {(err[big] / bound[big]).max():.3f}, slots below 1e-30: {int((~big).sum())}, largest there {got64[~big].max() if (~big).any() else 0:.1e}")
    assert (err[big] <= bound[big]).all(), where
    assert (got64[~big] <= 1e-29).all(), where
    slack = np.where(big, bound, 1e-29)
    assert (got64[..., 1:] <= got64[..., :-1] + slack[..., 1:] + slack[..., :-1]).all(), where
    assert (got >= 0).all() and (got <= 1).all(), where


@pytest.mark.parametrize("k", [2, 5, 8])
@pytest.mark.parametrize("n", [1, 5, 37])
def test_kernel_against_the_restatement(eng, n, k):
    x, r_ids, r_p64, r_d = _ref(n)
    ids, prob = eng.logits_alternatives(x, k)
    assert ids.shape == prob.shape == (n, 26, k)
    assert np.array_equal(ids, r_ids[..., :k])
    c_ids, c_prob, _ = eng.logits_confidence(x)
    assert np.array_equal(ids[..., 0], c_ids)
    assert prob[..., 0].tobytes() == c_prob.tobytes()                                    # slot 0 is prob, bit for bit
    _check_probs(prob, r_p64[..., :k], r_d[..., :k], f"n={n} k={k}")


def _mask(classes):
    m = np.zeros(3, np.uint32)
    for c in classes:
        m[c >> 5] |= np.uint32(1 << (c & 31))
    return m


def test_a_mask_of_three_classes_leaves_two_slots_empty(eng):
    x = _ref(5)[0]
    m = _mask([0, 7, 70])                                                                # the EOS and two characters, one in each half of the lanes
    ids, prob = eng.logits_alternatives(x, 5, set_of=np.zeros(5, np.int32), sets=m[None])
    r_ids, r_p64, r_d = AR.topk(x, 5, m)
    assert np.array_equal(ids, r_ids)
    assert (ids[..., 3:] == -1).all() and (prob[..., 3:] == 0).all() and (ids[..., :3] >= 0).all()
    assert set(np.unique(ids)) == {-1, 0, 7, 70}                                         # no blocked class anywhere
    c_ids, c_prob, _ = eng.logits_confidence(x, mask=m)
    assert np.array_equal(ids[..., 0], c_ids) and prob[..., 0].tobytes() == c_prob.tobytes()
    _check_probs(prob[..., :3], r_p64[..., :3], r_d[..., :3], "three classes")


def test_rows_of_different_sets_in_one_block(eng):
    from tuatara_amd.engine import charset_mask
    x = _adversarial_logits(9, 77)
    sets = np.stack([charset_mask(DIGITS), charset_mask(UPPER), charset_mask(None, LOWER), _mask([0, 3, 90])])
    set_of = np.array([0, 1, 2, 3, 3, 2, 1, 0, -1], np.int32)                            # (-1: the engine's own set - none here, every class)
    row_masks = np.stack([sets[s] if s >= 0 else _mask(range(95)) for s in set_of])
    ids, prob = eng.logits_alternatives(x, 5, set_of=set_of, sets=sets)
    r_ids, r_p64, r_d = AR.topk(x, 5, row_masks)
    assert np.array_equal(ids, r_ids)                                                    # each row under its own set
    c_ids, c_prob, _ = eng.logits_confidence(x, set_of=set_of, sets=sets)
    assert np.array_equal(ids[..., 0], c_ids) and prob[..., 0].tobytes() == c_prob.tobytes()
    for i, s in enumerate(set_of):
        assert set(np.unique(ids[i])) <= set(AR.allowed_classes(row_masks[i]).tolist()) | {-1}, i
    _check_probs(prob, r_p64, r_d, "four sets over nine rows")
    with _Alts(eng, 3):                                                                  # sets == None: the engine's own set
        eng.set_charset(DIGITS)
        try:
            ids, _ = eng.logits_alternatives(x, 3)
        finally:
            eng.set_charset()
    assert np.array_equal(ids, AR.topk(x, 3, sets[0])[0])


def _same_standard_fields(a, b):
    assert a.texts == b.texts
    for f in ("bbox", "ids", "conf", "prob"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert (a.quad is None) == (b.quad is None)


def _drain(eng, first):
    out = list(first)
    while True:
        r = eng.stream_flush()
        if not r:
            return out
        out += r


def test_engine_entry_points_agree_and_nothing_else_changes(eng, pages):
    from tuatara_amd.engine import DeviceBuffer
    buf = DeviceBuffer(2 * 1024 * 768 * 3)
    buf.upload(np.stack(pages))
    off = eng.pages_to_data_dev(buf, 2, 1024, 768)
    assert all(r.alt_ids is None and r.alt_prob is None and len(r) > 0 for r in off)
    assert all("alternatives" not in d for r in off for d in r)
    with _Alts(eng, 5):
        assert eng.alternatives == 5
        dev = eng.pages_to_data_dev(buf, 2, 1024, 768)
        single = [eng.image_to_data(p) for p in pages]                                   # the synchronous call
        many = eng.images_to_data(pages)                                                 # the list form
        vform = eng.pages_to_data_dev_v([(buf.ptr + k * 1024 * 768 * 3, 1024, 768) for k in range(2)])
        streamed = []
        for k in range(2):                                                               # push, push, flush: one page per batch, both slots
            streamed += eng.stream_push(buf.ptr + k * 1024 * 768 * 3, 1, 1024, 768)
        streamed = _drain(eng, streamed)
        # the raw result: K and the views
        arr = (C.c_void_p * 2)()
        assert eng.lib.ttr_pages_to_data_dev(eng.h, buf.ptr, 2, 1024, 768, arr) == 0
        for i in range(2):
            assert eng.lib.ttr_result_alt_k(arr[i]) == 5 and eng.lib.ttr_result_alt_ids_all(arr[i]) and eng.lib.ttr_result_alt_probs_all(arr[i])
            got = np.ctypeslib.as_array(eng.lib.ttr_result_alt_ids(arr[i], 1), (26, 5))
            assert np.array_equal(got, dev[i].alt_ids[1])
            eng.lib.ttr_result_free(arr[i])
    assert eng.alternatives == 0
    for a, b in zip(off, dev):
        _same_standard_fields(a, b)                                                      # every field that existed before: bit for bit those of K = 0
        assert [{k: v for k, v in d.items() if k != "alternatives"} for d in b] == list(a)
    for r in dev:
        n = len(r)
        assert r.alt_ids.shape == r.alt_prob.shape == (n, 26, 5) and r.alt_ids.dtype == np.int32 and r.alt_prob.dtype == np.float32
        assert np.array_equal(r.alt_ids[:, :, 0], r.ids)
        assert r.alt_prob[:, :, 0].tobytes() == r.prob.tobytes()
        assert ((r.alt_ids >= -1) & (r.alt_ids < 95)).all() and (r.alt_prob >= 0).all() and (r.alt_prob <= 1).all()
        for i in range(n):
            text, score = r.nbest(i, 1)[0]
            assert text == r.texts[i] and np.float32(score).tobytes() == r.conf[i:i + 1].tobytes(), i
            alts = r[i]["alternatives"]
            assert len(alts) == len(r.texts[i]) and all(a[0][0] == ch for a, ch in zip(alts, r.texts[i]))
        best = r.nbest(0, 8)
        assert [float(s) for _, s in best] == sorted((float(s) for _, s in best), reverse=True) and len({t for t, _ in best}) == len(best)
    assert [list(r) for r in dev] == single
    for other in (many, vform, streamed):
        assert len(other) == 2
        for a, b in zip(dev, other):
            _same_standard_fields(a, b)
            assert a.alt_ids.tobytes() == b.alt_ids.tobytes() and a.alt_prob.tobytes() == b.alt_prob.tobytes()
    # off again: no alternatives anywhere, the views are NULL, K is 0
    arr = (C.c_void_p * 2)()
    assert eng.lib.ttr_pages_to_data_dev(eng.h, buf.ptr, 2, 1024, 768, arr) == 0
    for i in range(2):
        assert eng.lib.ttr_result_alt_k(arr[i]) == 0 and not eng.lib.ttr_result_alt_ids_all(arr[i]) and not eng.lib.ttr_result_alt_probs_all(arr[i])
        assert not eng.lib.ttr_result_alt_ids(arr[i], 0) and not eng.lib.ttr_result_alt_probs(arr[i], 0)
        eng.lib.ttr_result_free(arr[i])
    again = eng.pages_to_data_dev(buf, 2, 1024, 768)
    for a, b in zip(off, again):
        _same_standard_fields(a, b)
        assert b.alt_ids is None
    buf.free()


def test_a_character_set_bounds_the_alternatives(eng, pages):
    allowed = {-1} | set(AR.allowed_classes(__import__("tuatara_amd.engine", fromlist=["charset_mask"]).charset_mask(DIGITS)).tolist())
    assert allowed == {-1} | set(range(11))                                              # the EOS and the ten digits
    eng.set_charset(DIGITS)
    try:
        with _Alts(eng, 8):
            r = eng.images_to_data([pages[0]])[0]
    finally:
        eng.set_charset()
    assert len(r) > 0 and set(np.unique(r.alt_ids)) <= allowed
    assert np.array_equal(r.alt_ids[:, :, 0], r.ids) and r.alt_prob[:, :, 0].tobytes() == r.prob.tobytes()
    assert all(ch in DIGITS for alts in r[0]["alternatives"] for ch, _ in alts)


def test_an_f32_engine_at_k_two(eng_f32, pages):
    plain = eng_f32.images_to_data([pages[0]])[0]
    with _Alts(eng_f32, 2):
        r = eng_f32.images_to_data([pages[0]])[0]
    _same_standard_fields(plain, r)
    assert r.alt_ids.shape == (len(r), 26, 2)
    assert np.array_equal(r.alt_ids[:, :, 0], r.ids) and r.alt_prob[:, :, 0].tobytes() == r.prob.tobytes()
    for i in range(len(r)):
        text, score = r.nbest(i, 1)[0]
        assert text == r.texts[i] and np.float32(score).tobytes() == r.conf[i:i + 1].tobytes()


def test_regions_keep_to_their_own_sets(eng, pages):
    from tuatara_amd.engine import charset_mask
    page = pages[1]
    words = eng.image_to_data(page)
    rects = [[int(v) for v in (np.floor(w["bbox"][0]), np.floor(w["bbox"][1]), np.ceil(w["bbox"][2]) + 1, np.ceil(w["bbox"][3]) + 1)] for w in words[:3]]
    charsets = [(DIGITS, None), (UPPER, None), (LOWER, None)]
    regions = [{"rect": rc, "set": s} for s, rc in enumerate(rects)]
    plain = eng.read_regions(page, regions, charsets)
    with _Alts(eng, 5):
        got = eng.read_regions(page, regions, charsets)
    assert len(got) == 3
    for s, (g, p) in enumerate(zip(got, plain)):
        assert {k: v for k, v in g.items() if k not in ("alt_ids", "alt_prob", "alternatives")} == p      # nothing else changes
        allowed = set(AR.allowed_classes(charset_mask(*charsets[s])).tolist()) | {-1}
        assert g["alt_ids"].shape == (26, 5) and set(np.unique(g["alt_ids"])) <= allowed, s
        assert g["alt_ids"][:, 0].tolist() == g["ids"] and g["alt_prob"][:, 0].tolist() == g["prob"]
        assert all(ch in charsets[s][0] for alts in g["alternatives"] for ch, _ in alts)
    assert len({tuple(np.unique(g["alt_ids"][:, 1:]).tolist()) for g in got}) == 3             # three sets, three different sets of runners-up


def test_refusals(eng, eng_bf16, weights, pages):
    from tuatara_amd.engine import Comm, DeviceBuffer, Engine, EngineError
    from tuatara_amd.launch import free_port
    for k in (1, 9, -1):
        with pytest.raises(EngineError, match="2..8"):
            eng.set_alternatives(k)
    assert eng.alternatives == 0
    with pytest.raises(EngineError, match="bf16"):
        eng_bf16.set_alternatives(3)
    eng_bf16.set_alternatives(0)                                                         # off is always accepted
    turned = Engine(weights["dir"], orient=1)
    with pytest.raises(EngineError, match="orientation"):
        turned.set_alternatives(3)
    assert turned.alternatives == 0
    turned.close()
    with pytest.raises(EngineError, match="orientation"):
        Engine(weights["dir"], orient=1, alts=3)
    buf = DeviceBuffer(1024 * 768 * 3)
    buf.upload(pages[0])
    x = np.zeros((1, 26, 95), np.float32)
    assert eng.stream_push(buf, 1, 1024, 768) == []
    with pytest.raises(EngineError, match="streamed batches"):                           # setting while batches stream
        eng.set_alternatives(3)
    with pytest.raises(EngineError, match="streamed batches"):
        eng.logits_alternatives(x, 3)
    assert eng.alternatives == 0
    plain = _drain(eng, [])
    assert len(plain) == 1 and plain[0].alt_ids is None
    with pytest.raises(EngineError, match="2..8"):
        eng.logits_alternatives(x, 9)
    # with a communicator: each rank's own results carry alternatives, the gathered payload is the standard block; the sharded call refuses
    comm = Comm(eng, 0, 1, "127.0.0.1", free_port(), transport="socket")
    try:
        with _Alts(eng, 3):
            want = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
            comm.attach(True)
            got = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
            _, g_ids = comm.last_gathered()
            g_conf, g_prob = comm.last_gathered_conf()
            comm.attach(False)
            with pytest.raises(EngineError, match="alternatives"):
                comm.pages_to_data_sharded(buf, 1, 1024, 768)
        _same_standard_fields(plain[0], got)
        assert got.alt_ids.tobytes() == want.alt_ids.tobytes() and got.alt_prob.tobytes() == want.alt_prob.tobytes()
        assert np.array_equal(g_ids, got.ids) and g_conf.tobytes() == got.conf.tobytes() and g_prob.tobytes() == got.prob.tobytes()
        assert [list(r) for r in comm.pages_to_data_sharded(buf, 1, 1024, 768)] == [list(plain[0])]      # off again: the sharded call runs
    finally:
        comm.attach(False)
        comm.close()
        buf.free()


# ------------------------------------------------------------------------------------------------- callers (a child process each)
PYT = r'''
import json, os, sys
import numpy as np
from PIL import Image
sys.path.insert(0, os.path.join({root!r}, "build", "bindings"))
import pytuatara
img = np.array(Image.open({png!r}).convert("RGB"))
plain = pytuatara.image_to_data(img, {wdir!r}, "o", conf=True)
got = pytuatara.image_to_data(img, {wdir!r}, "o", conf=True, alts=3)
many = pytuatara.images_to_data([img], {wdir!r}, "o", conf=True, alts=3)
digits = pytuatara.image_to_data(img, {wdir!r}, "o", alts=2, allowlist="0123456789", lines=True)
again = pytuatara.image_to_data(img, {wdir!r}, "o", conf=True)
errors = []
for kw in (dict(alts=1), dict(alts=9), dict(alts=3, orient="flip")):
    try:
        pytuatara.image_to_data(img, {wdir!r}, "o", **kw)
        errors.append(None)
    except Exception as ex:
        errors.append([type(ex).__name__, str(ex)])
print("RESULT " + json.dumps(dict(plain=plain, got=got, same=(many == [got]), digits=digits, again=(again == plain), errors=errors)))
'''


def test_pytuatara_alts_keyword(eng, weights, funsd):
    from tuatara_amd import build
    build.build_pytuatara()
    png = os.path.join(DATA, "funsd_0001129658.png")
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    out = subprocess.run([sys.executable, "-c", PYT.format(root=ROOT, png=png, wdir=weights["dir"])], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    with _Alts(eng, 3):
        want = eng.image_to_data(funsd, conf=True)
    assert len(want) > 20 and len(res["got"]) == len(want)
    for g, w in zip(res["got"], want):
        assert set(g) == {"text", "bbox", "conf", "char_conf", "alternatives"}
        assert (g["text"], g["bbox"], g["conf"], g["char_conf"]) == (w["text"], w["bbox"], w["conf"], w["char_conf"])
        assert [[tuple(a) for a in alts] for alts in g["alternatives"]] == w["alternatives"]
    assert [{k: v for k, v in g.items() if k != "alternatives"} for g in res["got"]] == res["plain"]      # alts change nothing else
    assert res["same"] and res["again"]                                                  # the list form agrees; the cached engine is left without alternatives
    assert all(set(d) == {"text", "bbox", "line", "word", "alternatives"} for d in res["digits"])
    assert all(ch in DIGITS and len(alts) <= 2 for d in res["digits"] for alts in d["alternatives"] for ch, _ in alts)
    assert res["errors"][0][0] == "ValueError" and res["errors"][1][0] == "ValueError"
    assert res["errors"][2] is not None and "orientation" in res["errors"][2][1]        # orient with alts: the engine's message


def test_ocr_cli_alts_and_nbest(eng, weights, funsd, tmp_path):
    from tuatara_amd import build as B
    B.build_examples()
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    png = os.path.join(DATA, "funsd_0001129658.png")
    cli = os.path.join(B.ROOT, "build", "examples", "ocr_cli")
    out = subprocess.run([cli, "--alts", "3", "--nbest", "4", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    with _Alts(eng, 3):
        want = eng.images_to_data([np.ascontiguousarray(funsd[:, :, ::-1])], conf=True)[0]      # the CLI feeds BGR
    lines = out.stdout.splitlines()
    at = 0
    assert len(want) > 20
    for i, g in enumerate(want):
        bb, conf, text = lines[at].split("\t")
        at += 1
        assert [float(v) for v in bb.split()] == g["bbox"] and text == g["text"] and conf == f"{g['conf']:.6f}"
        for ch, alts in zip(g["text"], g["alternatives"]):
            assert lines[at] == f"\t{ch}:" + "".join(f" {c}={p:.6f}" for c, p in alts)
            at += 1
        for j, (t, s) in enumerate(want.nbest(i, 4)):
            assert lines[at] == f"\t#{j} {float(s):.6f} {t}"
            at += 1
    assert at == len(lines)
    bad = subprocess.run([cli, "--nbest", "4", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=60)
    assert bad.returncode == 1 and "--alts" in bad.stderr
