"""GPU suite for character sets (DESIGN.md "Character sets"): decode_conf_kernel under a mask against float64, the recogniser under a set against the
oracle's forward restated with the masked argmax (tests/charset_ref.py), every place a token is chosen against the others bit for bit, and the page
entry points, the refusals and the callers under a set."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import charset_ref as CR
from tests.conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

DIGITS = "0123456789"
UPPER = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
LOWER = UPPER.lower()
TOL = 1e-3            # the project's logit bar
TAU = 2e-3            # twice the bar: the most a gap between two classes can move
CASES = {"digits": (7, DIGITS, None), "upper": (7, UPPER, None), "no-lower": (7, None, LOWER), "punct": (8, "\\-.", None)}


# ------------------------------------------------------------------------------------------------- 1. the decode kernel against float64
def _adversarial_logits(n, seed, blocked):
    """tests/test_gpu_conf.py's recipe, and additionally ties and +12 bumps on classes the mask blocks (kinds 7, 8)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 3.0, (n, 26, 95)).astype(np.float32)
    kind = rng.integers(0, 9, (n, 26))
    for i, p in zip(*np.nonzero(kind == 1)):                  # exact ties at the maximum: the first one wins
        t = rng.choice(95, rng.integers(2, 5), replace=False)
        x[i, p, t] = x[i, p].max() + 1.0
    for i, p in zip(*np.nonzero(kind == 2)):                  # all equal: id 0
        x[i, p] = np.float32(rng.normal())
    for i, p in zip(*np.nonzero(kind == 3)):                  # near one-hot
        x[i, p, rng.integers(0, 95)] += 40.0
    for i, p in zip(*np.nonzero(kind == 4)):                  # spreads up to +-1e30
        x[i, p] = rng.uniform(-1e30, 1e30, 95).astype(np.float32)
    for i, p in zip(*np.nonzero(kind == 5)):                  # an EOS (id 0) or a dropped id (88) at this position
        x[i, p, 0 if rng.random() < 0.5 else 88] += 12.0
    if len(blocked):
        for i, p in zip(*np.nonzero(kind == 7)):              # a blocked class ties with the maximum, in front of it or behind it
            x[i, p, rng.choice(blocked)] = x[i, p].max()
        for i, p in zip(*np.nonzero(kind == 8)):              # a blocked class towers over the row
            x[i, p, rng.choice(blocked)] = x[i, p].max() + 12.0
    return x


def test_decode_kernel_against_float64(eng_x4):
    from tuatara_amd.engine import charset_mask, confidence_from_probs
    masks = {"digits": charset_mask(DIGITS), "one": charset_mask("q"), "all-but-one": charset_mask(None, "e"), "full": charset_mask()}
    assert np.array_equal(masks["full"], CR.FULL)
    for name, m in masks.items():
        a = CR.allowed(m)
        blocked = np.nonzero(~a)[0]
        for n, seed in ((1, 1), (37, 2), (300, 3)):
            x = _adversarial_logits(n, seed, blocked)
            ids, prob, conf = eng_x4.logits_confidence(x, mask=m)
            r_ids, r_prob, r_conf = CR.masked_decode(x, m)
            assert np.array_equal(ids, r_ids), (name, n)
            assert a[ids].all(), (name, n)                                     # no id outside the mask
            rel = np.abs(prob.astype(np.float64) - r_prob) / r_prob
            print(f"{name} n={n}: max relative |prob - float64| {rel.max():.2e}; rows whose unconstrained argmax is blocked: {int((~a[x.argmax(-1)]).sum())}")
            assert rel.max() <= 2e-6, (name, n)
            assert (prob > 0).all() and (prob <= 1).all()
            for i in range(n):
                _, c = confidence_from_probs(ids[i], prob[i])
                assert c.tobytes() == conf[i:i + 1].tobytes(), (name, n, i, c, conf[i])
            if name == "full":                                                 # all 95 bits: the bits of the call without a mask
                p_ids, p_prob, p_conf = eng_x4.logits_confidence(x)
                assert ids.tobytes() == p_ids.tobytes() and prob.tobytes() == p_prob.tobytes() and conf.tobytes() == p_conf.tobytes(), n
            elif n > 1:
                assert (~a[x.argmax(-1)]).any()                                # the mask had something to do


# ------------------------------------------------------------------------------------------------- 2. the recogniser against the masked oracle
def _run_case(eng, parseq, case):
    """one case on one engine -> everything the comparisons need (the oracle's part is memoised in charset_ref)"""
    from tuatara_amd.engine import charset_mask
    seed, allow, deny = CASES[case]
    crops = CR.sweep_crops(seed)
    m = charset_mask(allow, deny)
    ref, ref_ar = CR.masked_oracle_logits(parseq, crops, m)
    assert np.array_equal(eng.charset, CR.FULL)
    eng.set_charset(allow, deny)
    try:
        assert np.array_equal(eng.charset, m)
        got, got_ar, ids = eng.parseq_logits(crops, want_ar=True)
    finally:
        eng.set_charset()
    assert np.array_equal(eng.charset, CR.FULL)
    return crops, m, ref, ref_ar, got, got_ar, np.asarray(ids).reshape(-1, 26)


@pytest.mark.parametrize("which", ["x4", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_recogniser_against_the_masked_oracle(which, case, eng_x4, eng_f32, oracle_models):
    from oracle import post
    from tuatara_amd.engine import decode_ids
    eng = eng_x4 if which == "x4" else eng_f32
    _, parseq = oracle_models
    crops, m, ref, ref_ar, got, got_ar, ids = _run_case(eng, parseq, case)
    a = CR.allowed(m)
    out = CR.left_out(ref, ref_ar, m, TAU)
    assert out.sum() <= 3, int(out.sum())
    keep = ~out
    r_ids, _, _ = CR.masked_decode(ref, m)
    r_ar, _, _ = CR.masked_decode(ref_ar, m)
    g_ar, _, _ = CR.masked_decode(got_ar, m)
    up = CR.upto_first_eos(r_ar)                                               # AR positions up to and including the oracle's AR EOS
    err, err_ar = np.abs(got - ref)[keep], np.abs(got_ar - ref_ar)[keep][up[keep]]
    print(f"{which} {case}: {int(out.sum())} of {len(crops)} crops left out; max |dlogit| refined {err.max():.2e}, AR up to EOS {err_ar.max():.2e}")
    assert np.isfinite(got).all() and np.isfinite(got_ar).all()
    assert err.max() < TOL and err_ar.max() < TOL
    assert np.array_equal(ids[keep], r_ids[keep])
    assert np.array_equal(g_ar[keep][up[keep]], r_ar[keep][up[keep]])
    assert a[ids].all()                                                        # every id inside the mask, the left-out crops' too
    s_ref, _ = post.decode_logits(np.where(a, ref, -np.inf).astype(np.float32))
    s_got = [decode_ids(r) for r in ids]
    assert [s for s, k in zip(s_got, keep) if k] == [s for s, k in zip(s_ref, keep) if k]
    # the test bites: the set changes what is read, and for A-Z the loop runs on without its early exit
    _, plain_ids = eng.parseq_logits(crops)
    differ = sum(decode_ids(p) != s for p, s in zip(np.asarray(plain_ids).reshape(-1, 26), s_got))
    never = int((~(g_ar == 0).any(1)).sum())
    print(f"   {differ} crops read differently from the unconstrained engine; {never} never emit EOS in the AR pass")
    assert differ >= 20, differ
    if case == "upper":
        assert never >= 10, never


# ------------------------------------------------------------------------------------------------- 3. every place a token is chosen
def test_every_place_a_token_is_chosen_agrees(eng_x4, oracle_models):
    _, parseq = oracle_models
    runs = {}
    try:
        for key in (None, "embed_fold", "argmax_fold", "ar_host_check"):
            if key:
                assert eng_x4.set_tuning(key, 0) == 0
            _, m, _, _, got, got_ar, ids = _run_case(eng_x4, parseq, "digits")
            runs[key] = (got, got_ar, ids)
            if key:
                assert eng_x4.set_tuning(key, 10 if key == "ar_host_check" else 1) == 0
    finally:
        eng_x4.set_charset()
        for key, v in (("embed_fold", 1), ("argmax_fold", 1), ("ar_host_check", 10)):
            eng_x4.set_tuning(key, v)
    base = runs[None]
    assert CR.allowed(m)[base[2]].all()
    for key, r in runs.items():
        for x, y in zip(r, base):
            assert np.array_equal(x, y), key


# ------------------------------------------------------------------------------------------------- 4. pages
@pytest.fixture(scope="module")
def pages():
    from tuatara_amd import synth
    return [synth.synthetic_page(60 + i, 1024, 768, n_words=14 + 6 * i) for i in range(2)]


def _same_page(x, y):
    return (x.texts == y.texts and x.ids.tobytes() == y.ids.tobytes() and x.bbox.tobytes() == y.bbox.tobytes() and x.prob.tobytes() == y.prob.tobytes()
            and x.conf.tobytes() == y.conf.tobytes())


def test_pages_under_a_set(eng_x4, weights, funsd, pages):
    from tuatara_amd.engine import DeviceBuffer, Engine, EngineError, charset_mask
    m = charset_mask(DIGITS)
    imgs = pages + [funsd]
    plain = eng_x4.images_to_data(imgs, conf=True)
    buf = DeviceBuffer(2 * 1024 * 768 * 3)
    try:
        eng_x4.set_charset(DIGITS)
        single = [eng_x4.image_to_data(p, conf=True) for p in imgs]
        many = eng_x4.images_to_data(imgs, conf=True)
        assert [list(r) for r in many] == single
        differ = 0
        for img, p, r in zip(imgs, plain, many):
            assert len(r) == len(p) > 0                                          # items, order, boxes: the detector's, untouched by the set
            assert r.bbox.tobytes() == p.bbox.tobytes()
            assert all(set(t) <= set(DIGITS) for t in r.texts)
            assert CR.allowed(m)[r.ids].all()
            differ += sum(s != t for s, t in zip(r.texts, p.texts))
            # each item's ids, prob and conf: the recogniser and the masked decode on the page's own crop batch (test_gpu_conf.py's composition)
            canvas, ratio = eng_x4.resize_canvas(img)
            crops, _ = eng_x4.pack_crops(img, eng_x4.ccl_boxes(eng_x4.craft_heatmap(canvas)), ratio)
            assert len(crops) == len(r)
            lg, ids = eng_x4.parseq_logits(crops)
            d_ids, d_prob, d_conf = eng_x4.logits_confidence(lg, mask=m)
            assert np.array_equal(ids, r.ids) and np.array_equal(d_ids, r.ids)
            assert d_prob.tobytes() == r.prob.tobytes() and d_conf.tobytes() == r.conf.tobytes()
        assert differ > 0
        # the other entry points, bit for bit
        buf.upload(np.stack(pages))
        dev = eng_x4.pages_to_data_dev(buf, 2, 1024, 768, conf=True)
        assert all(_same_page(x, y) for x, y in zip(dev, many[:2]))
        devv = eng_x4.pages_to_data_dev_v([(buf.ptr + k * 1024 * 768 * 3, 1024, 768) for k in range(2)], conf=True)
        assert all(_same_page(x, y) for x, y in zip(devv, many[:2]))
        streamed = []
        for k in range(2):
            streamed += eng_x4.stream_push(buf.ptr + k * 1024 * 768 * 3, 1, 1024, 768, conf=True)
            with pytest.raises(EngineError, match="in flight"):                  # between a push and its flush
                eng_x4.set_charset(UPPER)
            with pytest.raises(EngineError, match="in flight"):
                eng_x4.set_charset()
            assert np.array_equal(eng_x4.charset, m)                            # a refused call leaves the set in place
        while True:
            r = eng_x4.stream_flush(conf=True)
            if not r:
                break
            streamed += r
        assert len(streamed) == 2 and all(_same_page(x, y) for x, y in zip(streamed, many[:2]))
        with pytest.raises(EngineError, match="'~'"):                            # a failed call leaves it in place too
            eng_x4.set_charset("12~")
        assert np.array_equal(eng_x4.charset, m)
    finally:
        while eng_x4.stream_flush():
            pass
        eng_x4.set_charset(None)
        buf.free()
    # after the reset: the bits of an engine that never had a set
    again = eng_x4.images_to_data(imgs, conf=True)
    fresh = Engine(weights["dir"])
    never = fresh.images_to_data(imgs, conf=True)
    fresh.close()
    assert all(_same_page(x, y) for x, y in zip(again, plain)) and all(_same_page(x, y) for x, y in zip(again, never))


def test_orientation_and_character_boxes_under_a_set(weights, pages, funsd):
    from tuatara_amd.engine import Engine
    eng = Engine(weights["dir"], orient=1, chars=1)                              # TTR_ORIENT_FLIP
    base = Engine(weights["dir"])
    try:
        eng.set_charset(DIGITS)
        base.set_charset(DIGITS)
        turned = 0
        for img in pages + [funsd]:
            r, b = eng.images_to_data([img], conf=True)[0], base.images_to_data([img], conf=True)[0]
            assert len(r) == len(b) > 0 and r.bbox.tobytes() == b.bbox.tobytes()
            assert all(set(t) <= set(DIGITS) for t in r.texts)
            assert r.orient_conf.shape == (len(r), 2)
            assert r.orient_conf[:, 0].tobytes() == b.conf.tobytes()             # candidate 0: the constrained reading's conf, not the free one's
            z = r.orient == 0
            assert r.conf.tobytes() == r.orient_conf[np.arange(len(r)), r.orient // 2].tobytes()
            assert (r.orient_conf[~z, 1] > r.orient_conf[~z, 0]).all() and (r.orient_conf[z, 1] <= r.orient_conf[z, 0]).all()
            assert np.array_equal(r.ids[z], b.ids[z])
            assert (np.diff(r.char_first) == [len(t) for t in r.texts]).all()    # one box per character of the constrained text
            turned += int((~z).sum())
        print(f"{turned} words read turned under the set")
    finally:
        eng.close()
        base.close()


def test_bf16_refuses_a_restricting_set(eng_bf16):
    from tuatara_amd.engine import EngineError
    with pytest.raises(EngineError, match="bf16"):
        eng_bf16.set_charset(DIGITS)
    with pytest.raises(EngineError, match="bf16"):
        eng_bf16.set_charset(None, "|")
    assert np.array_equal(eng_bf16.charset, CR.FULL)
    eng_bf16.set_charset()                                                       # NULL, NULL and a full set succeed
    eng_bf16.set_charset("", "")
    assert np.array_equal(eng_bf16.charset, CR.FULL)


# ------------------------------------------------------------------------------------------------- callers
def test_pytuatara_keywords_and_ocr_cli(weights, pages, funsd, eng_x4, monkeypatch, tmp_path):
    from tuatara_amd import build as B
    B.build_pytuatara()
    B.build_examples()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ALLOWLIST", "TUATARA_BLOCKLIST"):
        monkeypatch.delenv(k, raising=False)
    page = pages[0]
    try:
        eng_x4.set_charset(DIGITS, "7")
        want = eng_x4.image_to_data(page, conf=True)
        eng_x4.set_charset(DIGITS)
        want_bgr = eng_x4.image_to_data(np.ascontiguousarray(funsd[:, :, ::-1]))     # the CLI feeds BGR
    finally:
        eng_x4.set_charset()
    plain = pytuatara.image_to_data(page, weights["dir"], "o")
    got = pytuatara.image_to_data(page, weights["dir"], "o", conf=True, allowlist=DIGITS, blocklist="7")
    assert [(r["text"], list(r["bbox"]), r["conf"]) for r in got] == [(g["text"], g["bbox"], g["conf"]) for g in want]
    assert all(set(r["text"]) <= set("012345689") for r in got) and any(r["text"] for r in got)
    assert pytuatara.images_to_data([page], weights["dir"], "o", conf=True, allowlist=DIGITS, blocklist="7") == [got]
    assert pytuatara.image_to_data(page, weights["dir"], "o") == plain             # reset after the call
    with pytest.raises(ValueError, match="'~'"):
        pytuatara.image_to_data(page, weights["dir"], "o", allowlist="~")
    assert pytuatara.image_to_data(page, weights["dir"], "o") == plain             # ... also when it raised
    monkeypatch.setenv("TUATARA_ALLOWLIST", DIGITS)
    monkeypatch.setenv("TUATARA_BLOCKLIST", "7")
    assert [r["text"] for r in pytuatara.image_to_data(page, weights["dir"], "o")] == [g["text"] for g in want]
    monkeypatch.delenv("TUATARA_ALLOWLIST")
    monkeypatch.delenv("TUATARA_BLOCKLIST")
    env = {k: v for k, v in os.environ.items() if k not in ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ALLOWLIST", "TUATARA_BLOCKLIST")}
    png = os.path.join(DATA, "funsd_0001129658.png")
    out = subprocess.run([os.path.join(B.ROOT, "build", "examples", "ocr_cli"), "--allowlist", DIGITS, png, weights["dir"], str(tmp_path)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = [ln.split("\t") for ln in out.stdout.splitlines()]
    assert len(lines) == len(want_bgr) > 20
    for (bb, text), g in zip(lines, want_bgr):
        assert [float(v) for v in bb.split()] == g["bbox"] and text == g["text"] and set(text) <= set(DIGITS)
