"""GPU suite for patterns (DESIGN.md "Patterns"): decode_pat_kernel alone against float64, the recogniser under a pattern against the oracle's forward
restated with the sequential choice (tests/pattern_ref.py), every tuning path against the default bit for bit, the page and region entry points, the
refusals, and the callers."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import charset_ref as CR
from tests import pattern_ref as PR
from tests.conftest import DATA, GOLDEN, ROOT
from tests.test_gpu_charset import _adversarial_logits
from tests.test_pattern_cpu import GPU_CASES

pytestmark = pytest.mark.gpu

DIGITS = "0123456789"
UPPER = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
TOL = 1e-3            # the project's logit bar
TAU = 2e-3            # twice the bar: the most a gap between two classes can move


@pytest.fixture(scope="module")
def itos():
    with open(os.path.join(GOLDEN, "g1_ref_tokenizer.json")) as f:
        return [chr(c) for c in json.load(f)["itos"]]


def _text(itos, row):
    """Tokenizer::decode on the usable classes: the characters before the first EOS"""
    row = list(row)
    return "".join(itos[c] for c in (row[:row.index(0)] if 0 in row else row) if c != 88)


# ------------------------------------------------------------------------------------------------- 1. the decode kernel alone against float64
DECODE_PATTERNS = [r"\d+", r"(ab)*", r"[A-Z]{2}\d{2,6}", r"\d+\.\d{2}"]


def _adversarial_rows(n, seed, dfas, never_eos):
    """tests/test_gpu_charset.py's recipe, then - position by position along the float64 walk, so that the states are the final ones - ties and +12 bumps on
    classes the state forbids, EOS bumps at non-accepting states, and rows that never prefer the EOS (the budget has to end them)"""
    x = _adversarial_logits(n, seed, np.zeros(0, np.int64))
    rng = np.random.default_rng(seed + 100)
    for i in range(n):
        d = dfas[i]
        if never_eos[i]:
            x[i] = np.clip(x[i], -60.0, 60.0)                               # (no +-1e30 row may lift the EOS back, or tie with it)
            x[i, :, 0] = -100.0
        s = d.start
        for p in range(26):
            a = PR.allowed_at(d.delta, d.mind, s, p)
            forbidden = np.nonzero(~a)[0]
            kind = int(rng.integers(0, 6))
            top = float(np.where(a, x[i, p], -np.inf).max())
            if len(forbidden) and np.isfinite(top) and abs(top) < 1e20:
                if kind == 0:                                                # a forbidden class ties with the best allowed one, in front of it or behind it
                    x[i, p, rng.choice(forbidden)] = top
                elif kind == 1:                                              # a forbidden class towers over the row
                    x[i, p, rng.choice(forbidden)] = top + 12.0
                elif kind == 2 and not a[0] and not never_eos[i]:            # the EOS towers at a state that does not accept
                    x[i, p, 0] = top + 12.0
            c = int(np.where(a, x[i, p].astype(np.float64), -np.inf).argmax())
            s = int(d.delta[s, c])
    return x


@pytest.mark.parametrize("n", [1, 7, 37])
def test_decode_kernel_against_float64(eng_x4, itos, n):
    from tuatara_amd.engine import confidence_from_probs
    assert eng_x4.pattern is None
    pattern_of = np.array([(i % 5) - 1 for i in range(n)] if n > 1 else [0], np.int32)           # four patterns and rows without one, in one call
    auto = [PR.compile_pattern(itos, p) for p in DECODE_PATTERNS]
    dfas = [auto[k] if k >= 0 else PR.none_pattern() for k in pattern_of]
    never = np.array([k in (0, 1) and i % 2 == 0 for i, k in enumerate(pattern_of)])              # \d+ and (ab)* rows that never prefer the EOS
    x = _adversarial_rows(n, 10 + n, dfas, never)
    ids, prob, conf = eng_x4.logits_decode_patterns(x, DECODE_PATTERNS, pattern_of)
    r_ids, r_prob, r_conf, _ = PR.sequential_decode(x, dfas)
    assert np.array_equal(ids, r_ids)
    rel = np.abs(prob.astype(np.float64) - r_prob) / r_prob
    print(f"n={n}: max relative |prob - float64| {rel.max():.2e}")
    assert rel.max() <= 2e-6
    assert (prob > 0).all() and (prob <= 1).all()
    plain = x.argmax(-1)
    for i in range(n):
        _, c = confidence_from_probs(ids[i], prob[i])
        assert c.tobytes() == conf[i:i + 1].tobytes(), (i, c, conf[i])
        k = int(pattern_of[i])
        if k >= 0:
            assert re.fullmatch(DECODE_PATTERNS[k], _text(itos, ids[i])), (i, DECODE_PATTERNS[k], _text(itos, ids[i]))
        if never[i]:                                                                              # the budget ended the row: (ab)* at position 24, \d+ at 25
            assert list(ids[i]).index(0) == (24 if k == 1 else 25), (i, k, ids[i])
    assert n == 1 or (ids != plain).any()                                                         # the patterns had something to do
    # a row without a pattern: the bits of the masked decode under its set (here the engine's own: every class)
    free = np.nonzero(pattern_of < 0)[0]
    if len(free):
        p_ids, p_prob, p_conf = eng_x4.logits_confidence(x[free])
        assert ids[free].tobytes() == p_ids.tobytes() and prob[free].tobytes() == p_prob.tobytes() and conf[free].tobytes() == p_conf.tobytes()


def test_decode_kernel_rows_under_their_own_sets(eng_x4, itos):
    """a pattern is compiled under the row's own set: [^a]+ under digits is \\d+, and a row without a pattern decodes as logits_confidence under its set"""
    from tuatara_amd.engine import charset_mask
    sets = np.stack([charset_mask(DIGITS), charset_mask(UPPER + DIGITS)])
    n = 12
    set_of = np.array([i % 3 - 1 for i in range(n)], np.int32)
    pattern_of = np.array([0 if i % 2 else -1 for i in range(n)], np.int32)
    masks = [None if s < 0 else sets[s] for s in set_of]
    dfas = [PR.compile_pattern(itos, r"[^a]+", m) if k >= 0 else PR.none_pattern(m) for k, m in zip(pattern_of, masks)]
    x = _adversarial_rows(n, 5, dfas, np.zeros(n, bool))
    ids, prob, conf = eng_x4.logits_decode_patterns(x, [r"[^a]+"], pattern_of, set_of=set_of, sets=sets)
    r_ids, r_prob, _, _ = PR.sequential_decode(x, dfas)
    assert np.array_equal(ids, r_ids)
    assert (np.abs(prob.astype(np.float64) - r_prob) / r_prob).max() <= 2e-6
    free = np.nonzero(pattern_of < 0)[0]
    p_ids, p_prob, p_conf = eng_x4.logits_confidence(x[free], set_of=set_of[free], sets=sets)
    assert ids[free].tobytes() == p_ids.tobytes() and prob[free].tobytes() == p_prob.tobytes() and conf[free].tobytes() == p_conf.tobytes()
    for i in np.nonzero((pattern_of >= 0) & (set_of == 0))[0]:
        assert re.fullmatch(r"\d+", _text(itos, ids[i]))


# ------------------------------------------------------------------------------------------------- 2. the recogniser against pattern_forward
def _run_case(eng, pattern, want_ar=True):
    crops = CR.sweep_crops(GPU_CASES[pattern])
    assert eng.pattern is None
    eng.set_pattern(pattern)
    try:
        assert eng.pattern == pattern
        out = eng.parseq_logits(crops, want_ar=want_ar)
    finally:
        eng.set_pattern()
    assert eng.pattern is None
    return (crops,) + tuple(out)


@pytest.mark.parametrize("which", ["x4", "f32"])
@pytest.mark.parametrize("pattern", list(GPU_CASES))
def test_recogniser_against_pattern_forward(which, pattern, eng_x4, eng_f32, oracle_models, itos):
    from tuatara_amd.engine import decode_ids
    eng = eng_x4 if which == "x4" else eng_f32
    _, parseq = oracle_models
    dfa = PR.compile_pattern(itos, pattern)
    crops, got, got_ar, ids = _run_case(eng, pattern)
    ids = np.asarray(ids).reshape(-1, 26)
    ref, ref_ar, r_tok, r_states = PR.pattern_oracle(parseq, crops, dfa, pattern)
    out = PR.left_out(ref, ref_ar, r_tok, r_states, dfa, TAU)
    assert out.sum() <= 3, int(out.sum())
    keep = ~out
    n = len(crops)
    r_ids, _, _, _ = PR.sequential_decode(ref, [dfa] * n)
    g_tok = PR.sequential_decode(got_ar, [dfa] * n)[0][:, :25]                 # the engine's AR choices: its own AR logits through the rule
    up = CR.upto_first_eos(r_tok)                                              # AR positions up to and including the oracle's AR EOS
    up26 = np.concatenate([up, np.zeros((n, 1), bool)], 1)
    err, err_ar = np.abs(got - ref)[keep], np.abs(got_ar - ref_ar)[keep][up26[keep]]
    print(f"{which} {pattern}: {int(out.sum())} of {n} crops left out; max |dlogit| refined {err.max():.2e}, AR up to EOS {err_ar.max():.2e}")
    assert np.isfinite(got).all() and np.isfinite(got_ar).all()
    assert err.max() < TOL and err_ar.max() < TOL
    assert np.array_equal(ids[keep], r_ids[keep])
    assert np.array_equal(g_tok[keep][up[keep]], r_tok[keep][up[keep]])
    s_got = [decode_ids(r) for r in ids]
    s_ref = [_text(itos, r) for r in r_ids]
    assert [s for s, k in zip(s_got, keep) if k] == [s for s, k in zip(s_ref, keep) if k]
    rx = re.compile(pattern)
    assert all(rx.fullmatch(s) for s in s_got), [s for s in s_got if not rx.fullmatch(s)]    # the left-out crops' too
    _, plain_ids = eng.parseq_logits(crops)
    differ = sum(decode_ids(p) != s for p, s in zip(np.asarray(plain_ids).reshape(-1, 26), s_got))
    print(f"   {differ} crops read differently from the unconstrained engine")
    assert differ >= 20, differ
    if pattern == r"\d{25}":
        assert not (g_tok == 0).any()                                          # no crop's AR pass emits EOS before column 26


# ------------------------------------------------------------------------------------------------- 3. every tuning path
def test_the_same_result_through_every_tuning_path(eng_x4):
    runs = {}
    try:
        for key in (None, "embed_fold", "argmax_fold", "ar_host_check"):
            if key:
                assert eng_x4.set_tuning(key, 0) == 0
            _, got, ids = _run_case(eng_x4, r"\d+\.\d{2}", want_ar=False)
            runs[key] = (got, ids)
            if key:
                assert eng_x4.set_tuning(key, 10 if key == "ar_host_check" else 1) == 0
    finally:
        eng_x4.set_pattern()
        for key, v in (("embed_fold", 1), ("argmax_fold", 1), ("ar_host_check", 10)):
            eng_x4.set_tuning(key, v)
    for key, r in runs.items():
        for x, y in zip(r, runs[None]):
            assert np.array_equal(x, y), key


# ------------------------------------------------------------------------------------------------- 4. pages and regions
@pytest.fixture(scope="module")
def pages():
    from tuatara_amd import synth
    return [synth.synthetic_page(60 + i, 1024, 768, n_words=14 + 6 * i) for i in range(2)]


def _same_page(x, y):
    return (x.texts == y.texts and x.ids.tobytes() == y.ids.tobytes() and x.bbox.tobytes() == y.bbox.tobytes() and x.prob.tobytes() == y.prob.tobytes()
            and x.conf.tobytes() == y.conf.tobytes())


def test_pages_under_an_engine_pattern(eng_x4, weights, funsd, pages):
    from tuatara_amd.engine import DeviceBuffer, Engine, EngineError
    pattern = r"[A-Z][a-z]*"
    rx = re.compile(pattern)
    imgs = pages + [funsd]
    plain = eng_x4.images_to_data(imgs, conf=True)
    buf = DeviceBuffer(2 * 1024 * 768 * 3)
    try:
        eng_x4.set_pattern(pattern)
        single = [eng_x4.image_to_data(p, conf=True) for p in imgs]
        many = eng_x4.images_to_data(imgs, conf=True)
        assert [list(r) for r in many] == single
        differ = 0
        for p, r in zip(plain, many):
            assert len(r) == len(p) > 0 and r.bbox.tobytes() == p.bbox.tobytes()     # items, order, boxes: the detector's
            assert all(rx.fullmatch(t) for t in r.texts), [t for t in r.texts if not rx.fullmatch(t)]
            differ += sum(s != t for s, t in zip(r.texts, p.texts))
        assert differ > 0
        buf.upload(np.stack(pages))
        dev = eng_x4.pages_to_data_dev(buf, 2, 1024, 768, conf=True)
        assert all(_same_page(x, y) for x, y in zip(dev, many[:2]))
        devv = eng_x4.pages_to_data_dev_v([(buf.ptr + k * 1024 * 768 * 3, 1024, 768) for k in range(2)], conf=True)
        assert all(_same_page(x, y) for x, y in zip(devv, many[:2]))
        streamed = []
        for k in range(2):
            streamed += eng_x4.stream_push(buf.ptr + k * 1024 * 768 * 3, 1, 1024, 768, conf=True)
            with pytest.raises(EngineError, match="ttr_engine_set_pattern: streamed batches are in flight"):     # between a push and its flush
                eng_x4.set_pattern(r"\d+")
            with pytest.raises(EngineError, match="in flight"):
                eng_x4.set_pattern()
            assert eng_x4.pattern == pattern                                          # a refused call leaves the pattern in place
        while True:
            r = eng_x4.stream_flush(conf=True)
            if not r:
                break
            streamed += r
        assert len(streamed) == 2 and all(_same_page(x, y) for x, y in zip(streamed, many[:2]))
        with pytest.raises(EngineError, match=r"ttr_engine_set_pattern: pattern: offset 0: '\(' without its '\)'"):
            eng_x4.set_pattern("(")
        assert eng_x4.pattern == pattern                                              # a failed call leaves it in place too
    finally:
        while eng_x4.stream_flush():
            pass
        eng_x4.set_pattern()
        buf.free()
    # after the reset: the bits of an engine that never had a pattern
    again = eng_x4.images_to_data(imgs, conf=True)
    fresh = Engine(weights["dir"])
    never = fresh.images_to_data(imgs, conf=True)
    fresh.close()
    assert all(_same_page(x, y) for x, y in zip(again, plain)) and all(_same_page(x, y) for x, y in zip(again, never))


def _items_equal(a, b):
    return (a["text"] == b["text"] and a["ids"] == b["ids"] and a["bbox"] == b["bbox"] and np.float32(a["conf"]).tobytes() == np.float32(b["conf"]).tobytes()
            and np.asarray(a["prob"], np.float32).tobytes() == np.asarray(b["prob"], np.float32).tobytes())


def test_regions_under_three_patterns_in_one_call(eng_x4, funsd):
    from tuatara_amd import synth
    from tuatara_amd.engine import DeviceBuffer, EngineError
    p0 = synth.synthetic_page(61, 768, 1024)
    p1 = np.ascontiguousarray(funsd[100:600, 30:730])
    pats = [r"\d{2}/\d{2}/\d{4}", r"[A-Z]{2}\d{2,6}", r"\d+\.\d{2}", None]
    rng = np.random.default_rng(4)
    regions, patterns = [], []
    for i in range(12):
        pg = (0, 1, 0, 1, 1, 0)[i % 6]
        h, w = (p0, p1)[pg].shape[:2]
        x0, y0 = int(rng.integers(0, w - 140)), int(rng.integers(0, h - 40))
        regions.append({"page": pg, "rect": (x0, y0, x0 + int(rng.integers(60, 140)), y0 + int(rng.integers(16, 40)))})
        patterns.append(pats[i % 4])
    bufs = [DeviceBuffer(a.nbytes) for a in (p0, p1)]
    try:
        for b, a in zip(bufs, (p0, p1)):
            b.upload(a)
        dev_pages = [(bufs[0], 768, 1024), (bufs[1], 500, 700)]
        got = eng_x4.read_regions(dev_pages, regions, patterns=patterns)
        flat = {it["region"]: it for page in got for it in page}
        assert sorted(flat) == list(range(12))
        for P in pats:                                                                 # each pattern alone through set_pattern, bit for bit
            eng_x4.set_pattern(P)
            alone = {it["region"]: it for page in eng_x4.read_regions(dev_pages, regions) for it in page}
            for i in range(12):
                if patterns[i] == P:
                    assert _items_equal(flat[i], alone[i]), (P, i)
                    assert P is None or re.fullmatch(P, flat[i]["text"]), (P, flat[i]["text"])
        eng_x4.set_pattern()
        # the host-image form, and None entries under the engine's own pattern
        local = [dict(r, page=0) for r in regions if r["page"] == 1]
        lp = [p for r, p in zip(regions, patterns) if r["page"] == 1]
        host = eng_x4.read_regions(p1, local, patterns=lp)
        assert all(_items_equal(a, b) for a, b in zip(host, got[1]))
        eng_x4.set_pattern(r"[a-z]+")
        own = eng_x4.read_regions(p1, local, patterns=lp)
        for a, b, P in zip(own, host, lp):
            assert (re.fullmatch(r"[a-z]+", a["text"]) is not None) if P is None else _items_equal(a, b)
        eng_x4.set_pattern()
        # refusals: a bad pattern names the region; the table's states are counted
        with pytest.raises(EngineError, match=r"regions: item 1: pattern: offset 0 holds '~'"):
            eng_x4.read_regions(p1, local[:2], patterns=[r"\d", "~"])
        big = [r"(a|b)*a(a|b){6}" + c for c in "cdefghijk"]                            # 129 states and a DONE state each
        with pytest.raises(EngineError, match=r"regions: the call's patterns need 1170 automaton states in all: at most 1024"):
            eng_x4.read_regions(p1, [local[0]] * 9, patterns=big)
        assert all(_items_equal(a, b) for a, b in zip(eng_x4.read_regions(p1, local, patterns=lp), host))   # the engine stayed usable
    finally:
        eng_x4.set_pattern()
        for b in bufs:
            b.free()


def test_lines_and_character_boxes_under_a_pattern(weights, pages, funsd):
    from tuatara_amd.engine import Engine
    eng = Engine(weights["dir"], lines=1, chars=1, pattern=r"[A-Z][a-z]*")
    base = Engine(weights["dir"], pattern=r"[A-Z][a-z]*")
    try:
        assert eng.pattern == base.pattern == r"[A-Z][a-z]*"
        for img in pages + [funsd]:
            r, b = eng.images_to_data([img], conf=True)[0], base.images_to_data([img], conf=True)[0]
            assert len(r) == len(b) > 0 and r.texts == b.texts and r.ids.tobytes() == b.ids.tobytes() and r.conf.tobytes() == b.conf.tobytes()
            assert (np.diff(r.char_first) == [len(t) for t in r.texts]).all()          # one box per character of the constrained text
            assert len(r.lines) > 0 and sorted(i for ln in r.lines for i in ln["items"]) == list(range(len(r)))
            assert all(re.fullmatch(r"[A-Z][a-z]*", w) for ln in r.lines for w in ln["text"].split())
    finally:
        eng.close()
        base.close()


# ------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_each_by_message(eng_x4, eng_bf16, weights):
    from tuatara_amd.engine import Engine, EngineError
    with pytest.raises(EngineError, match="ttr_engine_set_pattern: a pattern needs an f16x4 or f32 engine"):
        eng_bf16.set_pattern(r"\d+")
    assert eng_bf16.pattern is None
    eng_bf16.set_pattern()                                                             # a reset is always accepted
    with pytest.raises(EngineError, match="a pattern needs an f16x4 or f32 engine"):
        eng_bf16.logits_decode_patterns(np.zeros((1, 26, 95), np.float32), [r"\d+"], [0])
    turned = Engine(weights["dir"], orient=1)
    try:
        with pytest.raises(EngineError, match="ttr_engine_set_pattern: a pattern does not combine with word orientation"):
            turned.set_pattern(r"\d+")
        assert turned.pattern is None
    finally:
        turned.close()
    try:
        eng_x4.set_alternatives(3)
        with pytest.raises(EngineError, match="ttr_engine_set_pattern: a pattern does not combine with character alternatives"):
            eng_x4.set_pattern(r"\d+")
        eng_x4.set_alternatives(0)
        eng_x4.set_lexicon(["abc", "12"])
        with pytest.raises(EngineError, match="ttr_engine_set_pattern: a pattern does not combine with a lexicon"):
            eng_x4.set_pattern(r"\d+")
        eng_x4.set_lexicon(None)
        assert eng_x4.pattern is None
        eng_x4.set_pattern(r"\d+")                                                     # ... and in the other order
        with pytest.raises(EngineError, match="ttr_engine_set_alternatives: character alternatives do not combine with a pattern, and one is set"):
            eng_x4.set_alternatives(3)
        with pytest.raises(EngineError, match="ttr_engine_set_lexicon: lexicon matching does not combine with a pattern, and one is set"):
            eng_x4.set_lexicon(["abc"])
        assert eng_x4.pattern == r"\d+"
        # a set that empties the stored pattern's language fails and leaves both as they were
        with pytest.raises(EngineError, match=r"ttr_engine_set_charset: the engine's pattern does not survive this set: pattern: the language of \"\\d\+\" is empty"):
            eng_x4.set_charset(UPPER)
        assert np.array_equal(eng_x4.charset, CR.FULL) and eng_x4.pattern == r"\d+"
        eng_x4.set_charset("0123abc")                                                  # one that leaves it a language is taken, and the pattern recompiled under it
        crops = CR.sweep_crops(3, 6)
        _, ids = eng_x4.parseq_logits(crops)
        from tuatara_amd.engine import decode_ids
        assert all(re.fullmatch(r"[0123]+", decode_ids(r)) for r in np.asarray(ids).reshape(-1, 26))
        # more than 1024 states in one call
        big = [r"(a|b)*a(a|b){6}" + c for c in "cdefghijk"]
        eng_x4.set_charset()
        with pytest.raises(EngineError, match=r"ttr_logits_decode_patterns: the call's patterns need 1173 automaton states in all: at most 1024"):   # 9 x 130 and the engine's own 3
            eng_x4.logits_decode_patterns(np.zeros((10, 26, 95), np.float32), big, list(range(9)) + [-1])
        with pytest.raises(EngineError, match=r"item 2 names pattern 9, the call holds 9"):
            eng_x4.logits_decode_patterns(np.zeros((3, 26, 95), np.float32), big, [0, 0, 9])
    finally:
        eng_x4.set_alternatives(0)
        eng_x4.set_lexicon(None)
        eng_x4.set_pattern()
        eng_x4.set_charset()


# ------------------------------------------------------------------------------------------------- 6. callers
def test_pytuatara_keyword_region_key_environment_and_ocr_cli(weights, pages, funsd, eng_x4, monkeypatch, tmp_path):
    from tuatara_amd import build as B
    B.build_pytuatara()
    B.build_examples()
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    for k in ("TUATARA_PRECISION", "TUATARA_CROP_MODE", "TUATARA_ALLOWLIST", "TUATARA_BLOCKLIST", "TUATARA_PATTERN", "TUATARA_ORIENT", "TUATARA_LINES", "TUATARA_CHARS",
              "TUATARA_BLOCKS", "TUATARA_ALTS"):
        monkeypatch.delenv(k, raising=False)
    pattern, page = r"[A-Z][a-z]*", pages[0]
    regions = [{"rect": (40, 40, 200, 80), "pattern": r"\d{2}/\d{2}/\d{4}"}, {"rect": (60, 300, 260, 340)}, {"rect": (300, 500, 420, 530), "pattern": r"\d+", "allowlist": "0123"}]
    try:
        eng_x4.set_pattern(pattern)
        want = eng_x4.image_to_data(page, conf=True)
        want_bgr = eng_x4.image_to_data(np.ascontiguousarray(funsd[:, :, ::-1]))     # the CLI feeds BGR
        eng_x4.set_pattern()
        want_regions = eng_x4.read_regions(page, [{"rect": r["rect"], "set": 0 if "allowlist" in r else -1} for r in regions], charsets=[("0123", None)],
                                           patterns=[r.get("pattern") for r in regions])
    finally:
        eng_x4.set_pattern()
    plain = pytuatara.image_to_data(page, weights["dir"], "o")
    got = pytuatara.image_to_data(page, weights["dir"], "o", conf=True, pattern=pattern)
    assert [(r["text"], list(r["bbox"]), r["conf"]) for r in got] == [(g["text"], g["bbox"], g["conf"]) for g in want]
    assert all(re.fullmatch(pattern, r["text"]) for r in got) and len(got) > 0
    assert pytuatara.images_to_data([page], weights["dir"], "o", conf=True, pattern=pattern) == [got]
    assert pytuatara.image_to_data(page, weights["dir"], "o") == plain               # reset after the call
    with pytest.raises(ValueError, match=r"offset 0: '\(' without its '\)'"):
        pytuatara.image_to_data(page, weights["dir"], "o", pattern="(")
    assert pytuatara.image_to_data(page, weights["dir"], "o") == plain               # ... also when it raised
    got_regions = pytuatara.image_to_data(page, weights["dir"], "o", conf=True, regions=regions)
    assert [(r["text"], r["conf"]) for r in got_regions] == [(w["text"], w["conf"]) for w in want_regions]
    assert re.fullmatch(r"\d{2}/\d{2}/\d{4}", got_regions[0]["text"]) and re.fullmatch(r"[0123]+", got_regions[2]["text"])
    monkeypatch.setenv("TUATARA_PATTERN", pattern)
    assert [r["text"] for r in pytuatara.image_to_data(page, weights["dir"], "o")] == [g["text"] for g in want]
    monkeypatch.delenv("TUATARA_PATTERN")
    assert pytuatara.image_to_data(page, weights["dir"], "o") == plain
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    png = os.path.join(DATA, "funsd_0001129658.png")
    out = subprocess.run([os.path.join(B.ROOT, "build", "examples", "ocr_cli"), "--pattern", pattern, png, weights["dir"], str(tmp_path)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = [ln.split("\t") for ln in out.stdout.splitlines()]
    assert len(lines) == len(want_bgr) > 20
    for (bb, text), g in zip(lines, want_bgr):
        assert [float(v) for v in bb.split()] == g["bbox"] and text == g["text"] and re.fullmatch(pattern, text)


# ------------------------------------------------------------------------------------------------- 8. more rows than one recogniser group
def test_4097_crops_under_sets_and_patterns_equal_their_two_groups(eng_x4):
    """The recogniser takes more than 4096 rows in even groups (4097 = 2049 + 2048), and each group's row masks and start states must start where its crops
    do.  A crop's outputs do not depend on its batch and a group has the row count of the matching call of its own, so the one call equals the two calls on
    [:2049] and [2049:] bit for bit."""
    from tuatara_amd.engine import Pattern, charset_mask, decode_ids
    n, cut = 4097, 2049
    lower = "abcdefghijklmnopqrstuvwxyz"
    crops = np.random.default_rng(131).integers(0, 256, (n, 32, 128, 3), dtype=np.uint8)
    sets = np.stack([charset_mask(DIGITS + lower), charset_mask(DIGITS + lower + UPPER)])       # (both patterns have members under either set)
    patterns = [r"[0-9]+", r"[a-z]{2,8}"]
    set_of = np.array([i % 3 - 1 for i in range(n)], np.int32)                                   # two sets and the engine's own, period 3 ...
    pattern_of = np.array([i % 5 % 3 - 1 for i in range(n)], np.int32)                           # ... two patterns and none, period 5
    run = lambda s: eng_x4.parseq_logits(crops[s], set_of=set_of[s], sets=sets, pattern_of=pattern_of[s], patterns=patterns)
    lg, ids = run(slice(None))
    lg_a, ids_a = run(slice(0, cut))
    lg_b, ids_b = run(slice(cut, n))
    assert lg.tobytes() == np.concatenate([lg_a, lg_b]).tobytes()
    assert ids.tobytes() == np.concatenate([ids_a, ids_b]).tobytes()
    # the test bites: every row under a pattern matches it, and the two patterns read differently
    compiled = [Pattern(p) for p in patterns]
    texts = [decode_ids(r) for r in np.asarray(ids).reshape(n, 26)]
    for k in range(2):
        rows = np.nonzero(pattern_of == k)[0]
        assert len(rows) > 800 and all(compiled[k].matches(texts[i]) is True for i in rows), k
    assert {texts[i] for i in np.nonzero(pattern_of == 0)[0]} != {texts[i] for i in np.nonzero(pattern_of == 1)[0]}
    assert any(not compiled[0].matches(texts[i]) for i in np.nonzero(pattern_of == 1)[0])
