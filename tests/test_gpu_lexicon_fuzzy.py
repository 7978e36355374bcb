"""Fuzzy alignment of lexicon entries on the GPU (DESIGN.md "Lexicon matching", Fuzzy alignment): lexicon_fuzzy_score_kernel, its merge and the edits
kernel held to the host rule bit for bit on the tables the device itself forms (ttr_debug_lexicon_tables), band 0 against the rigid scorer, class masks and
-inf logits, and the mode through the engine: entries with a dropped or an extra character find their item again, every standard field keeps its bits, every
entry point agrees with the others, and the callers' layers on top."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lexicon_fuzzy_ref as FR
from tests import lexicon_ref as LR
from tests.conftest import DATA, GOLDEN, ROOT
from tests.test_gpu_lexicon import (CHUNK, DIGITS, LOWER, UPPER, _drain, _funsd_lexicon, _Lex, _mask, _qualifies, _same_standard_fields, adversarial_logits,
                                    unique_words)

pytestmark = pytest.mark.gpu

GAP = float(FR.GAP)
SIZES = (1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 428)      # one below, at and above a chunk; four chunks, the last one partial


@pytest.fixture(scope="module")
def eng(weights):
    """an f16x4 engine of this module's own: the tests set and clear its lexicon and its mode (and leave both cleared)"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine
    build_lib()
    return Engine(weights["dir"])


@pytest.fixture(scope="module")
def page():
    from tuatara_amd import synth
    return synth.synthetic_page(60, 1024, 768, n_words=20)


@pytest.fixture(scope="module")
def itos():
    with open(os.path.join(GOLDEN, "g1_ref_tokenizer.json")) as f:
        return [chr(c) for c in json.load(f)["itos"]]


@pytest.fixture(scope="module")
def vocabulary(itos):
    words = unique_words(SIZES[-1], 4, itos)
    return words, LR.encode(words, itos)


class _Fuzzy:
    """set_lexicon_fuzzy(band, gap) for a block, switched off again behind it"""

    def __init__(self, eng, band, gap=GAP):
        self.eng, self.band, self.gap = eng, band, gap

    def __enter__(self):
        self.eng.set_lexicon_fuzzy(self.band, self.gap)
        return self.eng

    def __exit__(self, *exc):
        self.eng.set_lexicon_fuzzy(None)


def host_ranking(lp, rec, band, gap, m):
    """the host rule on the device's tables lp [n, 26, 96] -> idx i32 [n, m], logp f32 [n, m], edits i32 [n, m] in the total order"""
    from tuatara_amd.engine import lexicon_fuzzy_from_lp
    n = len(lp)
    idx, logp, edits = np.full((n, m), -1, np.int32), np.full((n, m), -np.inf, np.float32), np.full((n, m), -1, np.int32)
    for i in range(n):
        s, e = lexicon_fuzzy_from_lp(lp[i], rec, band, gap)
        order = np.lexsort((np.arange(len(s)), -s.astype(np.float64)))
        order = order[np.isfinite(s[order])][:m]                 # -inf and NaN are left out
        idx[i, :len(order)], logp[i, :len(order)], edits[i, :len(order)] = order, s[order], e[order]
    return idx, logp, edits


def check_against_host_rule(eng, x, rec, band, gap, m, where, set_of=None, sets=None):
    lp = eng.debug_lexicon_tables(x, set_of=set_of, sets=sets)
    assert lp.shape == (len(x), 26, 96) and np.isneginf(lp[:, :, 95]).all()
    idx, logp, edits = eng.logits_lexicon_fuzzy(x, band, gap, set_of=set_of, sets=sets)
    want = host_ranking(lp, rec, band, gap, m)
    assert idx.shape == logp.shape == edits.shape == (len(x), m), where
    assert np.array_equal(idx, want[0]), (where, np.argwhere(idx != want[0])[:4])
    assert logp.tobytes() == want[1].tobytes(), where
    assert np.array_equal(edits, want[2]), (where, np.argwhere(edits != want[2])[:4])
    return idx, logp, edits


@pytest.mark.parametrize("n", [1, 5, 37])
def test_kernel_is_the_host_rule_bit_for_bit(eng, vocabulary, n):
    words, rec = vocabulary
    x = adversarial_logits(n, 100 + n)
    filled = 0
    for v in SIZES:
        for band, m in ((0, 3), (1, 3), (2, 3), (3, 3), (2, 1), (2, 8)):
            with _Lex(eng, words[:v], m):
                idx, _, edits = check_against_host_rule(eng, x, rec[:v], band, GAP, m, f"n={n} V={v} B={band} M={m}")
            filled += int((idx >= 0).sum())
            assert ((edits >= 0) == (idx >= 0)).all()
    assert filled > 0


def test_band_zero_is_the_rigid_scorer(eng, vocabulary):
    words, rec = vocabulary
    x = adversarial_logits(9, 17)
    with _Lex(eng, words[:CHUNK + 300], 8):
        idx0, logp0 = eng.logits_lexicon(x)
        idx, logp, edits = eng.logits_lexicon_fuzzy(x, 0, GAP)
    assert idx.tobytes() == idx0.tobytes() and logp.tobytes() == logp0.tobytes() and (idx >= 0).any()
    assert (edits[idx >= 0] == 0).all() and (edits[idx < 0] == -1).all()


def test_duplicates_few_words_masks_and_a_free_gap(eng, itos):
    from tuatara_amd.engine import charset_mask
    x = adversarial_logits(9, 77)
    # the same word twice, and fewer words than slots
    words = ["Total", "x", "Total"]
    with _Lex(eng, words, 8):
        idx, logp, _ = check_against_host_rule(eng, x, LR.encode(words, itos), 1, GAP, 8, "V=3 M=8")
    for i in range(9):
        got = idx[i].tolist()
        if 0 in got:                                             # identical bits, the lower index first
            a, b = got.index(0), got.index(2)
            assert b == a + 1 and logp[i, a].tobytes() == logp[i, b].tobytes(), i
        assert (idx[i, 3:] == -1).all()
    words = unique_words(60, 5, itos, DIGITS) + unique_words(60, 6, itos, UPPER) + unique_words(60, 8, itos, LOWER) + unique_words(120, 9, itos)
    rec = LR.encode(words, itos)
    digits = charset_mask(DIGITS)
    with _Lex(eng, words, 8):
        # blocked classes: a blocked character is never matched - it can only be dropped, at the gap's price (the host rule says which words that leaves);
        # at band 0 nothing can be dropped, and a word with a blocked class never appears
        idx, _, _ = check_against_host_rule(eng, x, rec, 2, GAP, 8, "digits", set_of=np.zeros(9, np.int32), sets=digits[None])
        assert (idx >= 0).any()
        idx, _, _ = check_against_host_rule(eng, x, rec, 0, GAP, 8, "digits, band 0", set_of=np.zeros(9, np.int32), sets=digits[None])
        assert all(set(words[k]) <= set(DIGITS) for k in idx[idx >= 0].tolist()) and (idx >= 0).any()
        # a mask that blocks a class of every word (the EOS stays): at band 0 nothing is returned; from band 1 on an alignment of drops and extras alone
        # reaches the EOS without one match, so every word keeps a score, all of it gaps - the host rule says which
        none = _mask([0, 94])
        every = [w for w in words if "}" not in w]
        eng.set_lexicon(every, 8)
        idx, logp, edits = check_against_host_rule(eng, x, LR.encode(every, itos), 0, GAP, 8, "every word blocked", set_of=np.zeros(9, np.int32), sets=none[None])
        assert (idx == -1).all() and np.isneginf(logp).all() and (edits == -1).all()
        idx, _, edits = check_against_host_rule(eng, x, LR.encode(every, itos), 3, GAP, 8, "every word blocked, band 3", set_of=np.zeros(9, np.int32), sets=none[None])
        assert (idx >= 0).all() and (edits >= 1).all()
        # four sets over nine rows in one launch; -1 = the engine's own set
        eng.set_lexicon(words, 3)
        sets = np.stack([digits, charset_mask(UPPER), charset_mask(None, LOWER), _mask([0, 3, 90])])
        set_of = np.array([0, 1, 2, 3, 3, 2, 1, 0, -1], np.int32)
        check_against_host_rule(eng, x, rec, 1, GAP, 3, "four sets over nine rows", set_of=set_of, sets=sets)
        idx, _, _ = check_against_host_rule(eng, x, rec, 0, GAP, 3, "four sets over nine rows, band 0", set_of=set_of, sets=sets)
        cls = LR.class_of(itos)
        for i, s in enumerate(set_of):
            if s >= 0:                                           # (band 0: no character can be dropped, so every character of a match is allowed)
                ok = LR.allowed(sets[s])
                assert all(ok[cls[ch]] for k in idx[i][idx[i] >= 0].tolist() for ch in words[k]), i
        # g = 0: dropping and adding characters is free
        for band in (1, 3):
            check_against_host_rule(eng, x, rec, band, 0.0, 3, f"g=0 B={band}")
        # -inf logits are never used
        rng = np.random.default_rng(31)
        y = x.copy()
        for i in range(9):
            for p in range(26):
                y[i, p, rng.choice(np.arange(1, 95), 30, replace=False)] = -np.inf
        _, logp, _ = check_against_host_rule(eng, y, rec, 2, GAP, 3, "-inf logits")
        assert np.isfinite(logp[np.isfinite(logp)]).all() and not np.isnan(logp).any()


# ------------------------------------------------------------------------------------------------- the engine
def _slipped(text, k):
    """the text with one character inserted (even k) or removed (odd k) at index 1"""
    if k % 2 == 0:
        ch = next(c for c in "xyzw" if c not in text)
        return text[:1] + ch + text[1:]
    return text[:1] + text[2:]


def _page_entries(r, itos):
    """up to eight items of 3..24 characters whose text can be an entry -> (item index, entry) pairs: the text with one slip"""
    cls = LR.class_of(itos)
    out, seen = [], set()
    for i in range(len(r)):
        if len(out) < 8 and 3 <= len(r.texts[i]) <= 24 and _qualifies(r.ids[i], r.texts[i], cls):
            w = _slipped(r.texts[i], len(out))
            if w not in seen:
                seen.add(w)
                out.append((i, w))
    return out


def _entry_logp(r, i, k):
    at = np.nonzero(r.lex_idx[i] == k)[0]
    return float(r.lex_logp[i, at[0]]) if len(at) else -np.inf


def test_entries_with_a_slip_find_their_item(eng, page, itos):
    off = eng.images_to_data([page])[0]
    entries = _page_entries(off, itos)
    assert len(entries) >= 4
    words = [w for _, w in entries]                              # V <= M: every entry's score comes back
    with _Lex(eng, words, 8):
        rigid = eng.images_to_data([page])[0]
        with _Fuzzy(eng, 1):
            assert eng.lexicon_fuzzy == (1, GAP)
            fuzzy = eng.images_to_data([page])[0]
    assert rigid.lex_edits is None and rigid.lex_band == -1 and fuzzy.lex_band == 1
    assert fuzzy.lex_edits.shape == (len(fuzzy), 8) and fuzzy.lex_edits.dtype == np.int32
    assert ((fuzzy.lex_edits >= 0) == (fuzzy.lex_idx >= 0)).all()
    _same_standard_fields(off, fuzzy)
    for k, (i, w) in enumerate(entries):
        # the item's own characters matched in order plus one gap is an alignment of the entry: logp(entry) >= log(conf) + g, up to the path's rounding
        L = len(off.texts[i])
        tol = (L + 1) * 2.5e-6 + 2.0 ** -19 * (np.abs(np.log(off.prob[i, :L + 1].astype(np.float64))).sum() + abs(GAP))
        got = _entry_logp(fuzzy, i, k)
        print(f"entry {w!r} of item {off.texts[i]!r}: fuzzy {got:.6f} rigid {_entry_logp(rigid, i, k):.6f} log(conf) + g {np.log(np.float64(off.conf[i])) + GAP:.6f}")
        assert got >= np.log(np.float64(off.conf[i])) + GAP - tol, (w, off.texts[i], got)
        assert _entry_logp(rigid, i, k) < got, (w, off.texts[i])                                     # the rigid rule scores the same entry lower
        d = fuzzy[i]
        assert len(d["lexicon_edits"]) == len(d["lexicon"]) and "lexicon_edits" not in rigid[i]


def test_bits_and_forms(eng, page, itos):
    from tuatara_amd.engine import DeviceBuffer, EngineError
    buf = DeviceBuffer(1024 * 768 * 3)
    buf.upload(page)
    off = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
    cls = LR.class_of(itos)
    own = sorted({t for t, ids in zip(off.texts, off.ids) if _qualifies(ids, t, cls)})
    words = [w for _, w in _page_entries(off, itos)] + own + unique_words(300, 41, itos)
    with _Lex(eng, words, 3):
        rigid = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
        with _Fuzzy(eng, 0):
            zero = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
        eng.set_lexicon_fuzzy(2, -3.0)
        eng.set_lexicon(words, 3)                                # the mode survives set_lexicon
        assert eng.lexicon_fuzzy == (2, -3.0)
        dev = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
        single = eng.image_to_data(page)                         # the synchronous call
        many = eng.images_to_data([page])[0]                     # the list form
        vform = eng.pages_to_data_dev_v([(buf.ptr, 1024, 768)])[0]
        streamed = eng.stream_push(buf.ptr, 1, 1024, 768)
        with pytest.raises(EngineError, match="streamed"):       # refused while batches stream, and nothing changes
            eng.set_lexicon_fuzzy(1)
        with pytest.raises(EngineError, match="streamed"):
            eng.logits_lexicon_fuzzy(np.zeros((1, 26, 95), np.float32), 1)
        with pytest.raises(EngineError, match="streamed"):
            eng.debug_lexicon_tables(np.zeros((1, 26, 95), np.float32))
        streamed = _drain(eng, streamed)[0]
        assert eng.lexicon_fuzzy == (2, -3.0)
        arr = (C.c_void_p * 1)()                                 # the raw result: the band and the views
        assert eng.lib.ttr_pages_to_data_dev(eng.h, buf.ptr, 1, 1024, 768, arr) == 0
        assert eng.lib.ttr_result_lex_band(arr[0]) == 2 and eng.lib.ttr_result_lex_edits_all(arr[0])
        assert np.array_equal(np.ctypeslib.as_array(eng.lib.ttr_result_lex_edits(arr[0], 1), (3,)), dev.lex_edits[1])
        assert not eng.lib.ttr_result_lex_edits(arr[0], len(dev))
        eng.lib.ttr_result_free(arr[0])
        for bad in ((4, -1.0), (-2, -1.0), (1, 1e-3), (1, float("nan")), (1, float("-inf")), (1, float("inf"))):   # every refusal: nothing changes
            with pytest.raises(EngineError):
                eng.set_lexicon_fuzzy(*bad)
            assert eng.lexicon_fuzzy == (2, -3.0)
        for bad in ((-1, -1.0), (4, -1.0), (1, 0.5), (1, float("nan"))):
            with pytest.raises(EngineError):
                eng.logits_lexicon_fuzzy(np.zeros((1, 26, 95), np.float32), *bad)
        eng.set_lexicon_fuzzy(-1, float("nan"))                  # off: the gap is ignored
        assert eng.lexicon_fuzzy is None
        arr = (C.c_void_p * 1)()                                 # switched off: the views are NULL
        assert eng.lib.ttr_pages_to_data_dev(eng.h, buf.ptr, 1, 1024, 768, arr) == 0
        assert eng.lib.ttr_result_lex_band(arr[0]) == -1 and not eng.lib.ttr_result_lex_edits_all(arr[0]) and not eng.lib.ttr_result_lex_edits(arr[0], 0)
        assert eng.lib.ttr_result_lex_idx_all(arr[0])
        eng.lib.ttr_result_free(arr[0])
        again = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
    with pytest.raises(EngineError, match="no lexicon"):
        eng.logits_lexicon_fuzzy(np.zeros((1, 26, 95), np.float32), 1)
    eng.set_lexicon_fuzzy(1)                                     # it may be set with no lexicon in place: nothing is scored
    bare = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
    eng.set_lexicon_fuzzy(None)
    assert bare.lex_idx is None and bare.lex_edits is None
    for r in (rigid, zero, dev, many, vform, streamed, again, bare):
        _same_standard_fields(off, r)                            # every standard field: bit for bit that of the engine without the mode
    assert zero.lex_idx.tobytes() == rigid.lex_idx.tobytes() and zero.lex_logp.tobytes() == rigid.lex_logp.tobytes()    # band 0 is band -1
    assert again.lex_idx.tobytes() == rigid.lex_idx.tobytes() and again.lex_logp.tobytes() == rigid.lex_logp.tobytes() and again.lex_edits is None
    assert (zero.lex_edits[zero.lex_idx >= 0] == 0).all()
    assert (dev.lex_edits > 0).any() and (dev.lex_logp >= rigid.lex_logp).all()
    assert list(dev) == list(single)
    for other in (many, vform, streamed):
        assert other.lex_band == 2
        for f in ("lex_idx", "lex_logp", "lex_edits"):
            assert getattr(dev, f).tobytes() == getattr(other, f).tobytes(), f
    assert [{k: v for k, v in d.items() if k not in ("lexicon", "lexicon_edits")} for d in dev] == list(off)
    buf.free()


def test_regions_under_two_sets(eng, page, itos):
    found = eng.image_to_data(page)
    rects = [[int(v) for v in (np.floor(w["bbox"][0]), np.floor(w["bbox"][1]), np.ceil(w["bbox"][2]) + 1, np.ceil(w["bbox"][3]) + 1)] for w in found[:4]]
    charsets = [(DIGITS, None), (UPPER, None)]
    regions = [{"rect": rc, "set": s % 2} for s, rc in enumerate(rects)]
    words = unique_words(60, 71, itos, DIGITS) + unique_words(60, 72, itos, UPPER) + unique_words(60, 74, itos)
    plain = eng.read_regions(page, regions, charsets)
    with _Lex(eng, words, 4):
        rigid = eng.read_regions(page, regions, charsets)
        with _Fuzzy(eng, 0):
            zero = eng.read_regions(page, regions, charsets)
        with _Fuzzy(eng, 2):
            got = eng.read_regions(page, regions, charsets)
    assert len(got) == 4
    for s, (g, z, r, p) in enumerate(zip(got, zero, rigid, plain)):
        assert {k: v for k, v in g.items() if k not in ("lex_idx", "lex_logp", "lex_edits", "lexicon", "lexicon_edits")} == p      # nothing else changes
        assert "lex_edits" not in r and z["lex_idx"].tobytes() == r["lex_idx"].tobytes() and z["lex_logp"].tobytes() == r["lex_logp"].tobytes()
        assert g["lex_idx"].shape == g["lex_edits"].shape == (4,) and (g["lex_idx"] >= 0).all() and (g["lex_edits"] >= 0).all()
        assert all(set(words[int(k)]) <= set(charsets[s % 2][0]) for k in z["lex_idx"]), s                                          # each region under its own set (band 0: nothing is dropped)
        assert g["lexicon_edits"] == g["lex_edits"].tolist() and len(g["lexicon"]) == 4
        assert (g["lex_logp"] >= r["lex_logp"]).all()


# ------------------------------------------------------------------------------------------------- callers (a child process each)
PYT = r'''
import json, os, sys
import numpy as np
from PIL import Image
sys.path.insert(0, os.path.join({root!r}, "build", "bindings"))
import pytuatara
img = np.array(Image.open({png!r}).convert("RGB"))
words = json.load(open({words!r}))
rigid = pytuatara.image_to_data(img, {wdir!r}, "o", conf=True, lexicon=words, lexicon_m=3)
got = pytuatara.image_to_data(img, {wdir!r}, "o", conf=True, lexicon=words, lexicon_m=3, lexicon_fuzzy=1)
many = pytuatara.images_to_data([img], {wdir!r}, "o", conf=True, lexicon=words, lexicon_m=3, lexicon_fuzzy=1, lexicon_gap=-6.9077554)
again = pytuatara.image_to_data(img, {wdir!r}, "o", conf=True, lexicon=words, lexicon_m=3)
errors = []
for kw in (dict(lexicon=words, lexicon_fuzzy=4), dict(lexicon=words, lexicon_fuzzy=1, lexicon_gap=0.5), dict(lexicon_fuzzy=1)):
    try:
        pytuatara.image_to_data(img, {wdir!r}, "o", **kw)
        errors.append(None)
    except Exception as ex:
        errors.append([type(ex).__name__, str(ex)])
print("RESULT " + json.dumps(dict(rigid=rigid, got=got, same=(many == [got]), again=(again == rigid), errors=errors)))
'''


def test_pytuatara_lexicon_fuzzy_keyword(eng, weights, funsd, itos, tmp_path):
    from tuatara_amd import build
    build.build_pytuatara()
    png = os.path.join(DATA, "funsd_0001129658.png")
    words = _funsd_lexicon(eng, funsd, itos)
    wfile = str(tmp_path / "words.json")
    with open(wfile, "w") as f:
        json.dump(words, f)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    out = subprocess.run([sys.executable, "-c", PYT.format(root=ROOT, png=png, wdir=weights["dir"], words=wfile)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][0][7:])
    with _Lex(eng, words, 3), _Fuzzy(eng, 1):
        want = eng.image_to_data(funsd, conf=True)
    assert len(want) > 20 and len(res["got"]) == len(want)
    for g, w in zip(res["got"], want):
        assert set(g) == {"text", "bbox", "conf", "char_conf", "lexicon", "lexicon_edits"}
        assert (g["text"], g["bbox"], g["conf"], g["char_conf"]) == (w["text"], w["bbox"], w["conf"], w["char_conf"])
        assert [a[0] for a in g["lexicon"]] == [a[0] for a in w["lexicon"]] and g["lexicon_edits"] == w["lexicon_edits"]
        assert all(abs(a[1] - b[1]) <= 2 * 2.0 ** -52 * b[1] for a, b in zip(g["lexicon"], w["lexicon"]))
    assert [{k: v for k, v in g.items() if k != "lexicon_edits"} for g in res["got"]] != [] and all("lexicon_edits" not in d for d in res["rigid"])
    assert [{k: v for k, v in g.items() if k not in ("lexicon", "lexicon_edits")} for g in res["got"]] == \
           [{k: v for k, v in g.items() if k != "lexicon"} for g in res["rigid"]]                          # the mode changes nothing else
    assert res["same"] and res["again"]                          # the list form agrees; the cached engine is left with the mode off
    assert [e[0] for e in res["errors"]] == ["ValueError"] * 3


def test_ocr_cli_lexicon_fuzzy(eng, weights, funsd, itos, tmp_path):
    from tuatara_amd import build as B
    B.build_examples()
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    png = os.path.join(DATA, "funsd_0001129658.png")
    cli = os.path.join(B.ROOT, "build", "examples", "ocr_cli")
    bgr = np.ascontiguousarray(funsd[:, :, ::-1])                # the CLI feeds BGR
    words = _funsd_lexicon(eng, bgr, itos)
    wfile = tmp_path / "words.txt"
    wfile.write_text("\n".join(words) + "\n")
    out = subprocess.run([cli, "--lexicon", str(wfile), "--lexicon-m", "2", "--lexicon-fuzzy", "1", png, weights["dir"], str(tmp_path)], capture_output=True,
                         text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    with _Lex(eng, words, 2), _Fuzzy(eng, 1):
        want = eng.images_to_data([bgr], conf=True)[0]
    lines = out.stdout.splitlines()
    at = 0
    assert len(want) > 20
    for i, g in enumerate(want):
        bb, conf, text = lines[at].split("\t")
        at += 1
        assert [float(v) for v in bb.split()] == g["bbox"] and text == g["text"] and conf == f"{g['conf']:.6f}"
        for k, (w, p), e in zip(want.lex_idx[i], g["lexicon"], g["lexicon_edits"]):
            assert lines[at] == f"\t={int(k)} {p:.6f} {w} {e}"
            at += 1
    assert at == len(lines)
    for args in (["--lexicon-fuzzy", "1"], ["--lexicon", str(wfile), "--lexicon-fuzzy", "4"], ["--lexicon", str(wfile), "--lexicon-gap", "-2"],
                 ["--lexicon", str(wfile), "--lexicon-fuzzy", "1", "--lexicon-gap", "0.5"]):
        bad = subprocess.run([cli] + args + [png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=60)
        assert bad.returncode == 1 and "--lexicon" in bad.stderr, args
