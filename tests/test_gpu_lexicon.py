"""GPU suite for lexicon matching (DESIGN.md "Lexicon matching"): the scorer and its merge against the float64 restatement (tests/lexicon_ref.py) on
adversarial logits, through ttr_logits_lexicon - every lexicon size at which the kernel takes another path, under one mask and under a table of row
masks; the exact rules; the engine's entry points against each other and against the same engine without a lexicon, bit for bit; regions under their own
sets; the refusals; and the callers (pytuatara lexicon=, ocr_cli --lexicon).

The words are unique and random over the classes a lexicon byte can name: the 93 character classes less the two the backslash names (ids 69 and 87), 91."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lexicon_ref as LR
from tests.conftest import DATA, GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DIGITS = "0123456789"
UPPER = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
LOWER = "abcdefghijklmnopqrstuvwxyz"
CHUNK = 1024                                              # kernels.h: kLexChunk, the scorer's words per workgroup
SIZES = (1, 3, 257, 4099, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 428)      # ... one below, at, one above; and four chunks, the last one partial


@pytest.fixture(scope="module")
def eng(weights):
    """an f16x4 engine of this module's own: the tests set and clear its lexicon (and leave it cleared)"""
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


class _Lex:
    """set_lexicon(words, m) for a block, cleared again behind it"""

    def __init__(self, eng, words, m=1):
        self.eng, self.words, self.m = eng, words, m

    def __enter__(self):
        self.eng.set_lexicon(self.words, self.m)
        return self.eng

    def __exit__(self, *exc):
        self.eng.set_lexicon(None)


KINDS = 5                                                 # a crop's kind: 0 normal, 1 peaked, 2 spreads of 1e30, 3 all equal, 4 mixed rows


def crop_kinds(n):
    return (np.arange(n) + n) % KINDS                     # (n = 1: a peaked crop; n = 5 and 37: every kind)


def adversarial_logits(n, seed):
    """tests/test_gpu_alts.py's kinds of rows.  A crop is of one kind - normal rows; peaked rows (near one-hot); spreads of 1e30; all-equal rows - or mixes
    them row by row, with exact ties at the maximum and an EOS or a dropped id on top as well.  All-equal rows tie every word of a length exactly, and one
    1e30 row among normal ones swallows the other rows' terms even in float64, so the last two kinds produce ties by construction."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 3.0, (n, 26, 95)).astype(np.float32)
    kind = rng.integers(0, 8, (n, 26)) + 10                   # the mixed crops: a kind per row
    for i, k in enumerate(crop_kinds(n)):
        if k < 4:
            kind[i] = (0, 3, 4, 2)[k] + 10
    kind -= 10
    for i, p in zip(*np.nonzero(kind == 1)):                  # exact ties at the maximum
        t = rng.choice(95, rng.integers(2, 5), replace=False)
        x[i, p, t] = x[i, p].max() + 1.0
    for i, p in zip(*np.nonzero(kind == 2)):                  # all equal
        x[i, p] = np.float32(rng.normal())
    for i, p in zip(*np.nonzero(kind == 3)):                  # near one-hot
        x[i, p, rng.integers(0, 95)] += 40.0
    for i, p in zip(*np.nonzero(kind == 4)):                  # spreads up to +-1e30
        x[i, p] = rng.uniform(-1e30, 1e30, 95).astype(np.float32)
    for i, p in zip(*np.nonzero(kind == 5)):                  # an EOS (id 0) or a dropped id (88) at this position
        x[i, p, 0 if rng.random() < 0.5 else 88] += 12.0
    return x


def unique_words(v, seed, itos, chars=None):
    """v unique random words over the 91 classes, lengths 1..25; word 0 has one character, word 1 twenty-five"""
    rng = np.random.default_rng(seed)
    chars = sorted(LR.class_of(itos)) if chars is None else list(chars)
    out, seen = [], set()
    while len(out) < v:
        L = 1 if len(out) == 0 else 25 if len(out) == 1 else int(rng.integers(1, 26))
        w = "".join(rng.choice(chars, L))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def check_against_restatement(idx, logp, s64, tol, m, where, count=None):
    """idx i32 / logp f32 [n, m] of a lexicon whose float64 scores and bounds are s64 / tol [n, V]: every returned logp within tol of float64; the float64
    score of slot j at least the j-th best minus the two bounds involved; the index equal to the restatement's wherever the float64 gap to both rank
    neighbours exceeds twice the larger bound; the slots past the words that can be scored -1 / -inf.  Returns (slots, slots whose index was compared),
    both counted over the crops of `count` (bool [n]; None = all) - every check above is made on every crop."""
    n, V = s64.shape
    assert idx.shape == logp.shape == (n, m) and idx.dtype == np.int32 and logp.dtype == np.float32, where
    slots = compared = 0
    worst = 0.0
    for i in range(n):
        order = LR.rank(s64[i], V)                                                   # every word that can be scored, best first
        q = min(m, len(order))
        assert (idx[i, q:] == -1).all() and np.isneginf(logp[i, q:]).all(), (where, i)
        assert (idx[i, :q] >= 0).all() and (idx[i, :q] < V).all() and len(set(idx[i, :q].tolist())) == q, (where, i)
        for j in range(q):
            w, r = int(idx[i, j]), int(order[j])
            counted = count is None or bool(count[i])
            slots += counted
            assert np.isfinite(s64[i, w]), (where, i, j)                             # a word of score -inf is never returned
            err = abs(float(logp[i, j]) - s64[i, w])
            worst = max(worst, err / tol[i, w])
            assert err <= tol[i, w], (where, i, j, err, tol[i, w])
            assert s64[i, w] >= s64[i, r] - tol[i, w] - tol[i, order[:j + 1]].max(), (where, i, j)
            nb = [int(order[k]) for k in (j - 1, j + 1) if 0 <= k < len(order)]
            if all(abs(s64[i, r] - s64[i, u]) > 2 * max(tol[i, r], tol[i, u]) for u in nb):
                compared += counted
                assert w == r, (where, i, j, w, r)
    print(f"{where}: {slots} slots, {compared} compared by index, max |logp - float64| / tol = {worst:.3f}")
    return slots, compared


_REF = {}


def _ref(n, itos):
    """the adversarial logits of n crops, the largest word list, its records and the restatement's scores and bounds for all of it (a smaller lexicon is
    its prefix), computed once"""
    if n not in _REF:
        x = adversarial_logits(n, 7 + n)
        words = unique_words(max(SIZES), 7, itos)
        rec = LR.encode(words, itos)
        lp, mag = LR.tables(x)
        _REF[n] = (x, words, rec) + LR.scores(rec, lp, mag)
    return _REF[n]


@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 5, 37])
def test_kernel_against_the_restatement(eng, itos, n, m):
    x, words, rec, s64, tol = _ref(n, itos)
    # the kinds that do not tie by construction (adversarial_logits), counted apart: a 1e30 crop's bound is of the order of 1e25, so the count that
    # says something about ordinary scores is the one over the normal and peaked crops
    groups = [crop_kinds(n) < 2, crop_kinds(n) == 2]
    totals = [[0, 0] for _ in groups]
    for v in SIZES:
        with _Lex(eng, words[:v], m):
            assert eng.lexicon_size == v and eng.lexicon_m == m
            idx, logp = eng.logits_lexicon(x)
        for g, count in enumerate(groups):
            a, b = check_against_restatement(idx, logp, s64[:, :v], tol[:, :v], m, f"n={n} m={m} V={v} {('normal + peaked', '1e30')[g]}", count)
            totals[g][0] += a
            totals[g][1] += b
    assert totals[0][0] > 0                                                              # (n = 1 is a peaked crop)
    for slots, compared in totals:
        assert compared >= 0.95 * slots, totals                                          # the index check may leave out at most 5 % of each group's slots


def test_the_same_word_twice_and_fewer_words_than_slots(eng, itos):
    x = adversarial_logits(5, 21)
    words = ["Total", "x", "Total"]
    with _Lex(eng, words, 8):                                                            # V < M
        idx, logp = eng.logits_lexicon(x)
    lp, mag = LR.tables(x)
    s64, tol = LR.scores(LR.encode(words, itos), lp, mag)
    check_against_restatement(idx, logp, s64, tol, 8, "V=3 m=8")
    for i in range(5):
        got = idx[i].tolist()
        if 0 in got:                                                                     # identical bits, the lower index first
            a, b = got.index(0), got.index(2)
            assert b == a + 1 and logp[i, a].tobytes() == logp[i, b].tobytes(), i
        assert (idx[i, 3:] == -1).all() and np.isneginf(logp[i, 3:]).all()
    assert (idx[:, 0] >= 0).any()


def _mask(classes):
    m = np.zeros(3, np.uint32)
    for c in classes:
        m[c >> 5] |= np.uint32(1 << (c & 31))
    return m


def test_blocked_classes_and_rows_of_different_sets(eng, itos):
    from tuatara_amd.engine import charset_mask
    x = adversarial_logits(9, 77)
    words = unique_words(60, 5, itos, DIGITS) + unique_words(60, 6, itos, UPPER) + unique_words(60, 8, itos, LOWER) + unique_words(120, 9, itos)
    rec = LR.encode(words, itos)
    # one mask for every row: a word with a blocked class never appears
    digits = charset_mask(DIGITS)
    with _Lex(eng, words, 8):
        idx, logp = eng.logits_lexicon(x, set_of=np.zeros(9, np.int32), sets=digits[None])
        s64, tol = LR.scores(rec, *LR.tables(x, digits))
        check_against_restatement(idx, logp, s64, tol, 8, "digits")
        assert all(set(words[k]) <= set(DIGITS) for k in idx[idx >= 0].tolist()) and (idx >= 0).any()
        # a mask that blocks a class of every word: nothing is returned
        none = _mask([0, 94])
        every = [w for w in words if "}" not in w]                                       # (class 94 is '}': the words without it all use a blocked class)
        eng.set_lexicon(every, 8)
        idx, logp = eng.logits_lexicon(x, set_of=np.zeros(9, np.int32), sets=none[None])
        assert (idx == -1).all() and np.isneginf(logp).all()
        # four sets over nine rows in one launch; -1 = the engine's own set (none here: every class)
        eng.set_lexicon(words, 3)
        sets = np.stack([digits, charset_mask(UPPER), charset_mask(None, LOWER), _mask([0, 3, 90])])
        set_of = np.array([0, 1, 2, 3, 3, 2, 1, 0, -1], np.int32)
        row_masks = np.stack([sets[s] if s >= 0 else _mask(range(95)) for s in set_of])
        idx, logp = eng.logits_lexicon(x, set_of=set_of, sets=sets)
        s64, tol = LR.scores(rec, *LR.tables(x, row_masks))
        check_against_restatement(idx, logp, s64, tol, 3, "four sets over nine rows")
        cls = LR.class_of(itos)
        for i in range(9):
            ok = LR.allowed(row_masks[i])
            assert all(ok[cls[ch]] for k in idx[i][idx[i] >= 0].tolist() for ch in words[k]), i
        # sets == None: the engine's own set
        eng.set_charset(DIGITS)
        try:
            idx2, logp2 = eng.logits_lexicon(x)
        finally:
            eng.set_charset()
        want, want_lp = eng.logits_lexicon(x, set_of=np.zeros(9, np.int32), sets=digits[None])
        assert idx2.tobytes() == want.tobytes() and logp2.tobytes() == want_lp.tobytes()


def test_minus_infinity_logits_are_never_used(eng, itos):
    rng = np.random.default_rng(31)
    x = adversarial_logits(5, 33)
    dead = np.zeros((5, 26, 95), bool)
    for i in range(5):
        for p in range(26):
            dead[i, p, rng.choice(np.arange(1, 95), 30, replace=False)] = True
    x[dead] = -np.inf
    words = unique_words(600, 12, itos)
    rec = LR.encode(words, itos)
    with _Lex(eng, words, 8):
        idx, logp = eng.logits_lexicon(x)
    s64, tol = LR.scores(rec, *LR.tables(x))
    check_against_restatement(idx, logp, s64, tol, 8, "-inf logits")
    cls = LR.class_of(itos)
    for i in range(5):
        for k in idx[i][idx[i] >= 0].tolist():
            assert not any(dead[i, p, cls[ch]] for p, ch in enumerate(words[k])), (i, k)
    assert np.isfinite(logp[idx >= 0]).all()


# ------------------------------------------------------------------------------------------------- the engine
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


def _qualifies(ids, text, cls):
    """an item whose text can be an entry: 1..25 characters a lexicon byte can name, and no id 88 before its EOS"""
    e = np.nonzero(ids == 0)[0]
    return len(e) > 0 and 1 <= len(text) <= 25 and not (ids[:e[0]] == 88).any() and all(ch in cls for ch in text)


def _page_lexicon(results, itos, decoys=400):
    cls = LR.class_of(itos)
    own = sorted({t for r in results for t, ids in zip(r.texts, r.ids) if _qualifies(ids, t, cls)})
    extra = [w for w in unique_words(decoys, 41, itos) if w not in set(own)]
    words = extra[:decoys // 2] + own + extra[decoys // 2:]                              # the pages' own texts in the middle of the list
    return words, cls


def _check_items(r, words, cls, m):
    """every qualifying item's slot 0 spells its text, with logp within the bound of log(conf)"""
    n_ok = 0
    assert r.lex_idx.shape == r.lex_logp.shape == (len(r), m) and r.lex_idx.dtype == np.int32 and r.lex_logp.dtype == np.float32
    for i in range(len(r)):
        filled = r.lex_idx[i] >= 0
        assert (r.lex_idx[i] < len(words)).all() and np.isfinite(r.lex_logp[i][filled]).all() and np.isneginf(r.lex_logp[i][~filled]).all()
        assert (np.diff(r.lex_logp[i][filled]) <= 0).all()                               # descending
        assert r[i]["lexicon"] == [(words[int(k)], float(np.exp(np.float64(l)))) for k, l in zip(r.lex_idx[i][filled], r.lex_logp[i][filled])]
        if not _qualifies(r.ids[i], r.texts[i], cls):
            continue
        n_ok += 1
        L = len(r.texts[i])
        assert words[int(r.lex_idx[i, 0])] == r.texts[i], (i, r.texts[i], r[i]["lexicon"])
        tol = (L + 1) * 2.5e-6 + 2.0 ** -19 * np.abs(np.log(r.prob[i, :L + 1].astype(np.float64))).sum()
        assert abs(float(r.lex_logp[i, 0]) - np.log(np.float64(r.conf[i]))) <= tol, (i, r.texts[i])
    return n_ok


def test_engine_entry_points_agree_and_nothing_else_changes(eng, pages, itos):
    from tuatara_amd.engine import DeviceBuffer
    buf = DeviceBuffer(2 * 1024 * 768 * 3)
    buf.upload(np.stack(pages))
    off = eng.pages_to_data_dev(buf, 2, 1024, 768)
    assert all(r.lex_idx is None and r.lex_logp is None and len(r) > 0 for r in off)
    assert all("lexicon" not in d for r in off for d in r)
    words, cls = _page_lexicon(off, itos)
    with _Lex(eng, words, 3):
        assert eng.lexicon_size == len(words) and eng.lexicon_m == 3 and eng.lexicon_word(5) == words[5] and eng.lexicon_word(len(words)) is None
        dev = eng.pages_to_data_dev(buf, 2, 1024, 768)
        single = [eng.image_to_data(p) for p in pages]                                   # the synchronous call
        many = eng.images_to_data(pages)                                                 # the list form ...
        vform = eng.pages_to_data_dev_v([(buf.ptr + k * 1024 * 768 * 3, 1024, 768) for k in range(2)])
        streamed = []
        for k in range(2):                                                               # push, push, flush: one page per batch, both slots
            streamed += eng.stream_push(buf.ptr + k * 1024 * 768 * 3, 1, 1024, 768)
        streamed = _drain(eng, streamed)
        arr = (C.c_void_p * 2)()                                                         # the raw result: M and the views
        assert eng.lib.ttr_pages_to_data_dev(eng.h, buf.ptr, 2, 1024, 768, arr) == 0
        for i in range(2):
            assert eng.lib.ttr_result_lex_m(arr[i]) == 3 and eng.lib.ttr_result_lex_idx_all(arr[i]) and eng.lib.ttr_result_lex_logp_all(arr[i])
            assert np.array_equal(np.ctypeslib.as_array(eng.lib.ttr_result_lex_idx(arr[i], 1), (3,)), dev[i].lex_idx[1])
            assert np.ctypeslib.as_array(eng.lib.ttr_result_lex_logp(arr[i], 1), (3,)).tobytes() == dev[i].lex_logp[1].tobytes()
            eng.lib.ttr_result_free(arr[i])
    assert eng.lexicon_size == 0 and eng.lexicon_m == 0
    for a, b in zip(off, dev):
        _same_standard_fields(a, b)                                                      # every field that existed before: bit for bit those of no lexicon
        assert [{k: v for k, v in d.items() if k != "lexicon"} for d in b] == list(a)
    assert sum(_check_items(r, words, cls, 3) for r in dev) >= 20
    assert [list(r) for r in dev] == single
    for other in (many, vform, streamed):
        assert len(other) == 2
        for a, b in zip(dev, other):
            _same_standard_fields(a, b)
            assert a.lex_idx.tobytes() == b.lex_idx.tobytes() and a.lex_logp.tobytes() == b.lex_logp.tobytes()
    # cleared again: no matches anywhere, the views are NULL, M is 0
    arr = (C.c_void_p * 2)()
    assert eng.lib.ttr_pages_to_data_dev(eng.h, buf.ptr, 2, 1024, 768, arr) == 0
    for i in range(2):
        assert eng.lib.ttr_result_lex_m(arr[i]) == 0 and not eng.lib.ttr_result_lex_idx_all(arr[i]) and not eng.lib.ttr_result_lex_logp_all(arr[i])
        assert not eng.lib.ttr_result_lex_idx(arr[i], 0) and not eng.lib.ttr_result_lex_logp(arr[i], 0)
        eng.lib.ttr_result_free(arr[i])
    again = eng.pages_to_data_dev(buf, 2, 1024, 768)
    for a, b in zip(off, again):
        _same_standard_fields(a, b)
        assert b.lex_idx is None
    buf.free()


def test_the_list_form_in_mixed_batches(weights, pages, itos):
    from tuatara_amd.engine import Engine
    mixed = Engine(weights["dir"], mixed_batches=1)
    try:
        off = mixed.images_to_data(pages)
        words, cls = _page_lexicon(off, itos)
        mixed.set_lexicon(words, 2)
        got = mixed.images_to_data([pages[0], pages[1][:700, :1000].copy(), pages[1]])  # two sizes that share one canvas
        mixed.set_lexicon(None)
        for a, b in zip(off, (got[0], got[2])):
            _same_standard_fields(a, b)
        assert _check_items(got[0], words, cls, 2) + _check_items(got[2], words, cls, 2) >= 20
        assert got[1].lex_idx.shape == (len(got[1]), 2)
    finally:
        mixed.close()


def test_a_character_set_bounds_the_matches(eng, pages, itos):
    words = unique_words(300, 51, itos) + unique_words(80, 52, itos, DIGITS)
    eng.set_charset(DIGITS)
    try:
        plain = eng.images_to_data([pages[0]])[0]
        with _Lex(eng, words, 8):
            r = eng.images_to_data([pages[0]])[0]
    finally:
        eng.set_charset()
    _same_standard_fields(plain, r)
    got = r.lex_idx[r.lex_idx >= 0].tolist()
    assert len(r) > 0 and len(got) > 0 and all(set(words[k]) <= set(DIGITS) for k in got)


def test_alternatives_are_unchanged(eng, pages, itos):
    eng.set_alternatives(3)
    try:
        plain = eng.images_to_data([pages[0]])[0]
        with _Lex(eng, unique_words(100, 61, itos), 2):
            r = eng.images_to_data([pages[0]])[0]
    finally:
        eng.set_alternatives(0)
    _same_standard_fields(plain, r)
    assert r.alt_ids.tobytes() == plain.alt_ids.tobytes() and r.alt_prob.tobytes() == plain.alt_prob.tobytes()
    assert r.lex_idx.shape == (len(r), 2) and (r.lex_idx[:, 0] >= 0).any()


def test_an_f32_engine_at_m_one(eng_f32, pages, itos):
    plain = eng_f32.images_to_data([pages[0]])[0]
    words, cls = _page_lexicon([plain], itos)
    with _Lex(eng_f32, words, 1):
        r = eng_f32.images_to_data([pages[0]])[0]
    _same_standard_fields(plain, r)
    assert _check_items(r, words, cls, 1) >= 10


def test_regions_keep_to_their_own_sets(eng, pages, itos):
    page = pages[1]
    found = eng.image_to_data(page)
    rects = [[int(v) for v in (np.floor(w["bbox"][0]), np.floor(w["bbox"][1]), np.ceil(w["bbox"][2]) + 1, np.ceil(w["bbox"][3]) + 1)] for w in found[:3]]
    charsets = [(DIGITS, None), (UPPER, None), (LOWER, None)]
    regions = [{"rect": rc, "set": s} for s, rc in enumerate(rects)]
    words = unique_words(60, 71, itos, DIGITS) + unique_words(60, 72, itos, UPPER) + unique_words(60, 73, itos, LOWER) + unique_words(60, 74, itos)
    plain = eng.read_regions(page, regions, charsets)
    with _Lex(eng, words, 4):
        got = eng.read_regions(page, regions, charsets)
    assert len(got) == 3
    for s, (g, p) in enumerate(zip(got, plain)):
        assert {k: v for k, v in g.items() if k not in ("lex_idx", "lex_logp", "lexicon")} == p              # nothing else changes
        assert g["lex_idx"].shape == (4,) and (g["lex_idx"] >= 0).all()
        assert all(set(words[int(k)]) <= set(charsets[s][0]) for k in g["lex_idx"]), s                         # each region under its own set
        assert [w for w, _ in g["lexicon"]] == [words[int(k)] for k in g["lex_idx"]]


def test_refusals(eng, eng_bf16, weights, pages):
    from tuatara_amd.engine import Comm, DeviceBuffer, Engine, EngineError
    from tuatara_amd.launch import free_port
    for m in (0, 9, -1):
        with pytest.raises(EngineError, match="1..8"):
            eng.set_lexicon(["a"], m)
    with pytest.raises(EngineError, match="1..1048576"):
        eng.set_lexicon([], 1)
    with pytest.raises(EngineError, match="word 1 "):
        eng.set_lexicon(["fine", "not fine"], 1)
    assert eng.lexicon_size == 0
    with pytest.raises(EngineError, match="no lexicon"):
        eng.logits_lexicon(np.zeros((1, 26, 95), np.float32))
    with pytest.raises(EngineError, match="bf16"):
        eng_bf16.set_lexicon(["a"], 1)
    eng_bf16.set_lexicon(None)                                                           # clearing is always accepted
    turned = Engine(weights["dir"], orient=1)
    with pytest.raises(EngineError, match="orientation"):
        turned.set_lexicon(["a"], 1)
    assert turned.lexicon_size == 0
    turned.close()
    with pytest.raises(EngineError, match="orientation"):
        Engine(weights["dir"], orient=1, lexicon=["a"], lexicon_m=2)
    buf = DeviceBuffer(1024 * 768 * 3)
    buf.upload(pages[0])
    x = np.zeros((1, 26, 95), np.float32)
    eng.set_lexicon(["a", "b"], 2)
    assert eng.stream_push(buf, 1, 1024, 768) == []
    with pytest.raises(EngineError, match="streamed batches"):                           # setting, clearing and the stage call while batches stream
        eng.set_lexicon(["c"], 1)
    with pytest.raises(EngineError, match="streamed batches"):
        eng.set_lexicon(None)
    with pytest.raises(EngineError, match="streamed batches"):
        eng.logits_lexicon(x)
    assert eng.lexicon_size == 2 and eng.lexicon_m == 2
    streamed = _drain(eng, [])
    assert len(streamed) == 1 and streamed[0].lex_idx.shape == (len(streamed[0]), 2)
    eng.set_lexicon(None)
    plain = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
    # with a communicator: each rank's own results carry matches, the gathered payload is the standard block; the sharded call refuses
    comm = Comm(eng, 0, 1, "127.0.0.1", free_port(), transport="socket")
    try:
        with _Lex(eng, ["a", "b", "The"], 2):
            want = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
            comm.attach(True)
            got = eng.pages_to_data_dev(buf, 1, 1024, 768)[0]
            _, g_ids = comm.last_gathered()
            g_conf, g_prob = comm.last_gathered_conf()
            comm.attach(False)
            with pytest.raises(EngineError, match="lexicon"):
                comm.pages_to_data_sharded(buf, 1, 1024, 768)
        _same_standard_fields(plain, got)
        assert got.lex_idx.tobytes() == want.lex_idx.tobytes() and got.lex_logp.tobytes() == want.lex_logp.tobytes()
        assert np.array_equal(g_ids, got.ids) and g_conf.tobytes() == got.conf.tobytes() and g_prob.tobytes() == got.prob.tobytes()
        assert [list(r) for r in comm.pages_to_data_sharded(buf, 1, 1024, 768)] == [list(plain)]      # cleared again: the sharded call runs
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
words = json.load(open({words!r}))
plain = pytuatara.image_to_data(img, {wdir!r}, "o", conf=True)
got = pytuatara.image_to_data(img, {wdir!r}, "o", conf=True, lexicon=words, lexicon_m=3)
many = pytuatara.images_to_data([img], {wdir!r}, "o", conf=True, lexicon=words, lexicon_m=3)
both = pytuatara.image_to_data(img, {wdir!r}, "o", lexicon=words, alts=2, allowlist="0123456789", lines=True)
again = pytuatara.image_to_data(img, {wdir!r}, "o", conf=True)
errors = []
for kw in (dict(lexicon=words, lexicon_m=0), dict(lexicon=["fine", "not fine"]), dict(lexicon=[]), dict(lexicon=words, orient="flip")):
    try:
        pytuatara.image_to_data(img, {wdir!r}, "o", **kw)
        errors.append(None)
    except Exception as ex:
        errors.append([type(ex).__name__, str(ex)])
print("RESULT " + json.dumps(dict(plain=plain, got=got, same=(many == [got]), both=both, again=(again == plain), errors=errors)))
'''


def _funsd_lexicon(eng, funsd, itos):
    cls = LR.class_of(itos)
    found = eng.images_to_data([funsd])[0]
    own = sorted({t for t, ids in zip(found.texts, found.ids) if _qualifies(ids, t, cls)})
    return own + [w for w in unique_words(200, 81, itos) if w not in set(own)]


def test_pytuatara_lexicon_keyword(eng, weights, funsd, itos, tmp_path):
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
    with _Lex(eng, words, 3):
        want = eng.image_to_data(funsd, conf=True)
    assert len(want) > 20 and len(res["got"]) == len(want)
    for g, w in zip(res["got"], want):
        assert set(g) == {"text", "bbox", "conf", "char_conf", "lexicon"}
        assert (g["text"], g["bbox"], g["conf"], g["char_conf"]) == (w["text"], w["bbox"], w["conf"], w["char_conf"])
        assert [a[0] for a in g["lexicon"]] == [a[0] for a in w["lexicon"]]
        # prob = exp(logp) in float64 on both sides, by two exp implementations (the C library's, numpy's) of at most one ulp each
        assert all(abs(a[1] - b[1]) <= 2 * 2.0 ** -52 * b[1] for a, b in zip(g["lexicon"], w["lexicon"]))
    assert [{k: v for k, v in g.items() if k != "lexicon"} for g in res["got"]] == res["plain"]           # the lexicon changes nothing else
    assert res["same"] and res["again"]                                                  # the list form agrees; the cached engine is left without a lexicon
    assert all(set(d) == {"text", "bbox", "line", "word", "alternatives", "lexicon"} for d in res["both"])
    assert all(set(w) <= set(DIGITS) for d in res["both"] for w, _ in d["lexicon"])
    assert res["errors"][0][0] == "ValueError" and res["errors"][1][0] == "ValueError" and "word 1 " in res["errors"][1][1]
    assert res["errors"][2][0] == "ValueError"
    assert res["errors"][3] is not None and "orientation" in res["errors"][3][1]        # orient with a lexicon: the engine's message


def test_ocr_cli_lexicon(eng, weights, funsd, itos, tmp_path):
    from tuatara_amd import build as B
    B.build_examples()
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    png = os.path.join(DATA, "funsd_0001129658.png")
    cli = os.path.join(B.ROOT, "build", "examples", "ocr_cli")
    bgr = np.ascontiguousarray(funsd[:, :, ::-1])                                        # the CLI feeds BGR
    words = _funsd_lexicon(eng, bgr, itos)
    wfile = tmp_path / "words.txt"
    wfile.write_text("\n".join(words) + "\n")
    out = subprocess.run([cli, "--lexicon", str(wfile), "--lexicon-m", "2", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr
    with _Lex(eng, words, 2):
        want = eng.images_to_data([bgr], conf=True)[0]
    lines = out.stdout.splitlines()
    at = 0
    assert len(want) > 20
    for i, g in enumerate(want):
        bb, conf, text = lines[at].split("\t")
        at += 1
        assert [float(v) for v in bb.split()] == g["bbox"] and text == g["text"] and conf == f"{g['conf']:.6f}"
        for k, (w, p) in zip(want.lex_idx[i], g["lexicon"]):
            assert lines[at] == f"\t={int(k)} {p:.6f} {w}"
            at += 1
    assert at == len(lines)
    bad = subprocess.run([cli, "--lexicon-m", "2", png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=60)
    assert bad.returncode == 1 and "--lexicon" in bad.stderr
    (tmp_path / "bad.txt").write_text("fine\nnot fine\n")
    bad = subprocess.run([cli, "--lexicon", str(tmp_path / "bad.txt"), png, weights["dir"], str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert bad.returncode == 1 and "word 1 " in bad.stderr
