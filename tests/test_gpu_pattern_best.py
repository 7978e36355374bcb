"""GPU suite for the best decode of patterns (DESIGN.md "Patterns", the likeliest member): pattern_best_kernel through ttr_logits_decode_patterns_best
against the float64 list-Viterbi of tests/pattern_best_ref.py on the lexicon suite's adversarial logits, against the greedy call, and against the lexicon
scorer on the enumerated language bit for bit; then the engine - both modes on the same crops and regions, the page forms against each other, lines and
character boxes, the refusals, and the callers in child processes.

Bounds.  A returned log-probability is the lexicon's chain of fp32 additions over the lexicon's table, so its distance from float64 is the lexicon suite's
tol(w) = (L + 1) * 2.5e-6 + 2^-19 * the sum of |x[c] - x[id]| + |log prob| along the word (tests/lexicon_ref.py).  A forced probability is
expf(d) / sum with d = x[id] - max_A rounded once: relative 2e-6 for the sum and the division (the greedy decode's bar) plus |d| * 2^-23 for the exponent."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import charset_ref as CR
from tests import lexicon_ref as LR
from tests import pattern_best_ref as BR
from tests import pattern_ref as PR
from tests.conftest import DATA, GOLDEN, ROOT
from tests.test_gpu_lexicon import adversarial_logits, crop_kinds
from tests.test_pattern_best_cpu import BIG, FINITE, PATTERNS

pytestmark = pytest.mark.gpu

DIGITS = "0123456789"
UPPER = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
LOWER = "abcdefghijklmnopqrstuvwxyz"
TRAP = r"(USD|EUR|GBP)\d+"


@pytest.fixture(scope="module")
def itos():
    with open(os.path.join(GOLDEN, "g1_ref_tokenizer.json")) as f:
        return [chr(c) for c in json.load(f)["itos"]]


def _word(row):
    """the classes in front of the first EOS of an ids row"""
    row = [int(c) for c in row]
    return tuple(row[:row.index(0)] if 0 in row else row)


def _text(itos, row):
    return "".join(itos[c] for c in _word(row) if c != 88)


def _tol(mag, w):
    return (len(w) + 1) * 2.5e-6 + 2.0 ** -19 * (sum(mag[p][c] for p, c in enumerate(w)) + mag[len(w)][0])


def _engine_dfa(pattern, mask):
    from tuatara_amd.engine import Pattern
    d, m, start, done = Pattern(pattern, mask).table()
    return PR.Dfa(np.array(d), np.array(m), start, done, mask)


def check_rows(eng, itos, x, patterns, pattern_of, set_of=None, sets=None, kinds=None, where=""):
    """One best call and one greedy call on the same rows, every assertion of the suite on every row.  Returns counts: rows with a pattern among the
    normal and peaked crops, how many of those the runner-up guard left out, rows whose two readings coincide, rows whose readings differ."""
    from tuatara_amd.engine import confidence_from_probs
    n = len(x)
    kinds = crop_kinds(n) if kinds is None else kinds
    masks = [None if set_of is None or set_of[i] < 0 else sets[set_of[i]] for i in range(n)]
    lp, mag = LR.tables(x, np.stack([CR.FULL if m is None else m for m in masks]))
    ids, prob, conf, logp = eng.logits_decode_patterns(x, patterns, pattern_of, set_of=set_of, sets=sets, best=True)
    g_ids, g_prob, g_conf = eng.logits_decode_patterns(x, patterns, pattern_of, set_of=set_of, sets=sets)
    p_ids, p_prob, p_conf = eng.logits_confidence(x, set_of=set_of, sets=sets) if set_of is not None else eng.logits_confidence(x)
    assert ids.dtype == np.int32 and prob.dtype == conf.dtype == logp.dtype == np.float32 and logp.shape == (n,)
    counted = left = same = differ = 0
    worst = 0.0
    for i in range(n):
        k = int(pattern_of[i])
        _, c = confidence_from_probs(ids[i], prob[i])
        assert c.tobytes() == conf[i:i + 1].tobytes(), (where, i)
        if k < 0:                                              # a row without a pattern: the masked decode's bits, no score
            assert ids[i].tobytes() == p_ids[i].tobytes() and prob[i].tobytes() == p_prob[i].tobytes() and conf[i].tobytes() == p_conf[i].tobytes(), (where, i)
            assert np.isneginf(logp[i]), (where, i)
            continue
        ref = PR.compile_pattern(itos, patterns[k], masks[i])
        top = BR.list_viterbi64(lp[i], ref)
        w, g = _word(ids[i]), _word(g_ids[i])
        if not top:                                            # no member of finite score: the greedy walk's reading, bit for bit
            assert ids[i].tobytes() == g_ids[i].tobytes() and prob[i].tobytes() == g_prob[i].tobytes() and conf[i].tobytes() == g_conf[i].tobytes(), (where, i)
            assert not np.isfinite(logp[i]), (where, i)
            continue
        text = _text(itos, ids[i])
        assert len(w) <= 25 and ids[i][len(w)] == 0 and re.fullmatch(patterns[k], text) and PR.matches(itos, ref, text), (where, i, patterns[k], text)
        assert (ids[i][len(w) + 1:] == p_ids[i][len(w) + 1:]).all() and prob[i][len(w) + 1:].tobytes() == p_prob[i][len(w) + 1:].tobytes(), (where, i)
        s_got, t_got = BR.score64(lp[i], w), _tol(mag[i], w)
        s_best, w_best = top[0]
        t_best = _tol(mag[i], w_best)
        assert np.isfinite(s_got), (where, i)
        err = abs(float(logp[i]) - s_got)
        worst = max(worst, err / t_got)
        print(f"{where} row {i} kind {kinds[i]} {patterns[k]!r}: {text!r} logp {logp[i]:.6f} float64 {s_got:.6f} best {s_best:.6f} |err| / tol {err / t_got:.3f}")
        assert err <= t_got, (where, i, err, t_got)
        assert s_got >= s_best - t_got - t_best, (where, i, s_got, s_best)
        # against the greedy reading of the same call
        s_g, t_g = BR.score64(lp[i], g), _tol(mag[i], g) if np.isfinite(BR.score64(lp[i], g)) else 0.0
        assert s_got >= s_g - t_got - t_g, (where, i, s_got, s_g)
        if w == g:
            same += 1
            assert ids[i].tobytes() == g_ids[i].tobytes() and prob[i].tobytes() == g_prob[i].tobytes() and conf[i].tobytes() == g_conf[i].tobytes(), (where, i)
        else:
            differ += 1
        # the forced path's probabilities in float64
        r_ids, r_prob, _ = BR.forced_decode64(x[i], ref, w)
        assert (r_ids == ids[i]).all(), (where, i)
        if abs(float(x[i].astype(np.float64).max()) - float(x[i].astype(np.float64).min())) < 1e6:
            for p in range(len(w) + 1):
                a = PR.allowed_at(ref.delta, ref.mind, int(_state(ref, w, p)), p)
                d = abs(float(x[i, p, ids[i, p]]) - float(np.where(a, x[i, p].astype(np.float64), -np.inf).max()))
                assert abs(float(prob[i, p]) - r_prob[p]) <= (2e-6 + d * 2.0 ** -23) * r_prob[p] + 1e-37, (where, i, p, prob[i, p], r_prob[p])
        # the string itself
        count = kinds[i] < 2
        counted += count
        runner = top[1][0] if len(top) > 1 else -np.inf
        t_run = _tol(mag[i], top[1][1]) if len(top) > 1 else 0.0
        if s_best - runner > 2 * max(t_best, t_run):
            assert w == w_best, (where, i, text)
        else:
            left += count
            if kinds[i] == 3:                                  # ties everywhere: the rule's own order, restated in fp32 on the table of the device's id0 / prob0
                lp32 = np.full((26, 96), -np.inf, np.float32)
                ok = CR.allowed(CR.FULL if masks[i] is None else masks[i])
                row_x = x[i][np.arange(26), p_ids[i]]
                with np.errstate(all="ignore"):
                    lp32[:, :95] = np.where(ok[None, :], (x[i] - row_x[:, None]) + np.log(p_prob[i])[:, None], -np.inf).astype(np.float32)
                want = BR.viterbi32(lp32, _engine_dfa(patterns[k], masks[i]))
                assert want is not None and w == want[0], (where, i, text)
    print(f"{where}: {counted} counted rows, {left} left out by the runner-up guard, {same} equal to greedy, {differ} not; max |logp - float64| / tol = {worst:.3f}")
    return counted, left, same, differ


def _state(dfa, w, p):
    s = dfa.start
    for c in w[:p]:
        s = int(dfa.delta[s, c])
    return s


def _stage_case(n):
    from tuatara_amd.engine import charset_mask
    sets = np.stack([charset_mask(DIGITS + UPPER + "./"), charset_mask(DIGITS + UPPER + LOWER + "./,")])
    pattern_of = np.array([(i % (len(PATTERNS) + 1)) - 1 for i in range(n)] if n > 1 else [0], np.int32)
    set_of = np.array([(i % 3) - 1 for i in range(n)], np.int32)
    set_of[(pattern_of == PATTERNS.index(BIG)) & (set_of == 0)] = 1      # (the first set has no lower case)
    return adversarial_logits(n, 40 + n), pattern_of, set_of, sets


BIG_CALL = [BIG, r"[cd]*c[cd]{7}", r"[ef]*e[ef]{7}", r"[gh]*g[gh]{6}", r"[ij]*i[ij]{4}", r".{0,25}", r"\d+\.\d{2}", r"(USD|EUR|GBP)\d{2}"]


def _big_case():
    n = 2 * len(BIG_CALL)
    return adversarial_logits(n, 77), np.array([i % len(BIG_CALL) for i in range(n)], np.int32)


def guard_counts(itos, x, patterns, pattern_of, masks):
    """on the float64 reference alone: (normal and peaked rows that have a pattern, those whose runner-up lies within twice the bound)"""
    lp, mag = LR.tables(x, np.stack([CR.FULL if m is None else m for m in masks]))
    counted = left = 0
    for i in np.nonzero((pattern_of >= 0) & (crop_kinds(len(x)) < 2))[0]:
        top = BR.list_viterbi64(lp[i], PR.compile_pattern(itos, patterns[pattern_of[i]], masks[i]))
        counted += 1
        left += len(top) > 1 and top[0][0] - top[1][0] <= 2 * max(_tol(mag[i], top[0][1]), _tol(mag[i], top[1][1]))
    return counted, left


def test_the_seeds_keep_the_guard_inside_five_percent(itos):
    """the condition on the float64 reference alone (no device): of the normal and peaked rows that have a pattern, at most 5 % have a runner-up within
    twice the bound - per call of the tests below"""
    for n in (1, 5, 37):
        x, pattern_of, set_of, sets = _stage_case(n)
        counted, left = guard_counts(itos, x, PATTERNS, pattern_of, [None if s < 0 else sets[s] for s in set_of])
        assert counted >= (1 if n < 37 else 10) and left <= 0.05 * counted, (n, counted, left)
    x, pattern_of = _big_case()
    counted, left = guard_counts(itos, x, BIG_CALL, pattern_of, [None] * len(x))
    assert counted >= 4 and left <= 0.05 * counted, (counted, left)


_TOTALS = {}


@pytest.mark.parametrize("n", [1, 5, 37])
def test_kernel_against_the_float64_list_viterbi(eng_x4, itos, n):
    assert eng_x4.pattern is None
    x, pattern_of, set_of, sets = _stage_case(n)
    _TOTALS[n] = check_rows(eng_x4, itos, x, PATTERNS, pattern_of, set_of, sets, where=f"n={n}")
    if n == 37:
        counted, left, same, differ = _TOTALS[n]
        assert counted >= 10 and left <= 0.05 * counted, _TOTALS[n]
        assert same > 0 and differ > 0, _TOTALS[n]


def test_one_call_close_to_1024_states_and_a_masked_winner(eng_x4, itos):
    from tuatara_amd.engine import Pattern
    patterns = BIG_CALL
    total = sum(Pattern(p).states + 1 for p in patterns)
    assert 960 < total <= 1024, total
    x, pattern_of = _big_case()
    n = len(x)
    kinds = crop_kinds(n)
    counted, left, _, _ = check_rows(eng_x4, itos, x, patterns, pattern_of, kinds=kinds, where="1024")
    assert left <= 0.05 * counted, (counted, left)
    # the same call again with one class of a winner masked out for its row: the winner moves, and is again the likeliest member of what is left
    ids, _, _, logp = eng_x4.logits_decode_patterns(x, patterns, pattern_of, best=True)
    row = next(i for i in range(n) if pattern_of[i] == patterns.index(r".{0,25}") and kinds[i] < 2 and len(_word(ids[i])) > 0)
    gone = _word(ids[row])[0]
    mask = CR.FULL.copy()
    mask[gone >> 5] &= np.uint32(~(1 << (gone & 31)) & 0xFFFFFFFF)
    set_of = np.full(n, -1, np.int32)
    set_of[row] = 0
    check_rows(eng_x4, itos, x, patterns, pattern_of, set_of, mask[None, :], kinds=kinds, where="1024, one class masked")
    ids2, _, _, logp2 = eng_x4.logits_decode_patterns(x, patterns, pattern_of, set_of=set_of, sets=mask[None, :], best=True)
    assert gone not in _word(ids2[row]) and _word(ids2[row]) != _word(ids[row])
    others = np.arange(n) != row
    assert ids2[others].tobytes() == ids[others].tobytes() and logp2[others].tobytes() == logp[others].tobytes()


def test_the_trap_reads_usd_here_and_eur_through_the_greedy_call(eng_x4, itos):
    cls = LR.class_of(itos)
    x = np.zeros((1, 26, 95), np.float32)
    x[0, 0, cls["E"]], x[0, 0, cls["U"]] = 2.0 + 1e-3, 2.0
    x[0, 1, cls["S"]], x[0, 2, cls["D"]] = 5.0, 5.0
    x[0, 3, cls["4"]], x[0, 4, cls["2"]], x[0, 5, 0] = 5.0, 5.0, 5.0
    ids, prob, conf, logp = eng_x4.logits_decode_patterns(x, [TRAP], [0], best=True)
    g_ids, _, g_conf = eng_x4.logits_decode_patterns(x, [TRAP], [0])
    assert _text(itos, ids[0]) == "USD42" and _text(itos, g_ids[0]) == "EUR42"
    lp, _ = LR.tables(x)
    assert float(logp[0]) > BR.score64(lp[0], _word(g_ids[0])) + 9.0
    check_rows(eng_x4, itos, x, [TRAP], np.zeros(1, np.int32), kinds=np.zeros(1, np.int64), where="trap")


def test_best_is_no_worse_than_greedy_in_float32_with_no_slack(eng_x4, itos):
    """score(best) >= score(greedy) is exact in fp32: both are the same chain of additions over the same table.  The lexicon scorer forms that chain on the
    device's own table, so with the two readings of a row as the word list it returns both scores: the best reading's has the bits of pattern_logp, and
    it is at least the greedy reading's as float32, no bound in between."""
    x, pattern_of, set_of, sets = _stage_case(37)
    ids, _, _, logp = eng_x4.logits_decode_patterns(x, PATTERNS, pattern_of, set_of=set_of, sets=sets, best=True)
    g_ids, _, _ = eng_x4.logits_decode_patterns(x, PATTERNS, pattern_of, set_of=set_of, sets=sets)
    nameable = set(LR.class_of(itos).values())
    compared = 0
    try:
        for i in np.nonzero(pattern_of >= 0)[0]:
            w, g = _word(ids[i]), _word(g_ids[i])
            if w == g or not w or not g or not (set(w) | set(g)) <= nameable or not np.isfinite(logp[i]):
                continue
            eng_x4.set_lexicon([_text(itos, ids[i]), _text(itos, g_ids[i])], 2)
            idx, lex_logp = eng_x4.logits_lexicon(x[i:i + 1], set_of=set_of[i:i + 1], sets=sets)
            score = {int(k): v for k, v in zip(idx[0], lex_logp[0]) if k >= 0}
            assert 0 in score and score[0].tobytes() == logp[i].tobytes(), (i, score, logp[i])
            if 1 in score:                                     # (a greedy reading of score -inf or NaN is never returned)
                compared += 1
                assert score[0] >= score[1], (i, score)
    finally:
        eng_x4.set_lexicon(None)
    assert compared >= 8, compared


@pytest.mark.parametrize("pattern", FINITE)
def test_cross_check_against_the_lexicon_bit_for_bit(eng_x4, itos, pattern):
    """the enumerated language as a lexicon: slot 0 is the likeliest member, and its logp has the same float32 bits - both are one expression on one table"""
    ref = PR.compile_pattern(itos, pattern)
    words = ["".join(itos[c] for c in w) for w in BR.members(ref)]
    assert all(len(w) >= 1 for w in words) and len(set(words)) == len(words) > 50
    x = adversarial_logits(37, 52)
    ids, _, _, logp = eng_x4.logits_decode_patterns(x, [pattern], np.zeros(37, np.int32), best=True)
    try:
        eng_x4.set_lexicon(words, 2)
        idx, lex_logp = eng_x4.logits_lexicon(x)
    finally:
        eng_x4.set_lexicon(None)
    compared = 0
    for i in range(37):
        if idx[i, 0] < 0:
            assert not np.isfinite(logp[i]), i
            continue
        assert logp[i:i + 1].tobytes() == lex_logp[i, :1].tobytes(), (i, logp[i], lex_logp[i])
        if lex_logp[i, 0] != lex_logp[i, 1]:                  # (an exact tie is broken by the two rules' own orders)
            compared += 1
            assert words[idx[i, 0]] == _text(itos, ids[i]), (i, words[idx[i, 0]], _text(itos, ids[i]))
    assert compared >= 12, compared                        # (the normal and the peaked crops alone are 15)


# ------------------------------------------------------------------------------------------------- the engine
ENGINE_PATTERNS = [r"[A-Z][a-z]*", r"\d{2,6}"]


@pytest.fixture(scope="module")
def page():
    from tuatara_amd import synth
    return synth.synthetic_page(60, 1024, 768, n_words=14)


@pytest.mark.parametrize("precision", ["f16x4", "f32"])
def test_engine_modes_on_crops_and_regions(eng_x4, eng_f32, itos, page, precision):
    from tuatara_amd.engine import PATTERN_BEST, PATTERN_GREEDY
    eng = eng_x4 if precision == "f16x4" else eng_f32
    assert eng.pattern is None and eng.pattern_decode == PATTERN_GREEDY
    crops = CR.sweep_crops(8)
    pattern_of = np.array([i % 3 - 1 for i in range(len(crops))], np.int32)
    rng = np.random.default_rng(9)
    regions, patterns = [], []
    for i in range(12):
        x0, y0 = int(rng.integers(0, 768 - 140)), int(rng.integers(0, 1024 - 40))
        regions.append({"rect": (x0, y0, x0 + int(rng.integers(60, 140)), y0 + int(rng.integers(16, 40)))})
        patterns.append((ENGINE_PATTERNS + [None])[i % 3])
    try:
        lg, g_ids = eng.parseq_logits(crops, pattern_of=pattern_of, patterns=ENGINE_PATTERNS)
        g_regions = eng.read_regions(page, regions, patterns=patterns)
        eng.set_pattern_decode(PATTERN_BEST)
        assert eng.pattern_decode == PATTERN_BEST
        lb, b_ids = eng.parseq_logits(crops, pattern_of=pattern_of, patterns=ENGINE_PATTERNS)
        assert lb.tobytes() == lg.tobytes()                   # the AR loop and the refinement pass do not know the mode
        s_ids, s_prob, s_conf, s_logp = eng.logits_decode_patterns(lb, ENGINE_PATTERNS, pattern_of, best=True)
        assert np.asarray(b_ids).reshape(-1, 26).tobytes() == s_ids.tobytes()
        free = pattern_of < 0
        assert np.asarray(b_ids).reshape(-1, 26)[free].tobytes() == np.asarray(g_ids).reshape(-1, 26)[free].tobytes()
        for i in np.nonzero(~free)[0]:
            assert re.fullmatch(ENGINE_PATTERNS[pattern_of[i]], _text(itos, s_ids[i])), i
        # the regions: the stage decode of their own logits, bit for bit
        b_regions = eng.read_regions(page, regions, patterns=patterns)
        quads = np.array([g["quad"] for g in g_regions], np.float32).reshape(-1, 8)      # (the caller's floats, as the call read them)
        r_of = np.array([i % 3 if i % 3 < 2 else -1 for i in range(12)], np.int32)
        r_lg, _ = eng.parseq_logits(eng.pack_regions(page, quads), pattern_of=r_of, patterns=ENGINE_PATTERNS)
        r_ids, r_prob, r_conf, r_logp = eng.logits_decode_patterns(r_lg, ENGINE_PATTERNS, r_of, best=True)
        changed = 0
        for k, (b, g) in enumerate(zip(b_regions, g_regions)):
            assert b["region"] == g["region"] == k and b["bbox"] == g["bbox"] and b["quad"] == g["quad"]
            assert b["ids"] == r_ids[k].tolist() and np.asarray(b["prob"], np.float32).tobytes() == r_prob[k].tobytes()
            assert np.float32(b["conf"]).tobytes() == r_conf[k:k + 1].tobytes() and np.float32(b["pattern_logp"]).tobytes() == r_logp[k:k + 1].tobytes()
            assert "pattern_logp" not in g
            if patterns[k] is None:                           # every field of a region without a pattern is greedy mode's
                assert {kk: v for kk, v in b.items() if kk != "pattern_logp"} == g and np.isneginf(b["pattern_logp"])
            else:
                assert re.fullmatch(patterns[k], b["text"]) and np.isfinite(b["pattern_logp"])
                changed += b["text"] != g["text"]
        print(f"{precision}: {changed} of 8 regions change their reading in best mode")
    finally:
        eng.set_pattern_decode(PATTERN_GREEDY)
        eng.set_pattern()


@pytest.mark.parametrize("precision", ["f16x4", "f32"])
def test_the_engines_own_pattern_on_a_page_against_the_stage_decode(eng_x4, eng_f32, itos, page, precision):
    """The engine's own pattern (set_pattern: no staged table, the extent and the mask filled in by parseq_forward) on a page and through ttr_parseq_logits,
    against ttr_logits_decode_patterns_best of the page's own logits - a staged table of the same pattern - bit for bit, and against the float64 reference."""
    from tuatara_amd.engine import PATTERN_BEST, PATTERN_GREEDY
    eng = eng_x4 if precision == "f16x4" else eng_f32
    pattern = ENGINE_PATTERNS[0]
    try:
        eng.set_pattern(pattern, best=True)
        assert eng.pattern_decode == PATTERN_BEST
        r = eng.images_to_data([page], conf=True)[0]
        canvas, ratio = eng.resize_canvas(page)                # the page's own crop batch (tests/test_gpu_charset.py's composition)
        crops, _ = eng.pack_crops(page, eng.ccl_boxes(eng.craft_heatmap(canvas)), ratio)
        n = len(crops)
        assert n == len(r) > 0
        lb, b_ids = eng.parseq_logits(crops)                   # ttr_parseq_logits: the own-pattern path, best ids
        own = np.full(n, -1, np.int32)
        s_ids, s_prob, s_conf, s_logp = eng.logits_decode_patterns(lb, None, own, best=True)
        assert np.asarray(b_ids).reshape(n, 26).tobytes() == s_ids.tobytes() == r.ids.tobytes()
        assert s_prob.tobytes() == r.prob.tobytes() and s_conf.tobytes() == r.conf.tobytes() and s_logp.tobytes() == r.pattern_logp.tobytes()
        eng.set_pattern_decode(PATTERN_GREEDY)
        lg, g_ids = eng.parseq_logits(crops)
        assert lg.tobytes() == lb.tobytes()                    # the same logits in both modes
        assert np.asarray(g_ids).reshape(n, 26).tobytes() == eng.logits_decode_patterns(lb, None, own)[0].tobytes()
        eng.set_pattern()
        # ... and the stage decode of these logits is the likeliest member by the float64 reference (every assertion of check_rows)
        _, _, same, differ = check_rows(eng, itos, lb, [pattern], np.zeros(n, np.int32), kinds=np.zeros(n, np.int64), where=f"page {precision}")
        t_ids = eng.logits_decode_patterns(lb, [pattern], np.zeros(n, np.int32), best=True)[0]
        assert t_ids.tobytes() == r.ids.tobytes() and same + differ == n
    finally:
        eng.set_pattern_decode(PATTERN_GREEDY)
        eng.set_pattern()


def _same_page(x, y):
    return (x.texts == y.texts and x.ids.tobytes() == y.ids.tobytes() and x.bbox.tobytes() == y.bbox.tobytes() and x.prob.tobytes() == y.prob.tobytes()
            and x.conf.tobytes() == y.conf.tobytes() and (x.pattern_logp is None) == (y.pattern_logp is None)
            and (x.pattern_logp is None or x.pattern_logp.tobytes() == y.pattern_logp.tobytes()))


def test_page_forms_agree_and_the_views(eng_x4, page):
    from tuatara_amd.engine import PATTERN_BEST, PATTERN_GREEDY, DeviceBuffer, EngineError
    pattern = ENGINE_PATTERNS[0]
    buf = DeviceBuffer(1024 * 768 * 3)
    try:
        eng_x4.set_pattern(pattern)
        greedy = eng_x4.images_to_data([page], conf=True)[0]
        assert greedy.pattern_logp is None and "pattern_logp" not in greedy[0]
        arr = (C.c_void_p * 1)()
        img = np.ascontiguousarray(page)
        eng_x4._check(eng_x4.lib.ttr_image_to_data(eng_x4.h, img.ctypes.data_as(C.POINTER(C.c_uint8)), 1024, 768, 768 * 3, arr))
        assert not eng_x4.lib.ttr_result_pattern_logp(arr[0])  # the view is NULL in greedy mode
        eng_x4.lib.ttr_result_free(arr[0])
        eng_x4.set_pattern(pattern, best=True)
        assert eng_x4.pattern_decode == PATTERN_BEST
        best = eng_x4.images_to_data([page], conf=True)[0]
        assert eng_x4.image_to_data(page, conf=True) == list(best)
        assert len(best) == len(greedy) > 0 and best.bbox.tobytes() == greedy.bbox.tobytes()      # items, order, boxes: the detector's
        assert best.pattern_logp.shape == (len(best),) and best.pattern_logp.dtype == np.float32 and np.isfinite(best.pattern_logp).all()
        assert all(re.fullmatch(pattern, t) for t in best.texts)
        for i in range(len(best)):
            assert best[i]["pattern_logp"] == float(best.pattern_logp[i])
            if best.texts[i] == greedy.texts[i]:              # the same reading: the same bits
                assert best.ids[i].tobytes() == greedy.ids[i].tobytes() and best.prob[i].tobytes() == greedy.prob[i].tobytes() and best.conf[i].tobytes() == greedy.conf[i].tobytes()
        eng_x4._check(eng_x4.lib.ttr_image_to_data(eng_x4.h, img.ctypes.data_as(C.POINTER(C.c_uint8)), 1024, 768, 768 * 3, arr))
        got = np.zeros(len(best), np.float32)
        assert eng_x4.lib.ttr_results_gather_pattern_logp(arr, 1, got.ctypes.data_as(C.POINTER(C.c_float))) == len(best)
        assert got.tobytes() == best.pattern_logp.tobytes()
        assert np.ctypeslib.as_array(eng_x4.lib.ttr_result_pattern_logp(arr[0]), (len(best),)).tobytes() == got.tobytes()
        eng_x4.lib.ttr_result_free(arr[0])
        many = eng_x4.images_to_data([page, page], conf=True)
        assert all(_same_page(m, best) for m in many)
        buf.upload(page)
        assert _same_page(eng_x4.pages_to_data_dev(buf, 1, 1024, 768, conf=True)[0], best)
        assert _same_page(eng_x4.pages_to_data_dev_v([(buf.ptr, 1024, 768)], conf=True)[0], best)
        streamed = eng_x4.stream_push(buf.ptr, 1, 1024, 768, conf=True)
        with pytest.raises(EngineError, match="ttr_engine_set_pattern_decode: streamed batches are in flight"):
            eng_x4.set_pattern_decode(PATTERN_GREEDY)
        assert eng_x4.pattern_decode == PATTERN_BEST
        while True:
            r = eng_x4.stream_flush(conf=True)
            if not r:
                break
            streamed += r
        assert len(streamed) == 1 and _same_page(streamed[0], best)
        with pytest.raises(EngineError, match=r"ttr_engine_set_pattern_decode: mode 2 is neither"):
            eng_x4.set_pattern_decode(2)
        eng_x4.set_pattern_decode(PATTERN_GREEDY)
        with pytest.raises(EngineError, match=r"without its"):                      # a refused pattern changes nothing, the mode included
            eng_x4.set_pattern("(", best=True)
        assert eng_x4.pattern_decode == PATTERN_GREEDY and eng_x4.pattern == pattern
        eng_x4.set_pattern_decode(PATTERN_BEST)
        eng_x4.set_pattern()                                  # best mode without a pattern: no effect, no view
        plain = eng_x4.images_to_data([page], conf=True)[0]
        eng_x4.set_pattern_decode(PATTERN_GREEDY)
        assert plain.pattern_logp is None and _same_page(plain, eng_x4.images_to_data([page], conf=True)[0])
    finally:
        while eng_x4.stream_flush():
            pass
        eng_x4.set_pattern_decode(PATTERN_GREEDY)
        eng_x4.set_pattern()
        buf.free()


def test_refusals_on_a_bf16_engine(eng_bf16):
    from tuatara_amd.engine import PATTERN_BEST, PATTERN_GREEDY, EngineError
    with pytest.raises(EngineError, match="ttr_engine_set_pattern_decode: the best decode needs an f16x4 or f32 engine"):
        eng_bf16.set_pattern_decode(PATTERN_BEST)
    assert eng_bf16.pattern_decode == PATTERN_GREEDY
    eng_bf16.set_pattern_decode(PATTERN_GREEDY)                # the default is always accepted
    with pytest.raises(EngineError, match="f16x4 or f32 engine"):
        eng_bf16.logits_decode_patterns(np.zeros((1, 26, 95), np.float32), [r"\d+"], [0], best=True)


def test_lines_and_character_boxes_consume_the_new_text(weights, page):
    from tuatara_amd.engine import Engine
    pattern = ENGINE_PATTERNS[0]
    eng = Engine(weights["dir"], lines=1, chars=1, pattern=pattern, pattern_best=True)
    base = Engine(weights["dir"], pattern=pattern, pattern_best=True)
    try:
        r, b = eng.images_to_data([page], conf=True)[0], base.images_to_data([page], conf=True)[0]
        assert len(r) == len(b) > 0 and r.texts == b.texts and r.ids.tobytes() == b.ids.tobytes() and r.pattern_logp.tobytes() == b.pattern_logp.tobytes()
        assert (np.diff(r.char_first) == [len(t) for t in r.texts]).all()          # one box per character of the best text
        assert all(re.fullmatch(pattern, w) for ln in r.lines for w in ln["text"].split())
    finally:
        eng.close()
        base.close()


_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "build", "bindings"))
sys.path.insert(0, sys.argv[1])
import pytuatara
from tuatara_amd import synth
page = synth.synthetic_page(60, 1024, 768, n_words=14)
w, pattern = sys.argv[2], sys.argv[3]
plain = pytuatara.image_to_data(page, w, "o", conf=True, pattern=pattern)
best = pytuatara.image_to_data(page, w, "o", conf=True, pattern=pattern, pattern_best=True)
many = pytuatara.images_to_data([page], w, "o", conf=True, pattern=pattern, pattern_best=True)
after = pytuatara.image_to_data(page, w, "o", conf=True, pattern=pattern)
raised = ""
try:
    pytuatara.image_to_data(page, w, "o", pattern="(", pattern_best=True)
except ValueError as e:
    raised = str(e)
again = pytuatara.image_to_data(page, w, "o", conf=True, pattern=pattern)
print(json.dumps({"plain": plain, "best": best, "many": many, "after": after, "again": again, "raised": raised}))
"""


def test_pytuatara_and_ocr_cli_in_child_processes(weights, page, eng_x4, tmp_path):
    from tuatara_amd import build as B
    B.build_pytuatara()
    B.build_examples()
    pattern = ENGINE_PATTERNS[0]
    try:
        eng_x4.set_pattern(pattern, best=True)
        want = eng_x4.images_to_data([page], conf=True)[0]
        funsd_png = os.path.join(DATA, "funsd_0001129658.png")
    finally:
        eng_x4.set_pattern(None, best=False)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TUATARA_")}
    script = os.path.join(str(tmp_path), "child.py")
    with open(script, "w") as f:
        f.write(_CHILD)
    out = subprocess.run([sys.executable, script, ROOT, weights["dir"], pattern], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    got = json.loads(out.stdout.splitlines()[-1])
    assert [(r["text"], r["bbox"]) for r in got["best"]] == [(t, b.tolist()) for t, b in zip(want.texts, want.bbox)]
    assert [np.float32(r["pattern_logp"]).tobytes() for r in got["best"]] == [v.tobytes() for v in want.pattern_logp]
    assert got["many"] == [got["best"]]
    assert all("pattern_logp" not in r for r in got["plain"]) and got["after"] == got["plain"] == got["again"]   # reset after the call, also when it raised
    assert "without its" in got["raised"]
    cli = subprocess.run([os.path.join(B.ROOT, "build", "examples", "ocr_cli"), "--pattern", pattern, "--pattern-best", funsd_png, weights["dir"], str(tmp_path)],
                         capture_output=True, text=True, env=env, timeout=600)
    assert cli.returncode == 0, cli.stderr[-3000:]
    lines = [ln.split("\t") for ln in cli.stdout.splitlines()]
    assert len(lines) > 20
    for bb, text, logp in lines:
        assert len(bb.split()) == 4 and re.fullmatch(pattern, text) and np.isfinite(float(logp)) and float(logp) <= 0.0
