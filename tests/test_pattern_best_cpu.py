"""The best decode of patterns (DESIGN.md "Patterns", the likeliest member) without a GPU: the exported symbols, the host rule ttr_pattern_best_from_lp
against the fp32 restatement of tests/pattern_best_ref.py bit for bit (path, length, score) on random, peaked, all-equal and -inf-laden tables, against
the brute-force maximum over the enumerated members of the finite languages, the hand-made trap that the greedy walk falls into, and what the new calls
refuse without a device.

The restatement walks the ENGINE's table (its state numbers decide the last tie), the float64 list-Viterbi and the enumerator tests/pattern_ref.py's own."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import lexicon_ref as LR
from tests import pattern_best_ref as BR
from tests import pattern_ref as PR
from tests.conftest import GOLDEN

BIG = r"[ab]*a[ab]{7}"                                       # 2^8 residual languages: a minimal automaton of 256 states
FINITE = [r"(USD|EUR|GBP)\d{2}", r"\d{2}/\d{2}", r"[A-C]{1,3}x?"]
PATTERNS = FINITE + [r"\d+\.\d{2}", r"\d*", r".{0,25}", BIG]
KINDS = ("random", "peaked", "equal", "holes")


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


@pytest.fixture(scope="module")
def itos():
    with open(os.path.join(GOLDEN, "g1_ref_tokenizer.json")) as f:
        return [chr(c) for c in json.load(f)["itos"]]


def table(kind, seed):
    """a table f32 [26, 96] of the given kind: rows of log-probabilities (column 95 unused, -inf)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 3.0, (26, 95))
    if kind == "peaked":
        x[np.arange(26), rng.integers(0, 95, 26)] += 30.0
    if kind == "equal":
        x[:] = rng.normal(0.0, 1.0, (26, 1))                   # every class of a row alike: members of one length tie exactly
    lp = np.full((26, 96), -np.inf, np.float32)
    lp[:, :95] = (x - np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)) - x.max(1, keepdims=True)).astype(np.float32)
    if kind == "holes":
        lp[:, :95][rng.random((26, 95)) < 0.35] = -np.inf
        lp[rng.integers(0, 26), rng.integers(0, 95)] = np.nan
    return lp


def engine_dfa(pat):
    d, m, start, done = pat.table()
    return PR.Dfa(np.array(d), np.array(m), start, done, None)


def test_symbols_are_exported(built):
    from tuatara_amd import engine
    lib = engine.load()
    for name in ("ttr_engine_set_pattern_decode", "ttr_engine_pattern_decode", "ttr_result_pattern_logp", "ttr_results_gather_pattern_logp",
                 "ttr_logits_decode_patterns_best", "ttr_pattern_best_from_lp"):
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in engine.SYMBOLS), name
    assert engine.PATTERN_GREEDY == 0 and engine.PATTERN_BEST == 1


def test_the_big_pattern_is_big(built):
    from tuatara_amd.engine import pattern_compile
    assert 200 <= pattern_compile(BIG).states <= 256


@pytest.mark.parametrize("pattern", PATTERNS)
def test_host_rule_against_the_restatement_bit_for_bit(built, itos, pattern):
    from tuatara_amd.engine import pattern_best_from_lp, pattern_compile
    pat = pattern_compile(pattern)
    dfa, ref = engine_dfa(pat), PR.compile_pattern(itos, pattern)
    members = BR.members(ref) if pattern in FINITE else None
    found = 0
    for kind in KINDS:
        for seed in range(4):
            lp = table(kind, 100 * KINDS.index(kind) + seed)
            got, want = pattern_best_from_lp(pat, lp), BR.viterbi32(lp, dfa)
            assert (got is None) == (want is None), (kind, seed)
            if got is None:
                continue
            found += 1
            path, logp = got
            assert tuple(path.tolist()) == want[0] and np.float32(logp).tobytes() == want[1].tobytes(), (kind, seed, path, want)
            text = "".join(itos[c] for c in path)
            assert pat.matches(text) and len(path) <= 25, (kind, seed, text)
            # the float64 list-Viterbi on the reference's own automaton: the returned member scores as the best one, up to the fp32 chain's rounding
            lp64 = lp[:, :95].astype(np.float64)
            lp64[~np.isfinite(lp64)] = -np.inf
            top = BR.list_viterbi64(lp64, ref)
            s_got = BR.score64(lp64, tuple(path.tolist()))
            bound = 2.0 ** -19 * max(abs(s_got), abs(top[0][0]))
            assert abs(float(logp) - s_got) <= bound and s_got >= top[0][0] - 2 * bound, (kind, seed)
            if len(top) > 1 and top[0][0] - top[1][0] > 4 * bound:
                assert tuple(path.tolist()) == top[0][1], (kind, seed)
            if members is not None:                            # ... and as the brute-force maximum over every member
                brute = max(BR.score64(lp64, w) for w in members)
                assert abs(brute - top[0][0]) <= 1e-9 * max(1.0, abs(brute)) and s_got >= brute - 2 * bound, (kind, seed)
    assert found >= 8, found


def test_the_empty_member_can_win(built, itos):
    from tuatara_amd.engine import pattern_best_from_lp, pattern_compile
    lp = table("random", 7)
    lp[0, 0] = -1e-3                                           # the end of the text at once: no digit string comes near
    path, logp = pattern_best_from_lp(pattern_compile(r"\d*"), lp)
    assert len(path) == 0 and np.float32(logp) == lp[0, 0]


def test_ties_everywhere_follow_the_rule(built, itos):
    """all rows equal in all classes: the shortest member, by the lower class at every position"""
    from tuatara_amd.engine import pattern_best_from_lp, pattern_compile
    lp = np.full((26, 96), np.float32(-2.5), np.float32)
    cls = LR.class_of(itos)
    for pattern, text in ((r"(USD|EUR|GBP)\d{2}", None), (r"[A-C]{1,3}x?", "A"), (r"\d*", ""), (r"\d+\.\d{2}", "0.00")):
        pat = pattern_compile(pattern)
        path, logp = pattern_best_from_lp(pat, lp)
        want = BR.viterbi32(lp, engine_dfa(pat))
        assert tuple(path.tolist()) == want[0] and np.float32(logp).tobytes() == want[1].tobytes()
        if text is not None:                                   # (one shortest length, then class order)
            assert "".join(itos[c] for c in path) == text
    # the three words meet in one state behind their third letter, and there the lower class of D, R, P wins: the tie is broken where paths merge
    path, _ = pattern_best_from_lp(pattern_compile(r"(USD|EUR|GBP)\d{2}"), lp)
    assert "".join(itos[c] for c in path) == min(("USD", "EUR", "GBP"), key=lambda w: cls[w[2]]) + "00"


def test_no_finite_member_returns_one(built, itos):
    from tuatara_amd import engine
    lib = engine.load()
    pat = engine.pattern_compile(r"\d{2}/\d{2}")
    lp = table("random", 3)
    lp[2, LR.class_of(itos)["/"]] = -np.inf                    # every member passes the slash at position 2
    assert engine.pattern_best_from_lp(pat, lp) is None
    path, ln, logp = np.full(26, 7, np.int32), C.c_int32(5), C.c_float(1.0)
    rc = lib.ttr_pattern_best_from_lp(pat.h, lp.ctypes.data_as(C.POINTER(C.c_float)), path.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ln), C.byref(logp))
    assert rc == 1 and ln.value == -1 and np.isneginf(logp.value) and not path.any()
    lp[:] = np.nan
    assert engine.pattern_best_from_lp(pat, lp) is None


def test_the_trap(built, itos):
    """position 0 prefers E by 1e-3, positions 1 and 2 prefer S and D by 5: the greedy walk must write EUR, the likeliest member is USD.."""
    from tuatara_amd.engine import pattern_best_from_lp, pattern_compile
    cls = LR.class_of(itos)
    x = np.zeros((26, 95), np.float32)
    x[0, cls["E"]], x[0, cls["U"]] = 2.0 + 1e-3, 2.0
    x[1, cls["S"]], x[2, cls["D"]] = 5.0, 5.0
    x[3, cls["4"]], x[4, cls["2"]], x[5, 0] = 5.0, 5.0, 5.0
    lp = np.full((26, 96), -np.inf, np.float32)
    x64 = x.astype(np.float64)
    lp[:, :95] = (x64 - np.log(np.exp(x64).sum(1, keepdims=True))).astype(np.float32)
    pat = pattern_compile(r"(USD|EUR|GBP)\d+")
    ref = PR.compile_pattern(itos, r"(USD|EUR|GBP)\d+")
    greedy = "".join(itos[c] for c in BR.greedy32(lp, ref))
    path, logp = pattern_best_from_lp(pat, lp)
    best = "".join(itos[c] for c in path)
    assert greedy == "EUR42" and best == "USD42", (greedy, best)
    assert float(logp) > BR.score64(lp[:, :95].astype(np.float64), BR.greedy32(lp, ref)) + 9.0


def test_refusals_that_need_no_device(built):
    from tuatara_amd import engine
    lib = engine.load()
    assert lib.ttr_engine_set_pattern_decode(None, engine.PATTERN_BEST) == -1 and b"null argument" in lib.ttr_last_error()
    assert lib.ttr_engine_pattern_decode(None) == -1
    assert not lib.ttr_result_pattern_logp(None)
    assert lib.ttr_results_gather_pattern_logp(None, 0, None) == -1
    assert lib.ttr_logits_decode_patterns_best(None, None, 0, None, 0, None, None, 0, None, None, None, None, None) == -1
    assert lib.ttr_pattern_best_from_lp(None, None, None, None, None) == -1
    pat = engine.pattern_compile(r"\d+")
    assert lib.ttr_pattern_best_from_lp(pat.h, None, None, None, None) == -1
    with pytest.raises(ValueError, match=r"\[26, 96\]"):
        engine.pattern_best_from_lp(pat, np.zeros((26, 95), np.float32))
