"""Character alternatives (DESIGN.md "Character alternatives") without a GPU: the host n-best rule (ttr_nbest_from_alts) against the brute-force
restatement of tests/alts_ref.py - texts and rank order identical, scores bit for bit -, its walk's bound, reading 0 against the confidence rule, its
refusals, the exported symbols, and the setter's refusals that need no device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import alts_ref as AR
from tests.conftest import GOLDEN

NEW_SYMBOLS = ("ttr_engine_set_alternatives", "ttr_engine_alternatives", "ttr_result_alt_k", "ttr_result_alt_ids", "ttr_result_alt_probs",
               "ttr_result_alt_ids_all", "ttr_result_alt_probs_all", "ttr_results_gather_alts", "ttr_logits_alternatives", "ttr_nbest_from_alts")


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


@pytest.fixture(scope="module")
def itos():
    with open(os.path.join(GOLDEN, "g1_ref_tokenizer.json")) as f:
        return [chr(c) for c in json.load(f)["itos"]]


def _table(k, rows, fill_id=0, fill_prob=1.0):
    """rows: per position a list of (id, prob) of at most k slots; the other slots hold -1 / 0, the positions behind them (fill_id, fill_prob) in slot 0"""
    ids = np.full((26, k), -1, np.int32)
    pr = np.zeros((26, k), np.float32)
    ids[:, 0], pr[:, 0] = fill_id, fill_prob
    for p, row in enumerate(rows):
        ids[p], pr[p] = -1, 0.0
        for j, (c, v) in enumerate(row):
            ids[p, j], pr[p, j] = c, v
    return ids, pr


def _random_word(rng, k, length, eos=True):
    """a word of `length` characters: descending probabilities, with -1, the EOS and id 88 sprinkled among the alternatives"""
    rows = []
    for _ in range(length):
        chars = rng.choice([c for c in range(1, 95) if c != 88], k, replace=False)
        p = np.sort(rng.dirichlet(np.ones(k) * 0.6))[::-1].astype(np.float32)
        row = [(int(chars[j]), float(p[j])) for j in range(k)]
        for j in range(1, k):
            u = rng.random()
            if u < 0.15:
                row[j] = (0, row[j][1])          # the EOS among the alternatives: not an option
            elif u < 0.25:
                row[j] = (88, row[j][1])         # id 88: decodes to nothing, not an option
            elif u < 0.35:
                row[j] = (-1, 0.0)               # an empty slot
        rows.append(row)
    if eos:
        rows.append([(0, 0.93), (5, 0.04)][:k])
    return _table(k, rows) if eos else _table(k, rows, fill_id=88, fill_prob=0.5)


def _same(got, want):
    assert [t for t, _ in got] == [t for t, _, _ in want]
    assert [np.float32(s).tobytes() for _, s in got] == [np.float32(s).tobytes() for _, s, _ in want], (got, want)


@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("m", [1, 5, 64])
def test_nbest_equals_the_brute_force_restatement(built, itos, k, m):
    from tuatara_amd.engine import nbest_from_alts
    rng = np.random.default_rng(100 * k + m)
    words = [_random_word(rng, k, length) for length in (1, 2, 3, 4)]
    words.append(_random_word(rng, k, 3, eos=False))                                    # no EOS: all 26 positions are looked at, id 88 fills them
    # exact ties in score: equal probabilities in two positions (the rank tuple decides), and a tie between a position's own options (the slot decides)
    words.append(_table(k, [[(11, 0.5), (12, 0.25)], [(13, 0.5), (14, 0.25)], [(15, 0.5), (16, 0.5)][:k], [(0, 1.0)]]))
    words.append(_table(k, [[(0, 0.75), (7, 0.2)]]))                                    # the empty word: EOS at position 0
    words.append(_table(k, [[(88, 0.5), (7, 0.3)], [(20, 0.625), (88, 0.25)], [(0, 0.5)]]))   # an id 88 on top: that position is no character
    for ids, pr in words:
        want = AR.nbest_brute(ids, pr, m, itos)
        _same(nbest_from_alts(ids, pr, m), want)
        walk, _ = AR.nbest_walk(ids, pr, m, itos)
        assert walk == want                                                             # the restatement's two forms agree
    got = nbest_from_alts(*words[-2], m)
    assert got == [("", np.float32(0.75))]                                              # one reading, "", with score alt_prob[0][0]


def test_the_ties_are_ordered_by_rank_tuple(built, itos):
    from tuatara_amd.engine import nbest_from_alts
    ids, pr = _table(3, [[(11, 0.5), (12, 0.25)], [(13, 0.5), (14, 0.25)], [(0, 1.0)]])
    got = nbest_from_alts(ids, pr, 64)
    a, b, c, d = itos[11], itos[12], itos[13], itos[14]
    assert got == [(a + c, np.float32(0.25)), (a + d, np.float32(0.125)), (b + c, np.float32(0.125)), (b + d, np.float32(0.0625))]   # (0, 1) before (1, 0)


def test_a_word_of_25_characters_is_a_bounded_walk(built, itos):
    from tuatara_amd.engine import nbest_from_alts
    rng = np.random.default_rng(7)
    ids, pr = _random_word(rng, 8, 25)
    want, pushed = AR.nbest_walk(ids, pr, 64, itos)                                     # (8^25 tuples: no brute force here)
    assert len(want) == 64 and pushed <= 64 * 25 + 1
    _same(nbest_from_alts(ids, pr, 64), want)
    assert len(want[0][0]) == 25
    scores = [float(s) for _, s, _ in want]
    assert scores == sorted(scores, reverse=True)


@pytest.mark.parametrize("k", [2, 3, 8])
def test_reading_zero_is_text_and_conf(built, itos, k):
    from tuatara_amd.engine import confidence_from_probs, decode_ids, nbest_from_alts
    rng = np.random.default_rng(k)
    for length, eos in ((1, True), (6, True), (25, True), (4, False), (0, True)):
        ids, pr = _random_word(rng, k, length, eos)
        for p in range(26):                                                            # every slot 0 on top of its row, as the kernel leaves it
            pr[p, 0] = max(pr[p, 0], pr[p].max())
        text, score = nbest_from_alts(ids, pr, 1)[0]
        cc, conf = confidence_from_probs(ids[:, 0], pr[:, 0])
        assert text == decode_ids(ids[:, 0]) and len(cc) == len(text) == length
        assert np.float32(score).tobytes() == np.float32(conf).tobytes()


def test_char_alternatives_follow_the_restatement(built, itos):
    from tuatara_amd.engine import char_alternatives
    rng = np.random.default_rng(3)
    for k in (2, 5, 8):
        ids, pr = _random_word(rng, k, 7)
        assert char_alternatives(ids, pr) == AR.char_options(ids, pr, itos)


def test_bad_arguments_return_minus_one_with_a_message(built):
    from tuatara_amd import engine
    lib = engine.load()
    ids, pr = _table(3, [[(5, 0.5)], [(0, 1.0)]])
    pi, pf = ids.ctypes.data_as(C.POINTER(C.c_int32)), pr.ctypes.data_as(C.POINTER(C.c_float))
    need = C.c_size_t()
    for args, word in (((None, pf, 3, 1), b"null"), ((pi, None, 3, 1), b"null"), ((pi, pf, 1, 1), b"k must"), ((pi, pf, 9, 1), b"k must"),
                       ((pi, pf, 3, 0), b"m must"), ((pi, pf, 3, 65), b"m must")):
        assert lib.ttr_nbest_from_alts(*args, None, 0, None, C.byref(need)) == -1, args
        assert word in lib.ttr_last_error(), (args, lib.ttr_last_error())
    # a buffer that is too small is not written; the count and the need still come back
    buf = C.create_string_buffer(b"\xff" * 8, 8)
    assert lib.ttr_nbest_from_alts(pi, pf, 3, 4, buf, 1, None, C.byref(need)) == 1 and need.value == 2
    assert buf.raw == b"\xff" * 8
    assert lib.ttr_nbest_from_alts(pi, pf, 3, 4, buf, 8, None, None) == 1 and buf.raw[:2] == engine.decode_ids([5]).encode() + b"\n"
    with pytest.raises(engine.EngineError):
        engine.nbest_from_alts(ids, pr, 0)
    with pytest.raises(ValueError):
        engine.nbest_from_alts(ids[:25], pr[:25], 1)


def test_symbols_are_exported_and_bound(built):
    from tuatara_amd import engine
    raw = C.CDLL(engine.lib_path())
    bound = {n for n, _, _ in engine.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in bound, name
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "tuatara_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name


def test_setter_refusals_that_need_no_device(built):
    from tuatara_amd import engine
    lib = engine.load()
    assert lib.ttr_engine_set_alternatives(None, 3) == -1 and b"null" in lib.ttr_last_error()
    assert lib.ttr_engine_alternatives(None) == 0
    assert lib.ttr_result_alt_k(None) == 0
    assert not lib.ttr_result_alt_ids_all(None) and not lib.ttr_result_alt_probs_all(None)
    assert lib.ttr_results_gather_alts(None, 0, None, None) == -1
    assert lib.ttr_logits_alternatives(None, None, 0, 3, None, 0, None, None, None) == -1 and b"null" in lib.ttr_last_error()
