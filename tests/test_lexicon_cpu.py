"""Lexicon matching (DESIGN.md "Lexicon matching") without a GPU: the exported symbols, ttr_lexicon_encode against the restatement of tests/lexicon_ref.py
and each of its refusals with the offending index in the message, and the setter's and the accessors' behaviour on NULL."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import lexicon_ref as LR
from tests.conftest import GOLDEN

NEW_SYMBOLS = ("ttr_engine_set_lexicon", "ttr_engine_lexicon_size", "ttr_engine_lexicon_m", "ttr_engine_lexicon_word", "ttr_result_lex_m",
               "ttr_result_lex_idx", "ttr_result_lex_logp", "ttr_result_lex_idx_all", "ttr_result_lex_logp_all", "ttr_lexicon_encode", "ttr_logits_lexicon")


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


@pytest.fixture(scope="module")
def itos():
    with open(os.path.join(GOLDEN, "g1_ref_tokenizer.json")) as f:
        return [chr(c) for c in json.load(f)["itos"]]


def test_symbols_exist(built):
    from tuatara_amd import engine as E
    lib = E.load()
    names = {s[0] for s in E.SYMBOLS}
    for s in NEW_SYMBOLS:
        assert s in names and getattr(lib, s) is not None, s


def test_encode_matches_the_restatement(built, itos):
    from tuatara_amd.engine import lexicon_encode
    chars = sorted(LR.class_of(itos))
    assert len(chars) == 91 and "\\" not in chars and "]" not in chars and " " not in chars      # 93 classes, less the two the backslash names
    rng = np.random.default_rng(3)
    words = ["7", "".join(rng.choice(chars, 25)), "Invoice", "".join(chars[:25]), "".join(chars[25:50]), "".join(chars[50:75]), "".join(chars[75:])]
    assert {len(w) for w in words} >= {1, 25}
    got = lexicon_encode(words)
    want = LR.encode(words, itos)
    assert got.dtype == np.uint8 and got.shape == (len(words), 32) and np.array_equal(got, want)
    assert (got[:, 26:] == 0).all() and got[0].tolist() == [1, 8] + [0] * 30                        # '7' is class 8; zeros behind the word
    assert lexicon_encode([w.encode() for w in words]).tobytes() == got.tobytes()                  # bytes and str alike
    assert np.array_equal(lexicon_encode(["a", "a"]), LR.encode(["a", "a"], itos))                  # duplicates are allowed


@pytest.mark.parametrize("words,index,what", [
    (["ok", ""], 1, "empty"),
    (["ok", "fine", "x" * 26], 2, "longer than 25"),
    (["a]b"], 0, "']'"),
    (["ab", "c d"], 1, "' '"),
    (["ab", "cd", b"caf\xe9"], 2, "\\xe9"),
    (["\\"], 0, "two recogniser classes"),
    (["good", "tab\there"], 1, "\\x09"),
    (["ab", "\u0141\u00f3d\u017a"], 1, "names no recogniser class"),       # a str outside latin-1: never a '?' in its place
    (["ab", "cd", "caf\u00e9"], 2, "\\xe9"),                                # a str inside latin-1, outside ASCII
    (["ab", "x\u4e2d"], 1, "names no recogniser class"),
    (["ab", "cd\x00ef"], 1, "\\x00"),                                      # a NUL would cut the word short on the way
    (["ab", b"cd\x00ef"], 1, "\\x00"),
    (["\udc80"], 0, "cannot be encoded"),
])
def test_encode_refuses_and_names_the_word(built, words, index, what):
    from tuatara_amd.engine import EngineError, lexicon_encode
    with pytest.raises(EngineError) as ex:
        lexicon_encode(words)
    assert f"word {index} " in str(ex.value) and what in str(ex.value), str(ex.value)


def test_a_question_mark_is_only_ever_the_callers(built, itos):
    from tuatara_amd.engine import lexicon_encode
    q = LR.class_of(itos)["?"]
    assert lexicon_encode(["a?b"])[0, :5].tolist() == [3, 11, q, 12, 0]


def test_result_accessors_check_the_item_index(built):
    from tuatara_amd import engine as E
    lib = E.load()
    for i in (-1, 0, 1 << 30):
        assert not lib.ttr_result_lex_idx(None, i) and not lib.ttr_result_lex_logp(None, i)


def test_encode_refuses_bad_counts_and_null(built):
    from tuatara_amd import engine as E
    lib = E.load()
    rec = np.zeros((4, 32), np.uint8)
    one = (C.c_char_p * 1)(b"a")
    assert lib.ttr_lexicon_encode(one, 0, E._u8(rec)) == -1 and "1..1048576" in lib.ttr_last_error().decode()
    assert lib.ttr_lexicon_encode(one, (1 << 20) + 1, E._u8(rec)) == -1 and "1..1048576" in lib.ttr_last_error().decode()      # (refused before a word is read)
    assert lib.ttr_lexicon_encode(one, -1, E._u8(rec)) == -1
    assert lib.ttr_lexicon_encode(None, 1, E._u8(rec)) == -1 and "null" in lib.ttr_last_error().decode()
    assert lib.ttr_lexicon_encode(one, 1, None) == -1 and "null" in lib.ttr_last_error().decode()
    null_word = (C.c_char_p * 2)(b"a", None)
    assert lib.ttr_lexicon_encode(null_word, 2, E._u8(rec)) == -1 and "word 1 is null" in lib.ttr_last_error().decode()
    assert not rec[2:].any()                                                                        # nothing past the words given is written
    assert lib.ttr_lexicon_encode(one, 1, E._u8(rec)) == 0 and rec[0, :2].tolist() == [1, 11]      # 'a' is class 11


def test_setter_and_accessors_on_null(built):
    from tuatara_amd import engine as E
    lib = E.load()
    one = (C.c_char_p * 1)(b"a")
    assert lib.ttr_engine_set_lexicon(None, one, 1, 1) == -1 and "null" in lib.ttr_last_error().decode()
    assert lib.ttr_engine_set_lexicon(None, None, 0, 0) == -1
    assert lib.ttr_engine_lexicon_size(None) == 0 and lib.ttr_engine_lexicon_m(None) == 0
    assert lib.ttr_engine_lexicon_word(None, 0) is None
    assert lib.ttr_result_lex_m(None) == 0
    assert not lib.ttr_result_lex_idx(None, 0) and not lib.ttr_result_lex_logp(None, 0)
    assert not lib.ttr_result_lex_idx_all(None) and not lib.ttr_result_lex_logp_all(None)
    idx, logp = np.zeros(1, np.int32), np.zeros(1, np.float32)
    x = np.zeros((1, 26, 95), np.float32)
    assert lib.ttr_logits_lexicon(None, E._f(x), 1, None, 0, None, E._i(idx), E._f(logp)) == -1 and "null" in lib.ttr_last_error().decode()


def test_the_restatement_ranks_by_score_then_index():
    s = np.array([-3.0, -1.0, -np.inf, -1.0, -2.0])
    assert LR.rank(s, 8).tolist() == [1, 3, 4, 0] and LR.rank(s, 2).tolist() == [1, 3]
