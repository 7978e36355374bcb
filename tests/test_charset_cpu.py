"""Character sets (DESIGN.md "Character sets") without a GPU: the host mask rule against tests/charset_ref.py on the reference tokenizer's own id table,
its refusals, the exported symbols, the masked oracle's full-mask identity, and pytuatara's keywords as far as they go without a device."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from tests import charset_ref as CR
from tests.conftest import GOLDEN, ROOT

DIGITS = "0123456789"


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


@pytest.fixture(scope="module")
def itos():
    with open(os.path.join(GOLDEN, "g1_ref_tokenizer.json")) as f:
        return [chr(c) for c in json.load(f)["itos"]]


def _bits(m):
    return [c for c in range(96) if (int(m[c >> 5]) >> (c & 31)) & 1]


def test_symbols_are_exported(built):
    from tuatara_amd import engine
    lib = engine.load()
    for name in ("ttr_charset_mask", "ttr_engine_set_charset", "ttr_engine_get_charset", "ttr_logits_confidence_masked"):
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in engine.SYMBOLS), name


def test_mask_rule_against_the_reference_table(built, itos):
    from tuatara_amd.engine import charset_mask
    assert len(itos) == 98 and itos[0] == "]"
    assert _bits(charset_mask(DIGITS)) == list(range(11))                       # EOS + ids 1..10
    assert _bits(charset_mask("\\")) == [0, 69, 87]                             # the table holds the backslash twice
    assert _bits(charset_mask("]")) == [0, 88]                                  # id 88 decodes to nothing
    upper = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"
    lower = upper.lower()
    cases = [(DIGITS, None), ("\\", None), ("]", None), (upper, None), (None, lower), ("\\-.", None), (DIGITS + lower, "13579xyz"), (None, "|"),
             ("[", None), (DIGITS * 3, ""), ("", "0"), ("abc", "b")]
    for allow, deny in cases:
        got, want = charset_mask(allow, deny), CR.mask_rule(itos, allow, deny)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (allow, deny, _bits(got), _bits(want))
        assert got[0] & 1
    assert _bits(charset_mask(DIGITS + lower, "13579xyz")) == [0] + [i for i in range(1, 37) if itos[i] not in "13579xyz"]
    for allow, deny in ((None, None), ("", ""), (None, ""), ("", None)):      # NULL and empty mean all
        assert np.array_equal(charset_mask(allow, deny), CR.FULL), (allow, deny)
    assert _bits(CR.FULL) == list(range(95))
    # the count the C call returns: the character classes set
    lib = __import__("tuatara_amd.engine", fromlist=["load"]).load()
    m = (C.c_uint32 * 3)()
    assert lib.ttr_charset_mask(DIGITS.encode(), None, m) == 10
    assert lib.ttr_charset_mask(None, None, m) == 94
    assert lib.ttr_charset_mask(b"\\", b"", m) == 2


@pytest.mark.parametrize("allow,deny,quoted", [("12~", None, "'~'"), ("a b", None, "' '"), (None, "x\xc8", "'\\xc8'"), (None, "~", "'~'")])
def test_a_character_without_a_class_is_refused_by_name(built, itos, allow, deny, quoted):
    from tuatara_amd.engine import EngineError, charset_mask
    with pytest.raises(ValueError):
        CR.mask_rule(itos, allow, deny)
    with pytest.raises(EngineError) as ei:
        charset_mask(allow, deny)
    assert quoted in str(ei.value), str(ei.value)
    lib = __import__("tuatara_amd.engine", fromlist=["load"]).load()
    m = (C.c_uint32 * 3)(7, 7, 7)
    assert lib.ttr_charset_mask(allow.encode("latin1") if allow else None, deny.encode("latin1") if deny else None, m) == -1
    assert list(m) == [7, 7, 7]                                                 # a failed call writes nothing
    assert quoted.encode("latin1") in lib.ttr_last_error()


def test_a_set_emptied_by_deny_is_refused(built, itos):
    from tuatara_amd.engine import EngineError, charset_mask
    with pytest.raises(ValueError):
        CR.mask_rule(itos, "abc", "cba")
    with pytest.raises(EngineError):
        charset_mask("abc", "cba")
    with pytest.raises(EngineError):
        charset_mask("\\", "\\")


def test_masked_decode_reference_is_the_plain_decode_under_the_full_mask():
    x = np.random.default_rng(3).normal(0, 3, (5, 26, 95)).astype(np.float32)
    x[0, 0, [7, 3]] = 50.0                                                     # a tie: the first index wins
    ids, prob, conf = CR.masked_decode(x, CR.FULL)
    assert np.array_equal(ids, x.argmax(-1)) and ids[0, 0] == 3
    x64 = x.astype(np.float64)
    assert np.allclose(prob, 1.0 / np.exp(x64 - x64.max(-1, keepdims=True)).sum(-1), rtol=1e-12)
    m = CR.mask_rule([chr(c) for c in range(33, 33 + 98)], "\"#$")             # any table will do: ids 1, 2, 3
    ids, prob, _ = CR.masked_decode(x, m)
    assert set(np.unique(ids)) <= {0, 1, 2, 3}
    e = np.exp(x64[..., :4] - x64[..., :4].max(-1, keepdims=True))
    assert np.allclose(prob, 1.0 / e.sum(-1), rtol=1e-12)


def test_masked_forward_is_the_oracle_forward_under_the_full_mask(oracle_models):
    import torch
    _, parseq = oracle_models
    crops = CR.sweep_crops(11, 4)
    x = CR.crops_to_images(crops)
    with torch.no_grad():
        ref, ref_ar = parseq(x, return_ar=True)
    got, got_ar = CR.masked_forward(parseq, x, CR.FULL)
    assert got.numpy().tobytes() == ref.numpy().tobytes() and got_ar.numpy().tobytes() == ref_ar.numpy().tobytes()
    digits = CR.mask_rule([chr(c) for c in json.load(open(os.path.join(GOLDEN, "g1_ref_tokenizer.json")))["itos"]], DIGITS)
    con, con_ar = CR.masked_forward(parseq, x, digits)
    assert con_ar.numpy()[:, 0].tobytes() == ref_ar.numpy()[:, 0].tobytes()     # the first step has seen no choice yet
    assert not np.array_equal(con.numpy(), ref.numpy())                         # later ones have: the constraint is context


def test_pytuatara_keywords_without_a_gpu(built, capfd):
    sys.path.insert(0, os.path.join(ROOT, "build", "bindings"))
    import pytuatara
    img = np.zeros((8, 8, 3), np.uint8)
    for fn, first in ((pytuatara.image_to_data, img), (pytuatara.images_to_data, [img])):
        with pytest.raises(TypeError):
            fn(first, "w", "o", False, False, None, False, False, False, False, DIGITS)   # keyword-only
        with pytest.raises(ValueError, match="'~'"):                                      # refused before anything runs
            fn(first, "/nonexistent/weights", "o", allowlist="12~")
        with pytest.raises(ValueError, match="' '"):
            fn(first, "/nonexistent/weights", "o", blocklist=" ")
        assert fn(first, "", "o", allowlist=DIGITS, blocklist="7") == []                    # the reference's conventions still come first
        assert "Please provide a value for weights_dir" in capfd.readouterr().err
        assert fn(first, "/nonexistent/weights", "o", allowlist=DIGITS) == []
        assert "error loading" in capfd.readouterr().err
        assert fn(first, "/nonexistent/weights", "o", allowlist=None, blocklist=None) == []
        capfd.readouterr()
