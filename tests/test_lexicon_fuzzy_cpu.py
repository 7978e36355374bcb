"""Fuzzy alignment of lexicon entries (DESIGN.md "Lexicon matching", Fuzzy alignment) without a GPU: the exported symbols, the host rule
(ttr_lexicon_fuzzy_from_lp) bit for bit against the float32 restatement of tests/lexicon_fuzzy_ref.py and within the path bound of the float64 one, what
follows from the rule (band 0 is the rigid sum, logp never falls as the band grows), hand-made slips on a peaked table, the 25-character edge, and every
refusal of the host rule and of the setter on NULL."""
import ctypes as C

import numpy as np
import pytest

from tests import lexicon_fuzzy_ref as FR
from tests import lexicon_ref as LR

NEW_SYMBOLS = ("ttr_engine_set_lexicon_fuzzy", "ttr_engine_lexicon_fuzzy", "ttr_result_lex_band", "ttr_result_lex_edits", "ttr_result_lex_edits_all",
               "ttr_lexicon_fuzzy_from_lp", "ttr_logits_lexicon_fuzzy", "ttr_debug_lexicon_tables")
KINDS = ("normal", "peaked", "spread", "equal", "blocked", "nan")
GAPS = (0.0, -6.9077554, -50.0)
CLASSES = np.array([c for c in range(1, 95) if c != 88])


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


def test_symbols_exist(built):
    from tuatara_amd import engine as E
    lib = E.load()
    names = {s[0] for s in E.SYMBOLS}
    for s in NEW_SYMBOLS:
        assert s in names and getattr(lib, s) is not None, s


def logits_of(kind, rng, read=None):
    """one crop's logits f32 [26, 95]; peaked: 20 above the rest at the classes of `read` (the EOS behind them)"""
    x = (rng.standard_normal((26, 95)) * 3).astype(np.float32)
    if kind == "peaked":
        x = (rng.standard_normal((26, 95)) * 0.1).astype(np.float32)
        read = list(read if read is not None else rng.choice(CLASSES, size=int(rng.integers(1, 26))))
        for p in range(26):
            x[p, read[p] if p < len(read) else 0] += 20.0
    elif kind == "spread":
        x[rng.random((26, 95)) < 0.3] = np.float32(1e30)
        x[rng.random((26, 95)) < 0.3] = np.float32(-1e30)
    elif kind == "equal":
        x[:] = np.float32(1.25)
    return x


def table_of(kind, rng, read=None):
    """one table f32 [26, 96] the way the scorers form it, column 95 -inf"""
    x = logits_of(kind, rng, read)
    lp = np.full((26, 96), -np.inf, np.float32)
    with np.errstate(all="ignore"):
        d = x - x.max(axis=1, keepdims=True)
        prob = (np.float32(1.0) / np.exp(d).sum(axis=1, dtype=np.float32)).astype(np.float32)
        lp[:, :95] = d + np.log(prob)[:, None]
    if kind == "blocked":
        lp[:, rng.choice(np.arange(1, 95), size=30, replace=False)] = -np.inf
    if kind == "nan":
        lp[:, :95][rng.random((26, 95)) < 0.05] = np.nan
    return lp


def records_of(rng, n, lengths=()):
    rec = np.zeros((n, 32), np.uint8)
    for i in range(n):
        L = lengths[i] if i < len(lengths) else int(rng.integers(1, 26))
        rec[i, 0] = L
        rec[i, 1:1 + L] = rng.choice(CLASSES, size=L)
    return rec


def record(classes):
    rec = np.zeros(32, np.uint8)
    rec[0] = len(classes)
    rec[1:1 + len(classes)] = classes
    return rec


def same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


def test_host_rule_is_the_float32_restatement_bit_for_bit(built):
    from tuatara_amd.engine import lexicon_fuzzy_from_lp
    rng = np.random.default_rng(20260501)
    pairs = 0
    for kind in KINDS:
        for band in range(4):
            for gap in GAPS:
                lp = table_of(kind, rng)
                rec = records_of(rng, 30, lengths=(1, 25, 24, 2))
                logp, edits = lexicon_fuzzy_from_lp(lp, rec, band, gap)
                want_s, want_e = FR.scores32(lp, rec, band, gap)
                assert not np.isnan(logp).any(), (kind, band, gap)                                # a NaN is never taken up
                assert same_bits(logp, want_s), (kind, band, gap, logp, want_s)
                assert np.array_equal(edits, want_e), (kind, band, gap, edits, want_e)
                pairs += len(rec)
    assert pairs >= 2000


@pytest.mark.parametrize("kind", ["normal", "peaked"])
def test_host_rule_against_float64(built, kind):
    from tuatara_amd.engine import lexicon_fuzzy_from_lp
    rng = np.random.default_rng(7 + len(kind))
    for band in range(4):
        for gap in GAPS:
            x = logits_of(kind, rng)
            lp64, mag = LR.tables(x[None])
            lp = np.full((26, 96), -np.inf, np.float32)
            lp[:, :95] = lp64[0].astype(np.float32)
            rec = records_of(rng, 20, lengths=(1, 25))
            logp, _ = lexicon_fuzzy_from_lp(lp, rec, band, gap)
            s64, _, tol = FR.scores64(lp64[0], mag[0], rec, band, gap)
            assert np.isfinite(s64).all()
            err = np.abs(logp.astype(np.float64) - s64)
            assert (err <= tol).all(), (kind, band, gap, float(err.max()), float(tol.min()))


def test_band_zero_is_the_rigid_sum_and_logp_never_falls_with_the_band(built):
    from tuatara_amd.engine import lexicon_fuzzy_from_lp
    rng = np.random.default_rng(11)
    for kind in KINDS:
        for gap in GAPS:
            lp = table_of(kind, rng)
            rec = records_of(rng, 25, lengths=(1, 25))
            by_band = [lexicon_fuzzy_from_lp(lp, rec, b, gap) for b in range(4)]
            rigid = np.array([FR.rigid32(lp, r) for r in rec], np.float32)
            rigid[np.isnan(rigid)] = -np.inf                                                     # the rule never takes a NaN up: such a word scores -inf
            assert same_bits(by_band[0][0], rigid), (kind, gap)
            assert (by_band[0][1] == 0).all()
            for b in range(3):
                assert (by_band[b + 1][0] >= by_band[b][0]).all(), (kind, gap, b)


def test_hand_made_slips_on_a_peaked_table(built):
    from tuatara_amd.engine import lexicon_fuzzy_from_lp
    rng = np.random.default_rng(3)
    gap = float(FR.GAP)
    word = [int(c) for c in rng.choice(CLASSES, size=14, replace=False)]
    other = [int(c) for c in CLASSES if c not in word]
    lp = table_of("peaked", rng, read=word)
    x, y = other[0], other[1]
    cases = {
        "itself": (word, 0),
        "inserted at the front": ([x] + word, 1),
        "inserted in the middle": (word[:7] + [x] + word[7:], 1),
        "inserted at the end": (word + [x], 1),
        "removed": (word[:5] + word[6:], 1),
    }
    rec = np.stack([record(c) for c, _ in cases.values()])
    logp, edits = lexicon_fuzzy_from_lp(lp, rec, 1, gap)
    own = float(logp[0])
    assert -0.01 < own < 0.0 and edits[0] == 0
    for k, (name, (_, e)) in enumerate(cases.items()):
        assert edits[k] == e, (name, edits[k])
        assert abs(float(logp[k]) - (own + e * gap)) <= 1e-3, (name, float(logp[k]), own)
    rigid, _ = lexicon_fuzzy_from_lp(lp, rec, 0, gap)
    assert (rigid[1:4] < -100).any() and float(rigid[4]) < -100                                    # what the rigid rule makes of the same entries
    # one character inserted and another removed further on: no alignment with fewer than two edits comes near
    two = record(word[:3] + [y] + word[3:9] + word[10:])
    s2, e2 = lexicon_fuzzy_from_lp(lp, two[None], 1, gap)
    assert s2[0] == -np.inf or e2[0] >= 2, (s2, e2)
    assert abs(float(s2[0]) - (own + 2 * gap)) <= 1e-3


def test_twenty_five_characters_and_the_last_position(built):
    from tuatara_amd.engine import lexicon_fuzzy_from_lp
    rng = np.random.default_rng(5)
    gap = float(FR.GAP)
    word = [int(c) for c in rng.choice(CLASSES, size=25, replace=False)]
    lp25 = table_of("peaked", rng, read=word)                    # read as 25 characters: the EOS at position 25, the table's last row
    lp24 = table_of("peaked", rng, read=word[:12] + word[13:])   # read as 24: character 12 was dropped
    rec = record(word)[None]
    for band in range(4):
        s, e = lexicon_fuzzy_from_lp(lp25, rec, band, gap)
        ws, we = FR.scores32(lp25, rec, band, gap)
        assert same_bits(s, ws) and e[0] == we[0] == 0 and -0.01 < float(s[0]) < 0.0, (band, s, e)
        s, e = lexicon_fuzzy_from_lp(lp24, rec, band, gap)
        ws, we = FR.scores32(lp24, rec, band, gap)
        assert same_bits(s, ws) and e[0] == we[0], (band, s, e)
        if band >= 1:
            assert e[0] == 1 and abs(float(s[0]) - gap) <= 1e-2, (band, s, e)
        else:
            assert float(s[0]) < -100


def test_refusals(built):
    from tuatara_amd import engine as E
    lib = E.load()
    lp = np.zeros((26, 96), np.float32)
    rec = record([11, 12, 13])[None].copy()
    logp, edits = np.zeros(1, np.float32), np.zeros(1, np.int32)
    call = lambda lp_, rec_, n, band, gap, a, b: lib.ttr_lexicon_fuzzy_from_lp(lp_, rec_, n, band, C.c_float(gap), a, b)
    ok = (E._f(lp), E._u8(rec), 1, 1, -1.0, E._f(logp), E._i(edits))
    assert call(*ok) == 0
    for k in (0, 1, 5, 6):                                        # each null argument
        bad = list(ok)
        bad[k] = None
        assert call(*bad) == -1, k
    for band in (-1, 4, 100):
        assert call(ok[0], ok[1], 1, band, -1.0, ok[5], ok[6]) == -1, band
    for gap in (1e-6, 1.0, float("inf"), float("-inf"), float("nan")):
        assert call(ok[0], ok[1], 1, 1, gap, ok[5], ok[6]) == -1, gap
    assert call(ok[0], ok[1], 1, 1, 0.0, ok[5], ok[6]) == 0 and call(ok[0], ok[1], 1, 1, -0.0, ok[5], ok[6]) == 0
    for length in (0, 26, 255):
        r2 = rec.copy()
        r2[0, 0] = length
        assert call(ok[0], E._u8(r2), 1, 1, -1.0, ok[5], ok[6]) == -1, length
    with pytest.raises(E.EngineError):
        E.lexicon_fuzzy_from_lp(lp, rec, 4)
    # the setter and the accessors on NULL
    assert lib.ttr_engine_set_lexicon_fuzzy(None, 1, C.c_float(-1.0)) == -1
    b, g = C.c_int(7), C.c_float(7.0)
    assert lib.ttr_engine_lexicon_fuzzy(None, C.byref(b), C.byref(g)) == -1 and b.value == 7
    assert lib.ttr_result_lex_band(None) == -1
    assert not lib.ttr_result_lex_edits(None, 0) and not lib.ttr_result_lex_edits_all(None)
    assert lib.ttr_logits_lexicon_fuzzy(None, None, 0, None, 0, None, 1, C.c_float(-1.0), None, None, None) == -1
    assert lib.ttr_debug_lexicon_tables(None, None, 0, None, 0, None, None) == -1
