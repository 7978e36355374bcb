"""-m gpu: the recogniser held to the CPU oracle on words longer than ten characters.

Every other recogniser parity test reads crops through the seed-0 synthetic PARSeq, whose designed strings end within ten characters: AR steps 11 .. 25 (the
self-attention kernel's mode 0 at qi0 >= 11, the skinny token prologue at tok_col >= 11, pos_queries rows >= 11), refinement rows that see more than 11 keys, a
crop with no EOS at all (the reference keeps all 26 characters: the loop at tuatara.cpp:497-502 never breaks), the AR loop running to its natural end (the done
counter never reaching N, the host's looks at it finding "not done", the pending argmax consumed at the last step, per-crop exits beside crops that decode
on for 15 more steps) and what sits behind the logits on 25- and 26-position readings were compared with nothing.  Here the same network is built with
max_len = 30 (tuatara_amd/weights.py: dfa_tables): on 128 noise crops the first EOS falls in every column 0 .. 25 and 17 crops have none.

The conditions that keep these tests from being vacuous (tests/parity_rules.py: long_word_lengths) are asserted wherever the oracle's logits are taken."""
import json
import os

import numpy as np
import pytest

from tests import parity_rules as R
from tests.conftest import GOLDEN
from tests.test_gpu_x4_parity import TOL, _assert_logits

pytestmark = pytest.mark.gpu

KNOBS = (("ar_early_exit", (0, 1), 1), ("ar_crop_exit", (0, 1), 1), ("ar_host_check", (0, 10), 10), ("argmax_fold", (0, 1), 1), ("embed_fold", (0, 1), 1),
         ("skx_ln_fuse", (0, 1), 1))                       # (key, the values compared with the default run, the default)


@pytest.fixture(scope="module")
def long(tmp_path_factory):
    """the long-word model: its .ttrw files, an f16x4 engine on them, the oracle from the same state dicts, the 128 noise crops"""
    from oracle import pipeline
    from tuatara_amd import weights as W
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine
    build_lib()
    d = str(tmp_path_factory.mktemp("weights_long"))
    c, p = W.make_synthetic_weights(d, seed=0, structured=True, max_len=30)
    eng = Engine(d, "f16x4")
    yield {"dir": d, "eng": eng, "parseq": pipeline.load_models(c, p)[1], "crops": R.long_word_crops()}
    eng.close()


@pytest.fixture(scope="module")
def got128(long):
    """the engine on the 128 crops, all 26 AR steps (want_ar): (refined, AR, ids), once for the tests that read it"""
    got, got_ar, ids = long["eng"].parseq_logits(long["crops"], want_ar=True)
    return got, got_ar, np.asarray(ids).reshape(-1, 26)


def _oracle(long, n=128):
    """the fp32 oracle on the first n crops (memoised across the tests), behind the non-vacuity conditions on the whole batch"""
    ref, ref_ar = R.oracle_logits(long["parseq"], long["crops"])
    R.long_word_lengths(ref)
    return ref[:n], ref_ar[:n]


def _budget(got, got_ar, ref32, ar32, r64, a64, min_same, label):
    """tests/test_gpu_x4_parity.py: test_x4_error_budget_against_fp64_parseq's rule - |engine - fp64| <= 1.5 x |fp32 oracle - fp64| in the maximum and at the
    99.99th percentile, on the refined logits (all 26 positions) and on the AR logits up to EOS, over the crops whose fp32 greedy path is the fp64 one."""
    up = R.upto_eos(r64.argmax(-1))
    pos = np.arange(26)[None, :]
    mask = pos < up[:, None]
    same = ((ar32.argmax(-1) == a64.argmax(-1)) | ~mask).all(1) & (ref32.argmax(-1) == r64.argmax(-1)).all(1)
    print(f"{label}: {int(same.sum())} of {len(same)} crops follow the fp64 greedy path in fp32")
    assert same.sum() >= min_same
    e_eng, e_f32 = np.abs(got.astype(np.float64) - r64)[same], np.abs(ref32.astype(np.float64) - r64)[same]
    e_eng_ar, e_f32_ar = np.abs(got_ar.astype(np.float64) - a64)[same][mask[same]], np.abs(ar32.astype(np.float64) - a64)[same][mask[same]]
    late = (mask & (pos >= 11))[same]                       # positions >= 11 up to EOS: a figure of their own
    for name, a, b in (("refined, positions >= 11 up to EOS", e_eng[late], e_f32[late]),
                       ("AR, steps >= 11 up to EOS", np.abs(got_ar.astype(np.float64) - a64)[same][late], np.abs(ar32.astype(np.float64) - a64)[same][late])):
        print(f"{label}: {name} ({int(late.sum())} positions): |engine - fp64| max {a.max():.2e} p99.99 {np.percentile(a, 99.99):.2e} mean {a.mean():.2e}   |fp32 oracle - fp64| max {b.max():.2e} "
              f"p99.99 {np.percentile(b, 99.99):.2e} mean {b.mean():.2e}")
    for name, a, b in (("refined, all 26 positions", e_eng, e_f32), ("AR up to EOS", e_eng_ar, e_f32_ar)):
        print(f"{label}: {name}: |engine - fp64| max {a.max():.2e} p99.99 {np.percentile(a, 99.99):.2e} mean {a.mean():.2e}   |fp32 oracle - fp64| max {b.max():.2e} "
              f"p99.99 {np.percentile(b, 99.99):.2e} mean {b.mean():.2e}   ratio max {a.max() / b.max():.2f} p99.99 {np.percentile(a, 99.99) / np.percentile(b, 99.99):.2f}")
        assert a.max() <= 1.5 * b.max(), (label, name, a.max(), b.max())
        assert np.percentile(a, 99.99) <= 1.5 * np.percentile(b, 99.99), (label, name, np.percentile(a, 99.99), np.percentile(b, 99.99))
    return same


def test_long_words_against_the_fp32_oracle(long, got128):
    """128 crops, all 26 AR steps: tests/test_gpu_x4_parity.py's rules unchanged - refined logits within 1e-3 at all 26 positions, AR logits up to and including
    the first EOS (for a crop without one: every step), ids and strings identical."""
    ref, ref_ar = _oracle(long)
    got, got_ar, ids = got128
    up = R.upto_eos(ref.argmax(-1))
    late = (np.arange(26)[None, :] < up[:, None]) & (np.arange(26)[None, :] >= 11)
    print(f"long words, f16x4 vs oracle: positions >= 11 up to EOS: max |dlogit| refined {np.abs(got - ref)[late].max():.2e}, AR {np.abs(got_ar - ref_ar)[late].max():.2e}; "
          f"logits >= {TOL}: {int((np.abs(got - ref) >= TOL).sum())} refined, {int((np.abs(got_ar - ref_ar)[np.arange(26)[None, :] < up[:, None]] >= TOL).sum())} AR up to EOS")
    assert int((np.abs(got_ar).max((0, 2)) > 0).sum()) == 26           # a crop with no EOS keeps the loop running to its last step
    _assert_logits(ref, ref_ar, got, got_ar, ids, "long words: f16x4, 128 crops vs oracle")


def test_long_words_error_budget_against_fp64(long, got128):
    """The engine's error against a float64 evaluation (tests/parity_rules.py: oracle_logits_fp64, the math attention path) stays within 1.5 x the fp32 oracle's
    own, in the maximum and at p99.99, on the refined logits and on the AR logits up to EOS - 26 steps for a crop that never ends."""
    ref32, ar32 = _oracle(long)
    r64, a64 = R.oracle_logits_fp64(long["parseq"], long["crops"])
    got, got_ar, ids = got128
    same = _budget(got, got_ar, ref32, ar32, r64, a64, 120, "long words, f16x4")
    assert np.array_equal(ids[same], r64.argmax(-1)[same])


def test_long_words_f32_engine(long):
    """The fp32-MFMA engine on the first 32 crops (8 of them never end): the same rules."""
    from tuatara_amd.engine import Engine
    ref, ref_ar = _oracle(long, 32)
    assert (~(ref.argmax(-1) == 0).any(1)).sum() >= 4 and (R.upto_eos(ref.argmax(-1)) == 26).sum() >= 5
    crops = long["crops"][:32]
    eng = Engine(long["dir"], "f32")
    try:
        got, got_ar, ids = eng.parseq_logits(crops, want_ar=True)
    finally:
        eng.close()
    _assert_logits(ref, ref_ar, got, got_ar, ids, "long words: f32 engine, 32 crops vs oracle")
    r64, a64 = R.oracle_logits_fp64(long["parseq"], long["crops"])
    _budget(got, got_ar, ref, ref_ar, r64[:32], a64[:32], 30, "long words, f32 engine")     # (30 of 32: the 128-crop cap's share)


@pytest.mark.parametrize("n", [52, 300])
def test_the_ar_loops_forms_are_bit_identical_on_crops_that_never_end(long, n):
    """One knob at a time against the default: the batch-level exit, the per-crop exit, the host's look at the done counter, the folded argmax, the folded
    embedding, the fused LayerNorm prologue - on a batch where some crops end at step 1 (stale rows beside crops that keep decoding) and some never end (the
    counter never reaches N, every host check finds "not done", the pending argmax is consumed at the last step).  52 crops run the <= 256-crop path (token
    prologue, host checks); 300 leave it.  Refined logits and ids bit for bit, AR logits bit for bit up to each crop's EOS.  Engine against engine: no oracle."""
    eng = long["eng"]
    if n == 52:
        crops = long["crops"][76:128]
    else:
        crops = np.concatenate([long["crops"]] * 3)[:300].copy()
        crops[:, 31, 127, 2] ^= (1 + np.arange(300) // 128).astype(np.uint8)          # one byte per crop: the three copies differ
    base, base_ar, base_ids = eng.parseq_logits(crops, want_ar=True)
    up = R.upto_eos(base_ar.argmax(-1))
    mask = np.arange(26)[None, :] < up[:, None]
    never = ~(base_ar.argmax(-1) == 0).any(1)
    print(f"{n} crops: {int((up == 1).sum())} end at step 1, {int(never.sum())} never end; AR steps run {int((np.abs(base_ar).max((0, 2)) > 0).sum())}")
    assert (up == 1).sum() >= 1 and never.sum() >= 5 and np.isfinite(base).all()
    assert int((np.abs(base_ar).max((0, 2)) > 0).sum()) == 26
    try:
        for key, values, default in KNOBS:
            for v in values:
                assert eng.set_tuning(key, v) == 0, key
                try:
                    b, b_ar, b_ids = eng.parseq_logits(crops, want_ar=True)
                finally:
                    eng.set_tuning(key, default)
                assert np.array_equal(base, b) and np.array_equal(base_ids, b_ids), (n, key, v, float(np.abs(base - b).max()))
                assert np.array_equal(base_ar[mask], b_ar[mask]), (n, key, v)
    finally:
        for key, _, default in KNOBS:
            eng.set_tuning(key, default)


def test_a_crop_that_never_ends_and_an_empty_string_do_not_see_their_batch(long, got128):
    """Batch invariance at the two ends: a crop with no EOS and a crop that reads "" - each alone and inside a batch of 9 - bit-exact (the sizes of
    tests/test_gpu_x4_parity.py's batch-invariance test: one kernel family; a batch of 128 runs other tiles and agrees to the last bits only)."""
    eng = long["eng"]
    ids128 = got128[2]
    never, empty = int(np.nonzero(~(ids128 == 0).any(1))[0][0]), int(np.nonzero(ids128[:, 0] == 0)[0][0])
    pick = [never, empty] + [i for i in range(128) if i not in (never, empty)][:7]
    nine, nine_ar, nine_ids = eng.parseq_logits(long["crops"][pick], want_ar=True)
    assert not (np.asarray(nine_ids).reshape(9, 26)[0] == 0).any() and np.asarray(nine_ids).reshape(9, 26)[1, 0] == 0
    for k in (0, 1):
        one, one_ar, one_ids = eng.parseq_logits(long["crops"][pick[k]:pick[k] + 1], want_ar=True)
        up = int(R.upto_eos(one_ar.argmax(-1))[0])
        assert np.array_equal(one[0], nine[k]) and np.array_equal(np.asarray(one_ids).ravel(), np.asarray(nine_ids).reshape(9, 26)[k]), k
        assert np.array_equal(one_ar[0, :up], nine_ar[k, :up]), k


# ------------------------------------------------------------------------------------------------- behind the logits
def _softmax_max64(x):
    x = x.astype(np.float64)
    return 1.0 / np.exp(x - x.max(-1, keepdims=True)).sum(-1)


def _itos():
    with open(os.path.join(GOLDEN, "g1_ref_tokenizer.json")) as f:
        return [chr(c) for c in json.load(f)["itos"]]


def _relabelled(x, ids):
    """Every designed chain of more than ~18 characters runs through class 88 (which the tokenizer drops, like the reference's: tuatara.cpp:31-48) and through a
    backslash class (69 / 87: a lexicon entry cannot name it), so the engine's own long readings decode to one character less than their positions.  The same
    logits with those three class columns swapped against three ordinary classes the rows never choose: the same numbers behind every decision, and readings of
    25 and 26 characters that a lexicon can spell."""
    itos = _itos()
    free = [c for c in range(1, 95) if c not in (69, 87, 88) and itos[c] not in ("]", "\\") and not (ids == c).any()][:3]
    assert len(free) == 3
    y = x.copy()
    for a, b in zip((69, 87, 88), free):
        y[..., [a, b]] = y[..., [b, a]]
    return y


def test_behind_the_logits_on_25_and_26_character_readings(long, got128):
    """The engine's long-word logits through the final decode (decode_conf_kernel against the float64 softmax of tests/test_gpu_conf.py, the host rule of
    tests/test_conf_cpu.py), decode_ids, the alternatives (reading 0 of the n-best = the text and its confidence) and a lexicon that holds a crop's exact reading:
    25 characters + EOS, and 26 characters with no EOS."""
    from tests import lexicon_ref as LR
    from tests.test_conf_cpu import rule
    from tuatara_amd.engine import confidence_from_probs, decode_ids, nbest_from_alts
    eng = long["eng"]
    got, _, ids128 = got128
    has = (ids128 == 0).any(1)
    rows = np.concatenate([np.nonzero(~has)[0][:4], np.nonzero(has & (R.upto_eos(ids128) == 26))[0][:4]])       # 4 that never end, 4 with the EOS in column 25
    assert len(rows) == 8
    raw = got[rows]
    for x, relabelled in ((raw, False), (_relabelled(raw, ids128[rows]), True)):
        ids, prob, conf = eng.logits_confidence(x)
        assert np.array_equal(ids, x.argmax(-1)) and (np.array_equal(ids, ids128[rows]) or relabelled)
        rel = np.abs(prob.astype(np.float64) - _softmax_max64(x)) / _softmax_max64(x)
        print(f"long readings{' (relabelled)' if relabelled else ''}: max relative |prob - float64| {rel.max():.2e}; conf {conf.min():.3f} .. {conf.max():.3f}")
        assert rel.max() <= 2e-6 and (prob > 0).all() and (prob <= 1).all()
        alt_ids, alt_prob = eng.logits_alternatives(x, 2)
        assert np.array_equal(alt_ids[..., 0], ids) and alt_prob[..., 0].tobytes() == prob.tobytes()
        for k in range(8):
            S, e, want = rule(ids[k], prob[k])
            cc, c = confidence_from_probs(ids[k], prob[k])
            text = decode_ids(ids[k])
            assert c.tobytes() == conf[k:k + 1].tobytes() == want.tobytes() and np.array_equal(cc, prob[k][S]), k
            dropped = int((ids[k] == 88).sum())
            assert len(text) == len(S) == (26 if k < 4 else 25) - dropped and e == (None if k < 4 else 25), (k, text)
            assert (dropped == 0) == relabelled                                         # (raw: one position of each reading is the dropped class)
            best = nbest_from_alts(alt_ids[k], alt_prob[k], 2)
            assert len(best) == 2 and best[0][0] == text and best[0][1].tobytes() == conf[k:k + 1].tobytes(), (k, best)
            assert best[1][1] <= best[0][1]
    # (x, ids, prob, conf: the relabelled rows from here on) a lexicon that holds the exact 25-character reading of a crop ranks it first
    itos = _itos()
    texts = [decode_ids(r) for r in ids]
    assert [len(t) for t in texts] == [26] * 4 + [25] * 4
    word = texts[4]
    other = next(ch for ch in "abcdefg" if ch != word[0] and ch != word[-1])
    words = [word[:24], word[:-1] + other, other + word[1:], texts[0][:25], word, texts[1][1:]]
    assert len(set(words)) == 6 and all(len(w) <= 25 for w in words)
    eng.set_lexicon(words, 3)
    try:
        idx, logp = eng.logits_lexicon(x[4:5])
    finally:
        eng.set_lexicon(None)
    lp, mag = LR.tables(x[4:5])
    score, tol = LR.scores(LR.encode(words, itos), lp, mag)
    order = LR.rank(score[0], 3)
    print(f"lexicon on a 25-character reading: entries {idx[0].tolist()} logp {logp[0].tolist()}; float64 {score[0][order].tolist()}; log conf {float(np.log(np.float64(conf[4]))):.6f}")
    assert idx[0, 0] == 4 and idx[0].tolist() == order.tolist()
    assert (np.abs(logp[0].astype(np.float64) - score[0][order]) <= tol[0][order]).all()
    # the exact reading's score is the logarithm of the word's confidence: 26 factors, each prob within 2e-6 relative of float64 and one fp32 rounding per product
    assert abs(float(logp[0, 0]) - float(np.log(np.float64(conf[4])))) <= tol[0][4] + 26 * (2e-6 + 2.0 ** -23)


def test_a_page_call_on_a_word_of_26_positions(long, got128):
    """With alternatives on, caller-given regions that frame long-word crops one to one: the page path's ids are the recogniser call's, a 26-position word
    keeps every position (the dropped class aside), and reading 0 of its two best readings is (text, conf)."""
    from tests import regions_ref as GR
    from tuatara_amd.engine import decode_ids, nbest_from_alts
    eng = long["eng"]
    ids128 = got128[2]
    has = (ids128 == 0).any(1)
    pick = np.concatenate([np.nonzero(~has)[0][:2], np.nonzero(has & (R.upto_eos(ids128) == 26))[0][:1], np.nonzero(ids128[:, 0] == 0)[0][:1]])
    image = np.ascontiguousarray(long["crops"][pick].reshape(len(pick) * 32, 128, 3))
    quads = np.stack([GR.region_from_rect(0, 32 * i, 128, 32 * i + 32) for i in range(len(pick))])
    assert np.array_equal(eng.pack_regions(image, quads), long["crops"][pick])
    eng.set_alternatives(2)
    try:
        items = eng.read_regions(image, [{"quad": q} for q in quads])
    finally:
        eng.set_alternatives(0)
    assert len(items) == 4
    for k, it in enumerate(items):
        assert it["ids"] == ids128[pick[k]].tolist(), k
        assert it["text"] == decode_ids(ids128[pick[k]]), k
        best = nbest_from_alts(it["alt_ids"], it["alt_prob"], 2)
        assert best[0][0] == it["text"] and float(best[0][1]) == it["conf"], (k, best, it["conf"])
    assert [len(it["text"]) for it in items] == [25, 25, 24, 0]
