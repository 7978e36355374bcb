"""CPU suite for the recognition confidence (DESIGN.md "Recognition confidence"): the host rule ttr_confidence_from_probs against a numpy
restatement on hand-made and random rows - which positions make up the text, the EOS's own probability, ids outside the table - and the
product bit for bit.  No GPU."""
import ctypes

import numpy as np
import pytest

EOS, DROP = 0, 88          # id 0 ends the text (its character is ']'); id 88 is filtered out


@pytest.fixture(scope="module")
def eng():
    from tuatara_amd import build, engine
    build.build_lib()
    return engine


def rule(ids, probs):
    """numpy restatement: (positions S of the text's characters, position of the EOS or None, conf as the sequential fp32 product)"""
    ids = np.asarray(ids)
    probs = np.asarray(probs, np.float32)
    e = next((p for p, i in enumerate(ids) if i == EOS), None)
    S = [p for p in range(len(ids) if e is None else e) if ids[p] != DROP and 0 <= ids[p] < 98]
    c = np.float32(1.0)
    for p in S + ([] if e is None else [e]):
        c = np.float32(c * probs[p])
    return S, e, c


def check(eng, ids, probs):
    ids = np.asarray(ids, np.int32)
    probs = np.asarray(probs, np.float32)
    cc, conf = eng.confidence_from_probs(ids, probs)
    S, e, want = rule(ids, probs)
    assert len(cc) == len(S) == len(eng.decode_ids(ids))
    assert np.array_equal(cc, probs[S])
    assert conf.tobytes() == want.tobytes(), (conf, want)
    return S, e, conf


def row(*pairs):
    """(id, prob) pairs, padded to 26 positions with id 5 (a character) and prob 0.5"""
    ids = [i for i, _ in pairs] + [5] * (26 - len(pairs))
    probs = [p for _, p in pairs] + [0.5] * (26 - len(pairs))
    return ids, probs


def test_eos_at_position_zero(eng):
    ids, probs = row((0, 0.75), (12, 0.9), (13, 0.8))
    S, e, conf = check(eng, ids, probs)
    assert S == [] and e == 0 and conf == np.float32(0.75)            # an empty text: conf = prob[EOS]
    assert eng.decode_ids(np.array(ids, np.int32)) == ""


def test_eos_in_the_middle(eng):
    ids, probs = row((11, 0.9), (12, 0.8), (13, 0.7), (0, 0.6), (14, 0.1), (0, 0.2))
    S, e, conf = check(eng, ids, probs)
    assert S == [0, 1, 2] and e == 3
    assert conf == np.float32(np.float32(np.float32(np.float32(0.9) * np.float32(0.8)) * np.float32(0.7)) * np.float32(0.6))


def test_no_eos(eng):
    ids = list(range(1, 27))
    probs = np.linspace(0.99, 0.6, 26, dtype=np.float32)
    S, e, conf = check(eng, ids, probs)
    assert e is None and S == list(range(26))                        # 26 characters, no EOS factor


def test_id_88_before_and_after_the_eos_and_several_zeros(eng):
    ids, probs = row((88, 0.3), (20, 0.9), (88, 0.25), (21, 0.8), (0, 0.7), (88, 0.1), (0, 0.05), (0, 0.04))
    S, e, conf = check(eng, ids, probs)
    assert S == [1, 3] and e == 4                                     # 88 never counts; only the FIRST zero does
    assert conf == np.float32(np.float32(np.float32(0.9) * np.float32(0.8)) * np.float32(0.7))


def test_ids_outside_the_table_are_dropped(eng):
    ids, probs = row((-1, 0.3), (97, 0.9), (98, 0.2), (1 << 30, 0.1), (7, 0.8), (0, 0.6))
    S, e, conf = check(eng, ids, probs)
    assert S == [1, 4] and e == 5


def test_random_rows(eng):
    rng = np.random.default_rng(3)
    for k in range(2000):
        ids = rng.integers(0, 95, 26).astype(np.int32)
        if k % 3 == 0:                                                # the ids the recogniser emits most: few zeros and 88s
            ids[rng.random(26) < 0.8] = rng.integers(1, 88)
        if k % 5 == 0:
            ids[rng.integers(0, 26)] = DROP
        probs = rng.uniform(1.0 / 95, 1.0, 26).astype(np.float32)
        probs[rng.random(26) < 0.2] = 1.0
        check(eng, ids, probs)


def test_conf_is_the_sequential_product_not_a_reordered_one(eng):
    """a row where the order of the fp32 multiplications changes the result: the host must take them in position order"""
    rng = np.random.default_rng(9)
    found = 0
    for _ in range(500):
        ids = rng.integers(1, 88, 26).astype(np.int32)
        probs = rng.uniform(0.01, 1.0, 26).astype(np.float32)
        _, conf = eng.confidence_from_probs(ids, probs)
        rev = np.float32(1.0)
        for p in probs[::-1]:
            rev = np.float32(rev * p)
        found += rev.tobytes() != conf.tobytes()
        _, _, want = rule(ids, probs)
        assert conf.tobytes() == want.tobytes()
    assert found > 0


def test_bad_arguments(eng):
    lib = eng.load()
    p = np.ones(26, np.float32)
    assert lib.ttr_confidence_from_probs(None, p.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 26, None, None, None) == -1
    ids = np.full(26, 5, np.int32)
    n = lib.ttr_confidence_from_probs(ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), p.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 26,
                                      None, None, None)
    assert n == 26                                                    # every output may be NULL
    with pytest.raises(ValueError):
        eng.confidence_from_probs(ids, p[:3])
