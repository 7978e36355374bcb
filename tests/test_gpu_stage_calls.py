"""GPU suite for the host-staged stage calls of the C ABI (capi.cpp: the decode calls on host logits, the crop calls on a host image, the recogniser
calls on host crops): the equivalences between them that their shared bodies lean on, bit for bit, and what each does with no rows and with null
output pointers.  Nothing here has a tolerance: two calls that are one computation return the same bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL_ALLOWED = np.array([0xFFFFFFFF, 0xFFFFFFFF, 0x7FFFFFFF], np.uint32)   # charset_mask's form: the 95 classes
OWN = np.full(3, -1, np.int32)                                            # set_of: every row under the engine's own set
MODES_TURNS = ((0, 0), (1, 0), (0, 1), (1, 2))


@pytest.fixture(scope="module")
def eng(weights):
    """an f16x4 engine of this module's own: no character set, no pattern, whatever the other modules did to theirs"""
    from tuatara_amd.build import build_lib
    from tuatara_amd.engine import Engine
    build_lib()
    e = Engine(weights["dir"])
    assert np.array_equal(e.charset, ALL_ALLOWED) and e.pattern is None
    return e


@pytest.fixture(scope="module")
def logits():
    return np.random.default_rng(11).normal(0.0, 3.0, (3, 26, 95)).astype(np.float32)


@pytest.fixture(scope="module")
def crops():
    return np.random.default_rng(12).integers(0, 256, (3, 32, 128, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def page(eng):
    """a 64 x 96 image and 3 heat-map rects {cx, cy, w, h, angle} (half the image's resolution at ratio 1): one upright, one rotated, one hanging
    over the image's right and bottom edges"""
    img = np.random.default_rng(13).integers(0, 256, (64, 96, 3), dtype=np.uint8)
    rects = np.array([[12, 10, 16, 6, 0], [24, 16, 20, 6, -17], [44, 28, 14, 10, 0]], np.float32)
    return img, rects, eng.canvas_geometry(64, 96)[2]


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)


def test_decode_equivalences(eng, logits):
    plain = eng.logits_confidence(logits)
    assert np.array_equal(plain[0], np.argmax(logits, -1))                  # (the calls did run: zeros would agree with each other too)
    _same(plain, eng.logits_confidence(logits, mask=ALL_ALLOWED))
    _same(plain, eng.logits_confidence(logits, set_of=OWN))
    alt_ids, _ = eng.logits_alternatives(logits, 2)
    assert np.array_equal(alt_ids[..., 0], plain[0])


def test_recogniser_equivalence(eng, crops):
    lg, ids = eng.parseq_logits(crops)
    assert np.abs(lg).max() > 0
    _same((lg, ids), eng.parseq_logits(crops, set_of=OWN))


def test_crop_equivalences(eng, page):
    img, rects, ratio = page
    from tuatara_amd.engine import CROP_BOUNDING, CROP_RECTIFIED
    assert (CROP_BOUNDING, CROP_RECTIFIED) == (0, 1)
    plain, _boxes = eng.pack_crops(img, rects, ratio)
    assert all(c.min() != c.max() for c in plain)                           # every crop, the overhanging one included, read some of the image
    assert np.array_equal(plain, eng.pack_crops_oriented(img, rects, ratio, 0, 0)[0])
    _same(eng.pack_crops_rectified(img, rects, ratio), eng.pack_crops_oriented(img, rects, ratio, 1, 0))
    for mode, turn in MODES_TURNS:
        _same(eng.pack_crops_batch([img], rects, np.zeros(3, np.int32), mode, turn), eng.pack_crops_oriented(img, rects, ratio, mode, turn))


def test_no_rows(eng, page):
    img, _, ratio = page
    x = np.zeros((0, 26, 95), np.float32)
    none = np.zeros(0, np.int32)
    for got in (eng.logits_confidence(x), eng.logits_confidence(x, mask=ALL_ALLOWED), eng.logits_confidence(x, set_of=none)):
        assert [a.shape for a in got] == [(0, 26), (0, 26), (0,)]
    assert [a.shape for a in eng.logits_alternatives(x, 2)] == [(0, 26, 2), (0, 26, 2)]
    c = np.zeros((0, 32, 128, 3), np.uint8)
    for got in (eng.parseq_logits(c), eng.parseq_logits(c, set_of=none)):
        assert [a.shape for a in got] == [(0, 26, 95), (0, 26)]
    r = np.zeros((0, 5), np.float32)
    assert [a.shape for a in eng.pack_crops(img, r, ratio)] == [(0, 32, 128, 3), (0, 5)]
    assert [a.shape for a in eng.pack_crops_rectified(img, r, ratio)] == [(0, 32, 128, 3), (0, 4, 2)]
    for mode, turn in MODES_TURNS:
        assert [a.shape for a in eng.pack_crops_oriented(img, r, ratio, mode, turn)] == [(0, 32, 128, 3), (0, 4, 2)]
        assert [a.shape for a in eng.pack_crops_batch([img], r, none, mode, turn)] == [(0, 32, 128, 3), (0, 4, 2)]


def test_null_outputs(eng, logits):
    """each decode call fills the outputs it is given and returns 0 for the ones it is not (through engine.lib: the wrappers always pass all of them)"""
    import ctypes as C
    from tuatara_amd.engine import _f, _i
    lib, n = eng.lib, len(logits)
    mask = (C.c_uint32 * 3)(*[int(v) for v in ALL_ALLOWED])
    calls = {
        "plain": lambda i, p, c: lib.ttr_logits_confidence(eng.h, _f(logits), n, i, p, c),
        "masked": lambda i, p, c: lib.ttr_logits_confidence_masked(eng.h, _f(logits), n, mask, i, p, c),
        "sets": lambda i, p, c: lib.ttr_logits_confidence_sets(eng.h, _f(logits), n, None, 0, _i(OWN), i, p, c),
        "patterns": lambda i, p, c: lib.ttr_logits_decode_patterns(eng.h, _f(logits), n, None, 0, None, None, 0, None, i, p, c),
    }
    for name, call in calls.items():
        ids0, prob0, conf0 = np.zeros((n, 26), np.int32), np.zeros((n, 26), np.float32), np.zeros(n, np.float32)
        assert call(_i(ids0), _f(prob0), _f(conf0)) == 0, name
        assert prob0.min() > 0, name                                        # (it ran)
        ids, prob, conf = np.zeros((n, 26), np.int32), np.zeros((n, 26), np.float32), np.zeros(n, np.float32)
        assert call(None, _f(prob), _f(conf)) == 0, name
        assert np.array_equal(prob, prob0) and np.array_equal(conf, conf0), name
        assert call(_i(ids), None, None) == 0, name
        assert np.array_equal(ids, ids0), name
        assert call(None, None, None) == 0, name
    alt_ids0, alt_prob0 = eng.logits_alternatives(logits, 2)
    alt_ids, alt_prob = np.zeros_like(alt_ids0), np.zeros_like(alt_prob0)
    assert lib.ttr_logits_alternatives(eng.h, _f(logits), n, 2, None, 0, None, None, _f(alt_prob)) == 0
    assert lib.ttr_logits_alternatives(eng.h, _f(logits), n, 2, None, 0, None, _i(alt_ids), None) == 0
    assert np.array_equal(alt_ids, alt_ids0) and np.array_equal(alt_prob, alt_prob0)
