"""CPU suite for word orientation (ttr_config.orient; DESIGN.md "Word orientation"): the host choice rule (ttr_orient_select) against the
numpy restatement tests/orient_ref.py, the engine's turned-quad coefficients against numpy bit for bit in both crop modes, the clockwise
convention on synthetic pages turned by np.rot90, and the config checks.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import orient_ref as O
from tests import rectify_ref as R
from tests.test_rectify_cpu import TABLE, _ncc


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


def _ids(word_len, rng=None):
    """26 ids of a text of word_len characters (ids 1..87), an EOS, then filler"""
    ids = np.full(26, 95, np.int32)
    ids[:word_len] = (rng.integers(1, 88, word_len) if rng is not None else np.arange(1, word_len + 1))
    if word_len < 26:
        ids[word_len] = 0
    return ids


def _check(conf, ids, per_page):
    from tuatara_amd.engine import orient_select
    got = orient_select(conf, ids, per_page)
    want = O.select(conf, ids, per_page)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1], (conf, got, want)
    return got


def test_select_hand_made(built):
    from tuatara_amd.engine import orient_select
    two, one = _ids(5), _ids(1)
    # ties go to the lower turn (k = 4: turns 0..3; k = 2: turns 0, 2)
    conf = np.array([[0.5, 0.5, 0.5, 0.5], [0.1, 0.7, 0.7, 0.2], [0.3, 0.2, 0.9, 0.9]], np.float32)
    ids = np.stack([np.stack([two] * 4)] * 3)
    turns, pt = _check(conf, ids, False)
    assert turns.tolist() == [0, 1, 2] and pt == 0                                    # one vote each for 0, 1, 2: the tie goes to 0
    turns, pt = _check(np.array([[0.4, 0.4], [0.1, 0.6], [0.2, 0.8]], np.float32), np.stack([np.stack([two] * 2)] * 3), False)
    assert turns.tolist() == [0, 2, 2] and pt == 2                                    # flip mode reports turns, not columns
    # one-character words do not vote: two short words at turn 3 lose to one long word at turn 1
    conf = np.array([[0.1, 0.2, 0.3, 0.9], [0.1, 0.2, 0.3, 0.9], [0.1, 0.9, 0.3, 0.2]], np.float32)
    ids = np.stack([np.stack([one] * 4), np.stack([one] * 4), np.stack([two] * 4)])
    turns, pt = _check(conf, ids, False)
    assert turns.tolist() == [3, 3, 1] and pt == 1
    turns, pt = _check(conf, ids, True)
    assert turns.tolist() == [1, 1, 1] and pt == 1                                    # page mode: every word at the page turn
    # an empty text with only an EOS, and id 88 does not count as a character
    e88 = _ids(2)
    e88[1] = 88
    conf = np.array([[0.9, 0.1], [0.1, 0.9]], np.float32)
    turns, pt = _check(conf, np.stack([np.stack([_ids(0)] * 2), np.stack([e88] * 2)]), False)
    assert turns.tolist() == [0, 2] and pt == 0                                       # no votes: page turn 0
    turns, pt = _check(conf, np.stack([np.stack([_ids(0)] * 2), np.stack([e88] * 2)]), True)
    assert turns.tolist() == [0, 0] and pt == 0
    # no words
    t, pt = orient_select(np.zeros((0, 4), np.float32), np.zeros((0, 4, 26), np.int32), True)
    assert len(t) == 0 and pt == 0
    # bad K
    from tuatara_amd.engine import EngineError
    with pytest.raises(EngineError):
        orient_select(np.zeros((2, 3), np.float32), np.zeros((2, 3, 26), np.int32))


def test_select_random_equals_numpy(built):
    rng = np.random.default_rng(3)
    for trial in range(300):
        k = (2, 4)[trial % 2]
        n = int(rng.integers(1, 40))
        # confs from a few levels, so that ties are common; texts of 0..5 characters
        conf = rng.choice(np.float32([0.1, 0.25, 0.5, 0.75, 1.0]), (n, k)).astype(np.float32)
        ids = np.stack([np.stack([_ids(int(rng.integers(0, 6)), rng) for _ in range(k)]) for _ in range(n)])
        for per_page in (False, True):
            turns, pt = _check(conf, ids, per_page)
            assert set(turns.tolist()) <= set(O.TURNS[k]) and pt in O.TURNS[k]
            if per_page:
                assert (turns == pt).all()


def test_turned_quad_coefficients_equal_numpy(built):
    from tuatara_amd.engine import orient_quad
    rng = np.random.default_rng(11)
    rects = list(TABLE) + [tuple(float(v) for v in np.float32([rng.uniform(-20, 620), rng.uniform(-20, 470), rng.uniform(0.5, 300),
                                                                rng.uniform(0.5, 60), rng.uniform(-90, 90)])) for _ in range(300)]
    h, w = 450, 600
    seen_edge = 0
    for r in rects:
        for mode in (0, 1):
            q0 = O.word_quad(r, mode, h, w)
            for t in range(4):
                q, fx = orient_quad(r, h, w, mode, t)
                assert np.array_equal(q, O.turn(q0, t)), (r, mode, t)
                assert np.array_equal(fx, O.turned_fixed(r, mode, t, h, w)), (r, mode, t, fx)
            if mode == 1:                                                   # turn 0 of crop_mode 1 is the deskew of the rectified mode
                assert np.array_equal(orient_quad(r, h, w, 1, 0)[1], R.deskew(r)[3])
        x0, y0, x1, y1 = O.clamped_rect(r, h, w)
        seen_edge += x0 == 0 or y0 == 0 or x1 == w or y1 == h
    assert seen_edge > 10
    with pytest.raises(Exception):
        orient_quad(TABLE[0], h, w, 0, 4)


def _rot_box(box, H, W):
    """[x0, x1) x [y0, y1) on an H x W page -> the same pixels after np.rot90(page, -1) (one quarter turn clockwise; the page becomes W x H)"""
    x0, y0, x1, y1 = box
    return (H - y1, x0, H - y0, x1)


def test_twin_at_the_matching_turn_reads_the_upright_word():
    """The clockwise convention, weight-free: a page turned by t quarter turns clockwise (np.rot90(page, -t)), its twin at turn t is the
    upright word's crop (NCC >= 0.95), and the crop at turn 0 is not (measured: NCC 1.0 at the matching turn; -0.02 - 0.15 at turn 0 for
    90 and 270 degrees, 0.12 - 0.37 upside down)."""
    from tuatara_amd import synth
    seen = 0
    for seed in (3, 4):
        page, words = synth.synthetic_rotated_page(seed, 320, 448, n_words=6, max_deg=0.0)
        assert len(words) >= 4
        for wd in words:
            th, tw = wd["tile"].shape
            cx, cy = wd["centre"]
            box = (int(round(cx - (tw - 1) / 2.0)), int(round(cy - (th - 1) / 2.0)), 0, 0)
            box = (box[0], box[1], box[0] + tw, box[1] + th)
            upright = R.sample(page, O.coef(O.box_quad(*box))[1])
            turned, b, (H, W) = page, box, page.shape[:2]
            for t in (1, 2, 3):
                turned = np.ascontiguousarray(np.rot90(turned, -1))
                b = _rot_box(b, H, W)
                H, W = turned.shape[:2]
                q = O.box_quad(*b)
                ncc = {k: _ncc(R.sample(turned, O.coef(O.turn(q, k))[1])[..., 0], upright[..., 0]) for k in range(4)}
                assert ncc[t] >= 0.95, (seed, t, ncc)
                assert ncc[0] < 0.8, (seed, t, ncc)
                assert ncc[t] == max(ncc.values()), (seed, t, ncc)
                seen += 1
    assert seen >= 24


def test_config_fields_and_checks(built, tmp_path):
    from tuatara_amd import engine
    cfg = engine.Config()
    engine.load().ttr_config_default(ctypes.byref(cfg))
    assert (cfg.orient, cfg.orient_page) == (engine.ORIENT_OFF, 0)
    assert engine.Config.orient.offset == engine.Config.crop_mode.offset + 4            # appended: the earlier fields keep their offsets
    assert engine.Config.orient_page.offset == engine.Config.orient.offset + 4
    for kw, msg in (({"orient": 3}, "orient must be"), ({"orient": -1}, "orient must be"), ({"orient": 1, "orient_page": 2}, "orient_page must be")):
        with pytest.raises(engine.EngineError, match=msg):
            engine.Engine(str(tmp_path), **kw)
