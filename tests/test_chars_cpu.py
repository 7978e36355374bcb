"""CPU suite for character boxes (ttr_config.chars; DESIGN.md "Character boxes"): the host rule (ttr_char_cuts_from_profile,
ttr_chars_from_map, ttr_char_quads_from_cuts) against the numpy restatement tests/chars_ref.py - the integer outputs are exact, so those
comparisons are np.array_equal -, the stated properties of the cuts, the functional test on hand-made maps of Gaussian blobs (every
interior cut lies strictly between the centres of the two characters it separates, and the even split of the word box does not), the
cells' corners against the formula in float64, and the config checks.  No GPU."""
import numpy as np
import pytest

from tests import chars_ref as R

KS = (0, 1, 2, 7, 13, 26)


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


def _profiles(seed):
    rng = np.random.default_rng(seed)
    out = {"random": rng.integers(0, 256, 128), "flat": np.full(128, 200), "zero": np.zeros(128), "saturated": np.full(128, 255)}
    spike = np.zeros(128); spike[int(rng.integers(0, 128))] = 255
    out["spike"] = spike
    smooth = 128 + 120 * np.sin(np.arange(128) / rng.uniform(1.5, 6.0) + rng.uniform(0, 6))
    out["waves"] = smooth
    part = np.zeros(128); a = int(rng.integers(0, 100)); part[a:a + int(rng.integers(1, 28))] = rng.integers(100, 256)
    out["short"] = part                                     # a short inked run: L < 2K for the larger K
    return {k: np.clip(v, 0, 255).astype(np.uint8) for k, v in out.items()}


@pytest.mark.parametrize("qlow", (0, 102, 254))
@pytest.mark.parametrize("K", KS)
def test_cuts_equal_numpy(built, K, qlow):
    from tuatara_amd.engine import char_cuts_from_profile
    seen = set()
    for seed in range(6):
        for name, q in _profiles(1000 * K + seed).items():
            cuts, mode = char_cuts_from_profile(q, K, qlow)
            want, wmode = R.cuts_from_profile(q, K, qlow)
            assert cuts.dtype == np.int32 and np.array_equal(cuts, want) and mode == wmode, (name, K, qlow, cuts, want)
            seen.add(mode)
            b = cuts[:K + 1]
            assert (cuts[K + 1:] == -1).all()
            if K == 0:
                assert (cuts == -1).all() and mode == 0
                continue
            ink = np.nonzero(q.astype(int) > qlow)[0]
            u0, u1 = (ink[0], ink[-1] + 1) if len(ink) else (0, 128)
            assert b[0] == 256 * u0 and b[K] == 256 * u1
            assert (np.diff(b) >= 0).all()
            if mode == 1:
                assert (np.diff(b) > 0).all() and (b % 256 == 0).all() and u1 - u0 >= 2 * K
            else:
                assert not len(ink) or u1 - u0 < 2 * K
    if 2 <= K <= 13 and qlow < 254:
        assert seen == {0, 1}


@pytest.mark.parametrize("K", (1, 2, 7, 13, 26))
def test_flat_profile_gives_even_cells(built, K):
    from tuatara_amd.engine import char_cuts_from_profile
    for u0, u1 in ((0, 128), (5, 123), (17, 17 + 2 * K), (3, 3 + 2 * K + 1), (40, 101)):
        if u1 - u0 < 2 * K:
            continue
        q = np.zeros(128, np.uint8); q[u0:u1] = 180
        cuts, mode = char_cuts_from_profile(q, K, 102)
        assert mode == 1
        w = np.diff(cuts[:K + 1]) // 256
        assert w.sum() == u1 - u0 and w.max() - w.min() <= 1, (K, u0, u1, w)


def test_bad_counts_are_refused(built):
    from tuatara_amd.engine import EngineError, char_cuts_from_profile
    for K in (-1, 27):
        with pytest.raises(EngineError):
            char_cuts_from_profile(np.zeros(128, np.uint8), K, 0)


@pytest.mark.parametrize("ratio", (1.0, 0.8))
@pytest.mark.parametrize("size", ((64, 96), (200, 333), (512, 384)))
@pytest.mark.parametrize("outside", (False, True))
def test_map_rule_equals_numpy(built, size, ratio, outside):
    from tuatara_amd.engine import chars_from_map
    H2, W2 = size
    T = R.random_map(H2 * 7 + W2, H2, W2)
    quads, turns, nchars = R.random_words(H2 + W2 + int(ratio * 10) + outside, 60, H2, W2, ratio, outside=outside)
    cuts, modes, prof = chars_from_map(T, ratio, 0.4, quads, turns, nchars)
    want = R.chars_from_map(T, ratio, 0.4, quads, turns, nchars)
    assert np.array_equal(prof, want[2])
    assert np.array_equal(cuts, want[0]) and np.array_equal(modes, want[1])
    assert set(turns.tolist()) == {0, 1, 2, 3} and prof.max() > 128 and len(set(modes.tolist())) == 2
    if outside:     # some samples were clamped
        k = R.scale(ratio)
        q = quads.reshape(-1, 4, 2) * k
        assert (q.min() < -1) and (q[..., 0].max() > W2 or q[..., 1].max() > H2)


def test_turn_changes_the_frame(built):
    """turn t reads along Q[t] -> Q[t + 1]: the same rectangle listed from its next corner, one turn less, gives the same profile"""
    from tuatara_amd.engine import chars_from_map
    T = R.random_map(5, 120, 160)
    q = R.rect_quad(150., 110., 180., 40., 17.).reshape(4, 2)
    ref = chars_from_map(T, 1.0, 0.4, [q.reshape(8)], [1], [5])
    alt = chars_from_map(T, 1.0, 0.4, [np.roll(q, -1, axis=0).reshape(8)], [0], [5])
    assert np.array_equal(ref[2], alt[2]) and np.array_equal(ref[0], alt[0])
    other = chars_from_map(T, 1.0, 0.4, [q.reshape(8)], [0], [5])
    assert not np.array_equal(ref[2], other[2])


def test_bad_quads_are_refused(built):
    from tuatara_amd.engine import EngineError, chars_from_map
    T = np.zeros((32, 32), np.float32)
    good = R.rect_quad(20., 20., 30., 10., 0.)
    for bad in (np.nan, np.inf, -np.inf, 32768.0, -40000.0):
        q = good.copy(); q[3] = bad
        assert R.chars_from_map(T, 1.0, 0.4, [q], [0], [3]) is None
        with pytest.raises(EngineError):
            chars_from_map(T, 1.0, 0.4, [q], [0], [3])
    for turn, K, ratio in ((4, 3, 1.0), (-1, 3, 1.0), (0, 27, 1.0), (0, 3, 0.0), (0, 3, float("nan"))):
        with pytest.raises(EngineError):
            chars_from_map(T, ratio, 0.4, [good], [turn], [K])
    cuts, modes, prof = chars_from_map(T, 1.0, 0.4, np.zeros((0, 8)), [], [])
    assert cuts.shape == (0, 27) and modes.shape == (0,) and prof.shape == (0, 128)


# ---------------------------------------------------------------- the functional test
BLOB_SEEDS = {0.5: (11, 12, 13, 14), 0.4: (21, 22, 23, 24)}
BLOB_WORDS = 300


@pytest.mark.parametrize("k", (0.5, 0.4))
def test_cuts_separate_the_blobs(built, k):
    """Words of K Gaussian blobs (tests/chars_ref.py: blob_words - amplitude 0.75..0.95, sigma 0.32 of the character's width along the
    baseline and 0.32 of the height across it, noise N(0, 0.03), K 2..12, height 20..48 px, widths 0.3..0.9 of the height, length <= 400 px,
    tilt within 40 degrees; 300 draws per seed, four fixed seeds per scale): EVERY interior cut of the rule lies strictly between the centres
    of the two characters it separates.  The even split of the word box breaks that on the same words.
    The sizes are pixels of the half-resolution map the blobs are drawn on; the scale k only places the quad in image pixels.  (Read as image
    pixels instead, the smallest characters are 2.4 map pixels wide with a sigma of 0.8 - below what nearest-pixel sampling resolves - and on
    such words the rule placed 14 of 14 000 cuts outside their two centres, all in 12-character words; that set is not asserted.)"""
    from tuatara_amd.engine import chars_from_map
    n_cuts = bad = even_bad = words = 0
    worst_even = 0.0
    for seed in BLOB_SEEDS[k]:
        for T, ratio, quad, K, centres in R.blob_words(seed, k, BLOB_WORDS):
            cuts, modes, _ = chars_from_map(T, ratio, 0.4, [quad], [0], [K])
            t = cuts[0][1:K] / 32768.0
            ok = (t > centres[:-1]) & (t < centres[1:])
            bad += int((~ok).sum()); n_cuts += K - 1; words += 1
            even = np.arange(1, K) / K
            eok = (even > centres[:-1]) & (even < centres[1:])
            even_bad += int((~eok).sum())
            off = np.maximum(centres[:-1] - even, even - centres[1:]) / np.diff(centres).clip(1e-9)
            worst_even = max(worst_even, float(off.max()))
    print(f"k = {k}: {words} words, {n_cuts} interior cuts, {bad} outside their two centres; even split: {even_bad} outside, worst by {worst_even:.2f} spacings")
    assert words >= len(BLOB_SEEDS[k]) * (BLOB_WORDS - 5) and n_cuts > 6500
    assert bad == 0
    assert even_bad > 0


# ---------------------------------------------------------------- cells and config
def test_cells_match_the_formula(built):
    from tuatara_amd.engine import char_cuts_from_profile, char_quads_from_cuts
    rng = np.random.default_rng(3)
    for i in range(200):
        quad = R.rect_quad(rng.uniform(0, 30000), rng.uniform(0, 30000), rng.uniform(10, 600), rng.uniform(5, 80), rng.uniform(-44, 44))
        quad = (quad + rng.uniform(-2, 2, 8)).astype(np.float32)             # any quadrilateral, not only rectangles
        K, turn = int(rng.integers(0, 27)), int(rng.integers(0, 4))
        cuts, _ = char_cuts_from_profile(rng.integers(0, 256, 128).astype(np.uint8), K, 102)
        cq, cb = char_quads_from_cuts(quad, turn, cuts, K)
        wq, wb = R.quads_from_cuts(quad, turn, cuts, K)
        assert cq.shape == (K, 8) and cb.shape == (K, 4)
        if K:
            assert np.abs(cq - wq).max() <= 2.0 ** -8 and np.abs(cb - wb).max() <= 2.0 ** -8
            # neighbours share their cut edge, and the cells tile the turned quad's extent b[0]..b[K]
            assert np.array_equal(cq[1:, 0:2], cq[:-1, 2:4]) and np.array_equal(cq[1:, 6:8], cq[:-1, 4:6])


def test_config_field(built):
    from tuatara_amd.engine import Config, load
    assert Config.chars.offset == Config.lines.offset + 4
    cfg = Config()
    load().ttr_config_default(cfg)
    assert cfg.chars == 0


def test_bad_config_values_are_refused(built, tmp_path):
    """chars = 2 and chars = -1: ttr_create fails with the documented message (the check precedes the device and the weights)"""
    from tuatara_amd.engine import Engine, EngineError
    for v in (2, -1):
        with pytest.raises(EngineError, match="chars must be 0 or 1"):
            Engine(str(tmp_path), chars=v)
