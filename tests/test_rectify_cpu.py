"""CPU suite for the rectified crop mode (crop_mode = TTR_CROP_RECTIFIED; DESIGN.md "Rectified crops"): the deskew rule on a table of
rects, the engine's host deskew (ttr_dbg_deskew) against the numpy restatement bit for bit, and the rectified crop of a rotated
synthetic word against its upright tile.  No GPU."""
import numpy as np
import pytest

from tests import rectify_ref as R


@pytest.fixture(scope="module")
def built():
    from tuatara_amd import build
    build.build_all()
    return build


# (cx, cy, w, h, angle): 0, +-10, +-44.9, +-45, 89.9, 90 and more, squares and thin boxes
TABLE = [(cx, cy, w, h, a)
         for (cx, cy) in [(200.0, 150.0), (37.25, 410.5)]
         for (w, h) in [(120.0, 30.0), (30.0, 120.0), (50.0, 50.0), (80.0, 1.0), (1.0, 80.0), (0.0, 17.0)]
         for a in [0.0, 10.0, -10.0, 44.9, -44.9, 45.0, -45.0, 89.9, -89.9, 90.0, -90.0, 135.0, 180.0, -180.0, 270.0, 17.25, -63.5]]


def _ncc(a, b):
    a = a.astype(np.float64).ravel(); b = b.astype(np.float64).ravel()
    a -= a.mean(); b -= b.mean()
    return float(a @ b / np.sqrt((a @ a) * (b @ b) + 1e-12))


def test_deskew_rule_table():
    from oracle import post
    for r in TABLE:
        kind, q, coef, fixed = R.deskew(r)
        w, h, a = r[2], r[3], r[4]
        assert kind == (0 if a % 90.0 == 0.0 else 1), r
        # the quad is the rect's four corners, cyclically reordered
        pts = post.rect_points(np.array(r, np.float32))
        assert any(np.array_equal(q, np.roll(pts, -s, 0)) for s in range(4)), r
        th = R.skew_degrees(q)
        base, side = np.hypot(*(q[1] - q[0])), np.hypot(*(q[3] - q[0]))
        if base > 0:
            assert -45.0 - 1e-3 <= th <= 45.0 + 1e-3, (r, th)
            assert q[1, 0] - q[0, 0] > 0, r                          # the baseline points right
        if min(w, h) > 0:
            assert q[3, 1] - q[0, 1] > 0, r                          # tl -> bl points down
            cross = (q[1, 0] - q[0, 0]) * (q[3, 1] - q[0, 1]) - (q[1, 1] - q[0, 1]) * (q[3, 0] - q[0, 0])
            assert cross > 0, r                                      # tl, tr, br, bl clockwise on screen (y down)
        if abs(a) == 45.0 and w != h and min(w, h) > 0:
            assert base >= side - 1e-3, r                            # a tie at 45 goes to the longer side
        if a == 45.0 and w == h:
            assert th > 0, r                                         # ... then to the side at +45
        # the coefficients: X0 = tl + half a step along both sides, in the documented order
        A, B = q[1].astype(np.float64) - q[0], q[3].astype(np.float64) - q[0]
        assert coef[1] == A[0] / 128 and coef[2] == B[0] / 32 and coef[4] == A[1] / 128 and coef[5] == B[1] / 32
        assert np.array_equal(fixed, np.rint(coef * 65536.0).astype(np.int64))
    # axis-aligned rects: the quad is the upright box whichever way round the rect is given
    for a in (0.0, 90.0, -90.0, 180.0):
        _, q, _, _ = R.deskew((100.0, 50.0, 60.0 if a in (0.0, 180.0) else 20.0, 20.0 if a in (0.0, 180.0) else 60.0, a))
        assert np.allclose(q, [[70, 40], [130, 40], [130, 60], [70, 60]], atol=1e-4), (a, q)


def test_host_deskew_equals_numpy(built):
    from tuatara_amd.engine import deskew
    rng = np.random.default_rng(7)
    rects = list(TABLE) + [tuple(float(v) for v in np.float32([rng.uniform(0, 900), rng.uniform(0, 900), rng.uniform(0.5, 300),
                                                                rng.uniform(0.5, 60), rng.uniform(-90, 90)])) for _ in range(400)]
    for r in rects:
        k, q, c, f = deskew(r)
        k2, q2, c2, f2 = R.deskew(r)
        assert k == k2, r
        assert np.array_equal(q, q2), r
        assert np.array_equal(c, c2), (r, c, c2)
        assert np.array_equal(f, f2), r


def test_sampler_identity_and_border():
    """the integer sampler on an exact pixel grid returns the pixels; outside the image it replicates the border"""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (40, 140, 3), dtype=np.uint8)
    fixed = np.array([5 << 16, 1 << 16, 0, 3 << 16, 0, 1 << 16], np.int64)     # (u, v) -> pixel (5 + u, 3 + v)
    assert np.array_equal(R.sample(img, fixed), img[3:35, 5:133])
    far = np.array([-(1000 << 16), 0, 0, -(1000 << 16), 0, 0], np.int64)
    assert (R.sample(img, far) == img[0, 0]).all()
    half = np.array([(5 << 16) + (1 << 15), 1 << 16, 0, 3 << 16, 0, 1 << 16], np.int64)   # half a pixel right: the rounded mean
    want = ((img[3:35, 5:133].astype(np.int64) * 1024 + img[3:35, 6:134].astype(np.int64) * 1024) * 2048 + (1 << 21)) >> 22
    assert np.array_equal(R.sample(img, half), want.astype(np.uint8))


def test_rectified_crop_reads_the_upright_word():
    """On a rotated synthetic page with ground-truth rects, the rectified crop is close to the upright word resized to the same
    32 x 128 and far closer than the boundingRect crop (measured: NCC 0.976 - 0.991 rectified, 0.07 - 0.26 boundingRect at |skew| >= 10)."""
    from oracle import post
    from tuatara_amd import synth
    seen = 0
    for seed in (1, 2):
        page, words = synth.synthetic_rotated_page(seed, 768, 768, n_words=12, max_deg=30.0)
        assert len(words) >= 8
        for wd in words:
            t = wd["tile"]
            th, tw = t.shape
            rect = np.array([wd["centre"][0], wd["centre"][1], tw, th, wd["angle"]], np.float32)
            c, q, kind = R.crop(page, rect)
            assert c is not None and kind == 1
            up = post.resize_linear(np.repeat(t[:, :, None], 3, 2), 32, 128)[..., 0]
            n_rect = _ncc(c[..., 0], up)
            n_bound = _ncc(post.crop_resize(page, rect)[..., 0], up)
            assert n_rect >= 0.93, (seed, wd["angle"], n_rect)
            if abs(wd["angle"]) >= 15.0:
                assert n_rect >= n_bound + 0.5, (seed, wd["angle"], n_rect, n_bound)
                seen += 1
    assert seen >= 6
