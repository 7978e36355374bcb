"""The deskew rule (DESIGN.md "Deskew"; tuatara_amd/csrc/deskew_rule.h) restated in numpy, and the pages the deskew test modules share.

Integers throughout (int64 arrays and Python ints), except for the constants table, which is float64 with correctly rounded sqrt and division and np.rint's
round-half-to-even, as the host forms it.  deskew_ref(img, max_slope, gain, ink) returns what engine.deskew_from_page returns."""
import math
import os

import numpy as np

from tests import tables_ref as T

MAX_SLOPE, GAIN, INK = 64, 288, 128          # the convenience layers' defaults
TILTS = (-100, -37, -9, -3, 2, 5, 18, 64, 120)


def consts(k: int):
    """step 4: (C, S) of slope k"""
    d = np.sqrt(np.float64(262144 + k * k))
    return int(np.rint(np.float64(33554432.0) / d)), int(np.rint(np.float64(65536 * k) / d))


def ink_mask(img, ink: int):
    """step 1: bool [h, w]"""
    return np.asarray(img).astype(np.int64).sum(axis=2) < 3 * ink


def scores(img, max_slope: int, ink: int):
    """step 2: Python ints [2 M + 1], slope k at k + M"""
    ys, xs = np.nonzero(ink_mask(img, ink))
    ys, xs = ys.astype(np.int64), xs.astype(np.int64)
    out = []
    for k in range(-max_slope, max_slope + 1):
        if len(ys) == 0:
            out.append(0)
            continue
        b = ys - ((xs * k + 256) >> 9)
        cnt = np.bincount(b - b.min()).astype(np.int64)
        out.append(int((cnt * cnt).sum()))
    return out


def choose(sc, max_slope: int, gain: int):
    """step 3: (slope, found)"""
    found = min(range(-max_slope, max_slope + 1), key=lambda k: (-sc[k + max_slope], abs(k), k))
    slope = found if found != 0 and sc[found + max_slope] * 256 >= sc[max_slope] * gain else 0
    return slope, found


def source_coords(C: int, S: int, h: int, w: int):
    """step 5: U, V int64 [h, w], the source coordinates of every output pixel in 1 / 131072 px"""
    dx = (2 * np.arange(w, dtype=np.int64) + 1 - w)[None, :]
    dy = (2 * np.arange(h, dtype=np.int64) + 1 - h)[:, None]
    return C * dx - S * dy + 65536 * (w - 1), S * dx + C * dy + 65536 * (h - 1)


def resample(img, C: int, S: int):
    """step 5: the page turned by the slope whose constants are C, S"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    U, V = source_coords(C, S, h, w)
    x0, fx, y0, fy = U >> 17, ((U >> 9) & 255)[..., None], V >> 17, ((V >> 9) & 255)[..., None]
    xa, xb, ya, yb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    p = img.astype(np.int64)
    v = p[ya, xa] * (256 - fx) * (256 - fy) + p[ya, xb] * fx * (256 - fy) + p[yb, xa] * (256 - fx) * fy + p[yb, xb] * fx * fy + 32768
    return (v >> 16).astype(np.uint8)


def deskew_ref(img, max_slope: int = MAX_SLOPE, gain: int = GAIN, ink: int = INK):
    img = np.asarray(img)
    h, w = img.shape[:2]
    sc = scores(img, max_slope, ink)
    slope, found = choose(sc, max_slope, gain)
    C, S = consts(slope)
    skew = {"slope": slope, "found": found, "C": C, "S": S, "w": w, "h": h, "mode": 1 if slope else 0, "score0": sc[max_slope], "score_found": sc[found + max_slope],
            "degrees": math.degrees(math.atan(slope / 512.0))}
    return {"image": resample(img, C, S), "skew": skew, "scores": np.array(sc, np.uint64)}


def tilt(img, slope: int):
    """a page whose level lines drop `slope` px per 512 px: the rule's own resampler under -slope"""
    return resample(img, *consts(-slope))


def to_page(skew, pts):
    """step 6 in float64: points [..., 2] of the upright page -> the source page"""
    p = np.asarray(pts, np.float64)
    cx, cy = (skew["w"] - 1) / 2.0, (skew["h"] - 1) / 2.0
    x, y = p[..., 0] - cx, p[..., 1] - cy
    return np.stack([cx + (skew["C"] * x - skew["S"] * y) / 65536.0, cy + (skew["S"] * x + skew["C"] * y) / 65536.0], axis=-1)


def from_page(skew, pts):
    """the inverse of to_page (float64): where a point of the source page lies on the upright page"""
    p = np.asarray(pts, np.float64)
    cx, cy = (skew["w"] - 1) / 2.0, (skew["h"] - 1) / 2.0
    x, y = (p[..., 0] - cx) * 65536.0, (p[..., 1] - cy) * 65536.0
    C, S = float(skew["C"]), float(skew["S"])
    det = C * C + S * S
    return np.stack([cx + (C * x + S * y) / det, cy + (-S * x + C * y) / det], axis=-1)


def tilt_points(pts, slope: int, h: int, w: int):
    """where points of a page lie on tilt(page, slope)"""
    C, S = consts(-slope)
    return from_page({"C": C, "S": S, "w": w, "h": h}, pts)


# ---- the shared pages
FORM_H, FORM_W = 480, 1000
FORM_ROWS, FORM_COLS = tuple(range(100, 341, 40)), tuple(range(60, 941, 176))   # a 6 x 5 grid of 2-px rulings, rows 40 px high


def form_page(words: bool = False):
    """the 480 x 1000 form: seven row lines, six column lines; words: a 64 x 14 bar of seeded noise at every cell's centre (what the test detector boxes)"""
    img = np.full((FORM_H, FORM_W, 3), 255, np.uint8)
    for y in FORM_ROWS:
        T.hline(img, y, FORM_COLS[0], FORM_COLS[-1] + 1)
    for x in FORM_COLS:
        T.vline(img, x, FORM_ROWS[0], FORM_ROWS[-1] + 1)
    if words:
        rng = np.random.default_rng(7)
        for q in form_words().reshape(-1, 4, 2):
            x0, y0, x1, y1 = int(q[0, 0]), int(q[0, 1]), int(q[2, 0]), int(q[2, 1])
            img[y0:y1, x0:x1] = np.where(rng.random((y1 - y0, x1 - x0, 1)) < 0.7, 0, 255)
    return img


def form_words():
    """one 64 x 14 word at the centre of every cell, row-major: f32 [30, 8]"""
    q = []
    for i in range(6):
        for j in range(5):
            cx, cy = (FORM_COLS[j] + FORM_COLS[j + 1]) // 2 + 1, (FORM_ROWS[i] + FORM_ROWS[i + 1]) // 2 + 1
            q.append([cx - 32, cy - 7, cx + 32, cy - 7, cx + 32, cy + 7, cx - 32, cy + 7])
    return np.array(q, np.float32)


def columns_page():
    from tuatara_amd.synth import synthetic_columns_page
    return synthetic_columns_page(3)[0]


def no_baseline_page():
    """512 x 384, words on a jittered grid: no two share a baseline"""
    from tuatara_amd.synth import synthetic_page
    return synthetic_page(1, 512, 384)


def funsd_page():
    from PIL import Image
    return np.array(Image.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "funsd_0001129658.png")).convert("RGB"))


def random_page(seed):
    """seeded ink of growing size and density (tables_ref.random_page: noise and some long lines), widths that are no multiples of 64"""
    return T.random_page(seed, h=80 + 7 * seed, w=120 + 11 * seed, p=0.1 + 0.1 * seed)


RANDOM_SEEDS = (0, 1, 2, 3, 4, 5)


def corner_page(h=40, w=70):
    """single ink pixels in the four corners: the first and the last bin under slopes +-M"""
    img = np.full((h, w, 3), 255, np.uint8)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        img[y, x] = 0
    return img


def same(got, want):
    """two result dicts agree in every output"""
    return (np.array_equal(got["image"], want["image"]) and got["image"].shape == want["image"].shape and
            np.array_equal(np.asarray(got["scores"], np.uint64), np.asarray(want["scores"], np.uint64)) and
            all(got["skew"][k] == want["skew"][k] for k in ("slope", "found", "C", "S", "w", "h", "mode", "score0", "score_found")))
