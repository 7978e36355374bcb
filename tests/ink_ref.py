"""The local ink rule (DESIGN.md "Local ink"; tuatara_amd/csrc/ink_rule.h) restated in numpy from a padded integral image, independent of geometry.cpp and
ink.hip, and the pages the ink test modules share.  Integers throughout (int64 arrays and Python ints).  ink_ref(img, radius, drop, polarity) returns what
engine.ink_from_page returns.  Not a test module."""
import math

import numpy as np

from tests import deskew_ref as D
from tests import tables_ref as T

RADIUS, DROP, POLARITY = 16, 38, 2           # the convenience layers' defaults
DARK, LIGHT, AUTO = 0, 1, 2


def pack_bits(mask):
    """bool [n, m] -> uint64 [n, ceil(m / 64)], bit j % 64 of word j // 64 (the kernels' layout)"""
    n, m = mask.shape
    nw = (m + 63) // 64
    pad = np.zeros((n, nw * 64), np.uint8)
    pad[:, :m] = mask
    return np.packbits(pad.reshape(n, nw, 8, 8)[:, :, :, ::-1], axis=3).reshape(n, nw, 8).copy().view("<u8").reshape(n, nw)


def ink_mask(img, radius: int = RADIUS, drop: int = DROP, polarity: int = POLARITY):
    """the rule -> (bool [h, w], the record)"""
    s = np.asarray(img).astype(np.int64).sum(axis=2)                     # 1
    h, w = s.shape
    total = int(s.sum())
    inverted = 1 if polarity == LIGHT or (polarity == AUTO and 2 * total < 765 * h * w) else 0   # 2
    if inverted:
        s = 765 - s
    I = np.zeros((h + 1, w + 1), np.int64)                               # 3: the integral image, one row and column of zeros in front
    I[1:, 1:] = s.cumsum(axis=0).cumsum(axis=1)
    y0, y1 = np.clip(np.arange(h) - radius, 0, h)[:, None], np.clip(np.arange(h) + radius + 1, 0, h)[:, None]
    x0, x1 = np.clip(np.arange(w) - radius, 0, w)[None, :], np.clip(np.arange(w) + radius + 1, 0, w)[None, :]
    S = I[y1, x1] - I[y0, x1] - I[y1, x0] + I[y0, x0]
    n = (y1 - y0) * (x1 - x0)
    mask = s * n * 256 < S * (256 - drop)                                # 4
    return mask, {"radius": radius, "drop": drop, "polarity": polarity, "inverted": inverted, "sum": total, "w": w, "h": h}


def ink_ref(img, radius: int = RADIUS, drop: int = DROP, polarity: int = POLARITY):
    mask, rec = ink_mask(img, radius, drop, polarity)
    return {"bits": pack_bits(mask), "bitsT": pack_bits(mask.T), "ink": rec}


def same(got, want):
    """two result dicts agree in every output"""
    return (got["bits"].shape == want["bits"].shape and np.array_equal(got["bits"], want["bits"]) and got["bitsT"].shape == want["bitsT"].shape and
            np.array_equal(got["bitsT"], want["bitsT"]) and got["ink"] == want["ink"])


def mask_page(mask):
    """a page whose fixed-rule bitmap (any ink in 1..255) is `mask`: what feeds a ready mask to tables_ref and deskew_ref"""
    return np.repeat(np.where(mask, 0, 255).astype(np.uint8)[:, :, None], 3, axis=2)


def tables_ref_ink(img, quads=None, min_len=48, local_ink=(RADIUS, DROP, DARK)):
    """the tables restatement behind the local mask"""
    return T.tables_ref(mask_page(ink_mask(img, *local_ink)[0]), quads, min_len, 128)


def deskew_ref_ink(img, max_slope: int = D.MAX_SLOPE, gain: int = D.GAIN, local_ink=(RADIUS, DROP, DARK)):
    """the deskew restatement behind the local mask: the scores are the mask's, the resampled page is the image's"""
    img = np.asarray(img)
    h, w = img.shape[:2]
    sc = D.scores(mask_page(ink_mask(img, *local_ink)[0]), max_slope, 128)
    slope, found = D.choose(sc, max_slope, gain)
    C, S = D.consts(slope)
    skew = {"slope": slope, "found": found, "C": C, "S": S, "w": w, "h": h, "mode": 1 if slope else 0, "score0": sc[max_slope], "score_found": sc[found + max_slope],
            "degrees": math.degrees(math.atan(slope / 512.0))}
    return {"image": D.resample(img, C, S), "skew": skew, "scores": np.array(sc, np.uint64)}


# ---- the shared pages
def shade(img, lo: float = 0.35):
    """a horizontal illumination ramp from 1.0 at the left edge to `lo` at the right, multiplied into the page and rounded"""
    img = np.asarray(img)
    ramp = np.linspace(1.0, lo, img.shape[1])[None, :, None]
    return np.rint(img.astype(np.float64) * ramp).astype(np.uint8)


def random_page(seed, h, w):
    """seeded noise over a seeded smooth gradient: every threshold is exercised somewhere"""
    rng = np.random.default_rng(1000 + seed)
    base = np.linspace(rng.integers(20, 120), rng.integers(130, 255), w)[None, :, None] * np.linspace(0.6, 1.0, h)[:, None, None]
    return np.clip(base + rng.integers(-60, 60, (h, w, 3)), 0, 255).astype(np.uint8)


def tie_page():
    """2 x 2: two pixels of s = 765 and two of s = 0, so that twice the sum equals 765 h w exactly"""
    img = np.zeros((2, 2, 3), np.uint8)
    img[0, 0] = img[1, 1] = 255
    return img
