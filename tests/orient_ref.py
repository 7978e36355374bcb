"""Numpy restatement of the word-orientation rule (ttr_config.orient; DESIGN.md "Word orientation"), written from the rule, not from the
engine: the word's quad Q (the deskewed quad in crop_mode 1, the clamped boundingRect's pixel edges in crop_mode 0), the turned quad
Q_t[k] = Q[(k + t) mod 4], its coefficients and int64 fixed point in rectify_ref.deskew's order, the twin crop by rectify_ref.sample, and
the choice between the candidate readings.  Every step is exact, so the GPU packer and orient_select_kernel must match it bit for bit."""
from __future__ import annotations

import numpy as np

from oracle import post
from tests import rectify_ref as R

TURNS = {1: (0,), 2: (0, 2), 4: (0, 1, 2, 3)}   # candidate turns by K


def clamped_rect(box5, h: int, w: int):
    """the clamped boundingRect [x0, x1) x [y0, y1) of an adjusted rect in image pixels (the engine's crop rectangle)"""
    x, y, bw, bh = post.bounding_rect(np.asarray(box5, np.float32))
    return max(x, 0), max(y, 0), min(x + bw, w), min(y + bh, h)


def box_quad(x0: int, y0: int, x1: int, y1: int) -> np.ndarray:
    """crop_mode 0's Q: the rectangle's pixel edges (pixel centres at integers) tl, tr, br, bl, f32 [4, 2]"""
    l, t, r, b = (np.float32(v) - np.float32(0.5) for v in (x0, y0, x1, y1))
    return np.array([[l, t], [r, t], [r, b], [l, b]], np.float32)


def word_quad(box5, crop_mode: int, h: int, w: int) -> np.ndarray:
    """Q of an adjusted rect: the deskewed quad (crop_mode 1) or the clamped boundingRect's edges (crop_mode 0)"""
    if crop_mode == 1:
        return R.deskew(box5)[1]
    return box_quad(*clamped_rect(box5, h, w))


def turn(quad, t: int) -> np.ndarray:
    """Q_t[k] = Q[(k + t) mod 4]"""
    return np.roll(np.asarray(quad, np.float32), -int(t), axis=0)


def coef(quad):
    """any quad tl, tr, br, bl -> (coef f64 [6] {X0, Ax, Bx, Y0, Ay, By}, fixed int64 [6]): rectify_ref.deskew's arithmetic, step for step"""
    q = np.asarray(quad, np.float32).astype(np.float64)
    tl, tr, bl = q[0], q[1], q[3]
    Ax, Bx = (tr[0] - tl[0]) / 128.0, (bl[0] - tl[0]) / 32.0
    Ay, By = (tr[1] - tl[1]) / 128.0, (bl[1] - tl[1]) / 32.0
    X0 = (tl[0] + 0.5 * Ax) + 0.5 * Bx
    Y0 = (tl[1] + 0.5 * Ay) + 0.5 * By
    c = np.array([X0, Ax, Bx, Y0, Ay, By], np.float64)
    return c, np.rint(c * 65536.0).astype(np.int64)


def turned_fixed(box5, crop_mode: int, t: int, h: int, w: int) -> np.ndarray:
    """the int64 coefficients of a word's twin at turn t"""
    return coef(turn(word_quad(box5, crop_mode, h, w), t))[1]


def twin(image: np.ndarray, box5, crop_mode: int, t: int):
    """the crop of a word read at turn t >= 1 (a kind-1 crop of the turned quad; zeros when the clamped boundingRect is empty) and Q_t"""
    image = np.ascontiguousarray(image, np.uint8)
    h, w = image.shape[:2]
    x0, y0, x1, y1 = clamped_rect(box5, h, w)
    qt = turn(word_quad(box5, crop_mode, h, w), t)
    if x1 <= x0 or y1 <= y0:
        return np.zeros((32, 128, 3), np.uint8), qt
    return R.sample(image, coef(qt)[1]), qt


def oriented_crop(image: np.ndarray, box5, crop_mode: int, t: int):
    """ttr_pack_crops_oriented's crop of one adjusted rect: turn 0 = the crop_mode's own crop, turn >= 1 = the twin"""
    if t == 0:
        image = np.ascontiguousarray(image, np.uint8)
        h, w = image.shape[:2]
        if crop_mode == 1:
            c, q, _ = R.zero_or_crop(image, box5)
            return c, q
        c = post.crop_resize(np.ascontiguousarray(image[:, :, ::-1]), box5, True)
        return (np.zeros((32, 128, 3), np.uint8) if c is None else c), box_quad(*clamped_rect(box5, h, w))
    return twin(image, box5, crop_mode, t)


def text_chars(ids) -> int:
    """|S| of the confidence rule: positions before the first EOS (id 0) whose id is not 88 and lies in [0, 98)"""
    k = 0
    for v in np.asarray(ids).ravel()[:26]:
        if v == 0:
            break
        if v != 88 and 0 <= v < 98:
            k += 1
    return k


def select(conf, ids, per_page: bool = False):
    """one page: conf f32 [n, K], ids [n, K, 26] -> (turns int [n], page turn).  Per word the largest conf (strict >, ascending turn);
    the page turn = argmax of the votes of words whose winning text has >= 2 characters, ties to the lower turn, 0 without votes."""
    conf = np.asarray(conf, np.float32)
    n, k = conf.shape
    ids = np.asarray(ids).reshape(n, k, 26)
    cols = []
    votes = [0] * k
    for i in range(n):
        best = 0
        for j in range(1, k):
            if conf[i, j] > conf[i, best]:
                best = j
        cols.append(best)
        if text_chars(ids[i, best]) >= 2:
            votes[best] += 1
    pc = 0
    for j in range(1, k):
        if votes[j] > votes[pc]:
            pc = j
    t = TURNS[k]
    return np.array([t[pc] if per_page else t[c] for c in cols], np.int32), t[pc]
