"""Numpy restatement of the rectified crop rule (crop_mode = TTR_CROP_RECTIFIED; DESIGN.md "Rectified crops"), written from the rule,
not from the engine: the deskew of a rotated rect into the quad tl, tr, br, bl, the six affine coefficients in double and their
int64 fixed point, and the integer bilinear sampler.  Kind-0 crops (axis-aligned rects) come from the oracle's boundingRect crop.
Every step is exact, so the GPU packer must match it bit for bit."""
from __future__ import annotations

import numpy as np

from oracle import post


def deskew(rect5):
    """rect {cx, cy, w, h, angle} in image pixels -> (kind, quad f32 [4, 2], coef f64 [6] {X0, Ax, Bx, Y0, Ay, By}, fixed int64 [6])."""
    r = np.asarray(rect5, np.float32)
    p = post.rect_points(r)                       # P0..P3, clockwise on screen; P[s] -> P[s+1] runs at angle + (s - 1) * 90 degrees
    w, h, a = np.float32(r[2]), np.float32(r[3]), float(r[4])
    j = np.ceil((a - 45.0) / 90.0) if np.isfinite(a) else 0.0
    theta = a - 90.0 * j                          # the baseline's direction in (-45, 45]
    s = int((1 - int(j)) % 4)
    if theta == 45.0:                             # tie: the side at -45 (P[s-1] -> P[s]) if it is longer; even s = an h side
        len_s, len_m = (w, h) if s & 1 else (h, w)
        if len_m > len_s:
            s = (s + 3) % 4
    quad = np.stack([p[(s + i) % 4] for i in range(4)]).astype(np.float32)
    tl, tr, bl = quad[0].astype(np.float64), quad[1].astype(np.float64), quad[3].astype(np.float64)
    Ax, Bx = (tr[0] - tl[0]) / 128.0, (bl[0] - tl[0]) / 32.0
    Ay, By = (tr[1] - tl[1]) / 128.0, (bl[1] - tl[1]) / 32.0
    X0 = (tl[0] + 0.5 * Ax) + 0.5 * Bx
    Y0 = (tl[1] + 0.5 * Ay) + 0.5 * By
    coef = np.array([X0, Ax, Bx, Y0, Ay, By], np.float64)
    fixed = np.rint(coef * 65536.0).astype(np.int64)
    kind = 0 if np.isfinite(a) and np.fmod(a, 90.0) == 0.0 else 1
    return kind, quad, coef, fixed


def skew_degrees(quad) -> float:
    """the baseline's angle (tl -> tr) in degrees, image coordinates (y down)"""
    q = np.asarray(quad, np.float64)
    return float(np.degrees(np.arctan2(q[1, 1] - q[0, 1], q[1, 0] - q[0, 0])))


def sample(image: np.ndarray, fixed) -> np.ndarray:
    """the kind-1 sampler: image u8 [H, W, 3] (caller's channel order), fixed int64 [6] -> crop u8 [32, 128, 3]"""
    H, W = image.shape[:2]
    X0, Ax, Bx, Y0, Ay, By = (np.int64(v) for v in fixed)
    u = np.arange(128, dtype=np.int64)[None, :]
    v = np.arange(32, dtype=np.int64)[:, None]
    sx, sy = X0 + u * Ax + v * Bx, Y0 + u * Ay + v * By
    ix, iy = sx >> 16, sy >> 16
    fx, fy = ((sx >> 5) & 2047)[..., None], ((sy >> 5) & 2047)[..., None]
    x0, x1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
    y0, y1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    img = image.astype(np.int64)
    top = (2048 - fx) * img[y0, x0] + fx * img[y0, x1]
    bot = (2048 - fx) * img[y1, x0] + fx * img[y1, x1]
    val = ((2048 - fy) * top + fy * bot + (1 << 21)) >> 22
    return np.clip(val, 0, 255).astype(np.uint8)


def crop(image: np.ndarray, box5, clamp: bool = True):
    """one rectified crop of the caller's image for an adjusted rect (image pixels) -> (crop u8 [32, 128, 3] or None when the
    boundingRect test drops the box, quad f32 [4, 2], kind)"""
    image = np.ascontiguousarray(image, np.uint8)
    kind, quad, _, fixed = deskew(box5)
    swapped = np.ascontiguousarray(image[:, :, ::-1])
    c0 = post.crop_resize(swapped, box5, clamp)   # the boundingRect crop (swap, crop, swap back: the caller's order); None = dropped
    if c0 is None:
        return None, quad, kind
    return (c0 if kind == 0 else sample(image, fixed)), quad, kind


def crops(image: np.ndarray, boxes, clamp: bool = True):
    """the rectified crops of every kept box -> (crops u8 [n, 32, 128, 3], quads f32 [n, 4, 2], kinds [n], kept box indices)"""
    out, quads, kinds, keep = [], [], [], []
    for i, b in enumerate(np.asarray(boxes, np.float32).reshape(-1, 5)):
        c, q, k = crop(image, b, clamp)
        if c is None:
            continue
        out.append(c); quads.append(q); kinds.append(k); keep.append(i)
    if not out:
        return np.zeros((0, 32, 128, 3), np.uint8), np.zeros((0, 4, 2), np.float32), [], []
    return np.stack(out), np.stack(quads), kinds, keep


def zero_or_crop(image: np.ndarray, box5):
    """the stage entry point's crop (ttr_pack_crops_rectified, clamp): a box whose clamped boundingRect is empty gives zeros"""
    c, q, k = crop(image, box5, True)
    return (np.zeros((32, 128, 3), np.uint8) if c is None else c), q, k
