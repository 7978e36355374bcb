"""Reference for regions and per-row character sets (DESIGN.md "Regions and per-row character sets"), numpy only, written from the rules and not from
the engine: the masked decode row by row, the region crop (the kind-1 sampler of tests/rectify_ref.py on a caller's quad), the pixel-edge quad of a
rectangle, the bbox rule and the host checks of a quad."""
from __future__ import annotations

import numpy as np

from tests import charset_ref as CR
from tests import rectify_ref as RR


def masked_decode_rows(logits, masks, set_of, own=CR.FULL):
    """charset_ref.masked_decode applied row by row: row i decodes under masks[set_of[i]], or under `own` where set_of[i] is -1.
    Returns ids [n, 26], prob f64 [n, 26], conf f64 [n], and the rows' masks uint32 [n, 3]."""
    x = np.asarray(logits).reshape(-1, 26, CR.N_CLS)
    rows = np.stack([np.asarray(own if s < 0 else masks[s], np.uint32) for s in set_of]) if len(set_of) else np.zeros((0, 3), np.uint32)
    ids, prob, conf = [], [], []
    for xi, m in zip(x, rows):
        i, p, c = CR.masked_decode(xi[None], m)
        ids.append(i[0]); prob.append(p[0]); conf.append(c[0])
    return np.array(ids).reshape(-1, 26), np.array(prob).reshape(-1, 26), np.array(conf).reshape(-1), rows


def region_from_rect(x0: int, y0: int, x1: int, y1: int) -> np.ndarray:
    """the pixel-edge quad of the pixels [x0, x1) x [y0, y1), pixel centres at integers: f32 [8] tl, tr, br, bl"""
    l, t, r, b = (np.float32(v) - np.float32(0.5) for v in (x0, y0, x1, y1))
    return np.array([l, t, r, t, r, b, l, b], np.float32)


def region_fixed(quad8) -> np.ndarray:
    """the sampler's coefficients of a caller's quad: double on the floats, one rounding per statement, then rint(65536 x) -> int64 [6]"""
    q = np.asarray(quad8, np.float32).reshape(4, 2).astype(np.float64)
    tl, tr, bl = q[0], q[1], q[3]
    Ax, Bx = (tr[0] - tl[0]) / 128.0, (bl[0] - tl[0]) / 32.0
    Ay, By = (tr[1] - tl[1]) / 128.0, (bl[1] - tl[1]) / 32.0
    X0 = (tl[0] + 0.5 * Ax) + 0.5 * Bx
    Y0 = (tl[1] + 0.5 * Ay) + 0.5 * By
    return np.rint(np.array([X0, Ax, Bx, Y0, Ay, By], np.float64) * 65536.0).astype(np.int64)


def region_crop(image: np.ndarray, quad8) -> np.ndarray:
    """the crop of one region: the kind-1 sampler on the quad's coefficients, no clamp of the quad, the border pixel replicated -> u8 [32, 128, 3]"""
    return RR.sample(np.ascontiguousarray(image, np.uint8), region_fixed(quad8))


def region_crops(image: np.ndarray, quads) -> np.ndarray:
    quads = np.asarray(quads, np.float32).reshape(-1, 8)
    return np.stack([region_crop(image, q) for q in quads]) if len(quads) else np.zeros((0, 32, 128, 3), np.uint8)


def region_bbox(quad8) -> np.ndarray:
    """{min x, min y, max x, max y} of the four corners, as floats"""
    q = np.asarray(quad8, np.float32).reshape(4, 2)
    return np.array([q[:, 0].min(), q[:, 1].min(), q[:, 0].max(), q[:, 1].max()], np.float32)


def quad_ok(quad8) -> bool:
    """every coordinate finite and |x| < 32768"""
    q = np.asarray(quad8, np.float32).ravel()
    return bool(np.isfinite(q).all() and (np.abs(q) < 32768).all())


def inside(quad8, h: int, w: int) -> bool:
    """every corner within the page's pixel edges [-0.5, w - 0.5] x [-0.5, h - 0.5] (the strict_crops rule)"""
    q = np.asarray(quad8, np.float32).reshape(4, 2)
    return bool((q[:, 0] >= -0.5).all() and (q[:, 0] <= w - 0.5).all() and (q[:, 1] >= -0.5).all() and (q[:, 1] <= h - 0.5).all())


def tilted_quad(cx: float, cy: float, w: float, h: float, degrees: float) -> np.ndarray:
    """a w x h rectangle about (cx, cy) whose baseline runs at `degrees` (image coordinates, y down): f32 [8] tl, tr, br, bl"""
    a = np.radians(degrees)
    u, v = np.array([np.cos(a), np.sin(a)]) * (w / 2), np.array([-np.sin(a), np.cos(a)]) * (h / 2)
    c = np.array([cx, cy])
    return np.concatenate([c - u - v, c + u - v, c + u + v, c - u + v]).astype(np.float32)
