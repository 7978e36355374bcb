"""The wide-word rule (DESIGN.md "Wide words") restated in numpy: plan, profile, cuts, piece coefficients, piece quads.  The host rule
(tuatara_amd/csrc/geometry.cpp) and wide_cut_kernel (wide.hip) must agree with it bit for bit on every integer output."""
from __future__ import annotations

import math

import numpy as np

NP_MAX, V, COLS, WLO, WHI, INF = 16, 32, 128, 64, 192, 0x3FFFFFFF


def plan(quad8, max_aspect):
    """quad f32 [8] tl, tr, br, bl -> (n, frame int64 [6] = {X0f, Axf, Bxf, Y0f, Ayf, Byf}): double on the floats, one rounding per statement"""
    q = [float(v) for v in np.asarray(quad8, np.float32).ravel()]
    Ax, Ay, Bx, By = q[2] - q[0], q[3] - q[1], q[6] - q[0], q[7] - q[1]
    a2, b2 = Ax * Ax + Ay * Ay, Bx * Bx + By * By
    n = 1
    if b2 != 0.0:
        n = max(1, min(NP_MAX, math.ceil(math.sqrt(a2 / b2) / float(np.float32(max_aspect)))))
    U = float(COLS * n)
    Axf, Bxf, Ayf, Byf = Ax / U, Bx / 32.0, Ay / U, By / 32.0
    X0 = (q[0] + 0.5 * Axf) + 0.5 * Bxf
    Y0 = (q[1] + 0.5 * Ayf) + 0.5 * Byf
    return n, np.rint(np.array([X0, Axf, Bxf, Y0, Ayf, Byf], np.float64) * 65536.0).astype(np.int64)


def positions(frame, u, v):
    """the nearest page pixel (before the clamp) of frame column u, row v (arrays broadcast): (ix, iy) int64"""
    X0, Ax, Bx, Y0, Ay, By = (np.int64(x) for x in frame)
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    return (X0 + u * Ax + v * Bx + 32768) >> 16, (Y0 + u * Ay + v * By + 32768) >> 16


def profile(image, frame, n):
    """q u16 [128 n]: per column max - min over the 32 rows of R + 2 G + B at the nearest pixel, clamped to the page"""
    image = np.asarray(image, np.uint8)
    H, W = image.shape[:2]
    ix, iy = positions(frame, np.arange(COLS * n)[None, :], np.arange(V)[:, None])
    px = image[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)].astype(np.int64)
    y = px[..., 0] + 2 * px[..., 1] + px[..., 2]
    return (y.max(0) - y.min(0)).astype(np.uint16)


def cuts_from_profile(q, n):
    """cuts int32 [17]: c_0 = 0 < ... < c_n = 128 n, widths in [64, 192], -1 beyond n; ties go to the smallest width"""
    q = np.asarray(q, np.int64)
    U = COLS * n
    widths = np.arange(WLO, WHI + 1)
    prev = np.full(U + 1, INF, np.int64)
    prev[0] = 0
    arg = np.zeros((n + 1, U + 1), np.int64)
    c = np.arange(U + 1)
    src = c[None, :] - widths[:, None]                       # [129, U + 1]
    ok = src >= 0
    for j in range(1, n + 1):
        d = np.where(ok, prev[np.clip(src, 0, U)], INF)
        gap = np.zeros(U + 1, np.int64)
        if j < n:
            gap[1:U] = q[0:U - 1] + q[1:U]
        cost = np.where(d < INF, d + 2 * np.abs(widths - COLS)[:, None] + gap[None, :], INF)
        live = (c >= 1) & (c <= U - 1) if j < n else c == U
        cost[:, ~live] = INF
        best = cost.argmin(0)                                # the first minimum: the smallest width
        cur = cost[best, c]
        arg[j] = np.where(cur < INF, best, 0)
        prev = cur
    out = np.full(17, -1, np.int32)
    at = U
    for j in range(n, 0, -1):
        out[j] = at
        at -= int(arg[j, at]) + WLO
    out[0] = at
    return out


def piece_coef(frame, c0, c1):
    """the packer row {1, X0_p, Ax_p, Bx_p, Y0_p, Ay_p, By_p, 0} of the piece over [c0, c1): Python integers, arithmetic shifts"""
    X0, Ax, Bx, Y0, Ay, By = (int(x) for x in frame)
    w = int(c1) - int(c0)
    Axp, Ayp = (Ax * w + 64) >> 7, (Ay * w + 64) >> 7
    return np.array([1, X0 + Ax * int(c0) + ((Axp - Ax) >> 1), Axp, Bx, Y0 + Ay * int(c0) + ((Ayp - Ay) >> 1), Ayp, By, 0], np.int64)


def piece_coefs(frame, cuts, n):
    return np.stack([piece_coef(frame, cuts[j], cuts[j + 1]) for j in range(n)])


def piece_quads(quad8, cuts, n):
    """the pieces' quads f32 [n, 8]: tl + t0 A, tl + t1 A, bl + t1 (br - bl), bl + t0 (br - bl) in double, cast to float"""
    q = np.asarray(quad8, np.float32).astype(np.float64).reshape(4, 2)
    tl, tr, br, bl = q
    A, Cd = tr - tl, br - bl
    U = float(COLS * n)
    out = np.zeros((n, 8), np.float32)
    for j in range(n):
        t0, t1 = float(cuts[j]) / U, float(cuts[j + 1]) / U
        out[j] = np.concatenate([tl + t0 * A, tl + t1 * A, bl + t1 * Cd, bl + t0 * Cd]).astype(np.float32)
    return out


def word(image, quad8, max_aspect):
    """the whole rule on one quad: (n, frame, q, cuts, coef int64 [n, 8])"""
    n, frame = plan(quad8, max_aspect)
    q = profile(image, frame, n)
    cuts = cuts_from_profile(q, n)
    return n, frame, q, cuts, piece_coefs(frame, cuts, n)


def quad_of(x0, y0, length, height, degrees=0.0):
    """a length x height rectangle whose top-left corner is (x0, y0) and whose baseline runs at `degrees`: f32 [8] tl, tr, br, bl"""
    a = math.radians(degrees)
    ux, uy, vx, vy = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    return np.array([x0, y0, x0 + length * ux, y0 + length * uy, x0 + length * ux + height * vx, y0 + length * uy + height * vy,
                     x0 + height * vx, y0 + height * vy], np.float32)
