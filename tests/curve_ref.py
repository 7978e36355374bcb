"""The curved-word rule (DESIGN.md "Curved words") restated in numpy and Python integers: frame, column statistics, knots, band, decision, knot table,
crop and outline.  The host rule (tuatara_amd/csrc/geometry.cpp) and curve_crop_kernel (curve.hip) must agree with it bit for bit on every integer output."""
from __future__ import annotations

import math

import numpy as np

U, V, S, K = 128, 64, 8, 9
T_INK, G_MIN, HB_MAX, HB_CURVED = 64, 16, V // 2, 3 * V // 8
ROW_MAX = (V - 1) * 256


def tdiv(a: int, b: int) -> int:
    """integer division that truncates toward zero, as C++ does (b > 0)"""
    q = abs(a) // b
    return q if a >= 0 else -q


def frame(quad8):
    """quad f32 [8] tl, tr, br, bl -> int64 [6] = {X0, Ax, Bx, Y0, Ay, By} in 2^-16 px over U columns and V rows: double, one rounding per statement"""
    q = [float(v) for v in np.asarray(quad8, np.float32).ravel()]
    Ax, Ay, Bx, By = (q[2] - q[0]) / float(U), (q[3] - q[1]) / float(U), (q[6] - q[0]) / float(V), (q[7] - q[1]) / float(V)
    X0 = (q[0] + 0.5 * Ax) + 0.5 * Bx
    Y0 = (q[1] + 0.5 * Ay) + 0.5 * By
    return np.rint(np.array([X0, Ax, Bx, Y0, Ay, By], np.float64) * 65536.0).astype(np.int64)


def frame_positions(fr):
    """pass 1: the page positions (px, py) int64 [V + 2, U] in 2^-16 px of frame column u, rows -1..V (one row beyond the quad on either side)"""
    X0, Ax, Bx, Y0, Ay, By = (np.int64(x) for x in fr)
    u, v = np.arange(U, dtype=np.int64)[None, :], np.arange(-1, V + 1, dtype=np.int64)[:, None]
    return X0 + u * Ax + v * Bx, Y0 + u * Ay + v * By


def band_positions(table):
    """pass 2: the same U columns and rows -1..V laid over the band of a knot table: column u at C(u) + ((2 v + 1 - V) H(u)) >> 6"""
    t = [[int(x) for x in row] for row in np.asarray(table)]
    px, py = np.zeros((V + 2, U), np.int64), np.zeros((V + 2, U), np.int64)
    for u in range(U):
        k = 2 * u + 1
        j, f = k >> 5, k & 31
        cx, cy, hx, hy = [(t[j][i] * (32 - f) + t[j + 1][i] * f) >> 5 for i in range(4)]
        for r, v in enumerate(range(-1, V + 1)):
            px[r, u], py[r, u] = cx + (((2 * v + 1 - V) * hx) >> 6), cy + (((2 * v + 1 - V) * hy) >> 6)
    return px, py


def columns(image, px, py):
    """(G, M, first, last) int32 [U] of the columns whose V + 2 rows sit at (px, py): the nearest pixel, clamped to the page"""
    image = np.asarray(image, np.uint8)
    H, W = image.shape[:2]
    ix, iy = (px + 32768) >> 16, (py + 32768) >> 16
    p = image[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)].astype(np.int64)
    y = p[..., 0] + 2 * p[..., 1] + p[..., 2]
    g = np.abs(np.diff(y, axis=0))                              # [V + 1, U]: edge e lies between rows e - 1 and e, at row e - 1/2
    e = np.arange(V + 1, dtype=np.int64)[:, None]
    ink = g > T_INK                                             # an ink edge; weaker steps (paper grain, noise) count for nothing
    g = np.where(ink, g, 0)
    G, M = g.sum(0), ((2 * e + 1) * g).sum(0)
    first = np.where(ink.any(0), ink.argmax(0), -1)
    last = np.where(ink.any(0), V - ink[::-1].argmax(0), -1)
    return G.astype(np.int32), M.astype(np.int32), first.astype(np.int32), last.astype(np.int32)


def spine_at(spine, u: int) -> int:
    """the spine row (1/256 row) at column u: linear between the knots at half-column k = 2 u + 1"""
    k = 2 * u + 1
    j, f = k >> 5, k & 31
    return (int(spine[j]) * (32 - f) + int(spine[j + 1]) * f) >> 5


def knots(G, M, first, last):
    """the statistics -> dict(inked u8 [U], valid u8 [U], own u8 [K], spine int32 [K] (1/256 row), hb): Python integers only"""
    G, M, first, last = ([int(x) for x in a] for a in (G, M, first, last))
    thr = max(G_MIN, sum(G) >> 9)                              # a quarter of the mean column
    inked = [G[u] >= thr and first[u] >= 0 for u in range(U)]
    emax = max([last[u] - first[u] for u in range(U) if inked[u]], default=0)
    valid = [inked[u] and 2 * (last[u] - first[u]) >= emax for u in range(U)]
    r, t, own = [0] * K, [0] * K, [0] * K                       # per window: the mean row (1/256), the mean column (1/16), whether it holds a valid column
    for j in range(K):
        sg = sm = su = 0
        for u in range(max(0, 16 * j - 16), min(U, 16 * j + 16)):
            if valid[u]:
                sg += G[u]; sm += M[u]; su += G[u] * (2 * u + 1)
        if sg:
            r[j], t[j], own[j] = (128 * sm) // sg - 256, (8 * su) // sg, 1
    spine = [0] * K
    for j in range(K):                                          # the window's mean sits at its mean column: carry it to the knot along the neighbours' slope
        if own[j]:
            a, b = j - 1 if j > 0 and own[j - 1] else j, j + 1 if j < K - 1 and own[j + 1] else j
            s = r[j]
            if t[b] > t[a]:
                s += tdiv((256 * j - t[j]) * (r[b] - r[a]), t[b] - t[a])
            spine[j] = min(max(s, 0), ROW_MAX)
    if not any(own):
        return dict(inked=np.array(inked, np.uint8), valid=np.array(valid, np.uint8), own=np.array(own, np.uint8), spine=np.zeros(K, np.int32), hb=0)
    filled = list(spine)
    for j in range(K):
        if not own[j]:
            filled[j] = spine[min((i for i in range(K) if own[i]), key=lambda i: (abs(i - j), i))]
    hb256 = 0
    for u in range(U):
        if inked[u]:
            sp = spine_at(filled, u)
            hb256 = max(hb256, sp - (2 * first[u] - 1) * 128, (2 * last[u] - 1) * 128 - sp)
    hb = min(HB_MAX, ((hb256 + 255) >> 8) + 1)
    return dict(inked=np.array(inked, np.uint8), valid=np.array(valid, np.uint8), own=np.array(own, np.uint8), spine=np.array(filled, np.int32), hb=hb)


def knot_table(C, length, Bx, By):
    """the centres C [K][2] and a half-band length (2^-16 px) -> (table int64 [K, 4] = {Cx, Cy, Hx, Hy}, ok): H is normal to the spine, on B's side; ok = 0
    when a tangent has no length"""
    C = [(int(x), int(y)) for x, y in C]
    out, ok = np.zeros((K, 4), np.int64), 1
    for j in range(K):
        if j == 0:
            tx, ty = [(4 * (C[1][i] - C[0][i]) - (C[2][i] - C[0][i])) >> 8 for i in (0, 1)]
        elif j == K - 1:
            tx, ty = [(4 * (C[8][i] - C[7][i]) - (C[8][i] - C[6][i])) >> 8 for i in (0, 1)]
        else:
            tx, ty = [(C[j + 1][i] - C[j - 1][i]) >> 8 for i in (0, 1)]
        nt = math.isqrt(tx * tx + ty * ty)
        px, py = -ty, tx
        if px * int(Bx) + py * int(By) < 0:
            px, py = -px, -py
        hx = hy = 0
        if nt == 0:
            ok = 0
        else:
            hx, hy = tdiv(px * int(length), nt), tdiv(py * int(length), nt)
        out[j] = (C[j][0], C[j][1], hx, hy)
    return out, ok


def bent(table, length) -> int:
    """1 when a centre lies at least half of `length` off the straight line through the first and the last"""
    t = [[int(x) for x in row] for row in np.asarray(table)]
    ex, ey = (t[8][0] - t[0][0]) >> 8, (t[8][1] - t[0][1]) >> 8
    ne = math.isqrt(ex * ex + ey * ey)
    dev = max(abs(((t[j][0] - t[0][0]) >> 8) * ey - ((t[j][1] - t[0][1]) >> 8) * ex) for j in range(K))
    return int(ne > 0 and 2 * dev >= (int(length) >> 8) * ne)


def word(image, quad8):
    """the whole rule on one quad: dict(frame, flag, hb int32 [2], spine int32 [2, K], table int64 [K, 4], stats1, stats2 (each G, M, first, last), table1)"""
    fr = frame(quad8)
    X0, Ax, Bx, Y0, Ay, By = (int(x) for x in fr)
    out = dict(frame=fr, flag=0, hb=np.zeros(2, np.int32), spine=np.zeros((2, K), np.int32), table=np.zeros((K, 4), np.int64), table1=np.zeros((K, 4), np.int64),
               stats1=columns(image, *frame_positions(fr)), stats2=None)
    k1 = knots(*out["stats1"])
    out["hb"][0], out["spine"][0] = k1["hb"], k1["spine"]
    if int(k1["own"].sum()) < 3:
        return out
    C1 = [(X0 + (((32 * j - 1) * Ax) >> 1) + ((int(k1["spine"][j]) * Bx) >> 8), Y0 + (((32 * j - 1) * Ay) >> 1) + ((int(k1["spine"][j]) * By) >> 8)) for j in range(K)]
    L = math.isqrt(Bx * Bx + By * By)
    t1, ok1 = knot_table(C1, k1["hb"] * L, Bx, By)
    out["table1"] = t1
    if not ok1:
        return out
    out["stats2"] = columns(image, *band_positions(t1))
    k2 = knots(*out["stats2"])
    out["hb"][1], out["spine"][1] = k2["hb"], k2["spine"]
    if int(k2["own"].sum()) < 3:
        return out
    mid = (V - 1) * 128                                         # the band's middle row, V / 2 - 1 / 2, in 1/256 row
    C2 = [(int(t1[j][0]) + (((int(k2["spine"][j]) - mid) * int(t1[j][2])) >> 13), int(t1[j][1]) + (((int(k2["spine"][j]) - mid) * int(t1[j][3])) >> 13)) for j in range(K)]
    L2 = (k1["hb"] * k2["hb"] * L) >> 5
    t2, ok2 = knot_table(C2, L2, Bx, By)
    out["table"] = t2
    out["flag"] = int(ok2 and k1["hb"] * k2["hb"] <= 32 * HB_CURVED and bent(t2, L2))
    return out


def positions(table):
    """the page positions (sx, sy) int64 [32, 128] in 2^-16 px that the crop's pixels sample"""
    t = [[int(x) for x in row] for row in np.asarray(table)]
    sx, sy = np.zeros((32, U), np.int64), np.zeros((32, U), np.int64)
    for u in range(U):
        k = 2 * u + 1
        j, f = k >> 5, k & 31
        cx, cy, hx, hy = ((t[j][i] * (32 - f) + t[j + 1][i] * f) >> 5 for i in range(4))
        for v in range(32):
            sx[v, u], sy[v, u] = cx + (((2 * v + 1 - 32) * hx) >> 5), cy + (((2 * v + 1 - 32) * hy) >> 5)
    return sx, sy


def sample_at(image, sx, sy):
    """the kind-1 sampler's arithmetic at given positions"""
    image = np.asarray(image, np.uint8)
    H, W = image.shape[:2]
    ix, iy = sx >> 16, sy >> 16
    fx, fy = ((sx >> 5) & 2047)[..., None], ((sy >> 5) & 2047)[..., None]
    x0, x1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
    y0, y1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    img = image.astype(np.int64)
    top = (2048 - fx) * img[y0, x0] + fx * img[y0, x1]
    bot = (2048 - fx) * img[y1, x0] + fx * img[y1, x1]
    return np.clip(((2048 - fy) * top + fy * bot + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def crop(image, table):
    return sample_at(image, *positions(table))


def outline(quad8, flag, table):
    """f32 [18, 2]: the top edge left to right, then the bottom edge right to left"""
    if flag:
        t = np.asarray(table, np.int64).astype(np.float64) / 65536.0
        top, bot = t[:, 0:2] - t[:, 2:4], t[:, 0:2] + t[:, 2:4]
    else:
        q = np.asarray(quad8, np.float32).astype(np.float64).reshape(4, 2)
        s = (np.arange(K, dtype=np.float64) / float(S))[:, None]
        top, bot = q[0] + s * (q[1] - q[0]), q[3] + s * (q[2] - q[3])
    return np.concatenate([top, bot[::-1]]).astype(np.float32)


def quad_of(cx, cy, length, height, degrees=0.0):
    """a length x height rectangle centred on (cx, cy) whose baseline runs at `degrees`: f32 [8] tl, tr, br, bl"""
    a = math.radians(degrees)
    ux, uy, vx, vy = math.cos(a), math.sin(a), -math.sin(a), math.cos(a)
    c = [(-length / 2, -height / 2), (length / 2, -height / 2), (length / 2, height / 2), (-length / 2, height / 2)]
    return np.array([v for (a_, b_) in c for v in (cx + a_ * ux + b_ * vx, cy + a_ * uy + b_ * vy)], np.float32)


def arc_word(n_bars, bar_h, sagitta, chord, degrees=0.0, up=True, dark=True, size=256, ink=0.6):
    """A page of `size` x `size` holding one word of n_bars equal bars set on a circular arc, as glyphs sit on a curved baseline: every bar is bar_h tall
    along the arc's normal and covers `ink` of its share of the arc; the arc's chord is `chord` px long at `degrees` and its sagitta `sagitta` px; up: the
    middle of the word rides above its ends.  Returns (image u8, quad f32 [8]): the quad is the tight rectangle over the whole word in the chord's frame, as
    minAreaRect would box it."""
    R = (chord * chord / 4.0 + sagitta * sagitta) / (2.0 * sagitta)
    half = math.asin(chord / 2.0 / R)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    a = math.radians(degrees)
    ca, sa = math.cos(a), math.sin(a)
    c0 = size / 2.0
    lx, ly = (xx - c0) * ca + (yy - c0) * sa, -(xx - c0) * sa + (yy - c0) * ca          # the chord's frame: x along the chord, y down
    sgn = 1.0 if up else -1.0
    oy = sgn * (R - sagitta / 2.0)                                                       # the circle's centre: below the word when it arches up
    r = np.hypot(lx, ly - oy)
    th = np.arctan2(lx, -sgn * (ly - oy))                                                # 0 at the apex, growing along x
    pitch = (2.0 * half) / (n_bars - 1 + ink)                                            # the last bar ends where the arc does
    inside = (np.abs(r - R) <= bar_h / 2.0) & (np.abs(th) <= half) & (((th + half) % pitch) <= ink * pitch)
    fg, bg = (20, 235) if dark else (235, 20)
    img = np.where(inside[..., None], fg, bg).astype(np.uint8).repeat(3, 2)
    pts = np.argwhere(inside)
    lxs, lys = lx[pts[:, 0], pts[:, 1]], ly[pts[:, 0], pts[:, 1]]
    x0, x1, y0, y1 = lxs.min() - 0.5, lxs.max() + 0.5, lys.min() - 0.5, lys.max() + 0.5
    corners = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    quad = np.array([v for (px, py) in corners for v in (c0 + px * ca - py * sa, c0 + px * sa + py * ca)], np.float32)
    return np.ascontiguousarray(img), quad


def ink_centroid(crop_u8, dark=True):
    """the per-column ink centroid of a crop u8 [32, 128, 3] in crop rows (pixel centres at v + 0.5) over the columns inside a bar, NaN elsewhere: a column
    counts when it and both its neighbours hold at least half the ink of the fullest column - the column at a bar's side holds a sliver of the bar's
    height, cut by the sampling grid, and says nothing about where the bar sits"""
    y = crop_u8.astype(np.float64).sum(-1) / 3.0
    m = (235.0 - y) / 215.0 if dark else (y - 20.0) / 215.0
    m = np.where(m >= 0.5, np.clip(m, 0.0, 1.0), 0.0)
    s = m.sum(0)
    full = 2.0 * s >= s.max()
    core = full & np.concatenate([[False], full[:-1]]) & np.concatenate([full[1:], [False]])
    rows = (np.arange(32, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(core & (s > 0), (m * rows).sum(0) / s, np.nan)
