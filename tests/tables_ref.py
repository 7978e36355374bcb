"""The tables rule (DESIGN.md "Tables") restated in numpy and Python integers, step by step, independent of tuatara_amd/csrc/tables_rule.h and geometry.cpp:
tests/test_tables_cpu.py holds the host rule to it bit for bit, tests/test_gpu_tables.py the two kernels.  Not a test module."""
import numpy as np

R, J = 12, 6
RUN_CAP, RULING_CAP, TABLE_CAP, LINE_CAP, CELL_CAP = 8192, 256, 32, 64, 1024


def ink_mask(image, ink):
    """step 1: bool [H, W]"""
    return np.asarray(image, np.int32).sum(axis=2) < 3 * int(ink)


def ink_bits(image, ink):
    """the bitmap as the kernels store it: uint64 [H, ceil(W / 64)], bit x % 64 of word x // 64"""
    m = ink_mask(image, ink)
    h, w = m.shape
    nw = (w + 63) // 64
    pad = np.zeros((h, nw * 64), np.uint8)
    pad[:, :w] = m
    return np.packbits(pad.reshape(h, nw, 8, 8)[:, :, :, ::-1], axis=3).reshape(h, nw, 8).copy().view("<u8").reshape(h, nw)


def runs_of(mask):
    """step 2 on rows: [(y, x0, x1)] in (y, x0) order; the vertical runs are runs_of(mask.T) as (x, y0, y1)"""
    out = []
    for y in range(mask.shape[0]):
        row = np.concatenate(([0], mask[y].astype(np.int8), [0]))
        d = np.diff(row)
        for a, b in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]):
            if b - a >= R:
                out.append((y, int(a), int(b) - 1))
    return out


class _UF:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, i):
        while self.p[i] != i:
            i = self.p[i]
        return i

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        if a < b:
            self.p[b] = a
        else:
            self.p[a] = b
        return True


def rulings_of(runs, min_len, direction):
    """steps 3 - 4 on one direction's runs -> [[dir, x0, y0, x1, y1]] by root, or None beyond the cap"""
    n = len(runs)
    uf = _UF(n)
    by_line = {}
    for i, (l, a, b) in enumerate(runs):
        by_line.setdefault(l, []).append(i)
    for i, (l, a0, a1) in enumerate(runs):
        for k in by_line.get(l + 1, ()):
            _, b0, b1 = runs[k]
            if a0 <= b1 + 1 and b0 <= a1 + 1:
                uf.union(i, k)
    comp = {}
    for i in range(n):
        comp.setdefault(uf.find(i), []).append(i)
    out = []
    for root in sorted(comp):
        mem = [runs[i] for i in comp[root]]
        amin, amax = min(m[1] for m in mem), max(m[2] for m in mem)
        lmin, lmax = min(m[0] for m in mem), max(m[0] for m in mem)
        L, T, A = amax - amin + 1, lmax - lmin + 1, sum(m[2] - m[1] + 1 for m in mem)
        if L >= min_len and 8 * T <= L and A <= 16 * L:
            out.append([0, amin, lmin, amax, lmax] if direction == 0 else [1, lmin, amin, lmax, amax])
    return out if len(out) <= RULING_CAP else None


def _chain(members, key):
    """step 6 on one axis: members sorted by (key, index) -> (positions, {member: line})"""
    order = sorted(members, key=lambda r: (key[r], r))
    pos, line_of, lo = [], {}, None
    for k, r in enumerate(order):
        if k == 0 or key[r] - key[order[k - 1]] > 2 * J:
            lo = key[r]
            pos.append(lo)
        pos[-1] = (lo + key[r]) // 2
        line_of[r] = len(pos) - 1
    return pos, line_of


def _empty(mode, nq):
    return {"mode": mode, "rulings": np.zeros((0, 6), np.int32), "tables": np.zeros((0, 8), np.int32), "lines": np.zeros(0, np.int32),
            "cells": np.zeros((0, 9), np.int32), "item_table": np.full(nq, -1, np.int32), "item_cell": np.full(nq, -1, np.int32), "line_lists": []}


def centre64(quad):
    """step 8: (cx, cy) = 64 x the centre: the sums of llrint(16 x) (round half to even, as llrint under the default rounding mode)"""
    q = np.asarray(quad, np.float32).astype(np.float64).reshape(4, 2)
    r = np.rint(16.0 * q).astype(np.int64)
    return int(r[:, 0].sum()), int(r[:, 1].sum())


def tables_ref(image, quads=None, min_len=48, ink=128):
    """the whole rule -> the dict engine.tables_from_page returns (plus "line_lists": per table (row lines, column lines))"""
    quads = np.zeros((0, 8), np.float32) if quads is None else np.asarray(quads, np.float32).reshape(-1, 8)
    nq = len(quads)
    mask = ink_mask(image, ink)
    runs_h, runs_v = runs_of(mask), runs_of(mask.T)
    if len(runs_h) > RUN_CAP or len(runs_v) > RUN_CAP:
        return _empty(-2, nq)
    H, V = rulings_of(runs_h, min_len, 0), rulings_of(runs_v, min_len, 1)
    if H is None or V is None:
        return _empty(-4, nq)
    rul = [r + [-1] for r in H + V]
    nh, n = len(H), len(H) + len(V)
    uf = _UF(n)
    for a in range(nh):                                      # step 5
        for b in range(nh, n):
            h, v = rul[a], rul[b]
            if v[1] - J <= h[3] and h[1] <= v[3] + J and h[2] - J <= v[4] and v[2] <= h[4] + J:
                uf.union(a, b)
    comp = {}
    for r in range(n):
        comp.setdefault(uf.find(r), []).append(r)
    key = [r[2] + r[4] if r[0] == 0 else r[1] + r[3] for r in rul]
    cand = []                                                # step 6
    for root in sorted(comp):
        hs, vs = [r for r in comp[root] if r < nh], [r for r in comp[root] if r >= nh]
        if len(hs) < 2 or len(vs) < 2:
            continue
        Y, row_of = _chain(hs, key)
        X, col_of = _chain(vs, key)
        if len(Y) > LINE_CAP or len(X) > LINE_CAP:
            return _empty(-6, nq)
        if len(Y) < 2 or len(X) < 2:
            continue
        mem = [rul[r] for r in comp[root]]
        box = [min(m[1] for m in mem), min(m[2] for m in mem), max(m[3] for m in mem), max(m[4] for m in mem)]
        cand.append((box[1], box[0], root, box, Y, X, row_of, col_of, hs, vs))
    if len(cand) > TABLE_CAP:
        return _empty(-6, nq)
    cand.sort(key=lambda c: c[:3])
    tables, lines, cells, line_lists = [], [], [], []
    for t, (_, _, root, box, Y, X, row_of, col_of, hs, vs) in enumerate(cand):
        for r in comp[root]:
            rul[r][5] = t
        rows, cols = len(Y) - 1, len(X) - 1
        uf = _UF(rows * cols)                                # step 7
        for i in range(rows):
            for j in range(cols):
                if j + 1 < cols:
                    mid = (Y[i] + Y[i + 1]) // 2
                    if not any(col_of[v] == j + 1 and 2 * (rul[v][2] - J) <= mid <= 2 * (rul[v][4] + J) for v in vs):
                        uf.union(i * cols + j, i * cols + j + 1)
                if i + 1 < rows:
                    mid = (X[j] + X[j + 1]) // 2
                    if not any(row_of[h] == i + 1 and 2 * (rul[h][1] - J) <= mid <= 2 * (rul[h][3] + J) for h in hs):
                        uf.union(i * cols + j, (i + 1) * cols + j)
        while True:                                          # a component that is not a rectangle takes in its bounding box
            box_of = {}
            for b in range(rows * cols):
                r = uf.find(b)
                i, j = divmod(b, cols)
                q = box_of.setdefault(r, [i, i, j, j])
                q[0], q[1], q[2], q[3] = min(q[0], i), max(q[1], i), min(q[2], j), max(q[3], j)
            changed = False
            for r in sorted(box_of):
                q = box_of[r]
                for i in range(q[0], q[1] + 1):
                    for j in range(q[2], q[3] + 1):
                        changed = uf.union(r, i * cols + j) or changed
            if not changed:
                break
        first = len(cells)
        for r in sorted(box_of):
            q = box_of[r]
            cells.append([t, q[0], q[2], q[1] - q[0] + 1, q[3] - q[2] + 1, X[q[2]] // 2, Y[q[0]] // 2, X[q[3] + 1] // 2, Y[q[1] + 1] // 2])
        if len(cells) > CELL_CAP:
            return _empty(-7, nq)
        tables.append(box + [rows, cols, first, len(cells) - first])
        lines += Y + X
        line_lists.append((np.array(Y, np.int32), np.array(X, np.int32)))
    item_table, item_cell = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
    for k in range(nq):                                      # step 8
        cx, cy = centre64(quads[k])
        for t, T in enumerate(tables):
            Y, X = line_lists[t]
            if not (32 * int(X[0]) <= cx < 32 * int(X[-1]) and 32 * int(Y[0]) <= cy < 32 * int(Y[-1])):
                continue
            i = max(a for a in range(len(Y) - 1) if 32 * int(Y[a]) <= cy)
            j = max(a for a in range(len(X) - 1) if 32 * int(X[a]) <= cx)
            for c in range(T[6], T[6] + T[7]):
                q = cells[c]
                if q[1] <= i < q[1] + q[3] and q[2] <= j < q[2] + q[4]:
                    item_table[k], item_cell[k] = t, c
            break
    return {"mode": 1, "rulings": np.array(rul, np.int32).reshape(-1, 6), "tables": np.array(tables, np.int32).reshape(-1, 8), "lines": np.array(lines, np.int32),
            "cells": np.array(cells, np.int32).reshape(-1, 9), "item_table": item_table, "item_cell": item_cell, "line_lists": line_lists}


# ---- the pages the two test modules share
def blank(h=160, w=200):
    return np.full((h, w, 3), 255, np.uint8)


def hline(img, y, x0, x1, t=2, v=0):
    img[y:y + t, x0:x1 + 1] = v


def vline(img, x, y0, y1, t=2, v=0):
    img[y0:y1 + 1, x:x + t] = v


GRID_ROWS, GRID_COLS = (20, 60, 100, 140), (10, 50, 100, 150, 190)   # a 3 x 4 grid of 2-px lines on a 200 x 160 page


def grid_page(colspan=False, rowspan=False):
    img = blank()
    for y in GRID_ROWS:
        hline(img, y, GRID_COLS[0], GRID_COLS[-1] + 1)
    for x in GRID_COLS:
        vline(img, x, GRID_ROWS[0], GRID_ROWS[-1] + 1)
    if colspan:      # cells (0, 1) and (0, 2) become one
        img[GRID_ROWS[0] + 2:GRID_ROWS[1], GRID_COLS[2]:GRID_COLS[2] + 2] = 255
    if rowspan:      # cells (1, 0) and (2, 0) become one
        img[GRID_ROWS[2]:GRID_ROWS[2] + 2, GRID_COLS[0] + 2:GRID_COLS[1]] = 255
    return img


def grid_words():
    """one 20 x 10 word in the middle of every base cell of grid_page, row-major: f32 [12, 8]"""
    q = []
    for i in range(3):
        for j in range(4):
            cx, cy = (GRID_COLS[j] + GRID_COLS[j + 1]) / 2 + 1, (GRID_ROWS[i] + GRID_ROWS[i + 1]) / 2 + 1
            q.append([cx - 10, cy - 5, cx + 10, cy - 5, cx + 10, cy + 5, cx - 10, cy + 5])
    return np.array(q, np.float32)


def rotated_grid(deg, h=200, w=240):
    """the grid drawn rotated by deg degrees about the page centre on a larger page (nearest pixel of the inverse map), and its words rotated alike"""
    src = np.full((h, w, 3), 255, np.uint8)
    ox, oy = (w - 200) // 2, (h - 160) // 2
    src[oy:oy + 160, ox:ox + 200] = grid_page()
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    dx, dy = xx - w / 2, yy - h / 2
    sx, sy = np.rint(c * dx + s * dy + w / 2).astype(int), np.rint(-s * dx + c * dy + h / 2).astype(int)
    ok = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    out = np.full_like(src, 255)
    out[ok] = src[sy[ok], sx[ok]]
    q = grid_words().reshape(-1, 4, 2).astype(np.float64) + [ox, oy]
    qx, qy = q[..., 0] - w / 2, q[..., 1] - h / 2
    rq = np.stack([c * qx - s * qy + w / 2, s * qx + c * qy + h / 2], axis=-1)
    return out, rq.reshape(-1, 8).astype(np.float32)


def two_tables_page():
    img = blank(160, 200)
    for y in (10, 40, 70):
        hline(img, y, 10, 91)
    for x in (10, 50, 90):
        vline(img, x, 10, 71)
    for y in (90, 120, 150):
        hline(img, y, 110, 191)
    for x in (110, 150, 190):
        vline(img, x, 90, 151)
    hline(img, 84, 10, 80, t=1)     # a loose underline
    return img


def dashes_page():
    """12-px dashes, 25 on each of 400 rows: 10000 horizontal runs, beyond the run cap"""
    img = blank(400, 400)
    for x in range(0, 400 - 12, 16):
        img[:, x:x + 12] = 0
    return img


def two_caps_page():
    """beyond two caps at once: 300 thin horizontal rulings (every second row, x = 4..35) and about 19 000 vertical runs (dashes of 12 on, 4 off at x =
    100..599).  The runs of both directions are counted before any ruling is formed: mode -2, not -4"""
    img = blank(600, 700)
    img[0:600:2, 4:36] = 0
    for y in range(0, 600 - 12, 16):
        img[y:y + 12, 100:600] = 0
    return img


def many_lines_page():
    """one table of 66 row lines (8 px apart, 1 px thick) and 2 column lines: beyond 64 lines per axis, mode -6"""
    img = blank(540, 100)
    for i in range(66):
        img[4 + 8 * i, 10:90] = 0
    img[4:4 + 8 * 65 + 1, 10] = 0
    img[4:4 + 8 * 65 + 1, 89] = 0
    return img


def many_tables_page():
    """36 tables of 2 x 2 lines, 40 px apart: beyond 32 tables, mode -6"""
    img = blank(250, 250)
    for ty in range(6):
        for tx in range(6):
            y, x = 5 + 40 * ty, 5 + 40 * tx
            img[y, x:x + 21] = 0
            img[y + 20, x:x + 21] = 0
            img[y:y + 21, x] = 0
            img[y:y + 21, x + 20] = 0
    return img


def many_cells_page():
    """one grid of 34 x 34 cells (35 lines per axis, 8 px apart): 1156 cells, beyond 1024, mode -7"""
    img = blank(290, 290)
    for i in range(35):
        img[5 + 8 * i, 5:5 + 8 * 34 + 1] = 0
        img[5:5 + 8 * 34 + 1, 5 + 8 * i] = 0
    return img


def random_page(seed, h=96, w=150, p=0.7):
    rng = np.random.default_rng(seed)
    img = np.where(rng.random((h, w, 1)) < p, 0, 255).astype(np.uint8).repeat(3, axis=2)
    for _ in range(6):              # some long lines, so that rulings, tables and cells do occur
        if rng.random() < 0.5:
            y, x0 = int(rng.integers(0, h - 2)), int(rng.integers(0, w // 3))
            img[y - 1:y + 2] = 255
            img[y, x0:int(rng.integers(x0 + 40, w))] = 0
        else:
            x, y0 = int(rng.integers(0, w - 2)), int(rng.integers(0, h // 3))
            img[:, max(x - 1, 0):x + 2] = 255
            img[y0:int(rng.integers(y0 + 40, h)), x] = 0
    return img


def random_quads(seed, n, h, w):
    rng = np.random.default_rng(seed + 1000)
    cx, cy = rng.uniform(0, w, n), rng.uniform(0, h, n)
    return np.stack([cx - 6, cy - 3, cx + 6, cy - 3, cx + 6, cy + 3, cx - 6, cy + 3], axis=1).astype(np.float32)


def same(a, b):
    """two result dicts agree in every output"""
    return (a["mode"] == b["mode"] and all(np.array_equal(a[k], b[k]) and a[k].shape == b[k].shape for k in ("rulings", "tables", "lines", "cells", "item_table", "item_cell")))
