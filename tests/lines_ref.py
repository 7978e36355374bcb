"""numpy restatement of the text-line rule (DESIGN.md "Text lines"), written from the rule and not from the C++.  Integer arithmetic only
(int64 numpy / python ints), so every comparison against the engine is exact.

    lines_from_quads(quads [n, 8] f32) -> (line i32 [n], word i32 [n], n_lines)
    reading_order(line, word, n_lines)  -> (order i32 [n], line_first i32 [n_lines + 1])
    line_bboxes / line_texts / page_text: the outputs derived from them

plus the layout builders the tests share (rectangle quads from centre, size and angle; rows of words from widths, a height and a gap)."""
import numpy as np


def fixed(quads):
    """[n, 8] f32 (tl, tr, br, bl) -> int64 [n, 4, 2] = llrint(16 x) (round half to even, as llrint in the default rounding mode)"""
    q = np.asarray(quads, np.float32).reshape(-1, 4, 2).astype(np.float64)
    if not np.all(np.isfinite(q)) or np.any(np.abs(q) >= 32768):
        raise ValueError("coordinate not finite or |x| >= 32768")
    return np.rint(16.0 * q).astype(np.int64)


def cuv(quads):
    p = fixed(quads)
    tl, tr, br, bl = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    return tl + tr + br + bl, (tr - tl) + (br - bl), (bl - tl) + (br - tr)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]


def _cross(a, b):
    return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]


def link_matrix(quads):
    """bool [n, n]: the symmetric link relation of the rule (step 3)"""
    c, u, v = cuv(quads)
    n = len(c)
    uu, vv, A = _dot(u, u), _dot(v, v), np.abs(_cross(u, v))
    ok = (uu != 0) & (vv != 0) & (A != 0)
    ui, uj = u[:, None, :], u[None, :, :]
    vi, vj = v[:, None, :], v[None, :, :]
    d = c[None, :, :] - c[:, None, :]                 # d[i, j] = c_j - c_i
    dot = _dot(ui, uj)
    same_dir = (dot > 0) & (64 * np.abs(_cross(ui, uj)) <= 17 * dot)
    height = (vv[:, None] <= 4 * vv[None, :]) & (vv[None, :] <= 4 * vv[:, None])
    band = np.abs(_dot(d, vi)) <= vv[:, None]         # in i's frame
    s = _dot(d, ui)
    e = np.abs(_dot(uj, ui)) + np.abs(_dot(vj, ui))
    gap = np.maximum(s - e - uu[:, None], -s - e - uu[:, None])
    near = gap <= 2 * A[:, None]
    frame = band & near
    L = ok[:, None] & ok[None, :] & same_dir & height & frame & frame.T
    L[np.arange(n), np.arange(n)] = False
    return L


def lines_from_quads(quads):
    quads = np.asarray(quads, np.float32).reshape(-1, 8)
    n = len(quads)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), 0
    c, u, _ = cuv(quads)
    L = link_matrix(quads)
    comp = np.full(n, -1, np.int64)                   # the line's smallest member
    for i in range(n):
        if comp[i] >= 0:
            continue
        comp[i] = i
        todo = [i]
        while todo:
            a = todo.pop()
            for b in np.flatnonzero(L[a] & (comp < 0)):
                comp[b] = i
                todo.append(int(b))
    word = np.zeros(n, np.int32)
    firsts = []
    for r in np.unique(comp):
        m = np.flatnonzero(comp == r)
        U = [int(u[m, 0].sum()), int(u[m, 1].sum())]
        keys = sorted((int(c[i, 0]) * U[0] + int(c[i, 1]) * U[1], int(i)) for i in m)
        for k, (_, i) in enumerate(keys):
            word[i] = k
        firsts.append(keys[0][1])
    firsts.sort(key=lambda f: (int(c[f, 1]), int(c[f, 0]), f))
    line = np.zeros(n, np.int32)
    for l, f in enumerate(firsts):
        line[comp == comp[f]] = l
    return line, word, len(firsts)


def reading_order(line, word, n_lines):
    n = len(line)
    line_first = np.zeros(n_lines + 1, np.int32)
    np.add.at(line_first, np.asarray(line, np.int64) + 1, 1)
    line_first = np.cumsum(line_first).astype(np.int32)
    order = np.full(n, -1, np.int32)
    for i in range(n):
        order[line_first[line[i]] + word[i]] = i
    return order, line_first


def line_bboxes(bbox, order, line_first):
    bbox = np.asarray(bbox, np.float32).reshape(-1, 4)
    out = np.zeros((len(line_first) - 1, 4), np.float32)
    for l in range(len(line_first) - 1):
        m = order[line_first[l]:line_first[l + 1]]
        out[l] = [bbox[m, 0].min(), bbox[m, 1].min(), bbox[m, 2].max(), bbox[m, 3].max()]
    return out


def line_texts(texts, order, line_first):
    return [" ".join(texts[i] for i in order[line_first[l]:line_first[l + 1]]) for l in range(len(line_first) - 1)]


def page_text(texts, order, line_first):
    return "\n".join(line_texts(texts, order, line_first))


# ---- layouts
def rect_quad(cx, cy, w, h, deg=0.0):
    """the corners tl, tr, br, bl of a w x h rectangle centred at (cx, cy) whose baseline is turned by deg (clockwise on screen, y down) -> [8]"""
    a = np.deg2rad(deg)
    ux, uy = np.cos(a) * w / 2, np.sin(a) * w / 2     # half the width vector
    vx, vy = -np.sin(a) * h / 2, np.cos(a) * h / 2    # half the height vector (down)
    return np.array([cx - ux - vx, cy - uy - vy, cx + ux - vx, cy + uy - vy, cx + ux + vx, cy + uy + vy, cx - ux + vx, cy - uy + vy], np.float32)


def row_quads(x0, y0, widths, h, gap, deg=0.0):
    """words of the given widths and height h along a baseline through (x0, y0) turned by deg, `gap` apart -> [len(widths), 8]"""
    a = np.deg2rad(deg)
    out, t = [], 0.0
    for w in widths:
        m = t + w / 2
        out.append(rect_quad(x0 + np.cos(a) * m, y0 + np.sin(a) * m, w, h, deg))
        t += w + gap
    return np.array(out, np.float32).reshape(-1, 8)


def random_quads(n, seed):
    """n quads on a 2000 x 1400 page: rows of rectangles at a few angles and sizes (so that links exist), loose rectangles at any angle,
    some degenerate quads (a point, a segment, zero height) and some non-rectangular ones (jittered corners)"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        kind = rng.integers(0, 10)
        if kind < 6:                                   # a row of words
            h = float(rng.choice([12, 18, 24, 40]))
            deg = float(rng.choice([0, 0, 0, 7, -12, 25, 90, 180]))
            widths = rng.uniform(1.0, 6.0, rng.integers(1, 9)) * h
            out.extend(row_quads(rng.uniform(50, 1500), rng.uniform(50, 1300), widths, h, float(rng.uniform(0.2, 1.4)) * h, deg))
        elif kind < 8:                                 # a loose rectangle
            out.append(rect_quad(rng.uniform(0, 2000), rng.uniform(0, 1400), rng.uniform(5, 300), rng.uniform(5, 80), rng.uniform(-180, 180)))
        elif kind == 8:                                # degenerate
            x, y = rng.uniform(0, 2000, 2)
            out.append([[x, y] * 4, [x, y, x + 30, y, x + 30, y, x, y], [x, y, x, y, x, y + 9, x, y + 9]][rng.integers(0, 3)])
        else:                                          # not a rectangle
            q = rect_quad(rng.uniform(0, 2000), rng.uniform(0, 1400), rng.uniform(20, 200), rng.uniform(10, 50), rng.uniform(-40, 40))
            out.append(q + rng.uniform(-6, 6, 8).astype(np.float32))
    q = np.array([np.asarray(v, np.float32) for v in out[:n]], np.float32).reshape(-1, 8)
    return q[rng.permutation(len(q))] if n else q
