"""The selection-marks rule (DESIGN.md "Selection marks") restated in numpy and Python integers, step by step, independent of tuatara_amd/csrc/marks_rule.h and
geometry.cpp: tests/test_marks_cpu.py holds the host rule to it bit for bit, tests/test_gpu_marks.py the kernels.  It works on a boolean ink mask, not on the
bitmaps' words.  Also the pages both suites share.  Not a test module."""
import numpy as np

CAP = 512
DEFAULTS = (10, 64, 24, 128)      # min_side, max_side, fill, ink


def ink_mask(image, ink):
    """step 1 under the fixed rule: bool [H, W]"""
    return np.asarray(image, np.int32).sum(axis=2) < 3 * int(ink)


def corners_of(m):
    """step 2: bool [H, W] - ink, no ink to the left, no ink above (outside the page is no ink)"""
    left = np.zeros_like(m)
    left[:, 1:] = m[:, :-1]
    up = np.zeros_like(m)
    up[1:, :] = m[:-1, :]
    return m & ~left & ~up


def _run(line, p):
    """the length of the maximal run of True in the 1-D line that starts at p"""
    rest = np.nonzero(~line[p:])[0]
    return int(rest[0]) if len(rest) else len(line) - p


def mark_at(m, x, y, min_side, max_side, fill):
    """steps 3 - 5 on the corner (x, y): the record (label -1) or None"""
    a, b = _run(m[y], x), _run(m[:, x], y)
    if not (min_side <= a <= max_side and min_side <= b <= max_side and 4 * abs(a - b) <= min(a, b)):
        return None
    x1, y1 = x + a - 1, y + b - 1
    if not (m[y1, x:x1 + 1].all() and m[y:y1 + 1, x1].all()):
        return None
    q = min(a, b) // 4
    lines = {"top": [m[y + k, x:x1 + 1] for k in range(q)], "bottom": [m[y1 - k, x:x1 + 1] for k in range(q)],
             "left": [m[y:y1 + 1, x + k] for k in range(q)], "right": [m[y:y1 + 1, x1 - k] for k in range(q)]}
    t = {}
    for side, ls in lines.items():
        n = 0
        while n < q and ls[n].all():
            n += 1
        t[side] = n
    if q in t.values():
        return None
    ix0, ix1, iy0, iy1 = x + t["left"] + 1, x1 - t["right"] - 1, y + t["top"] + 1, y1 - t["bottom"] - 1
    if ix0 > ix1 or iy0 > iy1:
        return None
    inked = int(m[iy0:iy1 + 1, ix0:ix1 + 1].sum())
    area = (ix1 - ix0 + 1) * (iy1 - iy0 + 1)
    return [x, y, x1, y1, ix0, iy0, ix1, iy1, inked, area, 1 if 256 * inked >= fill * area else 0, -1]


def centres_of(quads):
    """64 x the centre of every quad f32 [n, 8], as tables_word_centre forms it: the sums of rint(16 x) over the corners, in integers"""
    q = np.asarray(quads, np.float32).reshape(-1, 4, 2).astype(np.float64)
    return np.rint(16.0 * q).astype(np.int64).sum(axis=1)


def marks_of_mask(m, quads=None, min_side=10, max_side=64, fill=24):
    """steps 2 - 7 on an ink mask -> {"mode", "marks" i32 [n, 12], "item_mark" i32 [nq], "corners", "kept", "bands" i32 [ceil(H / 32), 2]}"""
    h, w = m.shape
    c = corners_of(m)
    recs, bands = [], np.zeros(((h + 31) // 32, 2), np.int32)
    ys, xs = np.nonzero(c)                                    # (row-major: (y, x) order)
    for y, x in zip(ys.tolist(), xs.tolist()):
        bands[y // 32, 1] += 1
        r = mark_at(m, x, y, min_side, max_side, fill)
        if r is not None:
            recs.append(r)
            bands[y // 32, 0] += 1
    cen = centres_of(quads) if quads is not None else np.zeros((0, 2), np.int64)
    nq, kept = len(cen), len(recs)
    item_mark = np.full(nq, -1, np.int32)
    mode = 1
    if kept > CAP:
        mode, recs = -6, []
    for i in range(nq):
        cx, cy = int(cen[i, 0]), int(cen[i, 1])
        for k, r in enumerate(recs):
            if 64 * r[0] <= cx < 64 * (r[2] + 1) and 64 * r[1] <= cy < 64 * (r[3] + 1):
                item_mark[i] = k
                break
    for r in recs:
        a, right, best = r[2] - r[0] + 1, 64 * (r[2] + 1), None
        for i in range(nq):
            cx, cy = int(cen[i, 0]), int(cen[i, 1])
            if item_mark[i] == -1 and 64 * r[1] <= cy < 64 * (r[3] + 1) and 0 <= cx - right <= 64 * 8 * a and (best is None or cx < best[0]):
                best = (cx, i)
        r[11] = -1 if best is None else best[1]
    return {"mode": mode, "marks": np.asarray(recs, np.int32).reshape(-1, 12), "item_mark": item_mark, "corners": int(c.sum()), "kept": kept, "bands": bands}


def marks_ref(image, quads=None, min_side=10, max_side=64, fill=24, ink=128):
    return marks_of_mask(ink_mask(image, ink), quads, min_side, max_side, fill)


# ---- the shared pages (white 255, ink 0)
def blank(h=120, w=160):
    return np.full((h, w, 3), 255, np.uint8)


def frame(img, x, y, side, t=1, side_y=None, v=0):
    """a frame with its top-left corner at (x, y), `side` px wide and side_y (= side) px tall, t px thick"""
    sy = side if side_y is None else side_y
    img[y:y + t, x:x + side] = v
    img[y + sy - t:y + sy, x:x + side] = v
    img[y:y + sy, x:x + t] = v
    img[y:y + sy, x + side - t:x + side] = v
    return img


def cross(img, x, y, n, v=0):
    """both diagonals of the n x n square at (x, y)"""
    for k in range(n):
        img[y + k, x + k] = v
        img[y + k, x + n - 1 - k] = v
    return img


def quad_box(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def hand_page():
    """200 x 300 (w x h): empty frames of side 16, 24, 40 and thickness 1, 2, 3, a 16-px frame holding an 8-px cross, a solid 20-px square"""
    img = blank(300, 200)
    frame(img, 20, 20, 16, 1)
    frame(img, 60, 20, 24, 2)
    frame(img, 110, 20, 40, 3)
    frame(img, 20, 100, 16, 1)
    cross(img, 24, 104, 8)
    img[160:180, 20:40] = 0
    return img


HAND_MARKS = [[20, 20, 35, 35, 22, 22, 33, 33, 0, 144, 0, -1],
              [60, 20, 83, 43, 63, 23, 80, 40, 0, 324, 0, -1],
              [110, 20, 149, 59, 114, 24, 145, 55, 0, 1024, 0, -1],
              [20, 100, 35, 115, 22, 102, 33, 113, 16, 144, 1, -1]]


def grid_with_box():
    """a drawn 3 x 4 grid of 2-px lines with a 14-px box inside its first cell -> (image, the box's frame)"""
    img = blank(180, 220)
    for y in (20, 60, 100, 140):
        img[y:y + 2, 10:192] = 0
    for x in (10, 50, 100, 150, 190):
        img[20:142, x:x + 2] = 0
    frame(img, 22, 32, 14, 1)
    return img, [22, 32, 35, 45]


def box_grid(n, side=8, pitch=10, per_row=32):
    """n boxes of `side` px at `pitch` px, per_row to a row"""
    rows = (n + per_row - 1) // per_row
    img = blank(rows * pitch + 4, per_row * pitch + 4)
    for k in range(n):
        frame(img, 2 + pitch * (k % per_row), 2 + pitch * (k // per_row), side, 1)
    return img


def form_page():
    """a small form without a detector: three boxes down the left, the second one ticked, an `x` item inside it and a label item beside each -> (image, quads)"""
    img = blank(140, 260)
    quads = []
    for k in range(3):
        y = 20 + 36 * k
        frame(img, 16, y, 16, 2)
        quads.append(quad_box(44, y + 2, 100, y + 14))        # the label
    cross(img, 20, 60, 8)
    quads.append(quad_box(19, 59, 29, 69))                    # the `x` the detector would report inside the ticked box
    quads.append(quad_box(120, 22, 200, 34))                  # a second word on the first line, farther away
    return img, np.asarray(quads, np.float32)


def random_page(seed, h=150, w=210):
    """frames of random size, thickness and aspect, some filled, some broken, over sparse noise"""
    rng = np.random.RandomState(seed)
    img = blank(h, w)
    noise = rng.rand(h, w) < 0.01
    img[noise] = 0
    for _ in range(14):
        side, sy = int(rng.randint(7, 40)), None
        if rng.rand() < 0.4:
            sy = max(4, side + int(rng.randint(-6, 7)))
        x, y = int(rng.randint(0, w - side)), int(rng.randint(0, h - (sy or side)))
        if y + (sy or side) > h:
            continue
        frame(img, x, y, side, int(rng.randint(1, 5)), sy)
        if rng.rand() < 0.4:
            n = max(2, side // 2)
            cross(img, x + side // 4, y + side // 4, min(n, (sy or side) // 2))
        if rng.rand() < 0.2:
            img[y, x + side // 2] = 255                       # a broken top side
    quads = [quad_box(x, y, x + 20, y + 8) for x, y in zip(rng.randint(0, w - 20, 12).tolist(), rng.randint(0, h - 8, 12).tolist())]
    return img, np.asarray(quads, np.float32)


def many_bands_page():
    """1300 x 1100 (w x h): 35 bands of 32 rows, a width of 21 words with a ragged last one; boxes of several sizes across band and word boundaries"""
    img = blank(1100, 1300)
    rng = np.random.RandomState(7)
    k = 0
    for y in range(6, 1040, 57):
        for x in range(5, 1240, 83):
            side = 10 + (k * 7) % 50
            if x + side <= 1300 and y + side <= 1100:
                frame(img, x, y, side, 1 + k % 3)
                if k % 4 == 0:
                    cross(img, x + side // 4, y + side // 4, side // 2)
            k += 1
    frame(img, 1300 - 20, 1100 - 20, 20, 1)                   # touching the right and bottom edges
    img[rng.rand(1100, 1300) < 0.002] = 0
    quads = [quad_box(x, y, x + 30, y + 10) for x, y in zip(rng.randint(0, 1260, 40).tolist(), rng.randint(0, 1080, 40).tolist())]
    return img, np.asarray(quads, np.float32)


def shared_pages():
    """name -> (image, quads or None): the pages the stage call is held to the host rule on"""
    g, _ = grid_with_box()
    f, fq = form_page()
    r, rq = random_page(3)
    straddle = frame(blank(60, 200), 58, 10, 17, 1)           # x = 58..74: across the first word boundary
    wide = frame(blank(160, 300), 30, 10, 128, 2)             # x = 30..157: three words
    edges = frame(frame(blank(64, 100), 0, 0, 12, 1), 88, 52, 12, 1)
    return {"hand": (hand_page(), None), "grid": (g, None), "form": (f, fq), "random": (r, rq), "straddle": (straddle, None), "wide": (wide, None),
            "edges": (edges, None), "boxes512": (box_grid(512), None), "boxes513": (box_grid(513), None)}
