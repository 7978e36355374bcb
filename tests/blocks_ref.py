"""numpy restatement of the text-block rule (DESIGN.md "Text blocks"), written from the rule and not from the C++.  Integer arithmetic only
(python ints / int64 numpy), so every comparison against the engine is exact.

    blocks_from_quads(quads [n, 8] f32) -> (line, word, n_lines, block i32 [n_lines], pos i32 [n_lines], n_blocks, mode)
    blocks_from_lines(quads, line, word, n_lines) -> (block, pos, n_blocks, mode)
    block_order / block_bboxes / block_texts / page_text_blocks: the outputs derived from them

plus the layout builders the tests share (paragraphs of words in rows, pages of columns)."""
import numpy as np

from tests import lines_ref as L

CAP = 512


def _tdiv(a: int, m: int) -> int:
    """C's truncating division"""
    return abs(a) // m if a >= 0 else -(abs(a) // m)


def descriptors(quads, line, word, n_lines):
    """per line: C (8 x the centre), D (4 x the axis vector), H (2 x the mean height vector) as python-int pairs, and ok"""
    c, u, v = L.cuv(quads)
    out = []
    for l in range(n_lines):
        m = np.flatnonzero(line == l)
        f, e = int(m[word[m] == 0][0]), int(m[word[m] == len(m) - 1][0])
        a = [int(c[f, k]) - int(u[f, k]) for k in (0, 1)]
        b = [int(c[e, k]) + int(u[e, k]) for k in (0, 1)]
        C = (a[0] + b[0], a[1] + b[1])
        D = (b[0] - a[0], b[1] - a[1])
        H = tuple(_tdiv(sum(int(x) for x in v[m, k]), len(m)) for k in (0, 1))
        DD, HH, X = D[0] * D[0] + D[1] * D[1], H[0] * H[0] + H[1] * H[1], abs(D[0] * H[1] - D[1] * H[0])
        out.append({"C": C, "D": D, "H": H, "DD": DD, "HH": HH, "ok": DD != 0 and HH != 0 and X != 0})
    return out


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1]


def _frame(A, B):
    d = (B["C"][0] - A["C"][0], B["C"][1] - A["C"][1])
    if abs(_dot(d, A["H"])) > 9 * A["HH"]:
        return False
    s, e = _dot(d, A["D"]), abs(_dot(B["D"], A["D"]))
    return min(A["DD"], s + e) - max(-A["DD"], s - e) >= min(A["DD"], e)


def link(A, B):
    if not (A["ok"] and B["ok"]):
        return False
    dot = _dot(A["D"], B["D"])
    if not (dot > 0 and 64 * abs(A["D"][0] * B["D"][1] - A["D"][1] * B["D"][0]) <= 17 * dot):
        return False
    if not (4 * A["HH"] <= 9 * B["HH"] and 4 * B["HH"] <= 9 * A["HH"]):
        return False
    return _frame(A, B) and _frame(B, A)


def precedence(x0, x1, cy):
    """bool [nb, nb]: P[a, b] = block a precedes block b (step 6); cy: one sortable tuple per block"""
    nb = len(x0)
    x0, x1 = np.asarray(x0, np.int64), np.asarray(x1, np.int64)
    rank = np.zeros(nb, np.int64)
    rank[sorted(range(nb), key=lambda b: cy[b])] = np.arange(nb)
    xov = (x0[:, None] < x1[None, :]) & (x0[None, :] < x1[:, None])
    P = xov & (rank[:, None] < rank[None, :])
    for a in range(nb):
        left = x1[a] <= x0                                                    # a left of b
        lo, hi = np.minimum(rank[a], rank), np.maximum(rank[a], rank)         # per b
        between = (rank[None, :] > lo[:, None]) & (rank[None, :] < hi[:, None])   # [b, s]
        spanned = (between & xov[None, :, a] & xov.T).any(axis=1)            # xov[s, a] and xov[s, b]
        P[a] |= left & ~spanned
    P[np.arange(nb), np.arange(nb)] = False
    return P


def blocks_from_lines(quads, line, word, n_lines):
    quads = np.asarray(quads, np.float32).reshape(-1, 8)
    line, word = np.asarray(line, np.int64), np.asarray(word, np.int64)
    if n_lines == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), 0, 1
    Ls = descriptors(quads, line, word, n_lines)
    # components
    comp = [-1] * n_lines
    for i in range(n_lines):
        if comp[i] >= 0:
            continue
        comp[i] = i
        todo = [i]
        while todo:
            a = todo.pop()
            for b in range(n_lines):
                if comp[b] < 0 and link(Ls[a], Ls[b]):
                    comp[b] = i
                    todo.append(b)
    comp = np.array(comp)
    roots = [int(r) for r in np.unique(comp)]
    pos = np.zeros(n_lines, np.int32)
    for r in roots:
        m = np.flatnonzero(comp == r)
        Hs = (sum(Ls[l]["H"][0] for l in m), sum(Ls[l]["H"][1] for l in m))
        for k, (_, l) in enumerate(sorted((_dot(Ls[l]["C"], Hs), int(l)) for l in m)):
            pos[l] = k
    # boxes over the blocks' words
    c, u, v = L.cuv(quads)
    ext = np.abs(u) + np.abs(v)
    lo, hi = c - ext, c + ext
    wroot = comp[line]
    x0, x1, y0, y1 = [], [], [], []
    for r in roots:
        m = wroot == r
        x0.append(int(lo[m, 0].min())); x1.append(int(hi[m, 0].max())); y0.append(int(lo[m, 1].min())); y1.append(int(hi[m, 1].max()))
    nb = len(roots)
    key = [(y0[b], x0[b], roots[b]) for b in range(nb)]
    cy = [(y0[b] + y1[b], roots[b]) for b in range(nb)]
    if nb > CAP:
        mode, seq = 0, sorted(range(nb), key=lambda b: key[b])
    else:
        mode, seq = 1, []
        P = precedence(x0, x1, cy)
        unplaced = np.ones(nb, bool)
        while unplaced.any():
            held = (P & unplaced[:, None]).any(axis=0)
            free = [b for b in np.flatnonzero(unplaced & ~held)]
            cand = free if free else [b for b in np.flatnonzero(unplaced)]
            b = min(cand, key=lambda b: key[b])
            seq.append(int(b))
            unplaced[b] = False
    rank = np.zeros(nb, np.int64)
    rank[seq] = np.arange(nb)
    of_root = {r: b for b, r in enumerate(roots)}
    block = np.array([rank[of_root[int(comp[l])]] for l in range(n_lines)], np.int32)
    return block, pos, nb, mode


def blocks_from_quads(quads):
    quads = np.asarray(quads, np.float32).reshape(-1, 8)
    line, word, nl = L.lines_from_quads(quads)
    return (line, word, nl) + blocks_from_lines(quads, line, word, nl)


def block_order(block, pos, n_blocks):
    """(block_order i32 [n_lines] the line indices in block reading order, block_first i32 [n_blocks + 1])"""
    return L.reading_order(block, pos, n_blocks)


def item_blocks(line, block):
    """each item's block"""
    return np.asarray(block, np.int32)[np.asarray(line, np.int64)] if len(line) else np.zeros(0, np.int32)


def block_bboxes(line_bbox, order, first):
    return L.line_bboxes(line_bbox, order, first)


def block_texts(line_texts, order, first):
    return ["\n".join(line_texts[l] for l in order[first[b]:first[b + 1]]) for b in range(len(first) - 1)]


def page_text_blocks(line_texts, order, first):
    return "\n\n".join(block_texts(line_texts, order, first))


# ---- layouts
def paragraph(x0, y0, width, n_rows, h, leading, deg=0.0, gap=0.4, last=0.6, seed=0):
    """n_rows rows of words of height h filling `width` (the last row `last` of it), `leading` x h apart, the whole turned by deg about (x0, y0):
    -> ([n, 8] quads, the number of rows).  Word widths come from a seeded generator, between 1.5 h and 4 h."""
    rng = np.random.default_rng(seed)
    a = np.deg2rad(deg)
    out = []
    for r in range(n_rows):
        room = width * (last if r == n_rows - 1 and n_rows > 1 else 1.0)
        widths, t = [], 0.0
        while True:
            w = float(rng.uniform(1.5, 4.0)) * h
            if t + w > room:
                break
            widths.append(w)
            t += w + gap * h
        rest = room - (t - gap * h)
        widths[-1] += rest                                 # flush right (of the row's room)
        d = leading * h * r
        out.append(L.row_quads(x0 - np.sin(a) * d, y0 + np.cos(a) * d, widths, h, gap * h, deg))
    return np.concatenate(out), n_rows


def two_section_page():
    """heading | left column (two paragraphs) , right column (two paragraphs) | heading 2 | left, right paragraph | footer.
    -> (quads, the parts' names in the reading order the rule must give, the rows of each part)"""
    h, ld = 20.0, 1.33
    parts = [("heading", paragraph(100, 60, 1300, 1, 30.0, ld, seed=1)),
             ("L1", paragraph(100, 160, 600, 4, h, ld, seed=2)), ("L2", paragraph(100, 160 + (4 + 1) * ld * h, 600, 3, h, ld, seed=3)),
             ("R1", paragraph(800, 160, 600, 3, h, ld, seed=4)), ("R2", paragraph(800, 160 + (3 + 1) * ld * h, 600, 4, h, ld, seed=5)),
             ("heading2", paragraph(100, 480, 1300, 1, 30.0, ld, seed=6)),
             ("L3", paragraph(100, 580, 600, 4, h, ld, seed=7)), ("R3", paragraph(800, 580, 600, 4, h, ld, seed=8)),
             ("footer", paragraph(100, 760, 1300, 1, 14.0, ld, seed=9))]
    quads = np.concatenate([p[1][0] for p in parts])
    return quads, [p[0] for p in parts], [p[1][1] for p in parts], [len(p[1][0]) for p in parts]


def random_page(seed):
    """a generated page of paragraphs: 1-3 columns, each a stack of paragraphs with a blank line between them, one leading in 1.2 .. 2.2 h and
    one tilt of 0, 7, -12 or 25 degrees for the page, words shuffled"""
    rng = np.random.default_rng(seed)
    h = float(rng.choice([14, 20, 26]))
    ld = float(rng.uniform(1.2, 2.2))
    deg = float(rng.choice([0, 7, -12, 25]))
    cols = int(rng.integers(1, 4))
    colw = 1500.0 / cols - 100
    a = np.deg2rad(deg)
    out = []
    for cidx in range(cols):
        x, t = 300 + cidx * (colw + 100), 0.0
        for _ in range(int(rng.integers(1, 4))):
            rows = int(rng.integers(1, 6))
            bx, by = x * np.cos(a) - t * np.sin(a), 300 + x * np.sin(a) + t * np.cos(a)
            out.append(paragraph(bx, by, colw, rows, h, ld, deg, seed=int(rng.integers(1 << 30)))[0])
            t += (rows + 1) * ld * h
    q = np.concatenate(out)
    return q[rng.permutation(len(q))]


def isolated_words(n, per_row=32):
    """n words far apart from each other: every word is its own line and its own block"""
    i = np.arange(n)
    return np.array([L.rect_quad(60 + 150.0 * (k % per_row), 40 + 90.0 * (k // per_row), 50, 20) for k in i], np.float32).reshape(-1, 8)
