"""Barcodes (DESIGN.md "Barcodes"): an encoder that draws Code 128 and Code 39 on a page, and the whole rule restated on run lists with Python integers,
independent of tuatara_amd/csrc/barcodes_rule.h and geometry.cpp: tests/test_barcodes_cpu.py holds the host rule to it bit for bit, tests/test_gpu_barcodes.py
the kernels.  The restatement works on a boolean ink mask and on each line's list of run lengths, not on the bitmaps' words.  Not a test module."""
import numpy as np

from tests.marks_ref import centres_of, ink_mask, quad_box  # noqa: F401  (step 1 and the items' centres are the other page layers')

CAP = 64
DEFAULTS = (8, 128, 3)            # min_lines, ink, symbologies
LINE_HITS = 8

PATTERNS_128 = """
212222 222122 222221 121223 121322 131222 122213 122312 132212 221213 221312 231212 112232 122132 122231 113222
123122 123221 223211 221132 221231 213212 223112 312131 311222 321122 321221 312212 322112 322211 212123 212321
232121 111323 131123 131321 112313 132113 132311 211313 231113 231311 112133 112331 132131 113123 113321 133121
313121 211331 231131 213113 213311 213131 311123 311321 331121 312113 312311 332111 314111 221411 431111 111224
111422 121124 121421 141122 141221 112214 112412 122114 122411 142112 142211 241211 221114 413111 241112 134111
111242 121142 121241 114212 124112 124211 411212 421112 421211 212141 214121 412121 111143 111341 131141 114113
114311 411113 411311 113141 114131 311141 411131 211412 211214 211232
""".split()
STOP_128 = "2331112"
START_A, START_B, START_C = 103, 104, 105
FNC3, FNC2, SHIFT, CODE_C, FNC1 = 96, 97, 98, 99, 102
ALPHABET_39 = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ-. $/+%*"
PATTERNS_39 = [int(v, 16) for v in """
034 121 061 160 031 130 070 025 124 064 109 049 148 019 118 058 00D 10C 04C 01C 103 043 142 013 112 052 007 106 046 016
181 0C1 1C0 091 190 0D0 085 184 0C4 0A8 0A2 08A 02A 094
""".split()]
VALUE_OF_128 = {p: v for v, p in enumerate(PATTERNS_128)}
CHAR_OF_39 = {p: c for p, c in zip(PATTERNS_39, ALPHABET_39)}


# ---------------------------------------------------------------------------------------------------------------- the encoder
def code128_symbols(start, values, check=None):
    """start value, data values -> every symbol's widths in modules: start, data, check (the right one unless given), Stop"""
    if check is None:
        check = (start + sum((i + 1) * v for i, v in enumerate(values))) % 103
    widths = []
    for v in [start] + list(values) + [check]:
        widths += [int(c) for c in PATTERNS_128[v]]
    return widths + [int(c) for c in STOP_128]


def code128_auto(data):
    """bytes below 128 -> (start, values): set C for runs of four digits or more (pairs of them), A for control characters, B otherwise"""
    data, out, cur, i = bytes(data), [], None, 0

    def go(to):
        nonlocal cur
        if cur is None:
            out.append({"A": START_A, "B": START_B, "C": START_C}[to])
        elif cur != to:
            out.append({"A": 101, "B": 100, "C": 99}[to])
        cur = to

    while i < len(data):
        n = 0
        while i + n < len(data) and 48 <= data[i + n] <= 57:
            n += 1
        if n >= 4 or (cur == "C" and n >= 2):
            go("C")
            for _ in range(n // 2):
                out.append(int(data[i:i + 2]))
                i += 2
            continue
        b = data[i]
        assert b < 128
        go("A" if b < 32 else "B" if b >= 96 or cur not in ("A", "B") else cur)
        out.append(b - 32 if b >= 32 else b + 64)
        i += 1
    if cur is None:
        go("B")
    return out[0], out[1:]


def code39_symbols(text, wide=3):
    """text (without the asterisks) -> widths in modules, the gaps between characters (one module) included"""
    widths = []
    for k, ch in enumerate("*" + text + "*"):
        bits = PATTERNS_39[ALPHABET_39.index(ch)]
        if k:
            widths.append(1)
        widths += [wide if bits >> (8 - i) & 1 else 1 for i in range(9)]
    return widths


def draw(page, widths, module, x, y, height, direction=0, spread=0):
    """Draws the runs (bar first, in modules) on page u8 [H, W, 3] in black: `module` px a module, every bar `spread` px longer at its end and the space behind
    it as much shorter.  direction 0: along x from (x, y) on, `height` rows; 2: the same place, drawn from its right end leftwards; 1 / 3: along y, `height`
    columns.  Returns the box (x0, y0, x1, y1) of the ink."""
    bars, pos = [], 0
    for i, m in enumerate(widths):
        if i % 2 == 0:
            bars.append((pos, pos + m * module + spread))
        pos += m * module
    total = bars[-1][1]
    for a, b in bars:
        if direction in (2, 3):
            a, b = total - b, total - a
        if direction in (0, 2):
            page[y:y + height, x + a:x + b] = 0
        else:
            page[y + a:y + b, x:x + height] = 0
    return (x, y, x + total - 1, y + height - 1) if direction in (0, 2) else (x, y, x + height - 1, y + total - 1)


def blank(h, w):
    return np.full((h, w, 3), 255, np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the rule
def runs_of(line):
    """a 1-D bool line -> (first value, run lengths, run starts)"""
    line = np.asarray(line, bool)
    cuts = np.flatnonzero(line[1:] != line[:-1]) + 1
    starts = np.concatenate(([0], cuts))
    lens = np.diff(np.concatenate((starts, [len(line)])))
    return bool(line[0]), lens.tolist(), starts.tolist()


def _measure(r, S, M):
    return [(2 * M * v + S) // (2 * S) for v in r]


def _value128(r):
    S = sum(r)
    m = _measure(r, S, 11)
    if any(v < 1 or v > 4 for v in m) or sum(m) != 11:
        return None
    return "".join(map(str, m))


def _quiet(lens, j, side, num, S, den):
    """the run j (no ink) as the quiet zone before (side -1) or behind (side 1) a code: beyond the list is the page's edge, and so is a run that touches it"""
    if j < 0 or j >= len(lens) or (j == 0 and side < 0) or (j == len(lens) - 1 and side > 0):
        return True
    return den * lens[j] >= num * S


def _text128(start, values):
    """data values under the sets -> (bytes, flags)"""
    cur, shift, out, flags = start - 103, False, bytearray(), 0
    for i, v in enumerate(values):
        if cur == 2:
            if v < 100:
                out += b"%02d" % v
            elif v == 100:
                cur = 1
            elif v == 101:
                cur = 0
            elif i == 0:
                flags |= 1
            else:
                out.append(0x1D)
            continue
        eff, shift = (1 - cur if shift else cur), False
        if v < 96:
            out.append(32 + v if eff == 1 or v < 64 else v - 64)
        elif v == FNC3:
            flags |= 4
        elif v == FNC2:
            flags |= 2
        elif v == SHIFT:
            shift = True
        elif v == CODE_C:
            cur = 2
        elif v == FNC1:
            if i == 0:
                flags |= 1
            else:
                out.append(0x1D)
        elif (v == 100 and eff == 0) or (v == 101 and eff == 1):
            cur = 1 - eff
        else:
            flags |= 8
    return bytes(out), flags


def decode128(lens, i):
    """step 4 from the ink run i of a line's run lengths (the line's first and last runs touch the page's edges).  -> (status, hit): status 0 no start
    pattern, 1 a start pattern and no hit, 2 a hit = (first run, one past the last run, text, flags, module64)"""
    n = len(lens)
    if i + 6 > n:
        return 0, None
    pat = _value128(lens[i:i + 6])
    start = VALUE_OF_128.get(pat, -1)
    if start not in (START_A, START_B, START_C):
        return 0, None
    S0 = sum(lens[i:i + 6])
    if not _quiet(lens, i - 1, -1, 5, S0, 11):
        return 1, None
    j, prev, values = i + 6, S0, []
    while True:
        if len(values) >= 2 and j + 7 <= n:
            r = lens[j:j + 7]
            S7 = sum(r)
            if "".join(map(str, _measure(r, S7, 13))) == STOP_128 and 4 * abs(11 * S7 - 13 * prev) <= 13 * prev and _quiet(lens, j + 7, 1, 5, S7, 13):
                break
        if j + 6 > n:
            return 1, None
        r = lens[j:j + 6]
        S = sum(r)
        if 4 * abs(S - prev) > prev:
            return 1, None
        v = VALUE_OF_128.get(_value128(r), 999)
        if v >= 103 or len(values) + 1 >= 80:
            return 1, None
        values.append(v)
        prev, j = S, j + 6
    data, check = values[:-1], values[-1]
    if (start + sum((k + 1) * v for k, v in enumerate(data))) % 103 != check:
        return 1, None
    text, flags = _text128(start, data)
    if len(text) > 48:
        return 1, None
    span = sum(lens[i:j + 7])
    return 2, (i, j + 7, text, flags, 64 * span // (11 * (len(values) + 1) + 13))


def _char39(r):
    mn, mx = min(r), max(r)
    wide = [2 * v > mn + mx for v in r]
    if sum(wide) != 3:
        return None
    if 2 * min(v for v, wd in zip(r, wide) if wd) < 3 * max(v for v, wd in zip(r, wide) if not wd):
        return None
    bits = 0
    for wd in wide:
        bits = bits << 1 | int(wd)
    ch = CHAR_OF_39.get(bits)
    return None if ch is None else (ch, mn, sum(v for v, wd in zip(r, wide) if not wd))


def decode39(lens, i):
    """step 5 from the ink run i; as decode128"""
    n = len(lens)
    if i + 9 > n:
        return 0, None
    c = _char39(lens[i:i + 9])
    if c is None or c[0] != "*":
        return 0, None
    if not _quiet(lens, i - 1, -1, 5, c[1], 1):
        return 1, None
    j, S, narrow, chars, text = i + 9, sum(lens[i:i + 9]), c[2], 1, ""
    while True:
        if j >= n - 1 or 3 * lens[j] > S or j + 10 > n:      # no gap, a gap that touches the edge or is too wide, no nine runs behind it
            return 1, None
        r = lens[j + 1:j + 10]
        c = _char39(r)
        if c is None or 4 * abs(sum(r) - S) > S:
            return 1, None
        j, S, narrow, chars = j + 10, sum(r), narrow + c[2], chars + 1
        if c[0] == "*":
            break
        if len(text) >= 48:
            return 1, None
        text += c[0]
    if not text or not _quiet(lens, j, 1, 5, c[1], 1):
        return 1, None
    return 2, (i, j, text.encode(), 0, 64 * narrow // (6 * chars))


def line_hits(line, symbologies=3):
    """steps 4 - 6 on one line (1-D bool), both readings -> {rev: (hits, [kept, dropped, candidates, starts])}; a hit = (sym, p0, p1, text, flags, module64),
    in ascending order of the pixel its reading begins at"""
    out = {}
    L = len(line)
    for rev in (0, 1):
        first, lens, starts = runs_of(line[::-1] if rev else line)
        hits, cands, matched = [], 0, 0
        for i in range(0 if first else 1, len(lens), 2):
            cands += 1
            hit = None
            if symbologies & 1:
                st, hit = decode128(lens, i)
                matched += st > 0
            if hit is None and symbologies & 2:
                st, hit = decode39(lens, i)
                matched += st > 0
                sym = 2
            else:
                sym = 1
            if hit is None:
                continue
            u0 = starts[hit[0]]
            u1 = starts[hit[1]] if hit[1] < len(lens) else L
            p0, p1 = (L - u1, L - 1 - u0) if rev else (u0, u1 - 1)
            hits.append((sym, p0, p1, hit[2], hit[3], hit[4]))
        if rev:
            hits.reverse()
        out[rev] = (hits[:LINE_HITS], [min(len(hits), LINE_HITS), max(len(hits) - LINE_HITS, 0), cands, matched])
    return out


def barcodes_of_mask(m, quads=None, min_lines=8, symbologies=3):
    """steps 2 - 9 on an ink mask -> {"mode", "barcodes": list of dicts, "records" i32 [n, 24], "item_barcode" i32 [nq], "counts" [6] = barcodes, candidates,
    starts, hits, dropped, chains below min_lines, "hits": {(kind, line, rev): [hit, ..]}}"""
    m = np.asarray(m, bool)
    h, w = m.shape
    cache, lines = {}, {}
    totals = [0, 0, 0, 0]
    for kind, count, get in ((0, h, lambda k: m[k]), (1, w, lambda k: m[:, k])):
        for k in range(count):
            line = np.ascontiguousarray(get(k))
            key = line.tobytes()
            if key not in cache:
                cache[key] = line_hits(line, symbologies)
            for rev in (0, 1):
                hs, c = cache[key][rev]
                lines[(kind, k, rev)] = hs
                for j in range(4):
                    totals[j] += c[j]

    def linked(a, b):
        if (a[0], a[3], a[4]) != (b[0], b[3], b[4]):
            return False
        over = min(a[2], b[2]) - max(a[1], b[1]) + 1
        return 2 * over >= min(a[2] - a[1] + 1, b[2] - b[1] + 1)

    # 7: a hit chains to the first hit that fits on the nearest of the three lines before it; a chain is the tree that grows from a hit without a partner
    root = {}
    chains = {}
    for kind, count in ((0, h), (1, w)):
        for rev in (0, 1):
            for k in range(count):
                for s, a in enumerate(lines[(kind, k, rev)]):
                    pred = None
                    for d in (1, 2, 3):
                        if k - d < 0:
                            break
                        for t, b in enumerate(lines[(kind, k - d, rev)]):
                            if linked(a, b):
                                pred = (kind, k - d, rev, t)
                                break
                        if pred:
                            break
                    me = (kind, k, rev, s)
                    root[me] = root[pred] if pred else me
                    chains.setdefault(root[me], []).append((k, a))
    found, below = [], 0
    for (kind, k0, rev, s), members in chains.items():
        if len(members) < min_lines:
            below += 1
            continue
        p0 = min(a[1] for _, a in members)
        p1 = max(a[2] for _, a in members)
        k1 = max(k for k, _ in members)
        a = members[0][1]
        box = (p0, k0, p1, k1) if kind == 0 else (k0, p0, k1, p1)
        found.append({"box": box, "symbology": a[0], "dir": 2 * rev + kind, "lines": len(members), "module64": sum(x[5] for _, x in members) // len(members),
                      "flags": a[4], "data": a[3], "_key": (box[1], box[0], 2 * rev + kind, k0, s)})
    counts = [0, totals[2], totals[3], totals[0], totals[1], below]
    nq = 0 if quads is None else len(np.asarray(quads).reshape(-1, 8))
    if len(found) > CAP:
        return {"mode": -7, "barcodes": [], "records": np.zeros((0, 24), np.int32), "item_barcode": np.full(nq, -1, np.int32), "counts": counts, "hits": lines}
    found.sort(key=lambda b: b["_key"])
    recs = np.zeros((len(found), 24), np.int32)
    for i, b in enumerate(found):
        recs[i, :10] = list(b["box"]) + [b["symbology"], b["dir"], b["lines"], b["module64"], b["flags"], len(b["data"])]
        recs[i, 12:] = np.frombuffer(b["data"].ljust(48, b"\0"), "<i4")
    counts[0] = len(found)
    items = np.full(nq, -1, np.int32)
    if nq:
        for i, (cx, cy) in enumerate(centres_of(quads).tolist()):
            for k, b in enumerate(found):
                x0, y0, x1, y1 = b["box"]
                if 64 * x0 <= cx < 64 * (x1 + 1) and 64 * y0 <= cy < 64 * (y1 + 1):
                    items[i] = k
                    break
    return {"mode": 1, "barcodes": found, "records": recs, "item_barcode": items, "counts": counts, "hits": lines}


def barcodes_of_page(image, quads=None, min_lines=8, ink=128, symbologies=3):
    return barcodes_of_mask(ink_mask(image, ink), quads, min_lines, symbologies)


# ---------------------------------------------------------------------------------------------------------------- the pages both suites share
def text128(data):
    return code128_symbols(*code128_auto(data))


def label(data, module=2, height=12, direction=0, margin=16, sym=1, spread=0):
    """a page that holds one code and `margin` px of white around it -> (page, box)"""
    widths = text128(data) if sym == 1 else code39_symbols(data.decode())
    n = sum(widths) * module + abs(spread)
    size = (height + 2 * margin, n + 2 * margin) if direction in (0, 2) else (n + 2 * margin, height + 2 * margin)
    page = blank(*size)
    return page, draw(page, widths, module, margin, margin, height, direction, spread)


OFFSET_RANGES = ((0, 44), (44, 88), (88, 131))


def offsets_page(x0=0, x1=131, step=1):
    """a short Code 128 at every x offset x0..x1 - 1, one under the other: runs across one word boundary and through three words"""
    n = (x1 - x0 + step - 1) // step
    page = blank(8 * n + 4, 200)
    for k in range(n):
        draw(page, text128(b"%c" % (65 + k % 26)), 1, x0 + k * step, 2 + 8 * k, 5)
    return page


def edges_page():
    """codes against all four edges of the page, in all four directions"""
    page = blank(150, 180)
    w = text128(b"Ed")
    n = sum(w)
    draw(page, w, 1, 0, 0, 6, 0)                    # top left corner, along x
    draw(page, w, 1, 180 - n, 144, 6, 2)            # bottom right corner, along x, backwards
    draw(page, w, 1, 0, 150 - n, 6, 3)              # bottom left, along y, upwards
    draw(page, code39_symbols("E"), 1, 174, 0, 6, 1)   # top right, along y
    return page


def many_codes_page(count, per_row=8):
    """`count` short Code 39 codes, per_row on a line, five rows high"""
    w = code39_symbols("A")
    n = sum(w) + 8
    page = blank(8 * ((count + per_row - 1) // per_row) + 2, n * max(per_row, 1) + 8)
    for k in range(count):
        draw(page, w, 1, 6 + n * (k % per_row), 2 + 8 * (k // per_row), 5)
    return page


def mixed_page():
    """two codes side by side, the same text twice, a Code 128 and a Code 39 that overlap in y, a vertical code, and words inside and outside the boxes"""
    page = blank(260, 520)
    boxes = [draw(page, text128(b"INV-2024-0042"), 1, 20, 10, 20), draw(page, text128(b"INV-2024-0042"), 1, 300, 10, 20),
             draw(page, text128(b"00123456789012"), 2, 20, 60, 24, 2), draw(page, code39_symbols("LOT 7/A"), 1, 300, 70, 30),
             draw(page, code39_symbols("UP"), 2, 480, 110, 16, 3), draw(page, text128(b"\x02ctl\x03"), 1, 20, 130, 9, 0)]
    quads = np.asarray([quad_box(40, 14, 90, 26), quad_box(310, 12, 330, 28), quad_box(240, 14, 280, 26), quad_box(30, 64, 60, 80), quad_box(320, 80, 350, 95),
                        quad_box(482, 120, 494, 160), quad_box(10, 200, 80, 220)], np.float32)
    return page, quads, boxes


def random_page(seed):
    """text-like noise - short dark strokes - plus a few codes at random places and directions"""
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(120, 260)), int(rng.integers(200, 420))
    page = blank(h, w)
    for _ in range(int(rng.integers(40, 160))):
        y, x = int(rng.integers(0, h - 8)), int(rng.integers(0, w - 12))
        page[y:y + int(rng.integers(1, 8)), x:x + int(rng.integers(1, 12))] = int(rng.integers(0, 120))
    for _ in range(int(rng.integers(1, 4))):
        d, mod = int(rng.integers(0, 4)), int(rng.integers(1, 3))
        data = bytes(rng.integers(32, 127, int(rng.integers(1, 6))).tolist())
        widths = text128(data) if rng.integers(0, 2) else code39_symbols("".join(ALPHABET_39[int(v)] for v in rng.integers(0, 43, 3)))
        n, hh = sum(widths) * mod, int(rng.integers(4, 20))
        along, across = (w, h) if d in (0, 2) else (h, w)
        if n + 2 > along or hh + 2 > across:
            continue
        a, b = int(rng.integers(0, along - n)), int(rng.integers(0, across - hh))
        draw(page, widths, mod, a if d in (0, 2) else b, b if d in (0, 2) else a, hh, d)
    quads = np.asarray([quad_box(x, y, x + 20, y + 10) for x, y in zip(rng.integers(0, w - 20, 12).tolist(), rng.integers(0, h - 10, 12).tolist())], np.float32)
    return page, quads


def many_bands_page():
    """1300 x 1100: codes in all four directions spread over many bands of lines, the last against the bottom right corner"""
    page = blank(1100, 1300)
    draw(page, text128(b"BAND-0001-xyz"), 3, 40, 30, 40, 0)
    draw(page, text128(b"998877665544"), 2, 700, 500, 30, 2)
    draw(page, code39_symbols("TRACK-42"), 2, 100, 300, 50, 1)
    draw(page, code39_symbols("Z9"), 3, 1200, 200, 40, 3)
    w = text128(b"corner")
    draw(page, w, 1, 1300 - sum(w), 1088, 12, 0)
    for k in range(60):
        page[200 + 13 * k:204 + 13 * k, 400:640] = 0
    return page


def partial_page(width):
    """Decodes that fail after their text has begun, between two valid codes on one line: a cut-off Code 39 (`*`, `A`, then a lone bar) and a Code 128 whose
    text is over 48 bytes.  `width` = 512, 1024 or 1536: an eighth of a line is 1, 2 or 3 words, the first valid code and the failing one begin in the last
    word of the first eighth, the second valid code in the next eighth."""
    wpl = width // 512
    x = 64 * (wpl - 1)
    page = blank(20, width)
    a, b = code39_symbols("A"), code39_symbols("B")
    draw(page, a, 1, x + 6, 2, 6)
    draw(page, a[:20] + [10], 1, x + 58, 2, 6)                     # `*`, `A`, a gap and a bar of 10 px: no character
    draw(page, b, 1, x + 134, 2, 6)
    long = text128(b"0123456789" * 5) if wpl == 1 else code128_symbols(START_B, [33 + i % 26 for i in range(49)])
    draw(page, a, 1, x + 6, 11, 6)
    draw(page, long, 1, x + 58, 11, 6)
    draw(page, b, 1, x + 58 + sum(long) + 8, 11, 6)
    return page
