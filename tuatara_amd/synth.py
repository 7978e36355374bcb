"""Synthetic workload of BASELINE.json config 5: 1024x768 pages, white background,
~40 random alphanumeric words drawn with PIL's built-in bitmap font at seeded positions."""
from __future__ import annotations

import numpy as np

ALNUM = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def synthetic_page(seed: int, h: int = 1024, w: int = 768, n_words: int = 40, scale: int = 2, layout: str = "jitter4") -> np.ndarray:
    """u8 [h,w,3].  layout "jitter4" (the parity tests' pages): words sit on a 4-column jittered grid so they never touch.  layout "cells5x8"
    (the benchmark's pages): one word inside each cell of the 5 x 8 grid whose 150 x 40 px boxes `bench_grid_boxes` hands to the recogniser
    (bench.py --boxes=grid40), so that the 40 crops of a page frame text and decode to strings of the words' lengths.  Glyphs are the PIL
    default font magnified `scale` x (nearest) so strokes survive the detector's stride-2 heat map; same words per seed in both layouts."""
    from PIL import Image, ImageDraw, ImageFont

    rng = np.random.default_rng(seed)
    font = ImageFont.load_default()
    page = Image.new("L", (w, h), 255)
    if layout == "cells5x8":
        for k in range(min(n_words, 40)):
            r, c = divmod(k, 5)
            word = "".join(rng.choice(list(ALNUM), size=int(rng.integers(3, 11))))
            tile = Image.new("L", (70, 14), 255)
            ImageDraw.Draw(tile).text((1, 1), word, fill=0, font=font)
            bbox = Image.eval(tile, lambda v: 255 - v).getbbox()
            # the word fills its box (the recogniser's crop is the box stretched to 128 x 32 with no regard for the aspect ratio,
            # tuatara.cpp:440: a short word left at font scale would leave most of the crop blank paper)
            tw, th = int(rng.integers(136, 145)), int(rng.integers(30, 35))
            tile = tile.crop((bbox[0], bbox[1], bbox[2] + 1, bbox[3] + 1)).resize((tw, th), Image.NEAREST)
            cx, cy = (c + 0.5) * w / 5.0, (r + 0.5) * h / 8.0                      # the grid box: 150 x 40 px about (cx, cy)
            x0, x1 = int(cx - 75) + 2, int(cx + 75) - 2 - tw
            y0, y1 = int(cy - 20) + 2, int(cy + 20) - 2 - th
            x = int(rng.integers(x0, max(x0 + 1, x1 + 1)))
            y = int(rng.integers(y0, max(y0 + 1, y1 + 1)))
            page.paste(tile, (x, y))
        a = np.asarray(page, dtype=np.uint8)
        return np.ascontiguousarray(np.repeat(a[:, :, None], 3, 2))
    if layout != "jitter4":
        raise ValueError("layout must be 'jitter4' or 'cells5x8'")
    cols, rows = 4, (n_words + 3) // 4
    cw, ch = w // cols, h // rows
    k = 0
    for r in range(rows):
        for c in range(cols):
            if k >= n_words:
                break
            word = "".join(rng.choice(list(ALNUM), size=int(rng.integers(3, 11))))
            tile = Image.new("L", (70, 14), 255)
            ImageDraw.Draw(tile).text((1, 1), word, fill=0, font=font)
            bbox = Image.eval(tile, lambda v: 255 - v).getbbox()
            tile = tile.crop((0, 0, bbox[2] + 1, 14)).resize(((bbox[2] + 1) * scale, 14 * scale), Image.NEAREST)
            x = c * cw + int(rng.integers(4, max(5, cw - tile.size[0] - 4)))
            y = r * ch + int(rng.integers(4, max(5, ch - tile.size[1] - 4)))
            page.paste(tile, (x, y))
            k += 1
    a = np.asarray(page, dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(a[:, :, None], 3, 2))


def synthetic_columns_page(seed: int, h: int = 512, w: int = 768, rows: int = 6, scale: int = 2, gutter: int = 96, ink: str = "glyphs"):
    """A two-column page: `rows` rows of words per column, drawn as synthetic_page draws them (PIL's default font magnified `scale` x), the rows
    of both columns on the same baselines 18 `scale` px apart, the columns `gutter` px apart (several text heights, so no text line crosses it).
    Every row is filled to its column's width, the last to at least half of it.  ink "glyphs": the words as drawn; "bars": every word a bar of seeded black-and-white noise of
    the word's size, the dark "words" of the smoke test - the synthetic detector follows ink density, so it shatters thin glyph strokes into
    fragments but gives exactly one box per bar.  Returns (page u8 [h, w, 3], words): per word a dict {"word",
    "column": 0 left / 1 right, "row", "box": (x0, y0, x1, y1) of its tile}, column after column, row after row."""
    from PIL import Image, ImageDraw, ImageFont

    if ink not in ("glyphs", "bars"):
        raise ValueError("ink must be 'glyphs' or 'bars'")
    rng = np.random.default_rng(seed)
    font = ImageFont.load_default()
    page = Image.new("L", (w, h), 255)
    margin, pitch, space = 24, 18 * scale, 10 * scale
    colw = (w - 2 * margin - gutter) // 2
    words = []
    for col in range(2):
        x_col = margin + col * (colw + gutter)
        for r in range(rows):
            room = colw if r < rows - 1 else int(colw * float(rng.uniform(0.55, 0.8)))
            x = x_col
            while True:
                word = "".join(rng.choice(list(ALNUM), size=int(rng.integers(3, 8))))
                tile = Image.new("L", (70, 14), 255)
                ImageDraw.Draw(tile).text((1, 1), word, fill=0, font=font)
                bbox = Image.eval(tile, lambda v: 255 - v).getbbox()
                tile = tile.crop((0, 0, bbox[2] + 1, 14)).resize(((bbox[2] + 1) * scale, 14 * scale), Image.NEAREST)
                if x + tile.size[0] > x_col + room:
                    break
                if ink == "bars":
                    bar = np.full((tile.size[1], tile.size[0]), 255, np.uint8)
                    bar[3 * scale:11 * scale, scale:-scale] = rng.integers(0, 2, (8 * scale, tile.size[0] - 2 * scale), dtype=np.uint8) * 255
                    tile = Image.fromarray(bar)
                y = margin + r * pitch
                page.paste(tile, (x, y))
                words.append({"word": word, "column": col, "row": r, "box": (x, y, x + tile.size[0], y + tile.size[1])})
                x += tile.size[0] + space
    a = np.asarray(page, dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(a[:, :, None], 3, 2)), words


def synthetic_rotated_page(seed: int, h: int = 1024, w: int = 768, n_words: int = 16, max_deg: float = 30.0):
    """Words drawn as synthetic_page draws them (PIL's default font magnified 2x), each rotated by a seeded skew in [-max_deg, max_deg]
    degrees (image coordinates, y down: positive turns the baseline clockwise on screen) and pasted where it overlaps no other word.
    Returns (page u8 [h, w, 3], words): per placed word a dict {"word", "centre": (cx, cy) in image pixels (pixel centres at integers),
    "angle": skew in degrees, "tile": the upright word u8 [th, tw] as it was rotated}.  Fewer than n_words are placed when the page is full."""
    from PIL import Image, ImageDraw, ImageFont

    rng = np.random.default_rng(seed)
    font = ImageFont.load_default()
    page = Image.new("L", (w, h), 255)
    taken = []                                     # axis-aligned bounds (x0, y0, x1, y1) of the rotated words placed so far, with a margin
    words = []
    for _ in range(n_words):
        word = "".join(rng.choice(list(ALNUM), size=int(rng.integers(4, 11))))
        tile = Image.new("L", (80, 16), 255)
        ImageDraw.Draw(tile).text((3, 2), word, fill=0, font=font)
        bb = Image.eval(tile, lambda v: 255 - v).getbbox()
        tile = tile.crop((bb[0] - 2, bb[1] - 2, bb[2] + 2, bb[3] + 2))
        tile = tile.resize((tile.size[0] * 2, tile.size[1] * 2), Image.NEAREST)
        ang = float(rng.uniform(-max_deg, max_deg))
        rot = tile.rotate(-ang, resample=Image.BILINEAR, expand=True, fillcolor=255)
        mask = tile.point(lambda v: 255).rotate(-ang, resample=Image.BILINEAR, expand=True, fillcolor=0)
        rw, rh = rot.size
        for _try in range(200):
            x = int(rng.integers(4, max(5, w - rw - 4)))
            y = int(rng.integers(4, max(5, h - rh - 4)))
            box = (x - 6, y - 6, x + rw + 6, y + rh + 6)
            if x + rw <= w - 4 and y + rh <= h - 4 and all(box[2] <= t[0] or t[2] <= box[0] or box[3] <= t[1] or t[3] <= box[1] for t in taken):
                break
        else:
            continue
        page.paste(rot, (x, y), mask)
        taken.append(box)
        # PIL's expand keeps the tile's centre at the centre of the rotated canvas; pixel centres sit at integer coordinates
        words.append({"word": word, "centre": (x + rw / 2.0 - 0.5, y + rh / 2.0 - 0.5), "angle": ang,
                      "tile": np.asarray(tile, dtype=np.uint8).copy()})
    a = np.asarray(page, dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(a[:, :, None], 3, 2)), words


def synthetic_arched_page(seed: int, h: int = 512, w: int = 640, n_words: int = 6):
    """Arched words for "Curved words": every word a band of seeded black-and-white noise (the dark "words" the synthetic detector boxes one by one, as
    synthetic_columns_page's bars) laid along a circular arc - chord 150 to 210 px at a seeded tilt within 12 degrees, 14 to 18 px thick along the arc's
    normal, sagitta 1.5 to 2.5 thicknesses, arching up or down in turn - one per cell of a 2-column grid; every third word is a straight bar of the same
    make.  Returns (page u8 [h, w, 3], words): per word a dict {"centre": (cx, cy), "chord", "thick", "sagitta" (0 for a straight bar), "up", "angle"}."""
    rng = np.random.default_rng(seed)
    page = np.full((h, w), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    rows = (n_words + 1) // 2
    words = []
    for k in range(n_words):
        r, c = divmod(k, 2)
        cx, cy = (c + 0.5) * w / 2.0 + float(rng.uniform(-12, 12)), (r + 0.5) * h / rows + float(rng.uniform(-6, 6))
        chord, thick = float(rng.uniform(150, 210)), float(rng.uniform(14, 18))
        sag = 0.0 if k % 3 == 2 else thick * float(rng.uniform(1.5, 2.5))
        up, ang = k % 2 == 0, float(rng.uniform(-12, 12))
        a = np.radians(ang)
        lx, ly = (xx - cx) * np.cos(a) + (yy - cy) * np.sin(a), -(xx - cx) * np.sin(a) + (yy - cy) * np.cos(a)
        if sag == 0.0:
            inside = (np.abs(lx) <= chord / 2.0) & (np.abs(ly) <= thick / 2.0)
        else:
            R = (chord * chord / 4.0 + sag * sag) / (2.0 * sag)
            sgn = 1.0 if up else -1.0
            oy = sgn * (R - sag / 2.0)
            rad = np.hypot(lx, ly - oy)
            th = np.arctan2(lx, -sgn * (ly - oy))
            inside = (np.abs(rad - R) <= thick / 2.0) & (np.abs(th) <= np.arcsin(chord / 2.0 / R))
        noise = (rng.integers(0, 2, (h // 2 + 1, w // 2 + 1), dtype=np.uint8) * 255).repeat(2, 0).repeat(2, 1)[:h, :w]
        page[inside] = noise[inside]
        words.append({"centre": (cx, cy), "chord": chord, "thick": thick, "sagitta": sag, "up": up, "angle": ang})
    return np.ascontiguousarray(np.repeat(page[:, :, None], 3, 2)), words
