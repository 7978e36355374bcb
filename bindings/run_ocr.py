#!/usr/bin/env python3
"""Counterpart of the reference's demo harness (bindings/run_ocr.py:85-107): open an image with PIL,
.convert("RGB"), hand the numpy array to pytuatara.image_to_data(image, weights_dir, outputs_dir), print the
result, and save an annotated copy (the reference's three panels: boxes on the page, text at the boxes, running text).  Drawing uses PIL only
(the reference draws with cv2 and opens a window; neither is needed for the results).

  python bindings/run_ocr.py [--rectify] [--curved] [image] [weights_dir] [outputs_dir]   (--rectify: deskewed crops, words drawn as their quads;
  --curved: words set on an arc are straightened along their spines and drawn as their 18-point outlines; --deskew: the page's skew is estimated and the page read upright; every box is mapped
  back through the call's own record (pytuatara.last_call_skew / last_call_to_page; DESIGN.md "Deskew") and drawn on the caller's image; --tables: every item carries its table and cell, and
  the page's rulings and cells are drawn over the first panel - the geometry from the host rule tuatara_amd.engine.tables_from_page, which the engine's kernels
  equal bit for bit)
"""
from __future__ import annotations

import os
import sys

import numpy as np
from PIL import Image, ImageDraw

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.join(HERE, "..", "build", "bindings"))   # where the build puts pytuatara (reference: run_ocr.py:6)


def annotate(image: np.ndarray, result, by_lines: bool = False, by_blocks: bool = False) -> Image.Image:
    """The reference's three panels side by side (run_ocr.py:10-82), drawn with PIL: the page with its boxes | each text at its
    box position | the texts as running text in reading order - sorted by (y1, x1) (:12), starting at (10, 30), wrapped at the
    page width, 10 px between words and lines (:20-25, :62-75).  by_lines=True (items read with lines=True, carrying "line" and
    "word"): the third panel follows the page's text lines instead - items in (line, word) order, a new row for every line.
    by_blocks=True (items read with blocks=True, carrying "block" too): the third panel follows the page's text blocks - items in (block, line,
    word) order, a new row for every line and an empty row between blocks, so a column is read to its end before the next begins."""
    page = Image.fromarray(image).convert("RGB")
    w, h = page.size
    boxes = page.copy()
    panel = Image.new("RGB", page.size, "black")
    running = Image.new("RGB", page.size, "black")
    db, dp, dr = ImageDraw.Draw(boxes), ImageDraw.Draw(panel), ImageDraw.Draw(running)
    tx, ty, gap = 10, 30, 10
    by_blocks = by_blocks and all("block" in it and "line" in it for it in result)
    by_lines = by_blocks or (by_lines and all("line" in it for it in result))
    last_line = last_block = None
    key = (lambda it: (it["block"], it["line"], it["word"])) if by_blocks else (lambda it: (it["line"], it["word"])) if by_lines else (lambda it: (it["bbox"][1], it["bbox"][0]))
    for item in sorted(result, key=key):
        x1, y1, x2, y2 = (int(v) for v in item["bbox"])
        text = item["text"]
        if item.get("curved"):   # curved words (curved=True): the band that was read, top edge and bottom edge
            db.polygon([tuple(p) for p in item["outline"]], outline=(255, 160, 0), width=2)
        elif "quad" in item:     # rectified crops (pytuatara.image_to_data(..., rectify=True)): the word's own quadrilateral
            db.polygon([tuple(p) for p in item["quad"]], outline=(0, 255, 0), width=2)
        else:
            db.rectangle([x1, y1, x2, y2], outline=(0, 255, 0), width=2)
        for ch in item.get("chars", ()):   # character boxes (chars=True): every cell of the word
            db.polygon([tuple(p) for p in ch["quad"]], outline=(0, 160, 255))
        dp.text((x1, y1), text, fill=(255, 0, 0))
        l, t, r, btm = dr.textbbox((0, 0), text or " ")
        tw, th = r - l, btm - t
        if by_lines and last_line is not None and item["line"] != last_line and tx > 10:   # a new text line starts a new row
            tx = 10
            ty += th + gap
        if by_blocks and last_block is not None and item["block"] != last_block:               # a new block: one empty row
            ty += th + gap
        last_line, last_block = item.get("line"), item.get("block")
        if tx + tw > w:
            tx = 10
            ty += th + gap
        dr.text((tx, ty - th), text, fill=(255, 0, 0))
        tx += tw + gap
    out = Image.new("RGB", (3 * w, h), "black")
    for k, im in enumerate((boxes, panel, running)):
        out.paste(im, (k * w, 0))
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    rectify, lines, chars, blocks, curved = "--rectify" in argv, "--lines" in argv, "--chars" in argv, "--blocks" in argv, "--curved" in argv
    tables, deskew, marks, barcodes = "--tables" in argv, "--deskew" in argv, "--marks" in argv, "--barcodes" in argv
    argv = [a for a in argv if a not in ("--rectify", "--lines", "--chars", "--blocks", "--curved", "--tables", "--deskew", "--marks", "--barcodes")]
    image_path = argv[0] if len(argv) > 0 else os.path.join(HERE, "..", "tests", "data", "funsd_0001129658.png")
    weights_dir = argv[1] if len(argv) > 1 else os.path.join(HERE, "..", "weights")
    outputs_dir = argv[2] if len(argv) > 2 else os.path.join(HERE, "..", "outputs")
    import pytuatara

    numpy_image = np.array(Image.open(image_path).convert("RGB"))
    kw = dict(rectify=True) if rectify else {}
    if lines:
        kw["lines"] = True
    if chars:
        kw["chars"] = True
    if blocks:                      # (blocks are made of lines: blocks=True turns lines on)
        kw["blocks"] = True
    if curved:                      # (curved words read on rectified crops: curved=True turns rectify on)
        kw["curved"] = True
    if tables:                      # (DESIGN.md "Tables": min_len 48, ink 128)
        kw["tables"] = True
    if marks:                       # (DESIGN.md "Selection marks": sides 10..64, fill 24, ink 128)
        kw["marks"] = True
    if barcodes:                    # (DESIGN.md "Barcodes": 8 lines, ink 128, Code 128 and Code 39)
        kw["barcodes"] = True
    if deskew:                      # (DESIGN.md "Deskew": max_slope 64, gain 288, ink 128; the result is in the upright page's frame)
        kw["deskew"] = True
    result = pytuatara.image_to_data(numpy_image, weights_dir, outputs_dir, **kw)
    print(result)
    os.makedirs(outputs_dir, exist_ok=True)
    stem = os.path.splitext(os.path.basename(image_path))[0]
    out = annotate(numpy_image, result, by_lines=lines, by_blocks=blocks)
    if tables:
        sys.path.insert(0, os.path.join(HERE, ".."))
        from tuatara_amd.engine import tables_from_page
        t = tables_from_page(numpy_image)
        d = ImageDraw.Draw(out)
        for c in t["cells"]:       # cells first, rulings over them
            d.rectangle([int(c[5]), int(c[6]), int(c[7]), int(c[8])], outline=(0, 160, 255), width=2)
        for r in t["rulings"]:
            d.rectangle([int(r[1]), int(r[2]), int(r[3]), int(r[4])], outline=(255, 0, 255) if r[5] >= 0 else (255, 160, 0))
    if marks:                       # every mark's frame over the first panel: green when selected, red when not, and its label's text beside it
        d = ImageDraw.Draw(out)
        for m in pytuatara.last_call_marks():
            print(("[x] " if m["selected"] else "[ ] ") + " ".join(str(v) for v in m["box"]) + "\t" + m["text"])
            d.rectangle([int(v) for v in m["box"]], outline=(0, 170, 0) if m["selected"] else (220, 0, 0), width=2)
    if barcodes:                    # every barcode's box over the first panel in blue, and a line per barcode
        d = ImageDraw.Draw(out)
        for b in pytuatara.last_call_barcodes():
            print(b["symbology"] + " " + str(b["direction"]) + " " + " ".join(str(v) for v in b["box"]) + "\t" + b["text"])
            d.rectangle([int(v) for v in b["box"]], outline=(0, 0, 230), width=2)
    if deskew:                      # every item's box mapped back to the caller's image through the call's own record and drawn there, over the first panel
        skew = pytuatara.last_call_skew()
        print(f"# page 0 slope {skew['slope']} degrees {skew['degrees']:.4f}")
        d = ImageDraw.Draw(out)
        for item in result:
            x0, y0, x1, y1 = item["bbox"]
            d.polygon(pytuatara.last_call_to_page([(x0, y0), (x1, y0), (x1, y1), (x0, y1)]), outline=(0, 200, 0))
    out.save(os.path.join(outputs_dir, stem + "_annotated_with_ocr_results.png"))
    return result


if __name__ == "__main__":
    main()
