"""Barcodes (DESIGN.md "Barcodes") without a GPU: the tables' structure, the host rule (ttr_barcodes_from_page) against tests/barcodes_ref.py bit for bit in
every output, round trips through the encoder in all four directions, each bound of the rule on both sides, the refusals that need no device, and the FUNSD
page.  Every test here but the two on the tables fails on the parent commit: ttr_barcodes_from_page and engine.barcodes_from_page are absent."""
import itertools
import os

import numpy as np
import pytest

from tests import barcodes_ref as R
from tests.conftest import ROOT

NEW_SYMBOLS = ("ttr_engine_set_barcodes", "ttr_engine_barcodes", "ttr_result_barcode_mode", "ttr_result_barcode_count", "ttr_result_barcodes",
               "ttr_result_item_barcode", "ttr_results_gather_barcodes", "ttr_barcodes_from_page", "ttr_barcodes_from_page_ink", "ttr_barcodes_page",
               "ttr_dbg_barcodes")


@pytest.fixture(scope="module")
def E():
    from tuatara_amd import build
    build.build_all()
    from tuatara_amd import engine
    return engine


def same(got, want):
    assert got["mode"] == want["mode"] and got["counts"] == want["counts"], (got["mode"], want["mode"], got["counts"], want["counts"])
    assert got["records"].shape == want["records"].shape and np.array_equal(got["records"], want["records"]), (got["records"][:, :12], want["records"][:, :12])
    assert np.array_equal(got["item_barcode"], want["item_barcode"])


def same_hits(got, want, h, w):
    """the raw hits of every line and reading against the restatement's"""
    for kind, count, base in ((0, h, 0), (1, w, h)):
        for k in range(count):
            for rev in (0, 1):
                hs = want["hits"][(kind, k, rev)]
                assert got["line_counts"][base + k, rev, 0] == len(hs), (kind, k, rev)
                for s, (sym, p0, p1, text, flags, mod) in enumerate(hs):
                    r = got["hits"][base + k, rev, s]
                    assert r[:6].tolist() == [p0, p1, mod, flags, len(text), sym] and r[8:].tobytes() == text.ljust(48, b"\0"), (kind, k, rev, s)


def both(E, img, quads=None, min_lines=8, ink=128, symbologies=3, hits=False, **kw):
    """the host rule's result, after holding it to the reference in every output"""
    got, want = E.barcodes_from_page(img, quads, min_lines, ink, symbologies, raw=hits, **kw), R.barcodes_of_page(img, quads, min_lines, ink, symbologies)
    same(got, want)
    if hits:
        same_hits(got, want, *np.asarray(img).shape[:2])
    return got


def texts(r):
    return [(b["symbology"], b["direction"], b["data"]) for b in r["barcodes"]]


def test_symbols_are_exported(E):
    lib = E.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert any(s[0] == name for s in E.SYMBOLS), name


def test_code128_table_is_the_108_compositions():
    """the 106 patterns, the Stop's first six widths and their reverse are exactly the six-part compositions of 11 into 1..4 with an even bar sum"""
    want = {"".join(map(str, c)) for c in itertools.product(range(1, 5), repeat=6) if sum(c) == 11 and (c[0] + c[2] + c[4]) % 2 == 0}
    have = R.PATTERNS_128 + [R.STOP_128[:6], R.STOP_128[::-1][:6]]      # (reversed: the Stop read from its other end)
    assert len(R.PATTERNS_128) == 106 and len(want) == 108 and len(set(have)) == 108 and set(have) == want


def test_code39_table_is_three_of_nine():
    assert len(R.PATTERNS_39) == 44 == len(R.ALPHABET_39) == len(set(R.PATTERNS_39))
    assert all(bin(p).count("1") == 3 and p < 512 for p in R.PATTERNS_39)
    # a character's bars and spaces: two of the five bars wide and one of the four spaces, or the four `$/+%` with three wide spaces
    for p, ch in zip(R.PATTERNS_39, R.ALPHABET_39):
        bars = sum(p >> (8 - i) & 1 for i in range(0, 9, 2))
        assert bars == (0 if ch in "$/+%" else 2), ch


def _stack(codes, module, direction, height=5, spread=0):
    """the codes (width lists) one beside the other across the reading direction, on one page -> (page, boxes)"""
    n = max(sum(w) for w in codes) * module + 24
    pitch = height + 3
    size = (pitch * len(codes) + 3, n) if direction in (0, 2) else (n, pitch * len(codes) + 3)
    page, boxes = R.blank(*size), []
    for k, w in enumerate(codes):
        pos = (12, 3 + pitch * k) if direction in (0, 2) else (3 + pitch * k, 12)
        boxes.append(R.draw(page, w, module, pos[0], pos[1], height, direction, spread))
    return page, boxes


SET_CASES = [(R.START_A, list(range(lo, min(lo + 16, 96))), bytes(32 + v if v < 64 else v - 64 for v in range(lo, min(lo + 16, 96)))) for lo in range(0, 96, 16)] + \
            [(R.START_B, list(range(lo, min(lo + 16, 96))), bytes(32 + v for v in range(lo, min(lo + 16, 96)))) for lo in range(0, 96, 16)] + \
            [(R.START_C, list(range(lo, min(lo + 20, 100))), b"".join(b"%02d" % v for v in range(lo, min(lo + 20, 100)))) for lo in range(0, 100, 20)]
# Shift, every code switch, FNC1 first and inside, FNC2 - 4: (start, values, text, flags)
SPECIAL_CASES = [
    (R.START_A, [33, 98, 65, 34], b"AaB", 0),                       # Shift in A: one symbol of B
    (R.START_B, [65, 98, 65, 66], b"a\x01b", 0),                    # Shift in B: one symbol of A
    (R.START_A, [33, 100, 65, 101, 65, 34], b"Aa\x01B", 0),         # Code B, Code A
    (R.START_A, [33, 99, 12, 34, 100, 65], b"A1234a", 0),           # A -> C -> B
    (R.START_B, [65, 99, 0, 99, 101, 64], b"a0099\x00", 0),         # B -> C -> A
    (R.START_C, [102, 1, 23, 45], b"012345", 1),                    # FNC1 first: GS1
    (R.START_C, [10, 102, 20], b"10\x1d20", 0),                     # FNC1 inside
    (R.START_B, [102, 33, 102, 34], b"A\x1dB", 1),
    (R.START_A, [97, 33], b"A", 2), (R.START_B, [96, 33], b"A", 4), (R.START_A, [101, 33], b"A", 8), (R.START_B, [100, 33], b"A", 8),
    (R.START_B, [33, 97, 96, 100], b"A", 14),
    (R.START_A, [96, 33], b"A", 4), (R.START_A, [102, 33, 102, 34], b"A\x1dB", 1),      # FNC3 and FNC1 under set A as well
]
CODE39_TEXTS = ["0123456789A", "BCDEFGHIJKL", "MNOPQRSTUVW", "XYZ-. $/+%0"]


@pytest.mark.parametrize("direction", range(4))
@pytest.mark.parametrize("module,spread", [(1, 0), (2, 0), (3, 0), (4, 0), (3, -1), (3, 1), (4, -1), (4, 1)])
def test_round_trips(E, module, spread, direction):
    """every value of the three sets, the special symbols and every Code 39 character, read back as encoded"""
    cases = [(s, v, t, 0) for s, v, t in SET_CASES] + SPECIAL_CASES
    codes = [R.code128_symbols(s, v) for s, v, _, _ in cases] + [R.code39_symbols(t) for t in CODE39_TEXTS]
    page, boxes = _stack(codes, module, direction, spread=spread)
    r = both(E, page, min_lines=5, hits=module == 1)
    assert r["mode"] == 1 and len(r["barcodes"]) == len(codes)
    got = {tuple(b["box"]): b for b in r["barcodes"]}
    for box, case in zip(boxes, cases + [(None, None, t.encode(), 0) for t in CODE39_TEXTS]):
        b = got[tuple(box)]
        assert b["data"] == case[2] and b["flags"] == case[3] and b["direction"] == direction and b["lines"] == 5, (case, b)
        assert b["symbology"] == ("code39" if case[0] is None else "code128") and b["gs1"] == bool(case[3] & 1)
        assert abs(b["module"] - module) <= 0.5


def test_auto_chooser_round_trip(E):
    for data in (b"Hello, World!", b"12345678", b"AB1234cd\x05", b"x\x7f\x00", b"123"):
        page, box = R.label(data)
        r = both(E, page)
        assert texts(r) == [("code128", 0, data)] and r["barcodes"][0]["box"] == list(box)


@pytest.mark.parametrize("lines,found", [(7, False), (8, True)])
def test_min_lines_bound(E, lines, found):
    page, _ = R.label(b"lines", height=lines)
    r = both(E, page)
    assert (len(r["barcodes"]) == 1) == found and r["counts"][5] == (0 if found else 1)


@pytest.mark.parametrize("sym,need", [(1, 10), (2, 10)])
@pytest.mark.parametrize("side", ["before", "behind"])
def test_quiet_zone_bound(E, sym, need, side):
    """module 2: Code 128 asks 11 q >= 5 * 22, Code 39 q >= 5 * 2: ten pixels either way; one short is no code"""
    for q, found in ((need, True), (need - 1, False)):
        page, box = R.label(b"QZ", sym=sym, margin=30)
        x = box[0] - q - 1 if side == "before" else box[2] + q + 1
        page[:, x] = 0
        r = both(E, page)
        assert (len(r["barcodes"]) == 1) == found, (q, r["counts"])


def test_wrong_check_symbol(E):
    st, v = R.code128_auto(b"check")
    good = (st + sum((i + 1) * x for i, x in enumerate(v))) % 103
    for check, found in ((good, True), ((good + 1) % 103, False)):
        page = R.blank(40, 200)
        R.draw(page, R.code128_symbols(st, v, check), 1, 20, 10, 12)
        assert (len(both(E, page)["barcodes"]) == 1) == found


@pytest.mark.parametrize("S,found", [(55, True), (56, False)])
def test_symbol_width_bound(E, S, found):
    """symbols of 44 px, one of 55 (a quarter more: 4 * 11 <= 44) or of 56 in the middle"""
    st, v = R.code128_auto(b"abcd")
    w = R.code128_symbols(st, v)
    px = [4 * m for m in w]
    px[12:18] = [5 * m for m in w[12:18]]
    px[13] += S - 55
    page = R.blank(40, sum(px) + 60)
    R.draw(page, px, 1, 30, 10, 12)
    assert (len(both(E, page)["barcodes"]) == 1) == found


@pytest.mark.parametrize("sym", [1, 2])
@pytest.mark.parametrize("n,found", [(48, True), (49, False)])
def test_text_length_bound(E, sym, n, found):
    data = bytes(65 + i % 26 for i in range(n))
    page, _ = R.label(data, module=1, sym=sym)
    r = both(E, page)
    assert texts(r) == ([("code128" if sym == 1 else "code39", 0, data)] if found else [])


@pytest.mark.parametrize("gap,codes", [(2, 1), (3, 2)])
def test_unreadable_lines_bound(E, gap, codes):
    page, box = R.label(b"gap", height=24)
    page[box[1] + 10:box[1] + 10 + gap] = 255
    r = both(E, page)
    assert len(r["barcodes"]) == codes and sum(b["lines"] for b in r["barcodes"]) == 24 - gap


def test_eight_and_nine_codes_on_a_line(E):
    r = both(E, R.many_codes_page(8), min_lines=4, hits=True)
    assert len(r["barcodes"]) == 8 and r["counts"][4] == 0
    r = both(E, R.many_codes_page(9, per_row=9), min_lines=4, hits=True)
    assert len(r["barcodes"]) == 8 and r["counts"][4] == 5 and r["counts"][3] == 40      # five lines drop their ninth


def test_cap(E):
    q = np.asarray([R.quad_box(10, 3, 20, 6)], np.float32)                                 # inside the first code
    r = both(E, R.many_codes_page(64), q, min_lines=4)
    assert r["mode"] == 1 and len(r["barcodes"]) == 64 and r["item_barcode"].tolist() == [0]
    r = both(E, R.many_codes_page(65), q, min_lines=4)
    assert r["mode"] == -7 and len(r["barcodes"]) == 0 and r["item_barcode"].tolist() == [-1] and r["counts"][3] == 65 * 5


def test_word_boundaries(E):
    """a code at every x offset 0..130: runs across one word boundary and through three words, forwards and - on the mirrored page - backwards"""
    for x0, x1 in R.OFFSET_RANGES:                                                       # (at most 64 codes a page)
        page = R.offsets_page(x0, x1)
        r = both(E, page, min_lines=4, hits=True)
        assert [b["box"][0] for b in r["barcodes"]] == list(range(x0, x1))
        r = both(E, np.ascontiguousarray(page[:, ::-1]), min_lines=4, hits=True)
        assert len(r["barcodes"]) == x1 - x0 and {b["direction"] for b in r["barcodes"]} == {2}
        r = both(E, np.ascontiguousarray(page.transpose(1, 0, 2)), min_lines=4, hits=True)
        assert len(r["barcodes"]) == x1 - x0 and {b["direction"] for b in r["barcodes"]} == {1}


@pytest.mark.parametrize("width", [512, 1024, 1536])
def test_decodes_that_fail_after_their_text_began(E, width):
    """a cut-off Code 39 and an over-long Code 128 between two valid codes on one line: the valid ones keep their text, in every direction"""
    page = R.partial_page(width)
    for img, d in ((page, 0), (page[:, ::-1], 2), (page.transpose(1, 0, 2), 1), (page.transpose(1, 0, 2)[::-1], 3)):
        r = both(E, np.ascontiguousarray(img), min_lines=4, hits=True)
        assert sorted(texts(r)) == [("code39", d, b"A"), ("code39", d, b"A"), ("code39", d, b"B"), ("code39", d, b"B")]
        assert r["counts"][2] >= 6                                                      # (the two failing codes matched their start patterns too)


def test_page_edges(E):
    r = both(E, R.edges_page(), min_lines=4, hits=True)
    assert sorted(texts(r)) == sorted([("code128", 0, b"Ed"), ("code128", 2, b"Ed"), ("code128", 3, b"Ed"), ("code39", 1, b"E")])


@pytest.mark.parametrize("w", list(range(1, 131)))
def test_every_width(E, w):
    """pages 1..130 px wide and as high: noise, and a code where it fits"""
    img = R.blank(20, w)
    img[np.random.RandomState(w).rand(20, w) < 0.3] = 0
    code = R.text128(b"w")
    if w >= sum(code):
        R.draw(img, code, 1, w - sum(code), 4, 6)
    both(E, img, min_lines=4, hits=True)
    both(E, np.ascontiguousarray(img.transpose(1, 0, 2)), min_lines=4, hits=True)


def test_padded_stride_and_channel_orders(E):
    img, quads, _ = R.mixed_page()
    want = both(E, img, quads)
    h, w = img.shape[:2]
    wide = np.full((h, w * 3 + 40), 7, np.uint8)
    wide[:, :w * 3] = img.reshape(h, w * 3)
    view = np.lib.stride_tricks.as_strided(np.ascontiguousarray(wide), (h, w, 3), (w * 3 + 40, 3, 1))
    same(E.barcodes_from_page(view, quads, row_stride=w * 3 + 40), want)
    tinted = img.copy()
    tinted[..., 0] = np.where(img[..., 0] == 0, 90, 255)      # ink that is dark in two channels only: s = 90 < 384
    a, b = both(E, tinted, quads), both(E, np.ascontiguousarray(tinted[..., ::-1]), quads)
    same(a, want), same(b, want)


def test_combinations(E):
    """two codes side by side with the same text, a Code 128 and a Code 39 overlapping in y, a vertical code; items inside and outside the boxes"""
    img, quads, boxes = R.mixed_page()
    r = both(E, img, quads, hits=True)
    assert [b["box"] for b in r["barcodes"]] == [list(b) for b in boxes]
    assert texts(r) == [("code128", 0, b"INV-2024-0042"), ("code128", 0, b"INV-2024-0042"), ("code128", 2, b"00123456789012"), ("code39", 0, b"LOT 7/A"),
                        ("code39", 3, b"UP"), ("code128", 0, b"\x02ctl\x03")]
    assert r["item_barcode"].tolist() == [0, 1, -1, 2, 3, 4, -1]
    assert [b["symbology"] for b in both(E, img, quads, symbologies=1)["barcodes"]] == ["code128"] * 4
    assert [b["symbology"] for b in both(E, img, quads, symbologies=2)["barcodes"]] == ["code39"] * 2


@pytest.mark.parametrize("seed", range(8))
def test_random_pages(E, seed):
    img, quads = R.random_page(seed)
    both(E, img, quads, min_lines=4, hits=True)
    both(E, img, quads, min_lines=6, ink=60, symbologies=1 + seed % 2)


def test_many_bands_page(E):
    r = both(E, R.many_bands_page())
    assert sorted(b["data"] for b in r["barcodes"]) == sorted([b"BAND-0001-xyz", b"998877665544", b"TRACK-42", b"Z9", b"corner"])


def test_local_ink_rule(E):
    """under local ink's bitmap the rule is the same: the host rule against the restatement on local ink's mask; a shaded label reads as the clean one"""
    from tests import ink_ref as I
    img, quads, _ = R.mixed_page()
    shaded = I.shade(img)
    for li in ((16, 38, 2), (8, 60, 0)):
        got, want = E.barcodes_from_page_ink(shaded, quads, local_ink=li), R.barcodes_of_mask(I.ink_mask(shaded, *li)[0], quads)
        same(got, want)
    clean, got = both(E, img, quads), E.barcodes_from_page_ink(shaded, quads)
    assert texts(got) == texts(clean) and np.array_equal(got["item_barcode"], clean["item_barcode"])


def test_refusals(E):
    img = R.blank(40, 40)
    for bad in [(3, 128, 3), (257, 128, 3), (8, 0, 3), (8, 256, 3), (8, 128, 0), (8, 128, 4)]:
        with pytest.raises(Exception, match="min_lines must lie in 4..256"):
            E.barcodes_from_page(img, None, *bad)
    for v in (np.nan, np.inf, 32768.0, -32768.0):
        q = np.asarray([R.quad_box(1, 1, 5, 5)], np.float32)
        q[0, 3] = v
        with pytest.raises(Exception, match="not finite or has"):
            E.barcodes_from_page(img, q)
    lib = E.load()
    buf = np.zeros(8, np.uint8)
    none = (None, 0, None, None, None, None, None, None)
    assert lib.ttr_barcodes_from_page(E._u8(buf), 32768, 1, 0, 8, 128, 3, *none) == -1
    assert b"32768" in lib.ttr_last_error()
    assert lib.ttr_barcodes_from_page(E._u8(buf), 1, 32768, 0, 8, 128, 3, *none) == -1
    assert lib.ttr_barcodes_from_page(None, 4, 4, 0, 8, 128, 3, *none) == -1
    assert lib.ttr_barcodes_from_page(E._u8(buf), 2, 2, 5, 8, 128, 3, *none) == -1       # a stride below 3 w
    with pytest.raises(Exception, match="radius"):
        E.barcodes_from_page_ink(img, None, local_ink=(0, 38, 2))
    with pytest.raises(Exception, match="barcodes must be"):
        E._barcodes_arg("yes")


def test_funsd_page(E):
    """the one real document in the tree has no barcode and must yield none, in any direction; the counters are the host rule's, held to the restatement"""
    from PIL import Image
    img = np.array(Image.open(os.path.join(ROOT, "tests", "data", "funsd_0001129658.png")).convert("RGB"))
    assert img.shape[:2] == (1000, 754)
    r = both(E, img)
    assert r["mode"] == 1 and len(r["barcodes"]) == 0
    assert r["counts"] == [0, 60288, 109, 0, 0, 0]
