"""Profile target for wide words (DESIGN.md "Wide words"): what the cut kernel and the extra rows cost, and that the default path costs what it cost.
    python tools/prof_wide.py kernel                 # wide_cut_kernel through the stage call: 1, 64 and 512 wide words of n = 4, and 64 of n = 16,
                                                     # one warm-up and 20 launches each; run it as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_wide.py kernel
    python tools/prof_wide.py kernel-report <dir>    # ... then this reads the trace: us per launch of each case (the launches in run order)
    python tools/prof_wide.py stages                 # the benchmark's pages (32 synthetic 1024 x 768 pages of 40 words, detected boxes, rectified crops, f16x4):
                                                     # packing and recogniser stage ms and pages/s with wide off, at 8.0 and at 2.0, alternated, three rounds,
                                                     # and the rows each setting added
    python tools/prof_wide.py page                   # one page, wide off, 10 calls (runs on a build without the feature too): under
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_wide.py page
    python tools/prof_wide.py launches <dir>         # ... the launches per kernel name of that trace (the default path's launch counts on this build and the parent's)
The headline is `python bench.py --gpus 1 --steps 20 --warmup 5`, this build and the parent's alternated, one process per run."""
import csv
import glob
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL_CASES = [(1, 4), (64, 4), (512, 4), (64, 16)]   # (wide words, n)
LAUNCHES = 20
mode = sys.argv[1] if len(sys.argv) > 1 else "stages"


def trace_rows(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {d}")
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return rows


if mode == "kernel-report":
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in trace_rows(sys.argv[2]) if "wide_cut_kernel" in r["Kernel_Name"]]
    per = LAUNCHES + 1
    assert len(us) == per * len(KERNEL_CASES), (len(us), per * len(KERNEL_CASES))
    for k, (words, n) in enumerate(KERNEL_CASES):
        t = us[k * per + 1:(k + 1) * per]                  # (the first launch of a case is its warm-up)
        print(f"wide_cut_kernel, {words} wide words of n = {n}: mean {np.mean(t):.1f} us, min {min(t):.1f}, max {max(t):.1f} over {len(t)} launches")
    raise SystemExit(0)

if mode == "launches":
    count = {}
    for r in trace_rows(sys.argv[2]):
        count[r["Kernel_Name"]] = count.get(r["Kernel_Name"], 0) + 1
    for k in sorted(count):
        print(f"{count[k]:6d}  {k[:150]}")
    print(f"{sum(count.values()):6d}  launches in all, {len(count)} kernel names")
    raise SystemExit(0)

from tuatara_amd import synth, weights as W                               # noqa: E402
from tuatara_amd.engine import CROP_RECTIFIED, DeviceBuffer, Engine     # noqa: E402

d = tempfile.mkdtemp()
W.make_synthetic_weights(d, seed=0, structured=True)
eng = Engine(d, crop_mode=CROP_RECTIFIED)

if mode == "kernel":
    from tests import wide_ref as WR
    img = synth.synthetic_page(0, 1024, 768, n_words=40)
    rng = np.random.default_rng(0)
    for words, n in KERNEL_CASES:
        h = 6.0 if n == 16 else 12.0
        quads = np.stack([WR.quad_of(float(rng.uniform(0, 100)), float(rng.uniform(0, 1000)), (n - 0.5) * 8.0 * h, h, float(rng.uniform(-3, 3))) for _ in range(words)])
        for _ in range(LAUNCHES + 1):
            got_n, cuts, _, _ = eng.wide_cuts(img, quads, 8.0)
        assert (got_n == n).all()
        print(f"{words} wide words of n = {n}: done")

elif mode == "page":
    page = synth.synthetic_page(0, 1024, 768, n_words=40)
    buf = DeviceBuffer(page.nbytes)
    buf.upload(page)
    for _ in range(10):
        res = eng.pages_to_data_dev(buf, 1, 1024, 768)
    print("words", len(res[0]))

else:
    pages = np.stack([synth.synthetic_page(i, 1024, 768, n_words=40) for i in range(32)])
    buf = DeviceBuffer(pages.nbytes)
    buf.upload(pages)
    for rnd in range(3):
        for wide in (0.0, 8.0, 2.0):
            eng.set_wide(wide)
            res = eng.pages_to_data_dev(buf, 32, 1024, 768)
            t0 = time.perf_counter()
            for _ in range(4):
                res = eng.pages_to_data_dev(buf, 32, 1024, 768)
            dt = time.perf_counter() - t0
            ms = eng.last_stage_ms()
            pack_ms, rec_ms = ms["pack"], ms["parseq"]
            items = sum(len(p) for p in res)
            rows = sum(int(p.piece_first[-1]) for p in res if p.piece_first is not None) if wide else items
            wide_items = sum(int((np.diff(p.piece_first) > 1).sum()) for p in res if p.piece_first is not None) if wide else 0
            print(f"round {rnd} wide {wide:4.1f}: {4 * 32 / dt:7.1f} pages/s  pack {pack_ms:.3f} ms  recogniser {rec_ms:.3f} ms  items {items}  wide items {wide_items}  rows added {rows - items}")
    eng.set_wide(0)
