"""Profile target for curved words (DESIGN.md "Curved words"): what the kernel costs, and that the default path costs what it cost.
    python tools/prof_curve.py kernel                # curve_crop_kernel through the stage call: 1, 8, 64 and 512 words (half of them arched), one warm-up and
                                                     # 20 launches each; run it as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_curve.py kernel
    python tools/prof_curve.py kernel-report <dir>   # ... then this reads the trace: us per launch of each case (the launches in run order)
    python tools/prof_curve.py stages                # the benchmark's pages (32 synthetic 1024 x 768 pages of 40 words, detected boxes, rectified crops, f16x4):
                                                     # packing and recogniser stage ms and pages/s with curved off and on, alternated, three rounds
    python tools/prof_curve.py page                  # one page, curved off, 10 calls (runs on a build without the feature too): under
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_curve.py page
    python tools/prof_curve.py launches <dir>        # ... the launches per kernel name of that trace (the default path's launch counts on this build and the parent's)
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

KERNEL_CASES = [1, 8, 64, 512]   # words per launch
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
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in trace_rows(sys.argv[2]) if "curve_crop_kernel" in r["Kernel_Name"]]
    per = LAUNCHES + 1
    assert len(us) == per * len(KERNEL_CASES), (len(us), per * len(KERNEL_CASES))
    for k, words in enumerate(KERNEL_CASES):
        t = us[k * per + 1:(k + 1) * per]                  # (the first launch of a case is its warm-up)
        print(f"curve_crop_kernel, {words} words: mean {np.mean(t):.1f} us, min {min(t):.1f}, max {max(t):.1f} over {len(t)} launches")
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
    from tests import curve_ref as CV
    img, quad = CV.arc_word(11, 10.0, 20.0, 150.0, 10.0, True, True)
    straight = CV.quad_of(128.0, 40.0, 150.0, 30.0, 3.0)
    for words in KERNEL_CASES:
        quads = np.stack([quad if i % 2 == 0 else straight for i in range(words)])
        for _ in range(LAUNCHES + 1):
            flag = eng.curve_crops(img, quads)[0]
        assert flag[0] == 1 and int(flag.sum()) == (words + 1) // 2
        print(f"{words} words: done")

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
        for on in (False, True):
            eng.set_curved(on)
            res = eng.pages_to_data_dev(buf, 32, 1024, 768)
            t0 = time.perf_counter()
            for _ in range(4):
                res = eng.pages_to_data_dev(buf, 32, 1024, 768)
            dt = time.perf_counter() - t0
            ms = eng.last_stage_ms()
            items = sum(len(p) for p in res)
            flagged = sum(int(p.curved.sum()) for p in res if p.curved is not None)
            print(f"round {rnd} curved {int(on)}: {4 * 32 / dt:7.1f} pages/s  pack {ms['pack']:.3f} ms  recogniser {ms['parseq']:.3f} ms  items {items}  curved items {flagged}")
    eng.set_curved(False)
