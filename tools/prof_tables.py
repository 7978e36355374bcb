"""Profile target for tables (DESIGN.md "Tables"): what the two kernels cost, what the layer costs a batch, and that the tables-off path costs what it cost.
The figures go to profiles/tables.md.
    python tools/prof_tables.py kernel                 # in this order, each after one warm-up: 5 batches of 16 synthetic 1024 x 768 pages through
                                                       # pages_to_data_dev with tables on; 10 stage calls on a synthetic 2480 x 3508 page; 10 on the FUNSD page;
                                                       # 10 on a page of exactly 8192 horizontal runs.  Run it in a run of its own as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_tables.py kernel
    python tools/prof_tables.py kernel-report <dir>    # ... then this reads the trace: us per launch of either kernel for each of the four, the pixel pass against
                                                       # its algorithmic bytes over the HBM rate
    python tools/prof_tables.py page                   # 16 synthetic 1024 x 768 pages per batch, tables off and on alternated, 4 rounds of 6 batches after 2
                                                       # warm-ups: pages per second and the recogniser-side stage ms of either
    python tools/prof_tables.py off-report <label=glob>...   # bench.py's JSON result lines of alternated runs: mean and spread per label
The tables-off comparison is `python bench.py --gpus 1 --steps 20 --warmup 5` on this build and on the parent's, alternated in one call, one process per run."""
import csv
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes/s, the part's specification; a float4 copy reaches 6.29e12 of it
HBM_COPY = 6.29e12
BATCHES, CALLS = 5, 10
A4 = (3508, 2480)
mode = sys.argv[1] if len(sys.argv) > 1 else "page"


def cap_page():
    """exactly 8192 horizontal runs: 256 rows of 32 dashes of 12 px"""
    img = np.full((256, 512, 3), 255, np.uint8)
    for x in range(0, 512, 16):
        img[:, x:x + 12] = 0
    return img


if mode == "kernel-report":
    files = glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {sys.argv[2]}")
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for kernel in ("table_ink_kernel", "table_grid_kernel"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if kernel in r["Kernel_Name"]]
        assert len(us) == BATCHES + 1 + 3 * (CALLS + 1), (kernel, len(us))
        parts, k = [], 0
        for name, n, nbytes in (("16 pages of 1024 x 768", BATCHES, 16 * 1024 * 768 * 3), ("one 2480 x 3508 page", CALLS, A4[0] * A4[1] * 3), ("the FUNSD page (754 x 1000)", CALLS, 754 * 1000 * 3),
                                ("a page at the run cap (512 x 256)", CALLS, 512 * 256 * 3)):
            t = us[k + 1:k + 1 + n]                    # (the first launch of each is the warm-up)
            k += n + 1
            line = f"{kernel}, {name}: mean {np.mean(t):.1f} us, min {min(t):.1f}, max {max(t):.1f} over {len(t)} launches"
            if kernel == "table_ink_kernel":
                alg = nbytes * (1 + 2 / 24)            # every page byte read once; two bitmaps of one bit per pixel written
                line += (f"; page bytes {nbytes / 1e6:.2f} MB (+ {nbytes / 12e6:.2f} MB of bitmaps): {alg / HBM_PEAK * 1e6:.2f} us at the 8.0 TB/s peak, {alg / HBM_COPY * 1e6:.2f} us at a "
                         f"float4 copy's 6.29 TB/s; mean launch = {100 * alg / HBM_PEAK / (np.mean(t) * 1e-6):.1f} % of the peak, {alg / (np.mean(t) * 1e-6) / 1e12:.2f} TB/s")
            parts.append(line)
        print("\n".join(parts))
    raise SystemExit(0)

if mode == "off-report":
    for arg in sys.argv[2:]:
        label, path = arg.split("=", 1)
        vals, disp = [], []
        for f in sorted(glob.glob(path)):
            for line in open(f):
                line = line.strip()
                if line.startswith("{"):
                    try:
                        r = json.loads(line)
                    except ValueError:
                        continue
                    v = r.get("pages_per_s", r.get("pages_per_sec", r.get("value")))
                    if v is not None:
                        vals.append(float(v))
                        disp += [r[k] for k in ("dispatches", "dispatch_count", "kernel_launches", "launches_per_step") if k in r][:1]
        print(f"{label}: {len(vals)} runs, pages/s {[round(v, 1) for v in vals]}, mean {np.mean(vals):.1f}, spread {max(vals) - min(vals):.1f}, dispatches {sorted(set(disp))}"
              if vals else f"{label}: no result lines")
    raise SystemExit(0)

from tuatara_amd import synth, weights as W_                           # noqa: E402
from tuatara_amd.engine import DeviceBuffer, Engine                    # noqa: E402

d = tempfile.mkdtemp()
W_.make_synthetic_weights(d, seed=0, structured=True)
eng = Engine(d)
pages = np.stack([synth.synthetic_page(s, 1024, 768) for s in range(16)])
for p in pages:                                                        # a 6 x 4 grid over every page, so that tables, cells and words in cells occur
    for i in range(7):
        p[40 + 150 * i:42 + 150 * i, 30:732] = 0
    for j in range(5):
        p[40:942, 30 + 175 * j:32 + 175 * j] = 0
buf = DeviceBuffer(pages.nbytes)
buf.upload(pages)

if mode == "kernel":
    from PIL import Image
    eng.set_tables(True)
    for _ in range(BATCHES + 1):
        res = eng.pages_to_data_dev(buf, 16, 1024, 768)
    eng.set_tables(False)
    print("batch: words", sum(len(r) for r in res), "tables", sum(len(r.tables) for r in res), "words in cells", sum(int((r.item_cell >= 0).sum()) for r in res if r.item_cell is not None))
    a4 = synth.synthetic_page(0, A4[0], A4[1], n_words=400)
    funsd = np.array(Image.open(os.path.join(ROOT, "tests", "data", "funsd_0001129658.png")).convert("RGB"))
    for name, img in (("a4", a4), ("funsd", funsd), ("cap", cap_page())):
        for _ in range(CALLS + 1):
            r = eng.tables_page(img, None, 48, 128)
        print(name, img.shape, "mode", r["mode"], "rulings", len(r["rulings"]), "tables", len(r["tables"]))
else:
    out = {False: [], True: []}
    ms = {}
    for on in (False, True):
        eng.set_tables(on)
        for _ in range(2):
            eng.pages_to_data_dev(buf, 16, 1024, 768, keep=False)
    for rnd in range(4):
        for on in (False, True):
            eng.set_tables(on)
            t0 = time.perf_counter()
            for _ in range(6):
                eng.pages_to_data_dev(buf, 16, 1024, 768, keep=False)
            out[on].append(16 * 6 / (time.perf_counter() - t0))
            ms[on] = eng.last_stage_ms()
    eng.set_tables(False)
    for on in (False, True):
        v = out[on]
        print(f"tables {'on ' if on else 'off'}: pages/s per round {[round(x, 1) for x in v]}, median {np.median(v):.1f}, min {min(v):.1f}, max {max(v):.1f}; stage ms of the last batch "
              f"{ {k: round(float(x), 3) for k, x in ms[on].items()} } (pack = crop packing and the layout layers, tables among them)")
