"""Profile target for barcodes (DESIGN.md "Barcodes"): what the two kernels cost beside the marks kernels of the same build on the same pages, what the layer
costs a batch, and that the barcodes-off path costs what it cost.  The figures go to profiles/barcodes.md.
    python tools/prof_barcodes.py kernel               # in this order, each after one warm-up: 5 batches of 16 synthetic 1024 x 768 pages (a drawn code each)
                                                       # through pages_to_data_dev with barcodes and marks on; 10 barcodes and 10 marks stage calls on a
                                                       # 1024 x 768 page dense with codes (48 of them).  Run it in a run of its own as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_barcodes.py kernel
    python tools/prof_barcodes.py kernel-report <dir>  # ... then this reads the trace: us per launch of barcode_scan_kernel, barcode_page_kernel, mark_cand_kernel
                                                       # and mark_page_kernel for each of the two
    python tools/prof_barcodes.py page                 # 16 synthetic 1024 x 768 pages per batch, barcodes off and on alternated, 4 rounds of 6 batches after 2
                                                       # warm-ups: pages per second and the recogniser-side stage ms of either
    python tools/prof_barcodes.py off-report <label=glob>...   # bench.py's JSON result lines of alternated runs: mean and spread per label
    python tools/prof_barcodes.py launches <dir>       # a kernel trace of `bench.py --gpus 1 --steps 20 --warmup 5` -> one line per kernel: its name and its launches;
                                                       # taken on both builds, the two outputs are compared line for line (diff)
    python tools/prof_barcodes.py write <dir>          # joins kernel.txt, page.txt, off.txt, launches.txt and reading.txt of <dir> into profiles/barcodes.md
The barcodes-off comparison is `python bench.py --gpus 1 --steps 20 --warmup 5` on this build and on a checkout of the parent commit, alternated in one call,
one process per run."""
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

BATCHES, CALLS = 5, 10
mode = sys.argv[1] if len(sys.argv) > 1 else "page"


def draw_code(p, data, module, x, y, height, direction=0):
    """clears the place and draws a Code 128 of `data` there (the tests' encoder)"""
    from tests import barcodes_ref as R
    w = R.text128(data)
    n = sum(w) * module
    if direction in (0, 2):
        p[max(y - 4, 0):y + height + 4, max(x - 14, 0):x + n + 14] = 255
    else:
        p[max(y - 14, 0):y + n + 14, max(x - 4, 0):x + height + 4] = 255
    R.draw(p, w, module, x, y, height, direction)
    return p


def dense_page():
    """1024 x 768 (h x w), white, 48 codes of 12 digits: 4 a row, 12 rows of 60 lines"""
    from tests import barcodes_ref as R
    p = R.blank(1024, 768)
    for k in range(48):
        draw_code(p, b"%012d" % (k * 7919), 1, 20 + 185 * (k % 4), 20 + 82 * (k // 4), 60, 2 * (k % 2))
    return p


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
    rows = trace_rows(sys.argv[2])
    for kernel in ("barcode_scan_kernel", "barcode_page_kernel", "mark_cand_kernel", "mark_page_kernel"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if kernel in r["Kernel_Name"]]
        assert len(us) == BATCHES + 1 + CALLS + 1, (kernel, len(us))
        k = 0
        for name, n in (("16 pages of 1024 x 768", BATCHES), ("one 1024 x 768 page dense with codes", CALLS)):
            t = us[k + 1:k + 1 + n]                    # (the first launch of each is the warm-up)
            k += n + 1
            print(f"{kernel}, {name}: mean {np.mean(t):.1f} us, min {min(t):.1f}, max {max(t):.1f} over {len(t)} launches")
    raise SystemExit(0)

if mode == "launches":
    count = {}
    for r in trace_rows(sys.argv[2]):
        name = r["Kernel_Name"].split("(")[0]
        count[name] = count.get(name, 0) + 1
    for name in sorted(count):
        print(f"{count[name]:7d}  {name}")
    print(f"{sum(count.values()):7d}  launches of {len(count)} kernels")
    raise SystemExit(0)

if mode == "write":
    d = sys.argv[2]

    def piece(name):
        p = os.path.join(d, name)
        return open(p).read().strip() if os.path.exists(p) else "(not measured)"
    with open(os.path.join(ROOT, "profiles", "barcodes.md"), "w") as f:
        f.write("# Barcodes: the two kernels, the layer on a batch, and the layer-off path against the parent build\n\n"
                "Commands (MI355X, synthetic structured weights, f16x4; `tools/prof_barcodes.py`'s docstring describes the workloads):\n\n"
                "    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_barcodes.py kernel ; python tools/prof_barcodes.py kernel-report <dir>   # (a)\n"
                "    python tools/prof_barcodes.py page                                                                                                                              # (b)\n"
                "    python bench.py --gpus 1 --steps 20 --warmup 5        # (c) the parent build and this build alternated, parent first, one process per run\n"
                "    python tools/prof_barcodes.py off-report \"parent=<logs>\" \"this=<logs>\"\n"
                "    rocprofv3 --kernel-trace ... -- python bench.py --gpus 1 --steps 20 --warmup 5 on either build ; python tools/prof_barcodes.py launches <dir> ; diff           # (d)\n\n"
                "Nothing here was fixed in advance.  Kernel times are per launch, each series after one warm-up launch that is dropped.\n\n"
                "## (a) The kernels of this build beside the marks kernels: 16 pages of 1024 x 768 (barcodes and marks on) and one page dense with codes (stage calls)\n\n" + piece("kernel.txt") + "\n\n"
                "## (b) The layer on a batch (16 pages of 1024 x 768 per batch, 4 rounds of 6 batches, off and on alternated)\n\n" + piece("page.txt") + "\n\n"
                "## (c) Barcodes off against the parent build (`bench.py --gpus 1 --steps 20 --warmup 5`, alternated, parent first)\n\n" + piece("off.txt") + "\n\n"
                "## (d) The benchmark's launches by kernel, this build against the parent's, line for line\n\n" + piece("launches.txt") + "\n\n"
                "## Reading\n\n" + piece("reading.txt") + "\n")
    raise SystemExit(0)

if mode == "off-report":
    for arg in sys.argv[2:]:
        label, path = arg.split("=", 1)
        vals = []
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
        print(f"{label}: {len(vals)} runs, pages/s {[round(v, 1) for v in vals]}, mean {np.mean(vals):.1f}, spread {max(vals) - min(vals):.1f}" if vals else f"{label}: no result lines")
    raise SystemExit(0)

from tuatara_amd import synth, weights as W_                           # noqa: E402
from tuatara_amd.engine import DeviceBuffer, Engine                    # noqa: E402

d = tempfile.mkdtemp()
W_.make_synthetic_weights(d, seed=0, structured=True)
eng = Engine(d)
pages = np.stack([draw_code(synth.synthetic_page(s, 1024, 768), b"PAGE-%04d" % s, 2, 40 + 20 * s, 60 + 40 * s, 40, s % 4) for s in range(16)])
buf = DeviceBuffer(pages.nbytes)
buf.upload(pages)

if mode == "kernel":
    eng.set_barcodes(True)
    eng.set_marks(True)
    for _ in range(BATCHES + 1):
        res = eng.pages_to_data_dev(buf, 16, 1024, 768)
    eng.set_marks(False)
    eng.set_barcodes(False)
    print("batch: words", sum(len(r) for r in res), "barcodes", sum(len(r.barcode_recs) for r in res), "items inside one", sum(int((r.item_barcode >= 0).sum()) for r in res))
    img = dense_page()
    for _ in range(CALLS + 1):
        r = eng.barcodes_page(img)
    for _ in range(CALLS + 1):
        m = eng.marks_page(img)
    print("dense page", img.shape, "mode", r["mode"], "barcodes", len(r["records"]), "counts (barcodes, candidates, starts, hits, dropped, short chains)", r["counts"], "| marks", len(m["marks"]))
else:
    out = {False: [], True: []}
    ms = {}
    for on in (False, True):
        eng.set_barcodes(on)
        for _ in range(2):
            eng.pages_to_data_dev(buf, 16, 1024, 768, keep=False)
    for rnd in range(4):
        for on in (False, True):
            eng.set_barcodes(on)
            t0 = time.perf_counter()
            for _ in range(6):
                eng.pages_to_data_dev(buf, 16, 1024, 768, keep=False)
            out[on].append(16 * 6 / (time.perf_counter() - t0))
            ms[on] = eng.last_stage_ms()
    eng.set_barcodes(False)
    for on in (False, True):
        v = out[on]
        print(f"barcodes {'on ' if on else 'off'}: pages/s per round {[round(x, 1) for x in v]}, median {np.median(v):.1f}, min {min(v):.1f}, max {max(v):.1f}; stage ms of the last batch "
              f"{ {k: round(float(x), 3) for k, x in ms[on].items()} } (pack = crop packing and the layout layers, barcodes among them)")
