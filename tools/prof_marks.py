"""Profile target for selection marks (DESIGN.md "Selection marks"): what the two kernels cost beside tables' grid pass on the same pages, what the layer costs a
batch, and that the marks-off path costs what it cost.  The figures go to profiles/marks.md.
    python tools/prof_marks.py kernel                  # in this order, each after one warm-up: 5 batches of 16 synthetic 1024 x 768 pages through
                                                       # pages_to_data_dev with marks and tables on; 10 marks and 10 tables stage calls on a synthetic
                                                       # 2480 x 3508 page; the same on the page of 513 boxes.  Run it in a run of its own as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_marks.py kernel
    python tools/prof_marks.py kernel-report <dir>     # ... then this reads the trace: us per launch of mark_cand_kernel, mark_page_kernel, table_ink_kernel and
                                                       # table_grid_kernel for each of the three, the candidate pass against the bitmaps' bytes over the HBM rate
    python tools/prof_marks.py page                    # 16 synthetic 1024 x 768 pages per batch, marks off and on alternated, 4 rounds of 6 batches after 2
                                                       # warm-ups: pages per second and the recogniser-side stage ms of either
    python tools/prof_marks.py off-report <label=glob>...   # bench.py's JSON result lines of alternated runs: mean and spread per label
    python tools/prof_marks.py tables-kernel           # the tables stage calls of `kernel` alone, through nothing the parent commit lacks: a copy of this file in
                                                       # a checkout of the parent commit gives table_grid_kernel's times of the parent build on the same pages
    python tools/prof_marks.py tables-report <dir>     # ... and reads that trace
    python tools/prof_marks.py launches <dir>          # a kernel trace of `bench.py --gpus 1 --steps 20 --warmup 5` -> one line per kernel: its name and its launches;
                                                       # taken on both builds, the two outputs are compared line for line (diff)
    python tools/prof_marks.py write <dir>             # joins kernel.txt, parent_grid.txt, page.txt, off.txt, launches.txt and reading.txt of <dir> into profiles/marks.md
The marks-off comparison is `python bench.py --gpus 1 --steps 20 --warmup 5` on this build and on a checkout of the parent commit, alternated in one call, one
process per run."""
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

HBM_PEAK = 8.0e12        # bytes/s, the part's specification
BATCHES, CALLS = 5, 10
A4 = (3508, 2480)
mode = sys.argv[1] if len(sys.argv) > 1 else "page"


def boxes_page(n=513):
    """the tests' page of n boxes of 8 px at 10-px pitch (tests/marks_ref.py)"""
    from tests import marks_ref
    return marks_ref.box_grid(n)


def draw_boxes(p, n, seed):
    """n 16-px frames at seeded places of page p, every third one crossed"""
    rng = np.random.default_rng(seed)
    h, w = p.shape[:2]
    for k in range(n):
        x, y = int(rng.integers(8, w - 30)), int(rng.integers(8, h - 30))
        p[y - 4:y + 20, x - 4:x + 20] = 255
        p[y:y + 2, x:x + 16] = 0; p[y + 14:y + 16, x:x + 16] = 0; p[y:y + 16, x:x + 2] = 0; p[y:y + 16, x + 14:x + 16] = 0
        if k % 3 == 0:
            for j in range(8):
                p[y + 4 + j, x + 4 + j] = 0; p[y + 4 + j, x + 11 - j] = 0
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
    sizes = (("16 pages of 1024 x 768", BATCHES, 16 * 1024 * 768), ("one 2480 x 3508 page", CALLS, A4[0] * A4[1]), ("the page of 513 boxes (324 x 174)", CALLS, 324 * 174))
    for kernel in ("mark_cand_kernel", "mark_page_kernel", "table_ink_kernel", "table_grid_kernel"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if kernel in r["Kernel_Name"]]
        # (the pixel pass runs once per batch and once per stage call of either layer: twice as many stage launches as the others)
        per = [BATCHES + 1] + [(CALLS + 1) * (2 if kernel == "table_ink_kernel" else 1)] * 2
        assert len(us) == sum(per), (kernel, len(us), per)
        k = 0
        for (name, n, px), m in zip(sizes, per):
            t = us[k + 1:k + 1 + n]                    # (the first launch of each is the warm-up; of the pixel pass's stage launches the marks calls' come first)
            k += m
            line = f"{kernel}, {name}: mean {np.mean(t):.1f} us, min {min(t):.1f}, max {max(t):.1f} over {len(t)} launches"
            if kernel == "mark_cand_kernel":
                alg = px / 8 * 2                       # both bitmaps read once, one bit per pixel each
                line += f"; both bitmaps {alg / 1e6:.3f} MB: {alg / HBM_PEAK * 1e6:.3f} us at the 8.0 TB/s peak; mean launch = {100 * alg / HBM_PEAK / (np.mean(t) * 1e-6):.2f} % of the peak"
            print(line)
    raise SystemExit(0)

if mode == "tables-report":
    rows = trace_rows(sys.argv[2])
    for kernel in ("table_ink_kernel", "table_grid_kernel"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if kernel in r["Kernel_Name"]]
        assert len(us) == BATCHES + 1 + 2 * (CALLS + 1), (kernel, len(us))
        k = 0
        for name, n in (("16 pages of 1024 x 768", BATCHES), ("one 2480 x 3508 page", CALLS), ("the page of 513 boxes (324 x 174)", CALLS)):
            t = us[k + 1:k + 1 + n]
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
    with open(os.path.join(ROOT, "profiles", "marks.md"), "w") as f:
        f.write("# Selection marks: the two kernels, the layer on a batch, and the layer-off path against the parent build\n\n"
                "Commands (MI355X, synthetic structured weights, f16x4; `tools/prof_marks.py`'s docstring describes the workloads):\n\n"
                "    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_marks.py kernel ; python tools/prof_marks.py kernel-report <dir>   # (a)\n"
                "    the same with `tables-kernel` / `tables-report` from a copy of the tool in a checkout of the parent commit                                              # (b)\n"
                "    python tools/prof_marks.py page                                                                                                                        # (c)\n"
                "    python bench.py --gpus 1 --steps 20 --warmup 5        # (d) the parent build and this build alternated, parent first, one process per run\n"
                "    python tools/prof_marks.py off-report \"parent=<logs>\" \"this=<logs>\"\n"
                "    rocprofv3 --kernel-trace ... -- python bench.py --gpus 1 --steps 20 --warmup 5 on either build ; python tools/prof_marks.py launches <dir> ; diff     # (e)\n\n"
                "Nothing here was fixed in advance.  Kernel times are per launch, each series after one warm-up launch that is dropped.\n\n"
                "## (a) The kernels of this build: 16 pages of 1024 x 768 (marks and tables on), one 2480 x 3508 page and the page of 513 boxes (stage calls)\n\n" + piece("kernel.txt") + "\n\n"
                "## (b) `table_ink_kernel` and `table_grid_kernel` of the parent build on the same pages\n\n" + piece("parent_grid.txt") + "\n\n"
                "## (c) The layer on a batch (16 pages of 1024 x 768 per batch, 4 rounds of 6 batches, off and on alternated)\n\n" + piece("page.txt") + "\n\n"
                "## (d) Marks off against the parent build (`bench.py --gpus 1 --steps 20 --warmup 5`, alternated, parent first)\n\n" + piece("off.txt") + "\n\n"
                "## (e) The benchmark's launches by kernel, this build against the parent's, line for line\n\n" + piece("launches.txt") + "\n\n"
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
pages = np.stack([draw_boxes(synth.synthetic_page(s, 1024, 768), 12, s) for s in range(16)])
buf = DeviceBuffer(pages.nbytes)
buf.upload(pages)

if mode == "tables-kernel":
    eng.set_tables(True)
    for _ in range(BATCHES + 1):
        res = eng.pages_to_data_dev(buf, 16, 1024, 768)
    eng.set_tables(False)
    a4 = draw_boxes(synth.synthetic_page(0, A4[0], A4[1], n_words=400), 60, 99)
    for name, img in (("a4", a4), ("513 boxes", boxes_page())):
        for _ in range(CALLS + 1):
            t = eng.tables_page(img, None, 48, 128)
        print(name, img.shape, "tables mode", t["mode"], "runs", t["runs"])
elif mode == "kernel":
    eng.set_marks(True)
    eng.set_tables(True)
    for _ in range(BATCHES + 1):
        res = eng.pages_to_data_dev(buf, 16, 1024, 768)
    eng.set_tables(False)
    eng.set_marks(False)
    print("batch: words", sum(len(r) for r in res), "marks", sum(len(r.mark_recs) for r in res), "selected", sum(int(r.mark_recs[:, 10].sum()) for r in res),
          "labelled", sum(int((r.mark_recs[:, 11] >= 0).sum()) for r in res))
    a4 = draw_boxes(synth.synthetic_page(0, A4[0], A4[1], n_words=400), 60, 99)
    for name, img, arg in (("a4", a4, (10, 64, 24, 128)), ("513 boxes", boxes_page(), (8, 64, 24, 128))):
        for _ in range(CALLS + 1):
            r = eng.marks_page(img, None, *arg)
        for _ in range(CALLS + 1):
            t = eng.tables_page(img, None, 48, 128)
        print(name, img.shape, "mode", r["mode"], "marks", len(r["marks"]), "corners", r["corners"], "kept", r["kept"], "| tables mode", t["mode"], "runs", t["runs"])
else:
    out = {False: [], True: []}
    ms = {}
    for on in (False, True):
        eng.set_marks(on)
        for _ in range(2):
            eng.pages_to_data_dev(buf, 16, 1024, 768, keep=False)
    for rnd in range(4):
        for on in (False, True):
            eng.set_marks(on)
            t0 = time.perf_counter()
            for _ in range(6):
                eng.pages_to_data_dev(buf, 16, 1024, 768, keep=False)
            out[on].append(16 * 6 / (time.perf_counter() - t0))
            ms[on] = eng.last_stage_ms()
    eng.set_marks(False)
    for on in (False, True):
        v = out[on]
        print(f"marks {'on ' if on else 'off'}: pages/s per round {[round(x, 1) for x in v]}, median {np.median(v):.1f}, min {min(v):.1f}, max {max(v):.1f}; stage ms of the last batch "
              f"{ {k: round(float(x), 3) for k, x in ms[on].items()} } (pack = crop packing and the layout layers, marks among them)")
