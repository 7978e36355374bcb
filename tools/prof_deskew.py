"""Profile target for deskew (DESIGN.md "Deskew"): what the two kernels cost, what the layer costs a batch, and that the layer-off path costs what it cost.
The figures go to profiles/deskew.md.
    python tools/prof_deskew.py kernel                 # in this order, each after one warm-up: 5 batches of 16 synthetic 1024 x 768 pages, each tilted by its own
                                                       # slope, through pages_to_data_dev with deskew on at max_slope 64, 5 more at 128; 5 stage calls on a synthetic
                                                       # 2480 x 3508 page at 64 and 5 at 128.  Run it in a run of its own as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_deskew.py kernel
    python tools/prof_deskew.py kernel-report <dir>    # ... then this reads the trace: us per launch of the pixel pass and the two kernels for each of the four,
                                                       # the rotate kernel against its bytes (a page read once and written once) over the HBM store rate
    python tools/prof_deskew.py page                   # the same 16 pages upright per batch (every slope 0: both settings read the same words), deskew off and on alternated, 4 rounds of 6 batches after 2 warm-ups: pages per
                                                       # second and the stage ms of either
    python tools/prof_deskew.py off-report <label=glob>...   # bench.py's JSON result lines of alternated runs: mean and spread per label
The layer-off comparison is `python bench.py --gpus 1 --steps 20 --warmup 5` on this build and on the parent's, alternated in one call, one process per run."""
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

HBM_STORE = 6.13e12      # bytes/s: what profiles/r06_store_rate.txt records for plain stores at one workgroup per CU
BATCHES, CALLS = 5, 5
A4 = (3508, 2480)
SLOPES = (-60, -45, -31, -18, -9, -5, 0, 0, 5, 7, 12, 18, 27, 37, 50, 64)
mode = sys.argv[1] if len(sys.argv) > 1 else "page"

if mode == "kernel-report":
    files = glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {sys.argv[2]}")
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cases = (("16 pages of 1024 x 768, max_slope 64", BATCHES, 16 * 1024 * 768 * 3), ("16 pages of 1024 x 768, max_slope 128", BATCHES, 16 * 1024 * 768 * 3),
             ("one 2480 x 3508 page, max_slope 64", CALLS, A4[0] * A4[1] * 3), ("one 2480 x 3508 page, max_slope 128", CALLS, A4[0] * A4[1] * 3))
    for kernel in ("table_ink_kernel", "deskew_score_kernel", "deskew_rotate_kernel"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if kernel in r["Kernel_Name"]]
        assert len(us) == sum(n + 1 for _, n, _ in cases), (kernel, len(us))
        k = 0
        for name, n, nbytes in cases:
            t = us[k + 1:k + 1 + n]                    # (the first launch of each is the warm-up)
            k += n + 1
            line = f"{kernel}, {name}: mean {np.mean(t):.1f} us, min {min(t):.1f}, max {max(t):.1f} over {len(t)} launches"
            if kernel == "deskew_rotate_kernel":
                alg = 2 * nbytes                       # every page byte read once and written once
                line += (f"; {alg / 1e6:.2f} MB to move: {alg / HBM_STORE * 1e6:.2f} us at the store rate of {HBM_STORE / 1e12:.1f} TB/s; mean launch = "
                         f"{100 * alg / HBM_STORE / (np.mean(t) * 1e-6):.1f} % of it, {alg / (np.mean(t) * 1e-6) / 1e12:.2f} TB/s")
            print(line)
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

from tests import deskew_ref as R                                      # noqa: E402
from tuatara_amd import synth, weights as W_                           # noqa: E402
from tuatara_amd.engine import DeviceBuffer, Engine                    # noqa: E402

d = tempfile.mkdtemp()
W_.make_synthetic_weights(d, seed=0, structured=True)
eng = Engine(d)
# (page mode reads the pages upright, so that layer off and layer on read the same words and differ by the layer's three launches and two copies alone)
pages = np.stack([R.tilt(synth.synthetic_columns_page(s, 1024, 768, rows=20)[0], k) if k and mode == "kernel" else synth.synthetic_columns_page(s, 1024, 768, rows=20)[0]
                  for s, k in enumerate(SLOPES)])
buf = DeviceBuffer(pages.nbytes)
buf.upload(pages)

if mode == "kernel":
    for m in (64, 128):
        eng.set_deskew((m, 288, 128))
        for _ in range(BATCHES + 1):
            res = eng.pages_to_data_dev(buf, 16, 1024, 768)
        print("batch at max_slope", m, ": slopes", [r.skew["slope"] for r in res], "words", sum(len(r) for r in res))
    eng.set_deskew(False)
    a4 = R.tilt(synth.synthetic_columns_page(0, A4[0], A4[1], rows=80)[0], 27)
    for m in (64, 128):
        for _ in range(CALLS + 1):
            r = eng.deskew_page(a4, m, 288, 128)
        print("a4 at max_slope", m, ":", r["skew"])
else:
    out = {False: [], True: []}
    ms = {}
    for on in (False, True):
        eng.set_deskew(on)
        for _ in range(2):
            eng.pages_to_data_dev(buf, 16, 1024, 768, keep=False)
    for rnd in range(4):
        for on in (False, True):
            eng.set_deskew(on)
            t0 = time.perf_counter()
            for _ in range(6):
                eng.pages_to_data_dev(buf, 16, 1024, 768, keep=False)
            out[on].append(16 * 6 / (time.perf_counter() - t0))
            ms[on] = eng.last_stage_ms()
    eng.set_deskew(False)
    for on in (False, True):
        v = out[on]
        print(f"deskew {'on ' if on else 'off'}: pages/s per round {[round(x, 1) for x in v]}, median {np.median(v):.1f}, min {min(v):.1f}, max {max(v):.1f}; stage ms of the last batch "
              f"{ {k: round(float(x), 3) for k, x in ms[on].items()} } (the layer's three launches run in front of the detector stage's first event: none of the four holds them)")
