"""Profile target for local ink (DESIGN.md "Local ink"): what the two kernels cost against the bytes they must move, what the layer costs a tables-on and a
deskew-on batch, and that the layer-off path costs what it cost.  The report modes write their sections; `write` joins them into profiles/ink.md.
    python tools/prof_ink.py kernel                 # in this order, each after one warm-up: 5 batches of 16 synthetic shaded 1024 x 768 pages through
                                                    # pages_to_data_dev with tables and local ink on at radius 16, 5 more at radius 64; 5 stage calls
                                                    # (ttr_ink_page) on a synthetic shaded 2480 x 3508 page at radius 16 and 5 at 64; then, for the fixed pixel pass
                                                    # beside them, 5 batches with tables on and local ink off.  Run it in a run of its own as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_ink.py kernel
    python tools/prof_ink.py kernel-report <dir>    # ... then this reads the trace: us per launch of ink_rows_kernel and ink_local_kernel for each of the four,
                                                    # against their algorithmic traffic over the HBM store rate, and table_ink_kernel's
    python tools/prof_ink.py page                   # 16 upright pages per batch; tables on, then deskew on: local ink off and on alternated, 4 rounds of 6 batches
                                                    # after 2 warm-ups: pages per second of either
    python tools/prof_ink.py off-report <label=glob>...   # bench.py's JSON result lines of alternated runs: mean and spread per label
    python tools/prof_ink.py write <dir>            # <dir>/kernel.txt, page.txt, off.txt (the outputs of the three above, off.txt set as a table) and reading.txt (what
                                                    # the figures say, written by hand) -> profiles/ink.md
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
RADII = (16, 64)
mode = sys.argv[1] if len(sys.argv) > 1 else "page"

if mode == "kernel-report":
    files = glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {sys.argv[2]}")
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cases = [(f"16 pages of 1024 x 768, radius {r}", BATCHES, 16 * 1024 * 768, r) for r in RADII] + [(f"one 2480 x 3508 page, radius {r}", CALLS, A4[0] * A4[1], r) for r in RADII]
    print("| kernel | page(s) | mean us | min - max us | algorithmic bytes | at 6.13 TB/s | share of that rate |")
    print("|---|---|---|---|---|---|---|")
    for kernel in ("ink_rows_kernel", "ink_local_kernel"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if kernel in r["Kernel_Name"]]
        assert len(us) == sum(n + 1 for _, n, _, _ in cases), (kernel, len(us))
        k = 0
        for name, n, px, R in cases:
            t = us[k + 1:k + 1 + n]                    # (the first launch of each is the warm-up)
            k += n + 1
            alg = px * 7 if kernel == "ink_rows_kernel" else px * 4 * (64 + 2 * R) / 64      # pass A reads 3 and writes 4 B/px; pass B reads 4 (64 + 2 R) / 64 B/px
            print(f"| `{kernel}` | {name} | {np.mean(t):.1f} | {min(t):.1f} - {max(t):.1f} | {alg / 1e6:.2f} MB | {alg / HBM_STORE * 1e6:.2f} us | "
                  f"{100 * alg / HBM_STORE / (np.mean(t) * 1e-6):.1f} % ({alg / (np.mean(t) * 1e-6) / 1e12:.2f} TB/s) |")
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if "table_ink_kernel" in r["Kernel_Name"]]
    assert len(us) == BATCHES + 1, len(us)
    print(f"\n`table_ink_kernel` (the fixed pixel pass) on the same 16 pages of 1024 x 768: mean {np.mean(us[1:]):.1f} us, min {min(us[1:]):.1f}, max {max(us[1:]):.1f} over {BATCHES} launches.")
    raise SystemExit(0)

if mode == "off-report":
    for arg in sys.argv[2:]:
        label, path = arg.split("=", 1)
        vals, tables = [], set()
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
                    by = (r.get("roofline_craft_family") or {}).get("by_kernel")
                    if by:
                        tables.add(json.dumps(sorted([str(b.get("kernel", b.get("kind"))), b.get("launches_per_pass")] for b in by)))
        print(f"{label}: {len(vals)} runs, pages/s {[round(v, 1) for v in vals]}, mean {np.mean(vals):.1f}, spread {max(vals) - min(vals):.1f}" if vals else f"{label}: no result lines")
        for t in sorted(tables):
            print(f"{label}: launch table {t}")
    raise SystemExit(0)

if mode == "write":
    d = sys.argv[2]

    def piece(name):
        p = os.path.join(d, name)
        return open(p).read().strip() if os.path.exists(p) else "(not measured)"
    with open(os.path.join(ROOT, "profiles", "ink.md"), "w") as f:
        f.write("# Local ink: the two kernels, the layer on a batch, and the layer-off path against the parent build\n\n"
                "Commands (MI355X, synthetic structured weights, f16x4; `tools/prof_ink.py`'s docstring describes the workloads):\n\n"
                "    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_ink.py kernel ; python tools/prof_ink.py kernel-report <dir>   # (a)\n"
                "    python tools/prof_ink.py page                                                                                                                    # (b)\n"
                "    python bench.py --gpus 1 --steps 20 --warmup 5        # (c) the parent build and this build alternated, parent first, one process per run\n"
                "    python tools/prof_ink.py off-report \"parent=<logs>\" \"this=<logs>\"\n\n"
                "Nothing here was fixed in advance.  The pages are synthetic two-column pages under the horizontal illumination ramp of tests/ink_ref.py (1.0 to 0.35);\n"
                "drop 38, dark polarity in (a), the convenience default (16, 38, 2) in (b).  Five launches per row, each after one warm-up.\n\n"
                "## (a) The two kernels against their algorithmic traffic\n\n" + piece("kernel.txt") + "\n\n"
                "## (b) The layer on a tables-on and on a deskew-on batch (16 pages of 1024 x 768 per batch, 4 rounds of 6 batches, off and on alternated)\n\n" + piece("page.txt") + "\n\n"
                "## (c) Local ink off against the parent build (`bench.py --gpus 1 --steps 20 --warmup 5`, alternated, parent first)\n\n" + piece("off.txt") + "\n\n"
                "## Reading\n\n" + piece("reading.txt") + "\n")
    raise SystemExit(0)

from tests import ink_ref as R                                         # noqa: E402
from tuatara_amd import synth, weights as W_                           # noqa: E402
from tuatara_amd.engine import DeviceBuffer, Engine                    # noqa: E402

d = tempfile.mkdtemp()
W_.make_synthetic_weights(d, seed=0, structured=True)
eng = Engine(d)
pages = np.stack([R.shade(synth.synthetic_columns_page(s, 1024, 768, rows=20)[0], 0.35) for s in range(16)])
buf = DeviceBuffer(pages.nbytes)
buf.upload(pages)

if mode == "kernel":
    eng.set_tables(True)
    for r in RADII:
        eng.set_local_ink((r, 38, 0))
        for _ in range(BATCHES + 1):
            res = eng.pages_to_data_dev(buf, 16, 1024, 768)
        print("batch at radius", r, ": words", sum(len(x) for x in res), "inverted", [x.ink["inverted"] if x.ink else None for x in res][:4])
    eng.set_local_ink(False)
    a4 = R.shade(synth.synthetic_columns_page(0, A4[0], A4[1], rows=80)[0], 0.35)
    for r in RADII:
        for _ in range(CALLS + 1):
            out = eng.ink_page(a4, r, 38, 0)
        print("a4 at radius", r, ":", out["ink"], "ink pixels", int(np.unpackbits(out["bits"].view(np.uint8)).sum()))
    for _ in range(BATCHES + 1):                                       # the fixed pixel pass beside them
        eng.pages_to_data_dev(buf, 16, 1024, 768)
    eng.set_tables(False)
else:
    print("| layers | local ink | pages/s per round | median |")
    print("|---|---|---|---|")
    for layer in ("tables", "deskew"):
        getattr(eng, "set_" + layer)(True)
        out = {False: [], True: []}
        for on in (False, True):
            eng.set_local_ink(on)
            for _ in range(2):
                eng.pages_to_data_dev(buf, 16, 1024, 768, keep=False)
        for rnd in range(4):
            for on in (False, True):
                eng.set_local_ink(on)
                t0 = time.perf_counter()
                for _ in range(6):
                    eng.pages_to_data_dev(buf, 16, 1024, 768, keep=False)
                out[on].append(16 * 6 / (time.perf_counter() - t0))
        eng.set_local_ink(False)
        getattr(eng, "set_" + layer)(False)
        for on in (False, True):
            v = out[on]
            print(f"| {layer} on | {'(16, 38, 2)' if on else 'off'} | {', '.join(f'{x:.1f}' for x in v)} | {np.median(v):.1f} |")
