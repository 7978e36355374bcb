"""Profile target for tiled pages (DESIGN.md "Tiled pages"): what the stitch kernel costs on an A4 scan, what such a page costs tiled, and that the
tiling-off path costs what it cost.  The figures go to profiles/tiles.md.
    python tools/prof_tiles.py kernel                # tile_stitch_kernel through the stage call on the 12 tile maps of a 2480 x 3508 page (overlap 128): one
                                                     # warm-up and 20 launches; run it in a run of its own as
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_tiles.py kernel
    python tools/prof_tiles.py kernel-report <dir>   # ... then this reads the trace: us per launch, against the kernel's algorithmic bytes over the HBM peak
    python tools/prof_tiles.py page                  # a synthetic 2480 x 3508 page, tiled (12 tiles of 1024 x 1024): pages per second over 8 calls after 2
                                                     # warm-ups, the detector stage's ms (CRAFT + stitch), and the words found; then the same page with tiling off
    python tools/prof_tiles.py off-report <file>...  # bench.py's JSON result lines of alternated runs, named label=path: mean and spread per label
The tiling-off comparison is `python bench.py --gpus 1 --steps 20 --warmup 5` on this build and on the parent's, alternated in one call, one process per run."""
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

H, W, OVERLAP, LAUNCHES = 3508, 2480, 128, 20
HBM_PEAK = 8.0e12        # bytes/s, the part's specification; a float4 copy reaches 6.29e12 of it
HBM_COPY = 6.29e12
mode = sys.argv[1] if len(sys.argv) > 1 else "page"

if mode == "kernel-report":
    files = glob.glob(os.path.join(sys.argv[2], "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {sys.argv[2]}")
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if "tile_stitch_kernel" in r["Kernel_Name"]]
    assert len(us) == LAUNCHES + 1, len(us)
    t = us[1:]                                         # (the first launch is the warm-up)
    from tuatara_amd import engine as E
    p = E.tile_plan(H, W, 1024, OVERLAP)
    out_bytes = p.H2 * p.W2 * 8
    alg = 2 * out_bytes                                # every page-map byte written once, and one tile byte read for it (the bands read two to four)
    print(f"tile_stitch_kernel, {H} x {W} page, {p.tiles} tiles, page map {p.H2} x {p.W2}: mean {np.mean(t):.1f} us, min {min(t):.1f}, max {max(t):.1f} over {len(t)} launches")
    print(f"algorithmic bytes {alg / 1e6:.1f} MB (read {out_bytes / 1e6:.1f} + write {out_bytes / 1e6:.1f}): {alg / HBM_PEAK * 1e6:.1f} us at the 8.0 TB/s peak, "
          f"{alg / HBM_COPY * 1e6:.1f} us at a float4 copy's 6.29 TB/s; mean launch = {100 * alg / HBM_PEAK / (np.mean(t) * 1e-6):.0f} % of the peak (bandwidth-bound)")
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

if mode == "kernel":
    p = eng.tile_plan(H, W, OVERLAP)
    tiles = np.random.default_rng(0).standard_normal((p.tiles, p.Hc // 2, p.Wc // 2, 2)).astype(np.float32)
    for _ in range(LAUNCHES + 1):
        out = eng.stitch_heat(tiles, p.oy, p.ox, p.Hc, p.Wc, p.H2, p.W2)
    print("page map", out.shape, "tiles", p.tiles)
else:
    page = synth.synthetic_page(0, H, W, n_words=400)
    buf = DeviceBuffer(page.nbytes)
    buf.upload(page)
    for overlap in (OVERLAP, 0):
        eng.set_tiled(overlap)
        for _ in range(2):
            res = eng.pages_to_data_dev(buf, 1, H, W)
        t0 = time.perf_counter()
        for _ in range(8):
            res = eng.pages_to_data_dev(buf, 1, H, W)
        dt = time.perf_counter() - t0
        ms = eng.last_stage_ms()
        print(f"{H} x {W} page, tiled {overlap}: {8 / dt:.2f} pages/s ({dt / 8 * 1e3:.1f} ms per page), stage ms {ms}, tiles {res[0].tiles}, words {len(res[0])}")
    eng.set_tiled(0)
