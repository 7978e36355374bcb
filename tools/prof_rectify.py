"""GPU box tool for the crop packers under rocprofv3 --kernel-trace --stats: one batch of 8 synthetic 1024x768 pages through the whole
hot path, a few steps, in either crop mode (pack_crops_kernel in mode 0, pack_crops_rect_kernel in mode 1, same crops).
    python tools/prof_rectify.py <rotated|grid> <crop_mode> [steps]
rotated: synth.synthetic_rotated_page (words at up to 30 degrees; mostly kind-1 crops in mode 1); grid: the benchmark's cells5x8 pages
with its 40 fixed boxes per page (tuning key bench_grid_boxes; every box is axis-aligned, so mode 1 makes kind-0 crops only)."""
import os, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tuatara_amd import synth, weights as W
from tuatara_amd.engine import DeviceBuffer, Engine

work, mode = sys.argv[1], int(sys.argv[2])
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 4
P, H, Wd = 8, 1024, 768
d = tempfile.mkdtemp()
W.make_synthetic_weights(d, seed=0, structured=True)
eng = Engine(d, crop_mode=mode)
if work == "grid":
    assert eng.set_tuning("bench_grid_boxes", 1) == 0
    pages = np.stack([synth.synthetic_page(i, H, Wd, n_words=40, layout="cells5x8") for i in range(P)])
else:
    pages = np.stack([synth.synthetic_rotated_page(i, H, Wd, n_words=40, max_deg=30.0)[0] for i in range(P)])
buf = DeviceBuffer(pages.nbytes)
buf.upload(pages)
for s in range(steps):
    res = eng.pages_to_data_dev(buf, P, H, Wd)
ms = eng.last_stage_ms()
print(f"{work} crop_mode={mode}: {P} pages, {sum(len(r) for r in res)} crops per step, {steps} steps; last step pack {ms['pack']:.3f} ms, parseq {ms['parseq']:.3f} ms")
