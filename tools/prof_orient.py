"""Profile target for word orientation (DESIGN.md "Word orientation"): 32 synthetic 1024 x 768 pages (config 5, f16x4, structured synthetic
weights) through pages_to_data_dev with K candidate turns per word, one warm-up and four more calls.
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/prof_orient.py <K>
K = 1 (orient off), 2 (TTR_ORIENT_FLIP) or 4 (TTR_ORIENT_QUARTER).  Prints the recogniser stage of the last call (packer + every recogniser
pass + the choice, between the stage events) and the page rate over the four timed calls."""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tuatara_amd import synth, weights as W                      # noqa: E402
from tuatara_amd.engine import DeviceBuffer, Engine             # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 4
orient = {1: 0, 2: 1, 4: 2}[K]
d = tempfile.mkdtemp()
W.make_synthetic_weights(d, seed=0, structured=True)
eng = Engine(d, orient=orient)
pages = np.stack([synth.synthetic_page(i, 1024, 768, n_words=28) for i in range(32)])
buf = DeviceBuffer(pages.nbytes)
buf.upload(pages)
res = eng.pages_to_data_dev(buf, 32, 1024, 768)
t0 = time.perf_counter()
for k in range(4):
    res = eng.pages_to_data_dev(buf, 32, 1024, 768)
dt = time.perf_counter() - t0
ms = eng.last_stage_ms()
turns = np.bincount(np.concatenate([r.orient for r in res]), minlength=4).tolist() if K > 1 else None
print(f"K={K}: crops per call {sum(len(r) for r in res)}, pack {ms['pack']:.3f} ms, recogniser stage {ms['parseq']:.3f} ms (last call), "
      f"{4 * 32 / dt:.1f} pages/s over 4 synchronous calls, chosen turns {turns}")
