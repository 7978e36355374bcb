"""Profile target for the recogniser's final decode (decode_conf_kernel; argmax_kernel on builds before it): 32 synthetic 1024 x 768 pages
(config 5, f16x4, structured synthetic weights) through pages_to_data_dev, one warm-up and four more calls.
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/prof_conf.py [<tree>]
<tree>: the checkout whose tuatara_amd to import (default: this one), so that two builds can be traced with the same script."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tuatara_amd import synth, weights as W                      # noqa: E402
from tuatara_amd.engine import DeviceBuffer, Engine             # noqa: E402

d = tempfile.mkdtemp()
W.make_synthetic_weights(d, seed=0, structured=True)
eng = Engine(d)
pages = np.stack([synth.synthetic_page(i, 1024, 768, n_words=28) for i in range(32)])
buf = DeviceBuffer(pages.nbytes)
buf.upload(pages)
for k in range(5):
    res = eng.pages_to_data_dev(buf, 32, 1024, 768)
print("crops per call", sum(len(r) for r in res))
