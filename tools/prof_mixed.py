"""GPU box tool for mixed-size batches (DESIGN.md "Mixed-size batches"; results in profiles/mixed_batches.md).
    python tools/prof_mixed.py gain [rounds] [lists]      # (a) the 64-page list of 16 sizes on one canvas: pages/s with mixed_batches 0 and 1, alternated in one process
    python tools/prof_mixed.py uniform [rounds] [lists]   # (b) a uniform 64-page list, flag off: pages/s of THIS tree's build (run the same file from a checkout of the
                                                          #     parent commit for the other side, the two processes alternated)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/prof_mixed.py kernels   # (c) the same 64-page list once with the flag off (uniform kernels,
                                                          #     16 batches of 4) and once with it on (table kernels, 2 batches of 32), after two warm-up lists of each;
                                                          #     `kernels 1`: crop_mode = 1 and orient = flip, so that both packer launches of a batch are the rect kernel
                                                          #     (the words' own crops of kind 0, their upside-down twins of kind 1)
The list: 64 windows of synthetic 1024 x 768 pages in 16 sizes (1024 - 2 i) x (768 - i), i = 0 .. 15, four of each, interleaved; every size has the
1024 x 768 canvas at ratio 1.  A measurement is `lists` calls of images_to_data (each ends with its results on the host); `rounds` measurements per
variant, alternated; min - max over the rounds is reported."""
import json, os, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tuatara_amd import synth, weights as W
from tuatara_amd.engine import Engine

mode = sys.argv[1] if len(sys.argv) > 1 else "gain"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
lists = int(sys.argv[3]) if len(sys.argv) > 3 else 5
N, SIZES = 64, 16


def mixed_list():
    pages = []
    for k in range(N):
        i = k % SIZES
        pages.append(np.ascontiguousarray(synth.synthetic_page(300 + k, 1024, 768, n_words=40)[:1024 - 2 * i, :768 - i]))
    return pages


def rate(eng, pages):
    t0 = time.perf_counter()
    for _ in range(lists):
        eng.images_to_data(pages, keep=False)
    return lists * len(pages) / (time.perf_counter() - t0)


d = tempfile.mkdtemp()
W.make_synthetic_weights(d, seed=0, structured=True)
if mode == "uniform":
    pages = [synth.synthetic_page(300 + k, 1024, 768, n_words=40) for k in range(N)]
    eng = Engine(d)
    for _ in range(2):
        eng.images_to_data(pages, keep=False)
    r = [rate(eng, pages) for _ in range(rounds)]
    print(json.dumps({"mode": "uniform", "lib": os.path.abspath(sys.modules["tuatara_amd.engine"].lib_path()), "pages_per_s": [round(x, 1) for x in r],
                      "min": round(min(r), 1), "max": round(max(r), 1)}))
    sys.exit(0)

pages = mixed_list()
assert len({p.shape for p in pages}) == SIZES
rect = mode == "kernels" and len(sys.argv) > 2 and sys.argv[2] == "1"
engs = {flag: Engine(d, mixed_batches=flag, **(dict(crop_mode=1, orient=1) if rect else {})) for flag in (0, 1)}
assert {engs[1].canvas_geometry(*p.shape[:2]) for p in pages} == {(1024, 768, 1.0)}
batches = {}
for flag, eng in engs.items():                          # warm-up: every shape, both engines
    for _ in range(2):
        eng.images_to_data(pages, keep=False)
    batches[flag] = eng.last_images_batches()
if mode == "kernels":                                   # one traced list per variant
    counts = {flag: sum(eng.images_to_data(pages, keep=False)) for flag, eng in engs.items()}
    print(json.dumps({"mode": "kernels", "rect": rect, "batches": {str(k): v for k, v in batches.items()}, "items": counts}))
    sys.exit(0)
r = {0: [], 1: []}
for _ in range(rounds):
    for flag in (0, 1):
        r[flag].append(rate(engs[flag], pages))
a, b = engs[0].images_to_data(pages), engs[1].images_to_data(pages)
same = all([x["text"] for x in p] == [x["text"] for x in q] and [x["bbox"] for x in p] == [x["bbox"] for x in q] for p, q in zip(a, b))
print(json.dumps({"mode": "gain", "pages": N, "sizes": SIZES, "lists_per_measurement": lists, "batches_flag0": batches[0], "batches_flag1": batches[1],
                  "items": sum(len(p) for p in a), "same_results": same,
                  "pages_per_s_flag0": [round(x, 1) for x in r[0]], "pages_per_s_flag1": [round(x, 1) for x in r[1]],
                  "flag0_min_max": [round(min(r[0]), 1), round(max(r[0]), 1)], "flag1_min_max": [round(min(r[1]), 1), round(max(r[1]), 1)]}))
