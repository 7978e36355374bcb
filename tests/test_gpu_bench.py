"""-m gpu: bench.py in a tree its user cannot write (built by another user): it runs the library build() left there, prints its line,
and --dump-outputs gives the same arrays as the same command in the writable tree.  A plain run measures what `value` needs; --full adds the rest."""
import json
import os
import shutil
import stat
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--pages", "8", "--buffers", "3", "--no-cpu-baseline", "--no-extras"]


def _bench(root, dump):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    out = subprocess.run([sys.executable, "-B", os.path.join(root, "bench.py"), *ARGS, "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["value"] > 0
    return {f[:-4]: np.load(os.path.join(dump, f)) for f in sorted(os.listdir(dump))}


def test_bench_runs_in_a_read_only_tree(tmp_path):
    if os.geteuid() == 0:
        pytest.skip("root writes through read-only permissions")
    from tuatara_amd.build import build_lib
    build_lib()
    tree = tmp_path / "tree"
    tree.mkdir()
    shutil.copy(os.path.join(ROOT, "bench.py"), tree / "bench.py")
    shutil.copytree(os.path.join(ROOT, "tuatara_amd"), tree / "tuatara_amd", ignore=shutil.ignore_patterns("__pycache__", "csrc"))
    paths = [tree] + [os.path.join(d, n) for d, ds, fs in os.walk(tree) for n in ds + fs]
    for p in paths:
        os.chmod(p, os.stat(p).st_mode & ~(stat.S_IWUSR | stat.S_IWGRP | stat.S_IWOTH))
    try:
        got = _bench(str(tree), tmp_path / "dump_ro")
    finally:
        for p in paths:
            os.chmod(p, os.stat(p).st_mode | stat.S_IWUSR)
    want = _bench(ROOT, tmp_path / "dump_rw")
    assert sorted(got) == ["bbox", "ids", "page_seed", "text", "words_per_page"] and sorted(got) == sorted(want)
    assert all(got[k].dtype == np.float32 and np.array_equal(got[k], want[k]) for k in got)
    assert got["words_per_page"].sum() == 8 * 40 and len(got["page_seed"]) == 8
    assert not (tree / "build").exists()


FULL_ONLY = ("value_full_ar", "value_detected_boxes", "p50_page_latency_ms", "h2d_included_pages_per_s", "bf16_pages_per_s", "f32_mfma_pages_per_s",
             "roofline_parseq_gemm", "roofline_craft_layers")


def _line(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    out = subprocess.run([sys.executable, "-B", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--pages", "8", "--buffers", "3", *extra],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_a_plain_run_leaves_the_other_measurements_to_full():
    plain = _line()
    assert plain["steps"] == 2 and plain["value"] > 0 and plain["roofline"]["avg_launch_us"] > 0      # (the timed region's own figures stay)
    assert [k for k in FULL_ONLY + ("cpu_baseline",) if k in plain] == [] and "frac_exclusive" not in plain["roofline"]
    full = _line("--full", "--no-cpu-baseline")        # (the CPU leg of a --full line: tests/test_gpu_dist.py)
    assert full["steps"] == 2 and full["value"] > 0
    assert [k for k in FULL_ONLY if k not in full] == [] and "cpu_baseline" not in full
    assert full["roofline"]["frac_exclusive"] > 0 and full["value_full_ar"] > 0 and full["bf16_pages_per_s"] > 0
