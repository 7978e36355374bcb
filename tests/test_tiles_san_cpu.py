"""CPU suite: tiled pages' host rule (tuatara_amd/csrc/geometry.cpp: tile_plan, tile_plan_from_origins, stitch_tiles; DESIGN.md "Tiled pages") under
AddressSanitizer and UBSan.  tests/native/tiles_san.cpp is a stand-alone program built with the host compiler - no HIP, nothing loaded into Python.  It plans
seeded pages (at and around the tile boundaries, pages of one tile, pages the rule refuses), walks every map coordinate of every accepted plan and stitches
seeded tile maps with every buffer sized exactly: any out-of-bounds access or signed overflow turns into a sanitizer report and a non-zero exit.  Fails on the
parent commit: geometry.cpp has no tile_plan there, so the program does not build - which this test treats as a failure, not a skip, once a plain build works."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "tuatara_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "native", "tiles_san.cpp"), os.path.join(CSRC, "geometry.cpp")]


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = str(tmp_path_factory.mktemp("tiles_san"))
    probe = os.path.join(d, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(flags + [probe, "-o", os.path.join(d, "probe")], capture_output=True).returncode != 0:
        pytest.skip("sanitizer build not available here")
    out = os.path.join(d, "tiles_san")
    r = subprocess.run(flags + SRC + ["-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_host_rule_under_sanitizers(san_bin, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([san_bin, str(seed), "400"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    assert words[0] == "plans" and int(words[1]) == 400 and int(words[3]) > 20 and int(words[5]) > 20   # (plans were stitched, and plans were refused)
