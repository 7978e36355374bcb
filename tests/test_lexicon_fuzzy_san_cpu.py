"""CPU suite: the host rule of the fuzzy alignment of lexicon entries (tuatara_amd/csrc/geometry.cpp: lexicon_fuzzy_from_lp; DESIGN.md "Lexicon matching",
Fuzzy alignment) under AddressSanitizer and UBSan.  tests/native/lexicon_fuzzy_san.cpp is a stand-alone program that links the host code - no HIP, nothing
loaded into Python.  It drives the rule over seeded tables of every kind and records of every length at every band, each in a heap block of its exact size;
any out-of-bounds access or overflow turns into a sanitizer report and a non-zero exit."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "tuatara_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "native", "lexicon_fuzzy_san.cpp"), os.path.join(CSRC, "geometry.cpp")]


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = str(tmp_path_factory.mktemp("lexicon_fuzzy_san"))
    out, probe = os.path.join(tmp, "lexicon_fuzzy_san"), os.path.join(tmp, "probe.cpp")
    flags = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(flags + [probe, "-o", os.path.join(tmp, "probe")], capture_output=True, text=True)
    if r.returncode != 0:                                      # no sanitizer runtimes here: the one reason to skip
        pytest.skip(f"sanitizer build not available here: {r.stderr[-400:]}")
    r = subprocess.run(flags + SRC + ["-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]                 # a compile error in the program or in geometry.cpp is a failure, not a skip
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_host_rule_under_sanitizers(san_bin, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([san_bin, str(seed), "12"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    scored, finite = int(words[1]), int(words[3])
    assert scored == 12 * 3 * 50 * 4 and 0 < finite < scored, r.stdout
