"""CPU suite: the pattern compiler (tuatara_amd/csrc/pattern.cpp; DESIGN.md "Patterns") under AddressSanitizer and UBSan.  tests/native/pattern_san.cpp is a
stand-alone program that links the host compiler - no HIP, nothing loaded into Python.  The good patterns and a corpus of malformed ones - every prefix of
each good pattern and 500 seeded random byte strings - must each compile or be refused with a C++ exception: any out-of-bounds access or overflow turns into
a sanitizer report and a non-zero exit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_pattern_cpu import PATTERNS

CSRC = os.path.join(ROOT, "tuatara_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "native", "pattern_san.cpp"), os.path.join(CSRC, "pattern.cpp"), os.path.join(CSRC, "geometry.cpp")]
GOOD = PATTERNS + [r"\d{2}/\d{2}/\d{4}", r"(a|b)*a(a|b){8}", r"((a{5}){5}){5}", r"(x|y|)(\w|\.){3,}[^a-z\d]?", r"[\--a\\]+", r"(a*)*b{0}"]


@pytest.fixture(scope="module")
def san_bin(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = os.path.join(str(tmp_path_factory.mktemp("pattern_san")), "pattern_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + SRC + ["-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip(f"sanitizer build not available here: {r.stderr[-400:]}")
    return out


def _run(binary, corpus, tmp_path):
    path = os.path.join(str(tmp_path), "corpus.txt")
    with open(path, "w") as f:
        for p in corpus:
            f.write(p.hex() + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([binary, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    words = r.stdout.split()
    return int(words[1]), int(words[3])


def test_good_patterns_and_their_prefixes(san_bin, tmp_path):
    good = [p.encode("latin1") for p in GOOD]
    compiled, refused = _run(san_bin, good, tmp_path)
    assert compiled + refused == 2 * len(good) and compiled >= len(PATTERNS)            # (each once without and once with a mask)
    prefixes = [g[:k] for g in good for k in range(1, len(g))]
    compiled, refused = _run(san_bin, prefixes, tmp_path)
    assert compiled + refused == 2 * len(prefixes) and compiled > 0 and refused > 0


def test_random_byte_strings(san_bin, tmp_path):
    rng = np.random.default_rng(20)
    meta = np.frombuffer(rb"\.[]()|?*+{},-^09azAZdw", np.uint8)
    corpus = []
    for k in range(500):
        n = int(rng.integers(1, 40))
        if k % 2:                                                                        # any bytes but NUL
            corpus.append(rng.integers(1, 256, n, dtype=np.uint8).tobytes())
        else:                                                                            # dense in metacharacters: these get past the first byte
            corpus.append(rng.choice(meta, n).astype(np.uint8).tobytes())
    compiled, refused = _run(san_bin, corpus, tmp_path)
    assert compiled + refused == 2 * len(corpus) and refused > compiled
