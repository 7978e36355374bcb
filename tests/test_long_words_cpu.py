"""CPU suite for the long-word synthetic PARSeq (tuatara_amd/weights.py: max_len) and the float64 yardstick the GPU tests measure against
(tests/parity_rules.py: oracle_logits_fp64).  The default weights read strings of at most ten characters, so AR steps 11 .. 25, refinement rows with more
than 11 visible keys and a crop with no EOS at all were never compared with anything; max_len = 30 makes strings of every length 0 .. 25 and beyond.  Here:
the default stays bit for bit what it was, the 128-crop batch of tests/test_gpu_long_words.py has the lengths those tests rely on, and the float64
evaluation agrees with the fp32 oracle at all 26 AR steps.  No GPU."""
import numpy as np
import pytest

from tests import parity_rules as R

PICK = [0, 3, 4, 49, 92, 1, 2, 5]          # of the 128-crop batch: two crops with no EOS, two with the EOS in column 25, an empty string, three shorter ones


@pytest.fixture(scope="module")
def long_parseq(tmp_path_factory):
    from oracle import pipeline
    from tuatara_amd import weights as W
    c, p = W.make_synthetic_weights(str(tmp_path_factory.mktemp("weights_long")), seed=0, structured=True, max_len=30)
    return pipeline.load_models(c, p)[1]


def _longest_chain(nxt) -> int:
    """the longest string the transition table spells: steps from a class to the EOS (class 0)"""
    best = 0
    for t in range(1, 95):
        n = 0
        while t != 0:
            t, n = int(nxt[t]), n + 1
            assert n <= 95
        best = max(best, n)
    return best


def test_default_weights_are_unchanged():
    """max_len = 10 is the default of every function that takes it: the tables and every tensor of the seed-0 model are bit for bit the ones without the keyword
    (bench.py, the golden files and every tool call these functions with defaults)."""
    from tuatara_amd import weights as W
    for a, b in zip(W.dfa_tables(0), W.dfa_tables(0, max_len=10)):
        assert np.array_equal(a, b)
    assert _longest_chain(W.dfa_tables(0)[1]) == 10 and _longest_chain(W.dfa_tables(0, max_len=30)[1]) == 30
    a, b = W.synth_parseq(0), W.synth_parseq(0, max_len=10)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    long = W.synth_parseq(0, max_len=30)
    differ = sorted(k for k in a if a[k].tobytes() != long[k].tobytes())
    assert differ == ["decoder.layers.0.linear2.weight"], differ      # only the transition detectors' outputs (the next class's code) know the chains


def test_the_batch_has_the_lengths_the_gpu_tests_rely_on(long_parseq):
    ref, _ = R.oracle_logits(long_parseq, R.long_word_crops())
    R.long_word_lengths(ref, "max_len = 30, seed 0, 128 noise crops")


def test_fp64_through_the_helper_agrees_with_fp32_at_all_26_ar_steps(long_parseq):
    """8 long-word crops: |fp64 - fp32| on the AR logits within 2e-3 at every one of the 26 steps (measured ~2e-4), and on the refined logits.  The fp32
    evaluation is a summation order of its own - its distance from float64 on this network is ~1e-3 at the worst - so 2e-3 says "the same function", which is
    all this asks; an evaluation that goes wrong (see oracle_logits_fp64's docstring) misses by 0.5 and more."""
    crops = R.long_word_crops()[PICK]
    ref32, ar32 = R.oracle_logits(long_parseq, crops)
    ref64, ar64 = R.oracle_logits_fp64(long_parseq, crops)
    assert ref64.dtype == np.float64 and ar64.dtype == np.float64
    ids = ref32.argmax(-1)
    has = (ids == 0).any(1)
    assert (~has).sum() >= 2 and (R.upto_eos(ids) == 26).sum() >= 4 and (R.upto_eos(ids) == 1).sum() >= 1, ids
    per_step = np.abs(ar64 - ar32).max((0, 2))
    print("max |fp64 - fp32| of the AR logits per step: " + " ".join(f"{v:.1e}" for v in per_step) + f"; refined {np.abs(ref64 - ref32).max():.1e}")
    assert per_step.shape == (26,) and per_step.max() < 2e-3, per_step
    assert np.abs(ref64 - ref32).max() < 2e-3
    assert np.array_equal(ar64.argmax(-1), ar32.argmax(-1)) and np.array_equal(ref64.argmax(-1), ids)
    again, _ = R.oracle_logits_fp64(long_parseq, crops)                # memoised, and the caller's copy is its own
    again[:] = 0
    assert np.array_equal(R.oracle_logits_fp64(long_parseq, crops)[0], ref64)
