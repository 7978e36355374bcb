"""-m gpu: the decoder's self-attention kernel on its own (ttr_dbg_dec_self_attn: dec_self_attn_kernel, launched the way each precision's decoder launches
it - exact f16 triples out on f16x4, fp32 rows on f32), against a float64 evaluation of softmax(q k^T / sqrt(32) + mask) v.

nn.MultiheadAttention(self_attn) of the decoder layer: 12 heads of 32, the position queries against the <= 26 context slots of a crop.  The masks are the
ones PARSeq.forward builds (oracle/models.py, forward):
  AR step i       query row i against keys 0 .. i (tgt_mask = triu(-inf, 1), rows i:i+1, columns :i+1); no key padding;
  refinement      query row i against 26 keys, key i + 1 hidden (query_mask: the triu(-inf, 1) mask with everything from the second diagonal on cleared), and
                  key j hidden for every row when the context tokens 0 .. j hold an EOS (tgt_padding_mask = (tgt_in == EOS).cumsum(-1) > 0; tgt_in[0] = BOS).
Every AR step 0 .. 25 is run - with the default weights the engine's loop stops near step 10, so the later steps were covered by no test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EOS, BOS, PAD = 0, 95, 96
BAR = 2e-6            # x max |v|: tests/test_gpu_cross_attn.py's bar for the same arithmetic over 128 keys


@pytest.fixture(params=["f16x4", "f32"])
def eng(request, eng_x4, eng_f32):
    return eng_x4 if request.param == "f16x4" else eng_f32


def _visible(tokens, rows, mode):
    """bool [N, R, 26]: what query row rows[r] of crop n may look at"""
    N = len(tokens)
    j = np.arange(26)
    if mode == 0:
        return np.broadcast_to((j[None, :] <= np.asarray(rows)[:, None])[None], (N, len(rows), 26)).copy()
    cloze = j[None, :] != np.asarray(rows)[:, None] + 1                              # [R, 26]
    padded = np.cumsum(tokens == EOS, axis=1) > 0                                    # [N, 26]
    return cloze[None, :, :] & ~padded[:, None, :]


def _ref(q, kv, vis, rows):
    """float64; kv rows that no query of the crop may see do not enter (their weight is an exact 0)"""
    N = len(kv)
    qq = q[rows].astype(np.float64).reshape(len(rows), 12, 32)
    seen = vis.any(1)                                                                # [N, 26]
    kv = np.where(seen[:, :, None], kv, 0.0).astype(np.float64)
    k, v = kv[..., :384].reshape(N, 26, 12, 32), kv[..., 384:].reshape(N, 26, 12, 32)
    s = np.einsum("rhd,njhd->nhrj", qq, k) / np.sqrt(32.0)
    s = np.where(vis[:, None, :, :], s, -np.inf)
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(-1, keepdims=True)
    return np.einsum("nhrj,njhd->nrhd", p, v).reshape(N, len(rows), 384)


def _inputs(N, seed, sharp):
    rng = np.random.default_rng(seed)
    q = (rng.standard_normal((26, 384)) * sharp).astype(np.float32)
    kv = rng.standard_normal((N, 26, 768)).astype(np.float32)
    kv[..., 384:] *= np.float32(3.0)                        # values of a few units
    return q, kv


def _token_rows(N, seed):
    """[N, 26]: BOS, then characters; the six kinds of the refinement pass in turn (N >= 6 holds them all)"""
    rng = np.random.default_rng(seed)
    tk = rng.integers(1, 95, (N, 26)).astype(np.int32)
    tk[:, 0] = BOS
    for n in range(N):
        kind = n % 6
        if kind == 0:
            tk[n, 1] = EOS                                  # an empty string: only the BOS slot stays visible
        elif kind == 1:
            tk[n, 13] = EOS
        elif kind == 2:
            tk[n, 25] = EOS                                 # 24 characters
        elif kind == 4:
            tk[n, 7] = tk[n, 15] = EOS                      # twice: the first one counts
        elif kind == 5:
            tk[n, 9] = EOS
            tk[n, 10:] = PAD                                # what the engine's token buffer holds behind an early exit
    return tk                                               # (kind 3: no EOS - 26 visible keys less the cloze one)


def _check(eng, q, kv, tokens, rows, mode, label):
    vis = _visible(tokens, rows, mode)
    ref = _ref(q, kv, vis, rows)
    got = eng.dbg_dec_self_attn(q, kv, tokens, len(rows) if mode else 1, 0 if mode else rows[0], mode)
    vmax = float(np.abs(kv[..., 384:][np.isfinite(kv[..., 384:])]).max())
    assert got.shape == ref.shape and np.isfinite(got).all(), label        # (a row the kernel did not write comes back as NaN)
    err = float(np.abs(got - ref).max()) / vmax
    return got, ref, err


@pytest.mark.parametrize("N", [1, 3, 37])
def test_every_ar_step_against_float64(eng, N):
    """mode 0, every step 0 .. 25: scores of a few units and near one-hot rows (|score| ~ 30).  Some crops hold an EOS in their tokens: without the AR loop's
    counter the kernel must not look at it."""
    tokens = _token_rows(N, 7)
    worst = {}
    for sharp, seed in ((1.0, 1), (6.0, 2)):
        q, kv = _inputs(N, seed + 10 * N, sharp)
        worst[sharp] = []
        for qi in range(26):
            _, _, err = _check(eng, q, kv, tokens, [qi], 0, (N, qi, sharp))
            worst[sharp].append(err)
            # fp32 evaluation: <= 26 products of p <= 1 and |v| <= vmax, exp and the 32-term dot products in fp32; the f16x4 triples are exact
            assert err < BAR, (N, qi, sharp, err)
    for sharp, e in worst.items():
        print(f"mode 0, N={N}, sharp={sharp}: max |err| / max |v| over steps 0..25 = {max(e):.2e} (steps >= 11: {max(e[11:]):.2e})")


@pytest.mark.parametrize("N", [6, 37])
def test_refinement_rows_against_float64(eng, N):
    """mode 1, 26 rows per crop: EOS in column 1, 13, 25, none, twice, and PAD behind the EOS."""
    tokens = _token_rows(N, 8)
    assert {int(np.argmax(t == EOS)) if (t == EOS).any() else -1 for t in tokens} == {1, 13, 25, -1, 7, 9}
    for sharp, seed in ((1.0, 3), (6.0, 4)):
        q, kv = _inputs(N, seed + 10 * N, sharp)
        got, ref, err = _check(eng, q, kv, tokens, list(range(26)), 1, (N, sharp))
        per_kind = [float(np.abs(got[k::6] - ref[k::6]).max()) for k in range(6)]
        print(f"mode 1, N={N}, sharp={sharp}: max |err| / max |v| = {err:.2e}; per kind (EOS at 1 / 13 / 25 / none / twice / PAD behind) abs " + " ".join(f"{v:.1e}" for v in per_kind))
        assert err < BAR, (N, sharp, err)
    # the empty string: every row sees the BOS slot alone (row 0 as well: its cloze key is slot 1, padded anyway) - the output is that slot's V (p = 1 exactly;
    # 2^-30: an f16 triple holds a value below 2^-13 to 2^-35 absolute, not to its last bit)
    v0 = kv[0::6, 0, 384:]
    assert np.abs(got[0::6] - v0[:, None, :]).max() <= 2.0 ** -30


def test_fewer_refinement_rows_and_a_single_crop(eng):
    """R < 26 (rows 0 .. R - 1 of each crop, the next crop's rows directly behind): every row equals the 26-row call's."""
    tokens = _token_rows(7, 9)
    q, kv = _inputs(7, 21, 1.0)
    whole = eng.dbg_dec_self_attn(q, kv, tokens, 26, 0, 1)
    for R in (1, 11, 25):
        part, _, err = _check(eng, q, kv, tokens, list(range(R)), 1, R)
        assert err < BAR and np.array_equal(part, whole[:, :R]), R
    one = eng.dbg_dec_self_attn(q, kv[3:4], tokens[3:4], 26, 0, 1)
    assert np.array_equal(one[0], whole[3])


def test_nan_behind_a_mask_is_never_read(eng):
    """The K / V rows of keys no query may see hold NaN (the engine's cache is zeroed once and keeps older rows behind an early exit; 0 x NaN would not be 0): the
    output is finite and bit for bit the output with zeros there - the AR steps (slots behind the step) and the refinement pass (slots from the EOS on)."""
    N = 13
    tokens = _token_rows(N, 10)
    q, kv = _inputs(N, 31, 1.0)
    for qi in (0, 10, 11, 24):
        dirty = kv.copy()
        dirty[:, qi + 1:] = np.nan
        clean = np.where(np.isnan(dirty), np.float32(0), dirty)
        a, _, err = _check(eng, q, dirty, tokens, [qi], 0, ("mode 0", qi))
        assert err < BAR and np.array_equal(a, eng.dbg_dec_self_attn(q, clean, tokens, 1, qi, 0)), qi
    padded = np.cumsum(tokens == EOS, axis=1) > 0
    assert padded.any(1).sum() >= 8 and (~padded.any(1)).sum() >= 2
    dirty = np.where(padded[:, :, None], np.float32(np.nan), kv)
    clean = np.where(padded[:, :, None], np.float32(0), kv)
    a, _, err = _check(eng, q, dirty, tokens, list(range(26)), 1, "mode 1")
    assert err < BAR and np.array_equal(a, eng.dbg_dec_self_attn(q, clean, tokens, 26, 0, 1))


def test_without_the_skip_counter_a_done_crop_is_written(eng):
    """The per-crop exit (a crop with an EOS in token columns 1 .. step returns at once) belongs to the AR loop's counter; a call without one writes every
    crop's row: crops whose tokens hold an EOS get the same output as with tokens that hold none."""
    N = 12
    q, kv = _inputs(N, 41, 1.0)
    done = _token_rows(N, 11)
    none = np.where(done == EOS, 5, done).astype(np.int32)
    assert ((done[:, 1:] == EOS).any(1)).sum() >= 8
    for qi in (1, 12, 25):
        a = eng.dbg_dec_self_attn(q, kv, done, 1, qi, 0)
        assert np.isfinite(a).all() and np.array_equal(a, eng.dbg_dec_self_attn(q, kv, none, 1, qi, 0)), qi


def test_bad_arguments_are_refused(eng, eng_bf16):
    from tuatara_amd.engine import EngineError
    q, kv = _inputs(2, 51, 1.0)
    tokens = _token_rows(2, 12)
    for R, qi, mode in ((2, 0, 0), (1, 26, 0), (1, -1, 0), (27, 0, 1), (0, 0, 1), (1, 0, 2)):
        with pytest.raises(EngineError):
            eng.dbg_dec_self_attn(q, kv, tokens, R, qi, mode)
    with pytest.raises(EngineError):
        eng_bf16.dbg_dec_self_attn(q, kv, tokens, 1, 0, 0)
    assert np.isfinite(eng.dbg_dec_self_attn(q, kv, tokens, 1, 0, 0)).all()
