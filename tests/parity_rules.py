"""Margin-aware equivalence rules for the bf16 throughput mode (hard part 1).

bf16 is not fp32: a decision (an argmax over 95 logits, a heat-map pixel against a threshold) whose fp32 margin is inside
the bf16 error can come out either way.  The rule used by every bf16 test:

  * PARSeq: a crop's greedy path (autoregressive tokens, then the refined ids, both up to and including the first EOS - the
    reference cuts the string there, tuatara.cpp:497-502) must equal the oracle's, except that the FIRST position where it
    differs must have an oracle top-2 margin below tau = 2 x E, E = the 99.9th percentile of the measured change of the top-2 gap
    over all positions of the crops that do follow the oracle's path (a flip is a tail event of that distribution).  Any divergence at a larger margin fails the test.  tau must
    itself stay well below the typical margin, and at least `min_same` of the crops must follow the oracle's path outright.
  * CRAFT: see tests/test_gpu_bf16_parity.py (heat-map error bound, boxes = the reference post-processing of the engine's own
    heat map, flipped-pixel accounting).
"""
from __future__ import annotations

import numpy as np


def upto_eos(ids: np.ndarray) -> np.ndarray:
    """[N, L] class ids -> number of positions up to and including the first EOS (id 0); L when there is none."""
    has = (ids == 0).any(1)
    return np.where(has, (ids == 0).argmax(1) + 1, ids.shape[1])


def _gap(ref: np.ndarray, got: np.ndarray):
    o = np.argsort(ref, -1)
    t1, t2 = o[..., -1:], o[..., -2:-1]
    m_ref = (np.take_along_axis(ref, t1, -1) - np.take_along_axis(ref, t2, -1))[..., 0]
    m_got = (np.take_along_axis(got, t1, -1) - np.take_along_axis(got, t2, -1))[..., 0]
    return m_ref, np.abs(m_ref - m_got)


def parseq_margin_rule(ref, ref_ar, got, got_ar, min_same: float = 0.9, label: str = "", tau_cap_frac: float = 0.7):
    """ref / ref_ar: the oracle's refined and autoregressive logits [N, 26, 95]; got / got_ar: the engine's.  Asserts the rule in the
    module docstring and returns the statistics it printed."""
    n = len(ref)
    ids_r, ids_g = ref.argmax(-1), got.argmax(-1)
    ar_r, ar_g = ref_ar.argmax(-1), got_ar.argmax(-1)
    up_ar, up_rf = upto_eos(ar_r), upto_eos(ids_r)
    pos = np.arange(ref.shape[1])[None, :]
    mask_ar, mask_rf = pos < up_ar[:, None], pos < up_rf[:, None]
    ar_same = ((ar_r == ar_g) | ~mask_ar).all(1)
    rf_same = ((ids_r == ids_g) | ~mask_rf).all(1)
    same = ar_same & rf_same
    m_ar, e_ar = _gap(ref_ar, got_ar)
    m_rf, e_rf = _gap(ref, got)
    sel_ar, sel_rf = same[:, None] & mask_ar, same[:, None] & mask_rf
    gap_err = np.concatenate([e_ar[sel_ar], e_rf[sel_rf]])
    margins = np.concatenate([m_ar[sel_ar], m_rf[sel_rf]])
    E = float(np.percentile(gap_err, 99.9)) if len(gap_err) else 0.0
    tau = 2.0 * E
    dl = np.abs(got - ref)[sel_rf]
    stats = dict(n=n, same=float(same.mean()), E=E, tau=tau, median_margin=float(np.median(margins)) if len(margins) else 0.0,
                 mean_dlogit=float(dl.mean()) if dl.size else 0.0, max_dlogit=float(dl.max()) if dl.size else 0.0,
                 frac_below_tau=float((margins < tau).mean()) if len(margins) else 0.0)
    print(f"{label}: {int(same.sum())}/{n} crops follow the oracle's greedy path (AR + refined, up to EOS); on those mean |dlogit| "
          f"{stats['mean_dlogit']:.4f} max {stats['max_dlogit']:.3f}; top-2 gap error p99.9 {E:.3f} -> tau {tau:.3f}; median margin "
          f"{stats['median_margin']:.2f}; {100 * stats['frac_below_tau']:.1f} % of positions have margin < tau")
    assert same.mean() >= min_same, (label, same.mean())
    assert tau < tau_cap_frac * stats["median_margin"], (label, tau, stats["median_margin"])   # the rule must stay meaningful
    bad = []
    for i in np.nonzero(~same)[0]:
        if not ar_same[i]:
            p = int(np.nonzero((ar_r[i] != ar_g[i]) & mask_ar[i])[0][0])
            m, where = float(m_ar[i, p]), "AR"
        else:
            p = int(np.nonzero((ids_r[i] != ids_g[i]) & mask_rf[i])[0][0])
            m, where = float(m_rf[i, p]), "refined"
        print(f"   crop {i}: first divergence at {where} position {p}, oracle margin {m:.3f}")
        if m >= tau:
            bad.append((int(i), where, p, m))
    assert not bad, (label, "divergence at a confident position (margin >= tau)", tau, bad)
    stats["same_mask"] = same
    return stats


def box_iou(a, b) -> float:
    ix = max(0.0, min(a[2], b[2]) - max(a[0], b[0]) + 1)
    iy = max(0.0, min(a[3], b[3]) - max(a[1], b[1]) + 1)
    inter = ix * iy
    ua = (a[2] - a[0] + 1) * (a[3] - a[1] + 1) + (b[2] - b[0] + 1) * (b[3] - b[1] + 1) - inter
    return inter / ua


def heatmap_flips(h_ref: np.ndarray, h_got: np.ndarray, low_text: float = 0.4, link_threshold: float = 0.4):
    """Min-max normalised maps as tuatara.cpp:120-121 forms them, then the pixels whose binary decision (:131-132) differs.
    Returns (flip mask [H, W], max |d normalised|, number of pixels the oracle sets)."""
    def norm(a):
        return (a - a.min()) / (a.max() - a.min())
    tr, tg = norm(h_ref[..., 0]), norm(h_got[..., 0])
    lr, lg = norm(h_ref[..., 1]), norm(h_got[..., 1])
    flips = ((tr > low_text) != (tg > low_text)) | ((lr > link_threshold) != (lg > link_threshold))
    err = max(float(np.abs(tr - tg).max()), float(np.abs(lr - lg).max()))
    return flips, err, int(((tr > low_text) | (lr > link_threshold)).sum())


# ---- the CPU oracle's PARSeq logits, memoised per (model, crops): several GPU tests compare different engines with the oracle on the SAME seeded crop batches
# (config 2's 256 crops, the 448-crop batch); the oracle runs all 26 AR steps on the host - seconds per hundred crops - once per batch and test session
_oracle_memo = {}


def oracle_logits(parseq, crops, batch=64):
    import hashlib
    import torch
    key = (id(parseq), batch, crops.shape, hashlib.sha1(np.ascontiguousarray(crops).tobytes()).hexdigest())
    if key not in _oracle_memo:
        refs, ars = [], []
        with torch.no_grad():
            for i in range(0, len(crops), batch):
                x = torch.from_numpy(crops[i:i + batch]).permute(0, 3, 1, 2).float().div(255.0)
                r, a = parseq(x, return_ar=True)
                refs.append(r.numpy())
                ars.append(a.numpy())
        _oracle_memo[key] = (np.concatenate(refs), np.concatenate(ars))
    r, a = _oracle_memo[key]
    return r.copy(), a.copy()


# ---- the same network evaluated in float64: the yardstick of the error-budget tests (|engine - fp64| against |fp32 oracle - fp64|)
_fp64_models = {}
_oracle_memo_fp64 = {}


def oracle_logits_fp64(parseq, crops, batch=64):
    """(refined, AR) logits [N, 26, 95] of a float64 deep copy of `parseq`, evaluated under torch's MATH attention backend; memoised like oracle_logits.

    Why the backend is pinned: seen with torch 2.10 on the CPU, the float64 copy on torch's default scaled-dot-product path returns AR logits that are off by
    0.5 - 1.3 at every AR step whose single query row sees 16 or more keys (steps 15 .. 25); the fp32 model is the same on both paths, and under
    sdpa_kernel(SDPBackend.MATH) the float64 model agrees with it to ~1e-4 at all 26 steps (tests/test_long_words_cpu.py holds that).  Words of up to ten
    characters never read those steps, so the default path went unnoticed; any float64 comparison beyond step 14 has to come through here."""
    import copy
    import hashlib
    import torch
    from torch.nn.attention import SDPBackend, sdpa_kernel
    key = (id(parseq), batch, crops.shape, hashlib.sha1(np.ascontiguousarray(crops).tobytes()).hexdigest())
    if key not in _oracle_memo_fp64:
        if id(parseq) not in _fp64_models:
            _fp64_models[id(parseq)] = (parseq, copy.deepcopy(parseq).double())          # (the fp32 model is kept alive: its id is the key)
        p64 = _fp64_models[id(parseq)][1]
        refs, ars = [], []
        with torch.no_grad(), sdpa_kernel(SDPBackend.MATH):
            for i in range(0, len(crops), batch):
                x = torch.from_numpy(crops[i:i + batch]).permute(0, 3, 1, 2).double().div(255.0)
                r, a = p64(x, return_ar=True)
                refs.append(r.numpy())
                ars.append(a.numpy())
        _oracle_memo_fp64[key] = (np.concatenate(refs), np.concatenate(ars))
    r, a = _oracle_memo_fp64[key]
    return r.copy(), a.copy()


# ---- long words: the synthetic PARSeq built with max_len = 30 (tuatara_amd/weights.py: dfa_tables) reads strings of every length 0 .. 25 and beyond
def long_word_crops() -> np.ndarray:
    """the 128 noise crops the long-word tests share"""
    return np.random.default_rng(0).integers(0, 256, (128, 32, 128, 3), dtype=np.uint8)


def long_word_lengths(ref: np.ndarray, label: str = "long words") -> dict:
    """ref: the oracle's refined logits of a long-word batch -> the length figures, printed; ASSERTS what keeps the long-word tests from being vacuous:
    >= 8 crops with no EOS, >= 4 with the EOS in column 25, >= 1 empty string, >= 500 positions >= 11 up to EOS."""
    ids = ref.argmax(-1)
    has, up = (ids == 0).any(1), upto_eos(ids)
    late = (np.arange(ids.shape[1])[None, :] < up[:, None]) & (np.arange(ids.shape[1])[None, :] >= 11)
    st = dict(no_eos=int((~has).sum()), eos_25=int((has & (up == 26)).sum()), empty=int((up == 1).sum()), late_positions=int(late.sum()))
    print(f"{label}: {len(ids)} crops, {st['no_eos']} with no EOS, {st['eos_25']} with the EOS in column 25, {st['empty']} empty strings, {st['late_positions']} positions >= 11 up to EOS; "
          f"first-EOS columns (26 = none) {np.bincount(np.where(has, up - 1, 26), minlength=27).tolist()}")
    assert st["no_eos"] >= 8 and st["eos_25"] >= 4 and st["empty"] >= 1 and st["late_positions"] >= 500, st
    return st
