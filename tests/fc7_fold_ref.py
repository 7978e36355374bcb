"""CRAFT's slice5.1 -> slice5.2 -> upconv1.0 on the CPU, as the reference chains them and as the f16x4 engine folds them.  TEST INFRASTRUCTURE ONLY
(tests/test_fc7_fold_cpu.py, tests/test_gpu_fc7_fold.py).

The reference (oracle/models.py: 72-76, 124-127): c6 = slice5.1(mp) (3x3, dilation 6, no activation), fc7 = slice5.2(c6) (1x1, no activation),
u1a = ReLU(upconv1.0(cat(fc7, relu5_3))).  The engine (tuning key fc7_fold, Engine::load_fc7_fold): with Wu = upconv1.0's weight,
A = Wu[:, :1024] . W52, Wf = A . W51, bf = A . b51 + Wu[:, :1024] . b52 + bu formed in float64 and rounded to fp32, then
z = Wu[:, 1024:] . relu5_3 (a split 1x1, fp32 out) and u1a = ReLU(conv3x3_dil6(mp; Wf) / S + bf + z) (a split 3x3, pairs or triples out).

chain(): the ORIGINAL three layers in a dtype - float64 is the truth the bar measures against, fp32 what the reference computes.
fold(): the derived weights.  model(): the folded pair with the split product of craft_layer_ref.Layer standing in for the kernels.
Tensors are NCHW torch tensors; W is the weight file as tuatara_amd.weights.read_ttrw returns it."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests import craft_layer_ref as R

NO_RELU = {"slice1.10", "slice2.17", "slice3.27", "slice4.37", "slice5.1", "slice5.2", "conv_cls.8"}


def chain(W, mp: torch.Tensor, skip: torch.Tensor, dt) -> torch.Tensor:
    """ReLU(upconv1.0(cat(slice5.2(slice5.1(mp)), skip))) in dtype dt"""
    H = mp.shape[2]
    L1 = R.Layer(W["slice5.1.w"], W["slice5.1.b"], dil=6, relu=False)
    L2 = R.Layer(W["slice5.2.w"], W["slice5.2.b"], relu=False)
    Lu = R.Layer(W["upconv1.0.w"], W["upconv1.0.b"], relu=True)
    fc7 = L2.plain(L1.plain(mp, 0, H, 0, H, dt), 0, H, 0, H, dt)
    return Lu.plain(torch.cat([fc7, skip.to(dt)], 1), 0, H, 0, H, dt)


def fold(W):
    """-> (Wf [512][3][3][512], bf [512], Wskip [512][1][1][512]) as fp32, the products formed in float64"""
    w51 = np.asarray(W["slice5.1.w"], np.float64).reshape(1024, 9 * 512)
    w52 = np.asarray(W["slice5.2.w"], np.float64).reshape(1024, 1024)
    wu = np.asarray(W["upconv1.0.w"], np.float64).reshape(512, 1536)
    b51, b52, bu = (np.asarray(W[k], np.float64) for k in ("slice5.1.b", "slice5.2.b", "upconv1.0.b"))
    A = wu[:, :1024] @ w52
    wf = (A @ w51).astype(np.float32).reshape(512, 3, 3, 512)
    bf = (A @ b51 + wu[:, :1024] @ b52 + bu).astype(np.float32)
    return wf, bf, np.ascontiguousarray(wu[:, 1024:].astype(np.float32).reshape(512, 1, 1, 512))


def model(W, mp: torch.Tensor, skip: torch.Tensor, planes: int = 2, order: str = "mfma"):
    """the folded pair as the kernels form it -> (z, out): z fp32 rows, out rounded to the planes the kernel stores"""
    H = mp.shape[2]
    wf, bf, wskip = fold(W)
    Lf = R.Layer(wf, bf, dil=6, relu=False, planes=planes)
    Ls = R.Layer(wskip, np.zeros(512, np.float32), relu=False, planes=planes)
    z = Ls.split_acc(skip, 0, H, 0, H, order=order)
    out = ((Lf.split_acc(mp, 0, H, 0, H, order=order) + Lf.b.view(1, -1, 1, 1)) + z).clamp_min(0)          # the epilogue: fma(acc, 1 / S, bias) + z, ReLU
    return z, R.join(R.split_act(out, planes))


def trunk32(W, canvas: np.ndarray):
    """the VGG trunk of the weight file in fp32 torch on canvases u8 [B, H, W, 3] -> (mp, relu5_3) at 1/16 resolution, each rounded to an exact pair as
    every tensor the engine hands a layer is"""
    def conv(name, x):
        L = R.Layer(W[name + ".w"], W[name + ".b"], relu=name not in NO_RELU)
        return L.plain(x, 0, x.shape[2], 0, x.shape[2], torch.float32)

    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(canvas)).permute(0, 3, 1, 2).float() / 255.0
        p1 = F.max_pool2d(conv("slice1.3", conv("slice1.0", x)), 2)
        c22 = conv("slice1.10", conv("slice1.7", p1))
        c32 = conv("slice2.17", conv("slice2.14", F.max_pool2d(c22, 2).clamp_min(0)))
        p3 = F.max_pool2d(conv("slice3.20", c32.clamp_min(0)), 2)
        c42 = conv("slice3.27", conv("slice3.24", p3))
        p4 = F.max_pool2d(conv("slice4.30", c42.clamp_min(0)), 2)
        c52 = R.join(R.split_act(conv("slice4.37", conv("slice4.34", p4)), 2))
        return F.max_pool2d(c52, 3, 1, 1), c52


def judge(out, W, mp: torch.Tensor, skip: torch.Tensor, pair_out: bool):
    """The project's bar (craft_layer_ref.bar) with ref64 / ref32 = the original three-layer chain in float64 / fp32 and nothing else on the right-hand side:
    |out - ref64| <= 1.5 x |ref32 - ref64| in the maximum and at the 99.99th percentile, plus one fp32 ulp where out is a pair.  out NHWC numpy.
    -> (ok, figures)"""
    with torch.no_grad():
        r64 = chain(W, mp, skip, torch.float64).permute(0, 2, 3, 1).numpy()
        r32 = chain(W, mp, skip, torch.float32).permute(0, 2, 3, 1).numpy()
    return R.bar(out, r64, r32, r32, pair_out=pair_out)
