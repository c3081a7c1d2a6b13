"""Surface-normal evaluation without a GPU: a float64 restatement of DSINE's compute_normal_error / compute_normal_metrics
(DSINE/utils/utils.py:150-178) reproduces the reference's outputs stored in tests/golden/normal_eval_golden.pt, agrees with torch.cosine_similarity,
and the three C entry points of csrc/normaleval.hip reject bad arguments through e2eft_last_error before anything is launched."""
import ctypes
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_normal_eval_golden import CASES, NAMES, THRESHOLDS, make_case  # noqa: E402

GOLD = torch.load(os.path.join(HERE, "golden", "normal_eval_golden.pt"), weights_only=False)


def cosine64(p, g):
    """torch.cosine_similarity(p, g, dim=1) in float64: each vector divided by max(|v|, 1e-8), then the dot product"""
    p, g = p.double(), g.double()
    pn = p / p.norm(dim=1, keepdim=True).clamp_min(1e-8)
    gn = g / g.norm(dim=1, keepdim=True).clamp_min(1e-8)
    return (pn * gn).sum(1)


def normal_error64(p, g):
    """compute_normal_error in float64: [B,1,H,W] degrees"""
    return (torch.acos(cosine64(p, g).clamp(-1.0, 1.0)) * 180.0 / math.pi).unsqueeze(1)


def normal_metrics64(e):
    """compute_normal_metrics in float64 over a 1-D tensor of errors -> tensor [8]"""
    e = e.double().numpy()
    n = e.shape[0]
    vals = [np.mean(e), np.median(e), math.sqrt(np.sum(e * e) / n)] + [100.0 * (np.sum(e < t) / n) for t in THRESHOLDS]
    return torch.tensor(vals, dtype=torch.float64)


def angle_bar(theta_deg):
    """the per-pixel tolerance of the tests, in degrees: about 4x the conditioning of acos on an fp32 cosine, plus the fp32 rounding of theta"""
    t = torch.as_tensor(theta_deg, dtype=torch.float64)
    s = torch.sin(t * math.pi / 180.0)
    return (180.0 / math.pi) * torch.minimum(2.0 ** -20 / s, torch.full_like(t, 2.0 ** -9)) + 2.0 ** -20 * t


def test_fixture_cases_are_regenerated_from_their_seeds():
    assert len(GOLD["cases"]) == len(CASES) and tuple(GOLD["names"]) == NAMES
    parities = set()
    for c, want in zip(CASES, GOLD["cases"]):
        pred, gt, mask = make_case(**c)
        assert torch.equal(pred, want["pred"]) and torch.equal(gt, want["gt"]) and torch.equal(mask, want["mask"])
        parities.add(want["n"] % 2)
    assert parities == {0, 1}


def test_float64_restatement_reproduces_reference_outputs():
    for ci, want in enumerate(GOLD["cases"]):
        e64 = normal_error64(want["pred"], want["gt"])[want["mask"]]
        ref = want["errors"].double()
        assert e64.shape == ref.shape
        d = (e64 - ref).abs()
        assert (d <= angle_bar(e64)).all(), (ci, d.max().item())
        m64 = normal_metrics64(e64)
        got = want["metrics"]
        n = want["n"]
        # the reference's fp32 errors differ from exact ones by up to the per-pixel bar (0 and 180 deg: ~0.03 deg); mean and rmse move by the
        # bars' first-order effect, plus the fp32 sums of numpy
        bar = angle_bar(e64)
        tol_mean = bar.mean().item() + 1e-5 * abs(got[0].item())
        tol_rmse = (e64 * bar).sum().item() / (n * got[2].item()) + 1e-5 * abs(got[2].item())
        assert abs(m64[0].item() - got[0].item()) <= tol_mean, (ci, m64[0].item(), got[0].item())
        assert abs(m64[2].item() - got[2].item()) <= tol_rmse, (ci, m64[2].item(), got[2].item())
        med = got[1].item()
        assert abs(m64[1].item() - med) <= angle_bar(med).item(), (ci, m64[1].item(), med)
        for j, t in enumerate(THRESHOLDS):
            near = int(((e64 - t).abs() <= angle_bar(t)).sum())
            assert abs(m64[3 + j].item() - got[3 + j].item()) <= 100.0 * near / n + 1e-12, (ci, NAMES[3 + j])


def test_restatement_matches_torch_cosine_similarity_including_zero_vectors():
    g = torch.Generator().manual_seed(5)
    p = torch.randn(2, 3, 7, 9, generator=g)
    q = torch.randn(2, 3, 7, 9, generator=g)
    p[0, :, 0, 0] = 0.0
    q[1, :, 2, 3] = 0.0
    p[1, :, 4, 4] = 0.0
    q[1, :, 4, 4] = 0.0
    ref = torch.cosine_similarity(p, q, dim=1)
    ours = cosine64(p, q)
    assert (ours - ref.double()).abs().max().item() < 1e-6
    assert ref[0, 0, 0].item() == 0.0 and ref[1, 2, 3].item() == 0.0 and ref[1, 4, 4].item() == 0.0
    assert ours[0, 0, 0].item() == 0.0 and ours[1, 2, 3].item() == 0.0 and ours[1, 4, 4].item() == 0.0
    assert torch.allclose(normal_error64(p, q)[0, 0, 0, 0], torch.tensor(90.0, dtype=torch.float64))


def test_normal_eval_entry_points_validate_arguments_without_gpu():
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    nws = lib.e2eft_normal_eval_workspace_bytes()
    assert nws > 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    d = _lib.NormalEvalDesc()
    d.batch, d.height, d.width = 1, 4, 5
    d.pred_stride[:] = [60, 20, 5, 1]
    d.gt_stride[:] = [60, 20, 5, 1]
    d.mask_stride[:] = [20, 5, 1]
    upd = lib.e2eft_normal_eval_update
    assert upd(None, p, p, None, p, 0, 20, p, p, nws, None) == 1 and b"null" in lib.e2eft_last_error()
    assert upd(ctypes.byref(d), None, p, None, p, 0, 20, p, p, nws, None) == 1 and b"null" in lib.e2eft_last_error()
    assert upd(ctypes.byref(d), p, p, None, p, 0, 20, None, p, nws, None) == 1 and b"null" in lib.e2eft_last_error()
    for b, h, w in ((0, 4, 5), (1, 0, 5), (1, 4, -1)):
        bad = _lib.NormalEvalDesc()
        ctypes.memmove(ctypes.byref(bad), ctypes.byref(d), ctypes.sizeof(d))
        bad.batch, bad.height, bad.width = b, h, w
        assert upd(ctypes.byref(bad), p, p, None, p, 0, 20, p, p, nws, None) == 1 and b"shape" in lib.e2eft_last_error()
    assert upd(ctypes.byref(d), p, p, None, p, 1, 20, p, p, nws, None) == 1 and b"capacity" in lib.e2eft_last_error()
    assert upd(ctypes.byref(d), p, p, None, p, 0, 19, p, p, nws, None) == 1 and b"capacity" in lib.e2eft_last_error()
    assert upd(ctypes.byref(d), p, p, None, p, 0, 20, p, p, nws - 1, None) != 0 and b"workspace" in lib.e2eft_last_error()
    fin = lib.e2eft_normal_eval_finalize
    assert fin(p, 20, None, p, p, nws, None) == 1 and b"null" in lib.e2eft_last_error()
    assert fin(None, 20, p, p, p, nws, None) == 1 and b"null" in lib.e2eft_last_error()
    assert fin(p, -1, p, p, p, nws, None) == 1 and b"count" in lib.e2eft_last_error()
    assert fin(p, 20, p, p, p, 16, None) != 0 and b"workspace" in lib.e2eft_last_error()
    assert ctypes.sizeof(_lib.NormalEvalDesc) == 4 * 4 + 11 * 8
