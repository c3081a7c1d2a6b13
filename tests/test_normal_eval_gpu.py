"""Surface-normal evaluation on the device (csrc/normaleval.hip, diffusion_e2e_ft_amd/evaluate.py) against the REFERENCE'S functions and against
its own errors.  tests/golden/normal_eval_golden.pt holds what DSINE/utils/utils.py:150-178 (compute_normal_error, compute_normal_metrics) return
on seeded synthetic cases (tests/golden/make_normal_eval_golden.py).  Per-pixel bar: (180/pi) * min(2^-20 / sin(theta), 2^-9) + 2^-20 * theta
degrees, about 4x the conditioning of acos on an fp32 cosine; the median, the shares and the order of the errors follow from it or are exact."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_normal_eval_cpu import GOLD, THRESHOLDS, angle_bar, normal_error64, normal_metrics64  # noqa: E402

pytestmark = pytest.mark.gpu


def _random_case(dev, B, H, W, seed, invalid=0.3):
    g = torch.Generator(device=dev).manual_seed(seed)
    gt = torch.randn(B, 3, H, W, device=dev, generator=g)
    pred = gt + 0.6 * torch.randn(B, 3, H, W, device=dev, generator=g)
    mask = torch.rand(B, 1, H, W, device=dev, generator=g) > invalid
    return pred, gt, mask


def _check_against_reference(res, e_dev, ref_errors, ref_metrics, n, ctx):
    """test 1's bars: res = result() dict, e_dev = errors() (or None), ref_* = the reference's errors / metrics"""
    ref = ref_errors.double()
    if e_dev is not None:
        e = e_dev.double().cpu()
        assert e.shape == ref.shape, ctx
        assert ((e - ref).abs() <= angle_bar(ref)).all(), (ctx, (e - ref).abs().max().item())
    assert res["n"] == n, ctx
    for i, name in ((0, "mean"), (2, "rmse")):
        w = ref_metrics[i].item()
        assert abs(res[name] - w) <= 1e-5 * abs(w), (ctx, name, res[name], w)
    med = ref_metrics[1].item()
    assert abs(res["median"] - med) <= angle_bar(med).item(), (ctx, res["median"], med)
    for j, t in enumerate(THRESHOLDS):
        near = int(((ref - t).abs() <= angle_bar(t)).sum())
        w = ref_metrics[3 + j].item()
        assert abs(res["a%d" % (j + 1)] - w) <= 100.0 * near / n + 1e-12, (ctx, j, res["a%d" % (j + 1)], w)


def test_normal_metrics_match_reference_functions(dev):
    from diffusion_e2e_ft_amd import evaluate
    for ci, c in enumerate(GOLD["cases"]):
        pred, gt, mask = c["pred"].to(dev), c["gt"].to(dev), c["mask"].to(dev)
        err = evaluate.normal_error(pred, gt)
        assert err.shape == (pred.shape[0], 1, pred.shape[2], pred.shape[3]) and err.dtype == torch.float32
        acc = evaluate.NormalMetricAccumulator()
        acc.update(pred, gt, mask)
        res = acc.result()
        _check_against_reference(res, acc.errors(), c["errors"], c["metrics"], c["n"], ci)
        assert torch.equal(acc.errors(), err[mask])
        one = evaluate.normal_metrics(pred, gt, mask)
        assert one == res
    assert tuple(evaluate.NORMAL_METRIC_NAMES) == tuple(GOLD["names"])


def test_exact_against_own_errors_64_images(dev):
    from diffusion_e2e_ft_amd import evaluate
    pred, gt, mask = _random_case(dev, 64, 480, 640, seed=7)
    acc = evaluate.NormalMetricAccumulator()
    acc.update(pred, gt, mask)
    full = evaluate.normal_error(pred, gt)
    e_ref = full[mask]
    e = acc.errors()
    assert torch.equal(e.view(torch.int32), e_ref.view(torch.int32))        # bit for bit, in the reference's order
    res = acc.result()
    en = e.cpu().numpy()
    n = en.shape[0]
    assert res["n"] == n
    med = np.median(en)
    assert np.float32(res["median"]).view(np.uint32) == np.float32(med).view(np.uint32) and float(np.float32(res["median"])) == res["median"]
    for j, t in enumerate(THRESHOLDS):
        assert res["a%d" % (j + 1)] == 100.0 * (np.sum(en < t) / n)
    e64 = en.astype(np.float64)
    assert abs(res["mean"] - e64.sum() / n) <= 1e-12 * abs(res["mean"])
    assert abs(res["rmse"] - math.sqrt((e64 * e64).sum() / n)) <= 1e-12 * res["rmse"]


@pytest.mark.parametrize("parity", [0, 1])
def test_streaming_updates_equal_one_update(dev, parity):
    """ten updates with changing H x W give the median and counts of ONE update over the concatenation of their pixels (laid out as a [1,3,1,N]
    image); mean and rmse within 1e-12 relative (the fp64 sums are added per update).  Both parities of n."""
    from diffusion_e2e_ft_amd import evaluate
    shapes = [(1, 436, 1024), (1, 37, 53), (2, 480, 640), (1, 64, 64), (3, 37, 53), (1, 436, 1024), (1, 5, 7), (2, 120, 160), (1, 1, 1), (1, 33, 97)]
    cases = [_random_case(dev, B, H, W, seed=100 + i) for i, (B, H, W) in enumerate(shapes)]
    if sum(int(m.sum()) for _, _, m in cases) % 2 != parity:
        cases[1][2][0, 0, 0, 0] = not bool(cases[1][2][0, 0, 0, 0])
    acc = evaluate.NormalMetricAccumulator(capacity=1000)          # small: the buffer doubles several times on the way
    for pred, gt, mask in cases:
        acc.update(pred, gt, mask)
    cat = lambda k: torch.cat([c[k].permute(1, 0, 2, 3).reshape(c[k].shape[1], -1) for c in cases], dim=1)
    pc, gc, mc = cat(0), cat(1), cat(2)
    n_pix = pc.shape[1]
    single = evaluate.NormalMetricAccumulator()
    single.update(pc.view(1, 3, 1, n_pix), gc.view(1, 3, 1, n_pix), mc.view(1, 1, 1, n_pix))
    assert torch.equal(acc.errors(), single.errors())
    assert torch.equal(acc.errors(), torch.cat([evaluate.normal_error(p, g)[m] for p, g, m in cases]))
    r, w = acc.result(), single.result()
    assert r["n"] == w["n"] and r["n"] % 2 == parity
    assert r["median"] == w["median"]
    for k in ("a1", "a2", "a3", "a4", "a5"):
        assert r[k] == w[k], k
    for k in ("mean", "rmse"):
        assert abs(r[k] - w[k]) <= 1e-12 * abs(w[k]), (k, r[k], w[k])
    assert np.float32(r["median"]) == np.median(acc.errors().cpu().numpy())


def test_layouts_permuted_view_and_null_mask(dev):
    from diffusion_e2e_ft_amd import evaluate
    pred, gt, mask = _random_case(dev, 1, 61, 83, seed=3)
    hwc = pred[0].permute(1, 2, 0).contiguous()                   # GeoWizard's normal_np layout [H,W,3]
    view = hwc.permute(2, 0, 1).unsqueeze(0)                     # DSINE's test.py:84 view: strides (.., 1, 3*W, 3)
    assert not view.is_contiguous()
    a = evaluate.NormalMetricAccumulator()
    a.update(view, gt, mask)
    b = evaluate.NormalMetricAccumulator()
    b.update(hwc.permute(2, 0, 1).contiguous(), gt, mask)
    assert torch.equal(a.errors(), b.errors()) and torch.equal(a.result_tensor(), b.result_tensor())
    gview = gt[0].permute(1, 2, 0).contiguous().permute(2, 0, 1)  # [3,H,W] view of an [H,W,3] array, no batch dimension
    assert torch.equal(evaluate.normal_error(view, gview), evaluate.normal_error(pred, gt))
    n1 = evaluate.NormalMetricAccumulator()
    n1.update(pred, gt, None)
    n2 = evaluate.NormalMetricAccumulator()
    n2.update(pred, gt, torch.ones_like(mask))
    assert torch.equal(n1.result_tensor(), n2.result_tensor()) and torch.equal(n1.errors(), n2.errors())
    assert n1.result()["n"] == 61 * 83


def test_edge_semantics(dev):
    from diffusion_e2e_ft_amd import evaluate
    pred, gt, mask = _random_case(dev, 1, 40, 50, seed=9)
    mask[0, 0, 3, 4] = True
    bad = pred.clone()
    bad[0, 1, 3, 4] = float("nan")
    acc = evaluate.NormalMetricAccumulator()
    acc.update(bad, gt, mask)
    r = acc.result()
    e = acc.errors().cpu().numpy()
    assert np.isnan(e).sum() == 1
    assert math.isnan(r["mean"]) and math.isnan(r["median"]) and math.isnan(r["rmse"])
    n = e.shape[0]
    for j, t in enumerate(THRESHOLDS):
        assert r["a%d" % (j + 1)] == 100.0 * (np.sum(e < t) / n)
    # n == 0
    none = evaluate.NormalMetricAccumulator()
    none.update(pred, gt, torch.zeros_like(mask))
    t = none.result_tensor().cpu()
    assert torch.isnan(t[:8]).all() and t[8].item() == 0.0 and none.result() is None
    assert evaluate.NormalMetricAccumulator().result() is None
    # one valid pixel: the median is its error
    one = torch.zeros_like(mask)
    one[0, 0, 17, 23] = True
    acc1 = evaluate.NormalMetricAccumulator()
    acc1.update(pred, gt, one)
    r1 = acc1.result()
    e1 = evaluate.normal_error(pred, gt)[0, 0, 17, 23].item()
    assert r1["n"] == 1 and r1["median"] == e1 and r1["mean"] == e1
    # the reset accumulator forgets
    acc1.reset()
    assert acc1.result() is None and acc1.errors().numel() == 0
    assert evaluate.format_normal_metrics(r1).splitlines()[0] == "mean median rmse 5 7.5 11.25 22.5 30"


def test_determinism_graph_capture_and_no_host_sync(dev):
    from diffusion_e2e_ft_amd import evaluate
    pred, gt, mask = _random_case(dev, 4, 96, 128, seed=21)
    runs = []
    for _ in range(2):
        acc = evaluate.NormalMetricAccumulator()
        for i in range(4):
            acc.update(pred[i], gt[i], mask[i])
        runs.append(acc.result_tensor())
    assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))
    acc = evaluate.NormalMetricAccumulator()
    acc.update(pred, gt, mask)
    eager = acc.result_tensor().clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                  # warm-up on the capture stream (the buffer and workspace exist already)
        acc.reset()
        acc.update(pred, gt, mask)
        acc.result_tensor()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc.reset()
        acc.update(pred, gt, mask)
        captured = acc.result_tensor()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.view(torch.int64), eager.view(torch.int64))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured.view(torch.int64), eager.view(torch.int64))
    # no host synchronisation inside update / result_tensor (growth included: capacity 1 forces a doubling on the second update)
    acc2 = evaluate.NormalMetricAccumulator(capacity=1)
    acc2.update(pred[0], gt[0], mask[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        acc2.update(pred[1], gt[1], mask[1])
        acc2.update(pred[2:], gt[2:], mask[2:])
        out = acc2.result_tensor()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert out[8].item() == eager[8].item() and out[1].item() == eager[1].item()
    assert torch.equal(out[3:], eager[3:]) and abs(out[0].item() - eager[0].item()) <= 1e-12 * eager[0].item()


def test_through_the_product_pipeline(dev):
    """test.py:92-113: a (tiny, synthetic) MarigoldPipeline called with normals=True, its normal_np [3,H,W] fed to the accumulator with a GT"""
    from diffusion_e2e_ft_amd import evaluate
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    from diffusion_e2e_ft_amd.pipeline import MarigoldPipeline
    from oracle import config, unet_ref, vae_ref, synth
    usd = synth.synth_state_dict(unet_ref.unet_param_shapes(config.TINY_UNET), seed=1234)
    vsd = synth.synth_state_dict(vae_ref.vae_param_shapes(config.TINY_VAE), seed=4321)
    _, ctx = synth.synth_inputs(1, 64, 64, 2, 128, seed=11)
    unet = UNet2DConditionModel(**config.TINY_UNET)
    unet.load_state_dict(usd)
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(vsd)
    pipe = MarigoldPipeline(unet.to(dev).eval(), vae.to(dev).eval(), DDIMScheduler())
    pipe.empty_text_embed = ctx.to(dev)
    g = torch.Generator().manual_seed(31)
    img = (torch.rand(3, 64, 64, generator=g) * 255).round().to(torch.uint8)
    out = pipe(img, denoising_steps=1, ensemble_size=1, processing_res=0, match_input_res=True, batch_size=1, color_map=None,
               show_progress_bar=False, noise="zeros", normals=True)
    normal_np = out.normal_np
    assert normal_np.shape == (3, 64, 64)
    pred_norm = torch.from_numpy(normal_np).unsqueeze(0).to(dev)        # test.py:106
    gt_norm = torch.randn(1, 3, 64, 64, generator=g)
    gt_mask = torch.rand(1, 1, 64, 64, generator=g) > 0.3
    acc = evaluate.NormalMetricAccumulator()
    acc.update(pred_norm, gt_norm.to(dev), gt_mask.to(dev))
    res = acc.result()
    e64 = normal_error64(torch.from_numpy(normal_np).unsqueeze(0), gt_norm)[gt_mask]
    _check_against_reference(res, acc.errors(), e64, normal_metrics64(e64), e64.numel(), "pipeline")
