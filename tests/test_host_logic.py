"""Host-side logic of the product package on CPU (no kernels run): parameter layout, weight packing, config surface,
scheduler, checkpoint round trip, rank sharding."""
import math
import os
import sys

import pytest
import torch

from oracle import config, unet_ref, vae_ref


def test_state_dict_keys_match_diffusers_layout():
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    for cfg in (config.TINY_UNET, config.TINY_GEOWIZARD_UNET):
        sd = UNet2DConditionModel(**cfg).state_dict()
        sh = unet_ref.unet_param_shapes(cfg)
        assert set(sd) == set(sh) and all(tuple(sd[k].shape) == tuple(sh[k]) for k in sh)
    sd = AutoencoderKL(**config.TINY_VAE).state_dict()
    sh = vae_ref.vae_param_shapes(config.TINY_VAE)
    assert set(sd) == set(sh) and all(tuple(sd[k].shape) == tuple(sh[k]) for k in sh)
    with torch.device("meta"):
        full = UNet2DConditionModel(in_channels=8)
    assert sum(p.numel() for p in full.parameters()) == 865_922_244


def test_packed_conv_weight_layout_and_cache():
    from diffusion_e2e_ft_amd.modules import Conv2d, packed_conv_weight
    c = Conv2d(3, 5, 3, 1, 1)
    w = packed_conv_weight(c)
    assert w.shape == (5, 9 * 4)  # fp32: Cin 3 -> 4
    ref = torch.nn.functional.pad(c.weight.detach().permute(0, 2, 3, 1), (0, 1)).reshape(5, -1)
    assert torch.equal(w, ref)
    assert packed_conv_weight(c) is w           # cached
    with torch.no_grad():
        c.weight.mul_(2.0)                      # in-place update (optimizer step) bumps _version -> repack
    w2 = packed_conv_weight(c)
    assert w2 is not w and torch.equal(w2, 2 * ref)
    h = Conv2d(3, 5, 3, 1, 1).half()
    assert packed_conv_weight(h).shape == (5, 9 * 8)  # fp16: Cin 3 -> 8


def test_config_surface_and_hooks():
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    m = UNet2DConditionModel(**dict(config.TINY_UNET, in_channels=4))
    assert m.config["in_channels"] == 4 and m.config.in_channels == 4
    assert isinstance(m.conv_in, torch.nn.Conv2d) and m.conv_in.out_channels == 64
    ref_prep = "/root/reference/training/util/unet_prep.py"
    if os.path.exists(ref_prep):  # run the reference's own hook on the product module
        import importlib.util
        spec = importlib.util.spec_from_file_location("ref_prep", ref_prep)
        prep = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(prep)
        w0, b0 = m.conv_in.weight.detach().clone(), m.conv_in.bias.detach().clone()
        prep.replace_unet_conv_in(m, repeat=2)
        assert m.config["in_channels"] == 8 and m.conv_in.weight.shape == (64, 8, 3, 3)
        assert torch.allclose(m.conv_in.weight, w0.repeat(1, 2, 1, 1) / 2) and torch.allclose(m.conv_in.bias, b0 / 2)
        assert "conv_in.weight" in m.state_dict()
    m.enable_gradient_checkpointing()
    m.enable_xformers_memory_efficient_attention()
    m.register_to_config(sample_size=32)
    assert m.config.sample_size == 32


def test_save_and_load_pretrained_roundtrip(tmp_path):
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    m = UNet2DConditionModel(**config.TINY_UNET)
    m.save_pretrained(str(tmp_path / "unet"))
    m2 = UNet2DConditionModel.from_pretrained(str(tmp_path), subfolder="unet")
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    assert tuple(m2.config.block_out_channels) == tuple(config.TINY_UNET["block_out_channels"])
    v = AutoencoderKL(**config.TINY_VAE)
    v.save_pretrained(str(tmp_path / "vae"))
    v2 = AutoencoderKL.from_pretrained(str(tmp_path / "vae"))
    assert all(torch.equal(a, b) for a, b in zip(v.state_dict().values(), v2.state_dict().values()))
    assert v2.config.scaling_factor == 0.18215


def test_scheduler_matches_oracle_constants():
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    from oracle import pipeline_ref
    s = DDIMScheduler()
    s.set_timesteps(1)
    assert s.timesteps.tolist() == [999]
    s.set_timesteps(4)
    assert s.timesteps.tolist() == [999, 749, 499, 249]
    sa, sb = s.x0_coefficients(999)
    assert abs(sa - 0.06826489) < 1e-7 and abs(sb - 0.99766725) < 1e-7
    s.set_timesteps(1)
    v, x = torch.randn(1, 4, 3, 3), torch.randn(1, 4, 3, 3)
    assert torch.allclose(s.step(v, 999, x).pred_original_sample, pipeline_ref.v_to_x0(v, x, 999), atol=1e-6)
    # the fused single-step paths take x0 = c * model_output at x_t = 0 from the scheduler's prediction_type, like step() (train.py:511-518)
    for pt in ("v_prediction", "epsilon", "sample"):
        sp = DDIMScheduler(prediction_type=pt)
        sp.set_timesteps(1)
        want = sp.step(v, 999, torch.zeros_like(v)).pred_original_sample
        assert torch.allclose(sp.zero_latent_x0_scale(999) * v, want, rtol=1e-5, atol=1e-6), pt
    import pytest
    with pytest.raises(NotImplementedError):
        DDIMScheduler(clip_sample=True).zero_latent_x0_scale(999)
    lead = DDIMScheduler(timestep_spacing="leading")
    lead.set_timesteps(1)
    assert lead.timesteps.tolist() == [1]  # why the reference forces trailing (Marigold/run.py:157-162)


def test_shard_range():
    from diffusion_e2e_ft_amd.dist import shard_range
    for n in (0, 1, 7, 8, 16, 17):
        for w in (1, 2, 3, 8):
            spans = [shard_range(n, r, w) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def test_training_host_mirrors_match_reference_fixtures():
    """training.IterExponential / replace_unet_conv_in against the values the REFERENCE's own lr_scheduler.py / unet_prep.py produced
    (tests/golden/hooks_golden.pt), and the GeoWizard class embedding against the oracle restatement"""
    from diffusion_e2e_ft_amd import training
    from oracle import pipeline_ref
    hooks = torch.load(os.path.join(os.path.dirname(__file__), "golden", "hooks_golden.pt"))
    sched = training.IterExponential(total_iter_length=20000, final_ratio=0.01, warmup_steps=100)
    for i, v in zip(hooks["lr_iters"].tolist(), hooks["lr_values"].tolist()):
        assert abs(sched(i) - v) < 1e-12, (i, sched(i), v)

    class _U:
        pass
    u = _U()
    u.conv_in = torch.nn.Conv2d(4, 32, 3, 1, 1)
    with torch.no_grad():
        u.conv_in.weight.copy_(hooks["conv_in_w0"])
        u.conv_in.bias.copy_(hooks["conv_in_b0"])
    u.config = {"in_channels": 4}
    training.replace_unet_conv_in(u, repeat=2)
    assert torch.equal(u.conv_in.weight.detach(), hooks["conv_in_w"]) and torch.equal(u.conv_in.bias.detach(), hooks["conv_in_b"])
    assert u.config["in_channels"] == int(hooks["conv_in_cfg"])
    for dom in ("indoor", "outdoor", "object"):
        assert torch.equal(training.geowizard_class_embedding(3, dom, torch.float32, "cpu"), pipeline_ref.geowizard_class_embedding(3, dom))


def test_pyramid_noise_like_draws_the_reference_sequence():
    """a13: multi-resolution noise (training/util/noise.py:8-18, marigold_pipeline.py:76-86) — same RNG draws in the same order as the
    reference's function imported from its file, or its recorded draws where the reference tree is absent (tests/golden/reference_pins.pt;
    the noise type is non-default; E2E-FT uses zeros)"""
    import random
    from diffusion_e2e_ft_amd.pipeline import pyramid_noise_like
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_reference_pins as pins
    for shape, want in zip(pins.NOISE_SHAPES, pins.pinned("pyramid_noise")):
        x = torch.zeros(shape)
        torch.manual_seed(5)
        random.seed(5)
        got = pyramid_noise_like(x)
        assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-6, atol=1e-6), shape
        assert abs(got.std().item() - 1.0) < 1e-5


def test_public_surface_is_importable():
    """every name callers of the reference's modules import from their counterparts here (a CPU-side guard: the GPU suite only runs at round end)"""
    from diffusion_e2e_ft_amd.pipeline import (MarigoldPipeline, MarigoldDepthOutput, DepthNormalEstimationPipeline, DepthNormalPipelineOutput,  # noqa: F401
                                               resize_max_res, pyramid_noise_like, find_batch_size, colorize_depth)
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel, UNet2DConditionOutput  # noqa: F401
    from diffusion_e2e_ft_amd.vae import AutoencoderKL  # noqa: F401
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler  # noqa: F401
    from diffusion_e2e_ft_amd.training import (e2e_ft_loss, geowizard_e2e_ft_loss, FlatAdamW, IterExponential, replace_unet_conv_in, train_step)  # noqa: F401
    from diffusion_e2e_ft_amd.clip import CLIPTextModel, CLIPVisionModelWithProjection  # noqa: F401
    import inspect
    sig = inspect.signature(DepthNormalEstimationPipeline.single_infer)
    assert list(sig.parameters)[:6] == ["self", "input_rgb", "num_inference_steps", "domain", "show_pbar", "noise"]   # geowizard_pipeline.py:252-258
    sig = inspect.signature(MarigoldPipeline.single_infer)
    assert list(sig.parameters)[:6] == ["self", "rgb_in", "num_inference_steps", "show_pbar", "noise", "normals"]     # marigold_pipeline.py:372-380


def test_small_gemm_families_of_the_sd2_unet():
    """unet.py::_batch_small_gemms (inference): the SD-v2 UNet has 22 ResnetBlock2D time projections (all reading the 1280-wide embedding) and
    16 cross-attention key / value pairs (all reading the 1024-wide context); the two concatenated GEMMs are 20160 and 24960 columns wide.
    Built on the meta device: no memory, no GPU."""
    import torch
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.modules import ResnetBlock2D, Attention
    with torch.device("meta"):
        m = UNet2DConditionModel(in_channels=8)
    res = [x for x in m.modules() if isinstance(x, ResnetBlock2D) and x.time_emb_proj is not None]
    att = [x for x in m.modules() if isinstance(x, Attention) and x.to_k.in_features != x.to_q.in_features and x.to_k.bias is None
           and x.to_q.in_features // x.heads == 64]
    assert len(res) == 22 and all(r.time_emb_proj.in_features == 1280 for r in res)
    assert len(att) == 16 and all(a.to_k.in_features == 1024 for a in att)
    assert sum(r.time_emb_proj.out_features for r in res) == 20160
    assert sum(2 * a.to_k.out_features for a in att) == 24960
    # the slices travel as ARGUMENTS of the call (modules.TimeCond / CtxCond, picked by identity), nothing is parked on the modules (re-entrancy)
    import inspect
    from diffusion_e2e_ft_amd import modules, unet
    assert "TimeCond" in inspect.getsource(modules.ResnetBlock2D.nhwc) and "CtxCond" in inspect.getsource(modules.Attention.forward)
    src = inspect.getsource(unet.UNet2DConditionModel._batch_small_gemms)
    assert "TimeCond(" in src and "CtxCond(" in src and "__dict__[\"_rowadd" not in src and "__dict__[\"_kv" not in src
    tc = modules.TimeCond(torch.zeros(2, 4), {1: "a"})
    assert tc.rows[1] == "a" and modules.CtxCond(torch.zeros(1)).kv == {}


def test_flat_adamw_is_a_torch_optimizer_with_live_lr_and_torch_format_state():
    """training/train.py:346-357 builds `torch.optim.AdamW(...)` + `LambdaLR(optimizer, IterExponential(...))`, :417-440,578-599 save / load the
    optimizer through accelerate (= optimizer.state_dict() / load_state_dict()).  FlatAdamW must be usable in exactly those places: host-side
    surface only here (the update itself is a HIP kernel: tests/test_train_gpu.py)."""
    from torch.optim.lr_scheduler import LambdaLR
    from diffusion_e2e_ft_amd.training import FlatAdamW, IterExponential
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 3))
    ref = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Linear(5, 3))
    ref.load_state_dict(net.state_dict())
    opt = FlatAdamW(net.parameters(), lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (3e-5, (0.9, 0.999), 1e-8, 1e-2) and len(g["params"]) == 4
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), ref.state_dict().values()))      # flattening keeps the values
    # the reference's scheduler drives the group's lr (train.py:356-357); the step itself is not run on the CPU
    lam = IterExponential(total_iter_length=20000, final_ratio=0.01, warmup_steps=100)
    sched = LambdaLR(opt, lr_lambda=lam)
    assert opt.param_groups[0]["lr"] == 0.0 and opt.lr == 0.0                                  # warm-up starts at 0
    sched.last_epoch = 49
    sched._step_count = 50
    opt._opt_called = True      # (silences LambdaLR's "step order" warning: no optimizer.step() on a CPU box)
    sched.step()
    assert abs(opt.param_groups[0]["lr"] - 3e-5 * 0.5) < 1e-12
    # state in torch's own format: a torch.optim.AdamW checkpoint loads, and ours loads into torch.optim.AdamW
    ropt = torch.optim.AdamW(ref.parameters(), lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    ref(torch.randn(4, 6)).sum().backward()
    ropt.step()
    opt.load_state_dict(ropt.state_dict())
    for p, rp, o in zip(opt.params, ref.parameters(), opt.offsets):
        assert torch.equal(opt.exp_avg[o:o + p.numel()].view(p.shape), ropt.state[rp]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], ropt.state[rp]["exp_avg_sq"])
        assert opt.state[p]["exp_avg"].data_ptr() == opt.exp_avg.data_ptr() + 4 * o            # state stays a VIEW of the flat moments
    assert opt.step_count == 1 and opt.skipped_steps() == 0
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "flat_adamw"} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    ropt2 = torch.optim.AdamW(ref.parameters(), lr=1.0)
    ropt2.load_state_dict({k: v for k, v in sd.items() if k != "flat_adamw"})
    assert ropt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] and float(ropt2.state[next(ref.parameters())]["step"]) == 1.0
    # a SECOND checkpoint must see what happened since the first (state_dict() used to re-bind state[p] to its clones)
    opt.exp_avg.fill_(5.0)
    opt._steps[0] = 7
    sd2 = opt.state_dict()
    for i, (p, o) in enumerate(zip(opt.params, opt.offsets)):
        assert opt.state[p]["exp_avg"].data_ptr() == opt.exp_avg.data_ptr() + 4 * o
        assert sd2["state"][i]["exp_avg"].eq(5.0).all() and float(sd2["state"][i]["step"]) == 7.0
        assert sd["state"][i]["exp_avg"].data_ptr() != sd2["state"][i]["exp_avg"].data_ptr() and float(sd["state"][i]["step"]) == 1.0
    # zero_grad(set_to_none=False): one memset, .grad stays bound to the flat buffer; a re-bound .grad is adopted back
    opt.zero_grad(set_to_none=False)
    p0 = opt.params[0]
    assert p0.grad is not None and p0.grad.data_ptr() == opt.flat_grad.data_ptr() and opt.flat_grad.eq(0).all()
    p0.grad = torch.ones_like(p0)
    opt._adopt_grads()
    assert p0.grad.data_ptr() == opt.flat_grad.data_ptr() and opt.flat_grad[:p0.numel()].eq(1).all()
    # direct_grads (the default): zero_grad() leaves .grad None and the buffer alone; a backward kernel may claim a parameter's slot ONCE per step
    # (autograd.grad_sink), adjacent slots as one span; whatever got no gradient is zeroed when the step adopts
    from diffusion_e2e_ft_amd import autograd as F
    opt.flat_grad.fill_(3.0)
    opt.zero_grad()
    assert all(q.grad is None for q in opt.params) and opt.flat_grad.eq(3).all()
    flat, views = F.grad_sink(p0)
    assert flat.data_ptr() == opt.flat_grad.data_ptr() and flat.numel() == p0.numel() and views[0].shape == p0.shape and views[0].stride() == p0.stride()
    assert F.grad_sink(p0) is None                                                               # second writer of the same step: the ordinary path
    flat.fill_(2.0)
    p0.grad = views[0]                                                                           # (what AccumulateGrad does with a gradient nobody else references)
    adj = [i for i in range(len(opt.params) - 1) if opt.offsets[i + 1] == opt.offsets[i] + opt.params[i].numel() and i > 0]
    if adj:
        i = adj[0]
        span = F.grad_sink(opt.params[i], opt.params[i + 1])
        assert span is not None and span[0].numel() == opt.params[i].numel() + opt.params[i + 1].numel() and len(span[1]) == 2
        assert span[1][1].data_ptr() == opt.flat_grad.data_ptr() + 4 * opt.offsets[i + 1]
        assert F.grad_sink(opt.params[i + 1]) is None
    assert F.grad_sink(opt.params[0], opt.params[-1]) is None                                    # not adjacent (and p0 is taken)
    other = torch.nn.Parameter(torch.zeros(3))
    assert F.grad_sink(other) is None                                                            # not FlatAdamW's
    opt._adopt_grads()
    assert opt.flat_grad[:p0.numel()].eq(2).all() and opt.flat_grad[opt.offsets[-1]:opt.offsets[-1] + opt.params[-1].numel()].eq(0).all()
    assert all(q.grad is not None and q.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * o for q, o in zip(opt.params, opt.offsets))
    opt.zero_grad()
    assert F.grad_sink(p0) is not None                                                           # re-armed
    opt.direct_grads = False
    opt.zero_grad()
    assert p0.grad is not None and opt.flat_grad.eq(0).all() and F.grad_sink(p0) is None
    with pytest.raises(ValueError):
        FlatAdamW([{"params": [torch.nn.Parameter(torch.zeros(2))]}, {"params": [torch.nn.Parameter(torch.zeros(2))]}])


def test_evaluate_rejects_multi_channel_input_instead_of_spinning():
    from diffusion_e2e_ft_amd import evaluate
    assert evaluate._b(torch.zeros(4, 5)).shape == (1, 4, 5) and evaluate._b(torch.zeros(2, 1, 4, 5)).shape == (2, 4, 5)
    with pytest.raises(ValueError):
        evaluate._b(torch.zeros(2, 3, 4, 5))
    with pytest.raises(ValueError):
        evaluate._b(torch.zeros(2, 4, 5, 1, 1))


def test_aa_bilinear_tables_are_atens_weights():
    """pipeline.aa_bilinear_tables restates aten's `_compute_indices_min_size_weights_aa`: applying the tables separably (numpy model of
    csrc/prepost.hip: horizontal pass, then vertical pass, fp32) must reproduce `F.interpolate(mode="bilinear", antialias=True)` — down-scaling
    (support grows), up-scaling, odd ratios, and the uint8-rounded form `resize_max_res` uses"""
    import numpy as np
    from diffusion_e2e_ft_amd.pipeline import aa_bilinear_tables
    g = torch.Generator().manual_seed(0)
    for (H, W, h, w) in [(480, 640, 576, 768), (1000, 750, 768, 576), (64, 96, 64, 96), (37, 53, 11, 200), (96, 64, 480, 640)]:
        img = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8)
        want = torch.nn.functional.interpolate(img[None].float(), size=(h, w), mode="bilinear", antialias=True, align_corners=False)[0].numpy()
        (xb, xw), (yb, yw) = aa_bilinear_tables(W, w, "cpu"), aa_bilinear_tables(H, h, "cpu")
        x = img.numpy().astype(np.float32)
        mid = np.zeros((3, H, w), np.float32)
        for o in range(w):
            a, n = int(xb[o, 0]), int(xb[o, 1])
            mid[:, :, o] = (x[:, :, a:a + n] * xw[o, :n].numpy()).sum(-1, dtype=np.float32)
        out = np.zeros((3, h, w), np.float32)
        for o in range(h):
            a, n = int(yb[o, 0]), int(yb[o, 1])
            out[:, o, :] = (mid[:, a:a + n, :] * yw[o, :n].numpy()[None, :, None]).sum(1, dtype=np.float32)
        assert np.abs(out - want).max() <= 2e-4, ((H, W, h, w), np.abs(out - want).max())        # 0..255 scale: fp32 summation order only
        bad = np.rint(out) != np.rint(want)          # a value within fp32 round-off of k + 0.5 may land on either side
        assert bad.mean() < 2e-3 and (np.abs(want[bad] - np.floor(want[bad]) - 0.5) < 1e-3).all()


def test_bench_prints_pmc_traffic_only_for_the_profiled_build_and_kernel_population(tmp_path):
    """bench.py's roofline.traffic comes from a committed PMC profile: it is attached only when the profile was collected ON THE BUILD THAT RUNS (its `build_id` =
    e2eft_build_id() of the loaded library: VERDICT r4 — round 4 cited a round-3 profile as "the same build" on launch counts alone) AND its launch counts per kernel
    of the igemm family equal the run's; the fraction over the launches without a fused GroupNorm must exclude exactly igemm6's NORM symbols"""
    import json
    import bench
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    line = json.loads(open(os.path.join(root, "profiles", "r03s_bench_default.json")).read().strip().splitlines()[-1])
    symbols = line["roofline"]["by_symbol"]
    mix = bench.kernel_mix(symbols)
    assert mix == {"igemm6_kernel": 62.0, "igemm5_kernel": 74.0, "igemm2_kernel": 126.0, "conv3x3_narrow": 1.0, "conv_thin_in_kernel": 3.0}, mix
    # the committed round-3 profile carries no build id: never attached any more, whatever the launch counts say
    t0, s0, n0, _ = bench.pmc_traffic(mix, True, build_id="0123456789abcdef")
    assert t0 is None and s0 is None and "no committed PMC profile was collected on this build" in n0 and "0123456789abcdef" in n0
    # the same profile stamped with a build id (what scripts/pmc_traffic.py writes since round 5)
    prof = json.load(open(os.path.join(root, "profiles", "r03s_pmc_hbm_traffic.json")))
    prof["build_id"] = "feedfacecafebeef"
    with open(tmp_path / "r99_pmc_hbm_traffic.json", "w") as f:
        json.dump(prof, f)
    traffic, source, note, others = bench.pmc_traffic(mix, True, prof_dir=str(tmp_path), build_id="feedfacecafebeef")
    assert source and "r99_pmc_hbm_traffic.json" in source and "feedfacecafebeef" in source and abs(traffic - line["roofline"]["traffic"]) < 1.0
    assert "attn_fwd" in others and "gn_apply" in others
    assert bench.pmc_traffic(mix, True, prof_dir=str(tmp_path), build_id="another0build0id")[0] is None
    for changed in (dict(mix, igemm6_kernel=61.0, igemm5_kernel=75.0), dict(mix, conv_thin_in_kernel=2.0, igemm2_kernel=127.0), {k: v for k, v in mix.items() if k != "conv3x3_narrow"}):
        t2, s2, n2, _ = bench.pmc_traffic(changed, True, prof_dir=str(tmp_path), build_id="feedfacecafebeef")      # same build, another population / one launch missing: no figure
        assert t2 is None and s2 is None and "no committed PMC profile" in n2, (changed, n2)
    assert bench.pmc_traffic(mix, False)[0] is None           # another workload: never
    extra = bench.plain_launch_fraction(symbols, 2500.0)
    nrm = [k for k in symbols if k.startswith("igemm6") and k.endswith(", true>")]
    assert len(nrm) == 2 and abs(extra["ms_per_step_of_launches_with_fused_groupnorm"] - sum(symbols[k]["ms_per_step"] for k in nrm)) < 1e-9
    assert extra["frac_launches_without_fused_groupnorm"] > line["roofline"]["frac"]
    assert bench.plain_launch_fraction({k: v for k, v in symbols.items() if k not in nrm}, 2500.0) == {}


def test_wgrad_pixel_split_fills_whole_rounds_of_the_machine():
    """e2eft_conv2d_wgrad_workspace_bytes is pure host arithmetic (wgrad_plan): the number of pixel splits it reserves partial buffers for must fill whole
    rounds of one workgroup per CU (256 CUs assumed without a device) and leave every workgroup at least 8 k-tiles — the conv 320 -> 320 of the 576^2 recipe
    (32 x 72^2 pixels) used to be cut 36 x 22 = 3.09 rounds, now 36 x 7 = 0.98"""
    import ctypes as C
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()

    def splits(batch, hw, cin, cout, k):
        d = _lib.ConvDesc()
        d.dtype = 1
        d.batch, d.hin, d.win, d.hl, d.wl, d.hout, d.wout = batch, hw, hw, hw, hw, hw, hw
        d.c1, d.ldx1, d.c2, d.ldx2 = cin, cin, 0, 0
        d.kh, d.kw, d.stride, d.pad_t, d.pad_l = k, k, 1, k // 2, k // 2
        d.cout, d.ldo, d.ldw, d.alpha = cout, cout, k * k * cin, 1.0
        nbytes = lib.e2eft_conv2d_wgrad_workspace_bytes(C.byref(d), cout)
        assert nbytes > 0, lib.e2eft_last_error()
        n = k * k * cin
        assert nbytes % (cout * n * 4) == 0
        ns = nbytes // (cout * n * 4)
        area2 = -(-cout // 128) * 128 * -(-n // 256) * 256
        area4 = -(-cout // 256) * 256 * -(-n // 128) * 128
        tiles = (-(-cout // 256)) * (-(-n // 128)) if area4 < area2 else (-(-cout // 128)) * (-(-n // 256))
        return ns, tiles, batch * hw * hw

    for (b, hw, cin, cout, k) in [(32, 72, 320, 320, 3), (32, 72, 320, 2560, 1), (32, 36, 640, 640, 3), (32, 18, 1280, 1280, 3), (32, 72, 320, 320, 1), (1, 72, 64, 64, 3)]:
        ns, tiles, pix = splits(b, hw, cin, cout, k)
        w = ns * tiles
        rounds = -(-w // 256)
        ktiles_per_split = -(-(-(-pix // 64)) // ns)
        assert ns == 1 or ktiles_per_split >= 8, (ns, ktiles_per_split)
        too_small = (-(-pix // 64) // 8) * tiles < 256          # even at 8 k-tiles per workgroup the problem does not fill one round
        assert w / (rounds * 256) >= 0.85 or too_small, ((b, hw, cin, cout, k), ns, tiles, rounds)
    assert splits(32, 72, 320, 320, 3)[:2] == (7, 36)          # 252 workgroups: one round, 98 % full
    # channel counts that are not multiples of 64 are not this kernel's: 0 bytes, the caller keeps the transpose + GEMM route; fp32 has its own form of the kernel since
    # round 6 (wgrad32_kernel): a workspace like the 16-bit one
    d = _lib.ConvDesc()
    d.dtype, d.batch, d.hin, d.win, d.hl, d.wl, d.hout, d.wout = 1, 1, 8, 8, 8, 8, 8, 8
    d.c1, d.ldx1, d.kh, d.kw, d.stride, d.pad_t, d.pad_l, d.cout, d.ldo, d.ldw, d.alpha = 48, 48, 3, 3, 1, 1, 1, 64, 64, 432, 1.0
    assert lib.e2eft_conv2d_wgrad_workspace_bytes(C.byref(d), 64) == 0
    d.dtype, d.c1, d.ldx1, d.ldw = 0, 64, 64, 576
    assert lib.e2eft_conv2d_wgrad_workspace_bytes(C.byref(d), 64) > 0


def _apply_tables(x, xt, yt):
    """numpy model of csrc/prepost.hip: horizontal pass, then vertical pass, fp32"""
    import numpy as np
    (xb, xw), (yb, yw) = xt, yt
    P, H, W = x.shape
    w, h = xb.shape[0], yb.shape[0]
    mid = np.zeros((P, H, w), np.float32)
    for o in range(w):
        a, n = int(xb[o, 0]), int(xb[o, 1])
        mid[:, :, o] = (x[:, :, a:a + n] * xw[o, :n].numpy()).sum(-1, dtype=np.float32)
    out = np.zeros((P, h, w), np.float32)
    for o in range(h):
        a, n = int(yb[o, 0]), int(yb[o, 1])
        out[:, o, :] = (mid[:, a:a + n, :] * yw[o, :n].numpy()[None, :, None]).sum(1, dtype=np.float32)
    return out


def test_aa_bicubic_and_nearest_tables_match_torch_and_pillow():
    """pipeline.aa_tables(kind="bicubic") = aten's antialiased bicubic (the CLIP preprocessing of geowizard_pipeline.py:236-245 through torchvision) = Pillow's
    `Image.resize` of a float image with its default BICUBIC (the depth resize-back of geowizard_pipeline.py:201-203); kind="nearest" = cv2.INTER_NEAREST (:205): OpenCV's
    resizeNN forms the inverse scale in DOUBLE (1 / (out / in)), torch's "nearest" forms in / out in float32 — the last case below is a ratio where the two pick
    different source pixels, and the table follows cv2."""
    import numpy as np
    from PIL import Image
    from diffusion_e2e_ft_amd.pipeline import aa_tables
    g = torch.Generator().manual_seed(1)
    differs = 0
    for (H, W, h, w) in [(768, 576, 224, 224), (96, 128, 480, 640), (61, 45, 224, 224), (576, 768, 1000, 1333), (58, 87, 577, 1000)]:
        img = torch.rand((2, H, W), generator=g)
        out = _apply_tables(img.numpy(), aa_tables(W, w, "cpu", "bicubic"), aa_tables(H, h, "cpu", "bicubic"))
        want = torch.nn.functional.interpolate(img[None], size=(h, w), mode="bicubic", antialias=True, align_corners=False)[0].numpy()
        assert np.abs(out - want).max() <= 2e-6, ((H, W, h, w), np.abs(out - want).max())
        pil = np.asarray(Image.fromarray(img[0].numpy()).resize((w, h)))                 # mode "F", default resample
        assert np.abs(out[0] - pil).max() <= 2e-4, ((H, W, h, w), np.abs(out[0] - pil).max())       # (Pillow builds its coefficients in double precision)
        near = _apply_tables(img.numpy(), aa_tables(W, w, "cpu", "nearest"), aa_tables(H, h, "cpu", "nearest"))
        iy = [min(int(math.floor(i * (1.0 / (h / H)))), H - 1) for i in range(h)]
        ix = [min(int(math.floor(i * (1.0 / (w / W)))), W - 1) for i in range(w)]
        assert np.array_equal(near, img.numpy()[:, iy][:, :, ix])
        differs += int(not np.array_equal(near, torch.nn.functional.interpolate(img[None], size=(h, w), mode="nearest")[0].numpy()))
    assert differs >= 1          # the float32 rule is NOT the same function: at least the last ratio tells them apart


def test_flat_adamw_keeps_convolution_weights_in_kernel_order():
    """FlatAdamW stores a convolution weight OHWI (the Parameter is a channels_last view of its slot): logical values / shape unchanged, gradients of torch's own
    conv backward land in the flat gradient buffer, optimizer state round-trips, and the parameters are tagged for autograd.FlatShadow (host-side surface only;
    the twin's cast and the packed-weight views are exercised on the GPU: tests/test_train_gpu.py)"""
    from diffusion_e2e_ft_amd.training import FlatAdamW
    from diffusion_e2e_ft_amd import autograd as F
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(8, 16, 3, padding=1), torch.nn.Conv2d(16, 4, 1), torch.nn.Flatten(), torch.nn.Linear(4 * 5 * 5, 3))
    ref = [p.detach().clone() for p in net.parameters()]
    opt = FlatAdamW(net.parameters())
    w0, w1 = net[0].weight, net[1].weight
    assert w0.shape == (16, 8, 3, 3) and w0.stride() == (72, 1, 24, 8) and F._is_ohwi(w0)            # OHWI storage, OIHW logical shape
    assert w1.is_contiguous()                                                                          # 1x1: nothing to reorder
    assert all(torch.equal(p.detach(), r) for p, r in zip(net.parameters(), ref))
    o0 = opt.offsets[0]
    assert torch.equal(opt.flat_param[o0:o0 + w0.numel()].view(16, 3, 3, 8), ref[0].permute(0, 2, 3, 1))    # the slot holds (co, ky, kx, ci)
    assert all(p._e2eft_flat[0] is opt.shadow and p._e2eft_flat[1] == o for p, o in zip(opt.params, opt.offsets))
    assert F.shadow_view(w0, torch.float32) is None                                                    # same dtype: no twin needed
    x = torch.randn(2, 8, 5, 5)
    net(x).sum().backward()
    g0 = w0.grad
    assert g0.data_ptr() == opt.flat_grad.data_ptr() + 4 * o0 and g0.stride() == w0.stride()
    want = torch.autograd.grad(torch.nn.functional.conv2d(x, ref[0].requires_grad_(True), ref[1], padding=1).pow(1).sum() * 0 + net(x).sum(), [w0])[0]
    assert torch.allclose(g0, want)
    assert torch.allclose(opt.flat_grad[o0:o0 + w0.numel()].view(16, 3, 3, 8), want.permute(0, 2, 3, 1))
    w0.grad = None                                                                                      # a generic loop's set_to_none
    net(x).sum().backward()
    opt._adopt_grads()
    assert w0.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * o0 and torch.allclose(w0.grad, want)
    opt.exp_avg.normal_()
    sd = opt.state_dict()
    assert sd["state"][0]["exp_avg"].shape == (16, 8, 3, 3) and torch.equal(sd["state"][0]["exp_avg"], opt.state[w0]["exp_avg"])
    keep = [opt.state[p]["exp_avg"].clone() for p in opt.params]
    opt.exp_avg.zero_()
    opt.load_state_dict(sd)
    assert all(torch.equal(opt.state[p]["exp_avg"], k) for p, k in zip(opt.params, keep))
    assert opt.state[w0]["exp_avg"].data_ptr() == opt.exp_avg.data_ptr() + 4 * o0
    assert torch.equal(net.state_dict()["0.weight"], ref[0].detach())


def test_ema_model_follows_the_diffusers_definition_and_round_trips(tmp_path):
    """training.EMAModel = diffusers.training_utils.EMAModel as GeoWizard's training script drives it (train_depth_normal.py:352-353,380-391,785-786,843-850;
    diffusers itself is not in the tree: the decay schedule and the update are its published formulas, evaluated here independently).  Per-tensor path (no
    flat buffer, CPU); the flat-buffer path is tests/test_train_gpu.py::test_ema_on_the_flat_buffer."""
    from oracle import config
    from diffusion_e2e_ft_amd.training import EMAModel
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.Linear(4, 2))
    net[1].bias.requires_grad_(False)
    ema = EMAModel(net.parameters(), decay=0.9, update_after_step=1)
    ref = [p.detach().clone() for p in net.parameters()]
    for it in range(1, 9):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.1 * torch.randn_like(p))
        ema.step(net.parameters())
        step = max(0, it - 1 - 1)
        decay = 0.0 if step <= 0 else max(min((1 + step) / (10 + step), 0.9), 0.0)
        assert ema.cur_decay_value == decay and ema.optimization_step == it
        for r, p in zip(ref, net.parameters()):
            if p.requires_grad:
                r.sub_((1 - decay) * (r - p.detach()))
            else:
                r.copy_(p.detach())
        assert all(torch.equal(a, b) for a, b in zip(ema.shadow_params, ref))
    w = EMAModel(net.parameters(), use_ema_warmup=True, inv_gamma=2.0, power=0.75, decay=0.9999)
    assert abs(w.get_decay(12) - (1 - (1 + 11 / 2.0) ** -0.75)) < 1e-15 and w.get_decay(1) == 0.0
    # store / copy_to / restore around validation
    live = [p.detach().clone() for p in net.parameters()]
    ema.store(net.parameters())
    ema.copy_to(net.parameters())
    assert all(torch.equal(p, s_) for p, s_ in zip(net.parameters(), ema.shadow_params))
    ema.restore(net.parameters())
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), live)) and ema.temp_stored_params is None
    with pytest.raises(RuntimeError):
        ema.restore(net.parameters())
    sd = ema.state_dict()
    assert sorted(sd) == sorted(["decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power", "shadow_params"])
    other = EMAModel(net.parameters())
    other.load_state_dict(sd)
    assert other.optimization_step == 8 and other.decay == 0.9 and all(torch.equal(a, b) for a, b in zip(other.shadow_params, ema.shadow_params))
    # save_pretrained / from_pretrained: a model checkpoint whose config carries the EMA state (the accelerate hooks of train_depth_normal.py:380-391)
    unet = UNet2DConditionModel(**config.TINY_UNET)
    e2 = EMAModel(unet.parameters(), decay=0.95, model_cls=UNet2DConditionModel, model_config=unet.config)
    with torch.no_grad():
        for p in unet.parameters():
            p.mul_(1.5)
    for _ in range(3):
        e2.step(unet.parameters())
    e2.save_pretrained(str(tmp_path / "unet_ema"))
    back = EMAModel.from_pretrained(str(tmp_path / "unet_ema"), UNet2DConditionModel)
    assert back.optimization_step == 3 and back.decay == 0.95 and len(back.shadow_params) == len(e2.shadow_params)
    assert all(torch.equal(a, b) for a, b in zip(back.shadow_params, e2.shadow_params))
    with pytest.raises(ValueError):
        EMAModel(net.parameters()).save_pretrained(str(tmp_path / "x"))


def test_conv_desc_builder_output_size_and_every_field():
    """ops._conv_desc is the one place a ConvDesc is made.  Its output grid is torch's convolution over the explicitly padded (and nearest-upsampled) tensor, and for
    the arguments of each of the five former fill sites — ops.conv2d, the split-plane descriptor, the tensor form of the backward wrappers, the weight gradient's
    16-bit planes, conv2d_dgrad — every field is what that site set, the fields it left to ctypes' zero initialisation included."""
    import itertools
    from diffusion_e2e_ft_amd import _lib, ops

    def fields(d):
        return {n: getattr(d, n) for n, _ in _lib.ConvDesc._fields_}

    B, c1, c2, cout = 2, 8, 16, 24
    for H, W, k, stride, pad, up in itertools.product((7, 8, 9), (7, 8, 9), (1, 3, 4), (1, 2), ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 0, 1)), (False, True)):
        pt, pb, pl, pr = pad
        up_to = (2 * H, 2 * W) if up else None
        hl, wl = up_to or (H, W)
        x = torch.zeros(B, H, W, 12)[..., :c1]                 # a channel slice of a wider buffer: pixel stride 12
        x2 = torch.zeros(B, H, W, c2)
        t = x.permute(0, 3, 1, 2)
        if up:
            t = torch.nn.functional.interpolate(t, size=up_to, mode="nearest")
        want = torch.nn.functional.conv2d(torch.nn.functional.pad(t, (pl, pr, pt, pb)), torch.zeros(cout, c1, k, k), stride=stride).shape
        hout, wout = want[2], want[3]
        case = (H, W, k, stride, pad, up)
        # 1. ops.conv2d: operands as tensors, every stride set
        d = ops._conv_desc(x, x2, cout, k, k, stride, pad, up_to, 0.5, 32, 40, k * k * (c1 + c2) + 8)
        assert (d.hout, d.wout) == (hout, wout), case
        assert fields(d) == dict(dtype=0, batch=B, hin=H, win=W, hl=hl, wl=wl, c1=c1, ldx1=12, c2=c2, ldx2=c2, kh=k, kw=k, stride=stride, pad_t=pt, pad_l=pl,
                                 hout=hout, wout=wout, cout=cout, ldo=32, ldr=40, ldw=k * k * (c1 + c2) + 8, alpha=0.5), case
        # 2. split planes of c1 fp32 channels (f16 pairs at pixel stride 2 c1, weight rows [w0 | w1 | w0]), one source, alpha 1 unless given
        d = ops._f32split_desc(B, H, W, c1, cout, k, k, stride, pad, 32, 40, up_to=up_to)
        assert fields(d) == dict(dtype=0, batch=B, hin=H, win=W, hl=hl, wl=wl, c1=c1, ldx1=2 * c1, c2=0, ldx2=0, kh=k, kw=k, stride=stride, pad_t=pt, pad_l=pl,
                                 hout=hout, wout=wout, cout=cout, ldo=32, ldr=40, ldw=k * k * 3 * c1, alpha=1.0), case
        # 3. the tensor form of the backward wrappers and the tests: ldr / ldw stay zero, one source
        d = ops._conv_desc(x.half(), None, cout, k, k, stride, pad, up_to, 1.0, ldo=cout)
        assert fields(d) == dict(dtype=1, batch=B, hin=H, win=W, hl=hl, wl=wl, c1=c1, ldx1=c1, c2=0, ldx2=0, kh=k, kw=k, stride=stride, pad_t=pt, pad_l=pl,
                                 hout=hout, wout=wout, cout=cout, ldo=cout, ldr=0, ldw=0, alpha=1.0), case
        if not up:
            # 4. the weight gradient's 16-bit planes of an fp32 tensor: geometry, f16, nothing but the source's stride
            d = ops._conv_desc((3, H, W, c1, 2 * c1), None, cout, k, k, stride, pad, None, 1.0, dtype=_lib.F16)
            assert fields(d) == dict(dtype=1, batch=3, hin=H, win=W, hl=H, wl=W, c1=c1, ldx1=2 * c1, c2=0, ldx2=0, kh=k, kw=k, stride=stride, pad_t=pt, pad_l=pl,
                                     hout=hout, wout=wout, cout=cout, ldo=0, ldr=0, ldw=0, alpha=1.0), case
        # 5. conv2d_dgrad: the forward's geometry over a dense dX of c1 + c2 channels
        d = ops._conv_desc((B, H, W, c1, c1), (c2, c2), 32, k, k, stride, pad, up_to, 0.25, dtype=_lib.BF16)
        assert fields(d) == dict(dtype=2, batch=B, hin=H, win=W, hl=hl, wl=wl, c1=c1, ldx1=c1, c2=c2, ldx2=c2, kh=k, kw=k, stride=stride, pad_t=pt, pad_l=pl,
                                 hout=hout, wout=wout, cout=32, ldo=0, ldr=0, ldw=0, alpha=0.25), case
    assert ops._conv_out_hw(64, 64, 3, 3, 1, (1, 1, 1, 1)) == (64, 64)


def test_wgrad_batch_step_limits():
    """ops._wgrad_batch_step: images per launch so that neither operand reaches the 4 GB of one 32-bit buffer descriptor nor the launch 2^24 output pixels"""
    from diffusion_e2e_ft_amd import ops
    assert ops._wgrad_batch_step(1 << 20, 64 * 64, 32) == 32                       # everything fits: the whole batch
    assert ops._wgrad_batch_step(576 * 576 * 256 * 2, 576 * 576, 32) == 25          # 170 MB per image: 25 images stay below 0xFFFF0000 bytes
    assert ops._wgrad_batch_step(1 << 10, 1 << 22, 32) == 3                         # 2^22 pixels per image: three images stay below 2^24
    assert ops._wgrad_batch_step(1 << 33, 1, 4) == 1 and ops._wgrad_batch_step(0, 0, 4) == 4


@pytest.mark.parametrize("header", ["igemm.h", "igemm_epilogue.h"])
def test_igemm_headers_compile_on_their_own(header, tmp_path):
    """each header of the implicit-GEMM family is a translation unit by itself: everything its templates name is declared by what it includes (device-side syntax
    check only, nothing is instantiated or linked)"""
    import shutil
    import subprocess
    from diffusion_e2e_ft_amd import build
    hipcc = next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    tu = tmp_path / "tu.hip"
    tu.write_text('#include "%s"\n' % header)
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-I", build.CSRC, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
