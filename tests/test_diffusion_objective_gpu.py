"""The diffusion objective of the GeoWizard trainer (GeoWizard/geowizard/training/train_depth_normal.py:598-717 without --e2e_ft) on the GPU: the four kernels of
csrc/diffusion.hip against the CPU restatement tests/diffusion_objective_ref.py, and `training.geowizard_diffusion_loss` against the golden micro-step
(tests/golden/diffusion_objective_golden.pt from tests/golden/make_diffusion_objective_golden.py).

Bars.  add_noise / get_velocity in fp32: 0 differing bits (every step is one correctly rounded IEEE operation on both sides).  Masked MSE forward and backward
against a float64 evaluation of the same fp32 inputs: 2^-22 relative — an fp32 difference and its square carry 3 x 2^-24 together with the final rounding, the sum
is fp64.  Whole micro-step: the bars of tests/test_train_gpu.py (loss 1e-4, gradient norms 2e-3, sampled gradients 2e-3 of their largest entry).  bf16 micro-step:
twice the error of the restatement run in bf16 on the CPU against its own fp32 loss (stored in the golden file)."""
import os

import pytest
import torch

import diffusion_objective_ref as ref
import golden_cases as gc
from oracle import config, pipeline_ref
from util import rel_err

pytestmark = pytest.mark.gpu

GOLD = torch.load(os.path.join(os.path.dirname(__file__), "golden", "diffusion_objective_golden.pt"))
BAR = 2.0 ** -22
T4 = (0, 999, 500, 1)


def _mask_72x88():
    g = torch.Generator().manual_seed(11)
    return torch.rand(2, 1, 72, 88, generator=g) > 0.01          # P(cell valid) = 0.99^64 = 0.53


_SMALL = {}


def _small():
    """R = 4 rows, c = 4, 9 x 11 cells, the mask of _mask_72x88() — CPU tensors and the restatement's results, computed once and never modified"""
    if not _SMALL:
        g = torch.Generator().manual_seed(12)
        x0, nz, pred = (torch.randn(4, 4, 9, 11, generator=g) for _ in range(3))
        t = torch.tensor(T4, dtype=torch.long)
        abar = pipeline_ref.alphas_cumprod()
        lm = ref.latent_mask_ref(_mask_72x88())
        _SMALL.update(x0=x0, nz=nz, pred=pred, t=t, abar=abar, lm=lm, x_t=ref.add_noise_ref(abar, x0, nz, t), v=ref.get_velocity_ref(abar, x0, nz, t),
                      sel=lm.repeat(2, 4, 1, 1))
    return _SMALL


def _nhwc(x, dev, dtype=torch.float32):
    return x.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=dtype)


def _nchw(x):
    return x.permute(0, 3, 1, 2).cpu()


def _dev_small(dev):
    from diffusion_e2e_ft_amd import ops
    s = _small()
    d = dict(x0=_nhwc(s["x0"], dev), nz=_nhwc(s["nz"], dev), pred=_nhwc(s["pred"], dev), t=s["t"].to(dev), abar=s["abar"].to(dev))
    d["lm"] = ops.latent_valid_mask(_mask_72x88().to(dev))
    return s, d


def _bits_differ(a, b):
    return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


# ---- 1. mask kernel ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["objective", "72x88", "all_valid", "all_invalid", "unaligned_uint8"])
def test_latent_valid_mask_equals_max_pool(dev, case):
    from diffusion_e2e_ft_amd import ops
    vm = {"objective": ref.objective_mask, "72x88": _mask_72x88, "all_valid": lambda: torch.ones(2, 1, 72, 88, dtype=torch.bool),
          "all_invalid": lambda: torch.zeros(2, 1, 72, 88, dtype=torch.bool), "unaligned_uint8": _mask_72x88}[case]()
    want = ref.latent_mask_ref(vm)[:, 0].to(torch.uint8)
    if case == "unaligned_uint8":      # nonzero = valid, base pointer one byte off an 8-byte boundary: the byte-wise form of the kernel
        flat = torch.zeros(vm.numel() + 1, dtype=torch.uint8, device=dev)
        dvm = flat[1:].view(2, 72, 88)
        dvm.copy_(vm[:, 0].to(torch.uint8) * 7)
        assert dvm.data_ptr() % 8 == 1
    else:
        dvm = vm.to(dev)
    got = ops.latent_valid_mask(dvm)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)
    if case == "objective":
        assert tuple(int(m.sum()) for m in got) == ref.SELECTED_CELLS
    if case == "72x88":
        assert 0 < int(got.sum()) < got.numel() and got.shape[1:] == (9, 11)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ops.latent_valid_mask(torch.ones(1, 1, 60, 64, dtype=torch.bool, device=dev))


# ---- 2. add_noise and the target ------------------------------------------------------------------------------------------------------------------------
def test_add_noise_and_targets_are_bit_equal_to_the_restatement_fp32(dev):
    from diffusion_e2e_ft_amd import ops, _lib
    s, d = _dev_small(dev)
    xin = torch.full((4, 9, 11, 8), -7.25, device=dev)           # the 8-channel UNet input: channels 0:4 must stay as they are
    out = ops.diffusion_mix_(d["x0"], d["nz"], d["t"], d["abar"], xin[..., 4:])
    assert out.data_ptr() == xin[..., 4:].data_ptr()
    assert _bits_differ(_nchw(xin[..., 4:]), s["x_t"]) == 0
    assert bool((xin[..., :4] == -7.25).all())
    vel = torch.empty((4, 9, 11, 4), device=dev)
    ops.diffusion_mix_(d["x0"], d["nz"], d["t"], d["abar"], vel, _lib.DIFFUSION_VELOCITY)
    assert _bits_differ(_nchw(vel), s["v"]) == 0
    _, _, tv = ops.masked_mse_fwd(d["pred"], d["x0"], d["nz"], d["t"], d["abar"], d["lm"], "v_prediction", want_target=True)
    assert _bits_differ(_nchw(tv), s["v"]) == 0
    _, _, te = ops.masked_mse_fwd(d["pred"], d["x0"], d["nz"], d["t"], d["abar"], d["lm"], "epsilon", want_target=True)
    assert _bits_differ(_nchw(te), s["nz"]) == 0
    # t outside the table is clamped (the kernel must not read outside it): the ends of the table
    t_out = torch.tensor([-5, 1000, 1 << 40, 999], device=dev)
    t_in = torch.tensor([0, 999, 999, 999], device=dev)
    a, b = torch.empty_like(vel), torch.empty_like(vel)
    ops.diffusion_mix_(d["x0"], d["nz"], t_out, d["abar"], a)
    ops.diffusion_mix_(d["x0"], d["nz"], t_in, d["abar"], b)
    assert torch.equal(a, b)
    # unaligned operands (a pixel stride of 5): the element-wise form gives the same bits
    wide = torch.zeros((4, 9, 11, 5), device=dev)
    x5, n5 = torch.zeros_like(wide), torch.zeros_like(wide)
    x5[..., 1:].copy_(d["x0"])
    n5[..., 1:].copy_(d["nz"])
    ops.diffusion_mix_(x5[..., 1:], n5[..., 1:], d["t"], d["abar"], wide[..., 1:])
    assert _bits_differ(_nchw(wide[..., 1:]), s["x_t"]) == 0 and bool((wide[..., 0] == 0).all())
    with pytest.raises(ValueError, match="Unknown prediction type"):
        ops.masked_mse_fwd(d["pred"], d["x0"], d["nz"], d["t"], d["abar"], d["lm"], "sample")


def test_coefficients_of_the_whole_table_are_correctly_rounded_roots(dev):
    """x0 = 1, noise = 0 makes x_t the coefficient sqrt(abar[t]) itself, x0 = 0, noise = 1 makes it sqrt(1 - abar[t]): all 1000 timesteps, one row each, against
    the correctly rounded roots (diffusion_objective_ref.root)"""
    from diffusion_e2e_ft_amd import ops
    abar = pipeline_ref.alphas_cumprod()
    t = torch.arange(1000, device=dev)
    one, zero = torch.ones((1000, 1, 1, 1), device=dev), torch.zeros((1000, 1, 1, 1), device=dev)
    sa = ops.diffusion_mix_(one, zero, t, abar.to(dev), torch.empty_like(one)).reshape(-1).cpu()
    sb = ops.diffusion_mix_(zero, one, t, abar.to(dev), torch.empty_like(one)).reshape(-1).cpu()
    bad_a, bad_b = (sa != ref.root(abar)).nonzero().reshape(-1).tolist(), (sb != ref.root(1 - abar)).nonzero().reshape(-1).tolist()
    assert not bad_a and not bad_b, ("sqrt(abar[t]) differs at t = %s, sqrt(1 - abar[t]) at t = %s" % (bad_a[:10], bad_b[:10]))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_add_noise_16bit_is_the_fp32_result_rounded_once(dev, dtype):
    from diffusion_e2e_ft_amd import ops
    s, d = _dev_small(dev)
    xin = torch.zeros((4, 9, 11, 8), dtype=dtype, device=dev)
    ops.diffusion_mix_(d["x0"], d["nz"], d["t"], d["abar"], xin[..., 4:])
    assert torch.equal(_nchw(xin[..., 4:]), s["x_t"].to(dtype))
    # 16-bit operands: read as their float values
    x16, n16 = d["x0"].to(dtype), d["nz"].to(dtype)
    ops.diffusion_mix_(x16, n16, d["t"], d["abar"], xin[..., 4:])
    want = ref.add_noise_ref(s["abar"], s["x0"].to(dtype).float(), s["nz"].to(dtype).float(), s["t"]).to(dtype)
    assert torch.equal(_nchw(xin[..., 4:]), want)


# ---- 3. masked MSE forward -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
def test_masked_mse_forward_against_float64(dev, pt):
    from diffusion_e2e_ft_amd import ops
    s, d = _dev_small(dev)
    target = s["nz"] if pt == "epsilon" else s["v"]
    want = float(((s["pred"].double() - target.double())[s["sel"]] ** 2).mean())
    loss, nsel, none = ops.masked_mse_fwd(d["pred"], d["x0"], d["nz"], d["t"], d["abar"], d["lm"], pt)
    assert none is None and loss.dtype == torch.float32 and nsel.dtype == torch.int64
    err = abs(loss.item() - want) / want
    print("masked MSE %s: loss %.9g, float64 %.9g, relative error %.3g (bar %.3g); torch fp32 %.3g" % (
        pt, loss.item(), want, err, BAR, abs(float(ref.masked_mse_ref(s["pred"], target, s["lm"])[0]) - want) / want))
    assert nsel.item() == int(s["sel"].sum()) and 0 < nsel.item() < s["sel"].numel()
    assert err <= BAR
    loss2, nsel2, _ = ops.masked_mse_fwd(d["pred"], d["x0"], d["nz"], d["t"], d["abar"], d["lm"], pt)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(nsel, nsel2)
    # an all-invalid mask: exactly 0.0, nothing selected, no NaN
    l0, n0, _ = ops.masked_mse_fwd(d["pred"], d["x0"], d["nz"], d["t"], d["abar"], torch.zeros_like(d["lm"]), pt)
    assert l0.view(torch.int32).item() == 0 and n0.item() == 0
    # a 16-bit prediction is read as its float value
    for dt16 in (torch.float16, torch.bfloat16):
        p16 = d["pred"].to(dt16)
        want16 = float(((s["pred"].to(dt16).double() - target.double())[s["sel"]] ** 2).mean())
        l16, n16, _ = ops.masked_mse_fwd(p16, d["x0"], d["nz"], d["t"], d["abar"], d["lm"], pt)
        assert abs(l16.item() - want16) <= BAR * want16 and n16.item() == nsel.item(), (dt16, l16.item(), want16)


# ---- 4. backward ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
def test_masked_mse_backward_against_float64(dev, pt):
    from diffusion_e2e_ft_amd import ops, autograd as F
    s, d = _dev_small(dev)
    target = s["nz"] if pt == "epsilon" else s["v"]
    sel = s["sel"]
    gout = torch.tensor([0.75], device=dev)
    _, nsel, _ = ops.masked_mse_fwd(d["pred"], d["x0"], d["nz"], d["t"], d["abar"], d["lm"], pt)
    dp = ops.masked_mse_bwd(d["pred"], d["x0"], d["nz"], d["t"], d["abar"], d["lm"], pt, nsel, gout)
    got = _nchw(dp)
    want = 0.75 * 2.0 * (s["pred"].double() - target.double()) / float(sel.sum())
    err = ((got.double() - want).abs() / want.abs())[sel]
    print("masked MSE backward %s: worst relative error %.3g (bar %.3g)" % (pt, float(err.max()), BAR))
    assert float(err.max()) <= BAR
    assert bool((got[~sel].view(torch.int32) == 0).all()) and int((~sel).sum()) > 0
    z = ops.masked_mse_fwd(d["pred"], d["x0"], d["nz"], d["t"], d["abar"], torch.zeros_like(d["lm"]), pt)[1]
    dz = ops.masked_mse_bwd(d["pred"], d["x0"], d["nz"], d["t"], d["abar"], torch.zeros_like(d["lm"]), pt, z, gout)
    assert bool((dz.view(torch.int32) == 0).all())
    # through the autograd Function: pred as the UNet hands it over (logical NCHW)
    pred = d["pred"].permute(0, 3, 1, 2).detach().requires_grad_(True)
    out = F.masked_mse(pred, d["x0"], d["nz"], d["t"], d["abar"], d["lm"], pt)
    assert len(out) == 2 and out[0].requires_grad and not out[1].requires_grad
    (g,) = torch.autograd.grad(out[0], pred, grad_outputs=gout[0])
    assert g.shape == pred.shape and torch.equal(g, dp.permute(0, 3, 1, 2))


# ---- 5-8, 10. the whole micro-step ---------------------------------------------------------------------------------------------------------------------
def _models(dev, compute=None):
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    unet = UNet2DConditionModel(**config.TINY_GEOWIZARD_UNET)
    unet.load_state_dict(gc.tiny_geo_sd())
    unet = unet.to(dev).train()
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(gc.tiny_vae_sd())
    vae = vae.to(dev).eval()
    vae.requires_grad_(False)
    if compute is not None:
        unet.set_compute_dtype(compute)
        vae = vae.to(compute)
    return unet, vae


def _check_grads(named, gold, tol=2e-3, sampled=True):
    """tests/test_train_gpu.py's bars, unchanged"""
    bad = []
    floor = 1e-6 * max(gold["grad_norms"].values())
    for k, n_ref in gold["grad_norms"].items():
        g = named[k].grad
        assert g is not None, k
        n = g.float().norm().item()
        if abs(n - n_ref) > tol * n_ref + floor:
            bad.append((k, n, n_ref))
    assert not bad, bad[:10]
    for k, r in gold["grads"].items() if sampled else ():
        if gold["grad_norms"][k] <= floor:
            continue
        e = rel_err(gc.sample_grad(named[k].grad.float()), r)
        assert e < tol, (k, e)


@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
def test_micro_step_against_the_golden_fp32(dev, pt):
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.scheduler import DDPMScheduler
    unet, vae = _models(dev)
    batch, emb, timesteps, noise = ref.objective_inputs()
    gold = GOLD[pt]
    loss, nsel, target, x_t = training.geowizard_diffusion_loss(unet, vae, batch, emb, "indoor", noise_scheduler=DDPMScheduler(), noise=noise, timesteps=timesteps,
                                                                prediction_type=pt, return_parts=True)
    print("micro-step %s: loss %.8g, golden %.8g" % (pt, loss.item(), gold["loss"].item()))
    assert abs(loss.item() - gold["loss"].item()) <= 1e-4 * abs(gold["loss"].item()), (loss.item(), gold["loss"].item())
    assert nsel.item() == gold["n_selected"] == 2 * 4 * sum(ref.SELECTED_CELLS)
    assert tuple(target.shape) == tuple(x_t.shape) == (4, 4, 8, 8) and target.dtype == torch.float32
    assert rel_err(target.reshape(-1)[::ref.TARGET_STRIDE], gold["target"]) < 1e-3
    assert rel_err(x_t.reshape(-1)[::ref.TARGET_STRIDE], gold["x_t"]) < 1e-3
    if pt == "epsilon":
        assert torch.equal(target.cpu(), noise)
    loss.backward()
    _check_grads(dict(unet.named_parameters()), gold)
    for p in vae.parameters():
        assert p.grad is None
    # the scheduler's own prediction type is the default; an unknown one is refused as the trainer refuses it (:682)
    with torch.no_grad():
        again = training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_scheduler=DDPMScheduler(prediction_type=pt), noise=noise, timesteps=timesteps)
    assert again.item() == loss.item()
    with pytest.raises(ValueError, match="Unknown prediction type"):
        training.geowizard_diffusion_loss(unet, vae, batch, emb, noise=noise, timesteps=timesteps, prediction_type="sample")


def test_empty_mask_gives_zero_loss_and_zero_gradients(dev):
    from diffusion_e2e_ft_amd import training
    unet, vae = _models(dev)
    batch, emb, timesteps, noise = ref.objective_inputs()
    batch["val_mask"] = torch.zeros_like(batch["val_mask"])
    loss, nsel, _, _ = training.geowizard_diffusion_loss(unet, vae, batch, emb, noise=noise, timesteps=timesteps, return_parts=True)
    assert loss.item() == 0.0 and nsel.item() == 0
    loss.backward()
    assert all(p.grad is not None and bool((p.grad == 0).all()) for p in unet.parameters())


def test_reference_call_form_equals_the_fused_path(dev):
    """the trainer's own lines 671, 680 and 717 on the product scheduler and torch's boolean-mask mse_loss, against the fused kernels"""
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.scheduler import DDPMScheduler
    unet, vae = _models(dev)
    batch, emb, timesteps, noise = ref.objective_inputs()
    noise_scheduler = DDPMScheduler()
    with torch.no_grad():
        fused, nsel, f_target, f_x_t = training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_scheduler=noise_scheduler, noise=noise, timesteps=timesteps,
                                                                         return_parts=True)
        images = torch.cat((batch["rgb"], batch["depth"], batch["normals"] * -1), dim=0).to(dev)
        batch_latents = training.encode_image(vae, images) * vae.config.scaling_factor
        rgb_latents, depth_latents, normal_latents = torch.chunk(batch_latents, 3, dim=0)
        geo_latents = torch.cat((depth_latents, normal_latents), dim=0)
        ts = timesteps.to(dev).repeat(2).long()
        nz = noise.to(dev)
        noisy_geo_latents = noise_scheduler.add_noise(geo_latents, nz, ts)                     # :671
        target = noise_scheduler.get_velocity(geo_latents, nz, ts)                             # :680
        assert torch.equal(noisy_geo_latents, f_x_t) and torch.equal(target, f_target)
        assert noise_scheduler.alphas_cumprod_on(dev) is noise_scheduler.alphas_cumprod_on(dev)      # uploaded once per (scheduler, device)
        latent_mask = ~torch.max_pool2d((~batch["val_mask"].to(dev)).float(), 8, 8).bool()
        latent_mask = latent_mask.repeat((2, 4, 1, 1))
        unet_input = torch.cat((rgb_latents.repeat(2, 1, 1, 1), noisy_geo_latents), dim=1)
        cls = training.geowizard_class_embedding(2, "indoor", torch.float32, dev)
        noise_pred = unet(unet_input, ts, emb.to(dev).repeat(2, 1, 1), class_labels=cls, return_dict=False)[0]
        loss = torch.nn.functional.mse_loss(noise_pred[latent_mask].float(), target[latent_mask].float(), reduction="mean")      # :717
    print("reference call form %.9g, fused %.9g" % (loss.item(), fused.item()))
    assert int(latent_mask.sum()) == nsel.item()
    assert abs(loss.item() - fused.item()) <= BAR * abs(loss.item())


def test_device_drawn_noise_and_timesteps(dev):
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    unet, vae = _models(dev)
    batch, emb, _, _ = ref.objective_inputs()
    runs = []
    with torch.no_grad():
        for _ in range(2):
            torch.manual_seed(1234)
            runs.append(training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_type="gaussian", generator=DeviceNoise(9), prediction_type="epsilon",
                                                          return_parts=True))
        (l0, n0, tg0, xt0), (l1, n1, tg1, xt1) = runs
        assert torch.equal(l0, l1) and torch.equal(n0, n1) and torch.equal(tg0, tg1) and torch.equal(xt0, xt1)
        assert 0.5 < float(tg0.std()) < 1.5 and not torch.equal(tg0[:2], tg0[2:])      # standard normals, depth and normal rows drawn apart
        # the parts reproduce the loss through the explicit form: the epsilon target IS the noise, the timesteps are torch's next draw
        torch.manual_seed(1234)
        ts = torch.randint(0, 1000, (2,), device=dev)
        l2, n2, tg2, xt2 = training.geowizard_diffusion_loss(unet, vae, batch, emb, noise=tg0, timesteps=ts, prediction_type="epsilon", return_parts=True)
        assert torch.equal(l0, l2) and torch.equal(n0, n2) and torch.equal(xt0, xt2) and torch.equal(tg0, tg2)
        lz = training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_type="zeros", timesteps=ts)
        assert torch.isfinite(lz) and lz.item() != l0.item()
    with pytest.raises(ValueError, match="t / 1000"):
        training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_type="pyramid", generator=DeviceNoise(9))
    with pytest.raises(ValueError, match="t / 1000"):
        training.geowizard_e2e_ft_loss(unet, vae, batch, emb, noise_type="pyramid", generator=DeviceNoise(9))
    with pytest.raises(TypeError, match="DeviceNoise"):
        training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_type="gaussian")


def test_gradient_checkpointing_gives_bit_equal_gradients(dev):
    from diffusion_e2e_ft_amd import training
    batch, emb, timesteps, noise = ref.objective_inputs()

    def run(ckpt):
        unet, vae = _models(dev)
        if ckpt:
            unet.enable_gradient_checkpointing()
            assert unet.gradient_checkpointing
        loss = training.geowizard_diffusion_loss(unet, vae, batch, emb, noise=noise, timesteps=timesteps)
        loss.backward()
        return loss.item(), {k: p.grad.clone() for k, p in unet.named_parameters()}

    l0, g0 = run(False)
    l1, g1 = run(True)
    assert l0 == l1
    assert all(torch.equal(g0[k], g1[k]) for k in g0), [k for k in g0 if not torch.equal(g0[k], g1[k])][:5]


@pytest.mark.parametrize("pt", ["epsilon", "v_prediction"])
def test_micro_step_bf16_compute(dev, pt):
    from diffusion_e2e_ft_amd import training
    unet, vae = _models(dev, torch.bfloat16)
    batch, emb, timesteps, noise = ref.objective_inputs()
    gold = GOLD[pt]
    bar = 2.0 * gold["bf16_loss_error"]
    loss, nsel, target, x_t = training.geowizard_diffusion_loss(unet, vae, batch, emb, noise=noise, timesteps=timesteps, prediction_type=pt, return_parts=True)
    err = abs(loss.item() - gold["loss"].item()) / abs(gold["loss"].item())
    print("bf16 micro-step %s: loss %.6g, fp32 golden %.6g, relative error %.3g, bar %.3g (twice the bf16 restatement's %.3g)" % (
        pt, loss.item(), gold["loss"].item(), err, bar, gold["bf16_loss_error"]))
    assert nsel.item() == gold["n_selected"] and x_t.dtype == torch.bfloat16 and target.dtype == torch.float32
    assert err <= bar
    loss.backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()) for p in unet.parameters())


# ---- 9. no synchronisation: the four kernels in one captured graph ---------------------------------------------------------------------------------------
def test_objective_kernels_replay_from_one_captured_graph(dev):
    from diffusion_e2e_ft_amd import ops
    s, d = _dev_small(dev)
    vm = _mask_72x88().to(dev)
    xin = torch.zeros((4, 9, 11, 8), device=dev)
    gout = torch.tensor([1.0], device=dev)
    t, pred = d["t"].clone(), d["pred"].clone()

    def objective():
        lm = ops.latent_valid_mask(vm)
        ops.diffusion_mix_(d["x0"], d["nz"], t, d["abar"], xin[..., 4:])
        loss, nsel, _ = ops.masked_mse_fwd(pred, d["x0"], d["nz"], t, d["abar"], lm, "v_prediction")
        return loss, nsel, ops.masked_mse_bwd(pred, d["x0"], d["nz"], t, d["abar"], lm, "v_prediction", nsel, gout)

    objective()                                   # code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, nsel, dp = objective()
    # new contents, in place: another mask, other timesteps, another prediction
    g = torch.Generator().manual_seed(13)
    vm.copy_(torch.rand(2, 1, 72, 88, generator=g) > 0.004)
    t.copy_(torch.tensor([17, 3, 998, 640]))
    pred.copy_(_nhwc(torch.randn(4, 4, 9, 11, generator=g), dev))
    graph.replay()
    torch.cuda.synchronize()
    got = (loss.clone(), nsel.clone(), dp.clone(), xin.clone())
    want = objective()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]) and torch.equal(got[3], xin)
    assert got[1].item() != int(s["sel"].sum())     # the replay saw the new mask


# ---- 11. geowizard_e2e_ft_loss with noise ------------------------------------------------------------------------------------------------------------------
def test_geowizard_e2e_ft_loss_default_is_unchanged_and_noise_matches_the_restatement(dev):
    from diffusion_e2e_ft_amd import training
    batch, emb = gc.geo_train_inputs()
    _, _, _, noise = ref.objective_inputs()

    def run(**kw):
        unet, vae = _models(dev)
        loss = training.geowizard_e2e_ft_loss(unet, vae, batch, emb, "indoor", **kw)
        loss.backward()
        return loss, dict(unet.named_parameters())

    l0, p0 = run()
    l1, p1 = run(noise_type="zeros", generator=None, noise=None)
    assert torch.equal(l0, l1) and all(torch.equal(p0[k].grad, p1[k].grad) for k in p0)
    gold = GOLD["e2e_ft_noise"]
    l2, p2 = run(noise=noise)
    print("E2E-FT with x_t = noise: loss %.8g, restatement %.8g" % (l2.item(), gold["loss"].item()))
    assert abs(l2.item() - gold["loss"].item()) <= 1e-4 * abs(gold["loss"].item())
    _check_grads(p2, gold)
    assert l2.item() != l0.item()
