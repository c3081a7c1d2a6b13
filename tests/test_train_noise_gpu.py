"""training.e2e_ft_loss with a non-zero noise latent, device-drawn noise and no noise channels (training/train.py:483-518), and the pipelines'
device-noise path, on the tiny models of tests/test_train_gpu.py.  The oracle is torch autograd over the CPU restatements of oracle/pipeline_ref.py,
composed here with the SAME explicit noise tensor; tolerances are those of test_micro_step_gradients_fp32 (loss 1e-4, estimate 1e-3, gradients 2e-3)."""
import functools
import math
import random

import pytest
import torch

import golden_cases as gc
from oracle import config, pipeline_ref, unet_ref
from oracle.losses_ref import angular_loss_ref, ssi_loss_ref
from util import rel_err

pytestmark = pytest.mark.gpu


def _models(dev, in4=False):
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    unet = UNet2DConditionModel(**_unet_cfg(in4))
    unet.load_state_dict(_unet_sd(in4))
    unet = unet.to(device=dev).train()
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(gc.tiny_vae_sd())
    vae = vae.to(device=dev).eval()
    vae.requires_grad_(False)
    return unet, vae


def _unet_cfg(in4):
    return dict(config.TINY_UNET, in_channels=4) if in4 else config.TINY_UNET


def _unet_sd(in4):
    sd = gc.tiny_unet_sd()
    if in4:      # plain SD-v2: its own 4-channel conv_in = the first four input channels of the tiny one
        sd["conv_in.weight"] = sd["conv_in.weight"][:, :4].clone()
    return sd


def _noise():
    return 0.9 * torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(77))


@functools.lru_cache(maxsize=None)
def _oracle(modality, noisy_input):
    """loss, estimate and parameter gradients of one micro-step through the CPU oracle: x_t = _noise() in channels 4:8 (noisy_input) or a 4-channel UNet fed
    the rgb latent alone, x0 by v_to_x0 from that x_t (zeros without noise channels, train.py:484-485)"""
    batch, text = gc.train_batch()
    in4 = not noisy_input
    usd = {k: v.clone().requires_grad_(True) for k, v in _unet_sd(in4).items()}
    vsd = gc.tiny_vae_sd()
    rgb_latents = pipeline_ref.encode_rgb_ref(vsd, config.TINY_VAE, batch["rgb"])
    noisy = _noise() if noisy_input else torch.zeros_like(rgb_latents)
    x = torch.cat([rgb_latents, noisy], dim=1) if noisy_input else rgb_latents
    v = unet_ref.unet_forward(usd, _unet_cfg(in4), x, 999, text.repeat(rgb_latents.shape[0], 1, 1))
    x0 = pipeline_ref.v_to_x0(v, noisy, 999)
    est = pipeline_ref.decode_ref(vsd, config.TINY_VAE, x0)
    mask = batch["val_mask"].bool()
    if modality == "depth":
        est = torch.clamp(est.mean(dim=1, keepdim=True), -1, 1)
        loss = ssi_loss_ref(est, batch["metric"], mask)
    else:
        est = torch.clamp(est / (torch.norm(est, p=2, dim=1, keepdim=True) + 1e-5), -1, 1)
        loss = angular_loss_ref(est, batch["normals"], mask)
    loss.backward()
    return {"loss": loss.detach(), "estimate": est.detach(), "grads": {k: p.grad.detach() for k, p in usd.items()}}


def _check(loss, est, unet, gold, tol=2e-3):
    assert abs(loss.item() - gold["loss"].item()) <= 1e-4 * abs(gold["loss"].item()), (loss.item(), gold["loss"].item())
    assert rel_err(est.float(), gold["estimate"]) < 1e-3
    norms = {k: float(g.norm()) for k, g in gold["grads"].items()}
    floor = 1e-6 * max(norms.values())
    bad = []
    for k, p in unet.named_parameters():
        assert p.grad is not None, k
        n = p.grad.float().norm().item()
        if abs(n - norms[k]) > tol * norms[k] + floor:
            bad.append((k, n, norms[k]))
        elif norms[k] > floor and rel_err(p.grad.float(), gold["grads"][k]) >= tol:      # every entry of every gradient, against its largest
            bad.append((k, "entries", rel_err(p.grad.float(), gold["grads"][k])))
    assert not bad, bad[:10]


@pytest.mark.parametrize("modality", ["depth", "normals"])
def test_explicit_noise_matches_oracle_fp32(dev, modality):
    from diffusion_e2e_ft_amd import training
    unet, vae = _models(dev)
    batch, text = gc.train_batch()
    loss, est = training.e2e_ft_loss(unet, vae, batch, text, modality, return_estimate=True, noise=_noise())
    loss.backward()
    _check(loss, est, unet, _oracle(modality, True))
    assert all(p.grad is None for p in vae.parameters())


@pytest.mark.parametrize("noise_type", ["gaussian", "pyramid"])
def test_device_drawn_noise(dev, noise_type):
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    unet, vae = _models(dev)
    batch, text = gc.train_batch()
    zeros = training.e2e_ft_loss(unet, vae, batch, text, "depth").item()
    losses = []
    for _ in range(2):
        random.seed(3)          # the pyramid's level sizes come from Python's `random`, as in the reference
        g = DeviceNoise(41, draw=6)
        losses.append(training.e2e_ft_loss(unet, vae, batch, text, "depth", noise_type=noise_type, generator=g))
        assert g.draw == 7
    assert math.isfinite(losses[0].item()) and torch.equal(losses[0], losses[1])
    assert losses[0].item() != zeros
    random.seed(3)
    other = training.e2e_ft_loss(unet, vae, batch, text, "depth", noise_type=noise_type, generator=DeviceNoise(41, draw=7))
    assert other.item() != losses[0].item()
    losses[0].backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in unet.parameters())
    with pytest.raises(TypeError, match="DeviceNoise"):
        training.e2e_ft_loss(unet, vae, batch, text, "depth", noise_type=noise_type, generator=torch.Generator())


def test_no_noise_channels(dev):
    from diffusion_e2e_ft_amd import training
    unet, vae = _models(dev, in4=True)
    batch, text = gc.train_batch()
    loss, est = training.e2e_ft_loss(unet, vae, batch, text, "depth", return_estimate=True, noise_type=None)
    loss.backward()
    _check(loss, est, unet, _oracle("depth", False))
    unet8, _ = _models(dev)
    with pytest.raises(ValueError, match="in_channels"):
        training.e2e_ft_loss(unet8, vae, batch, text, "depth", noise_type=None)
    with pytest.raises(ValueError, match="nowhere to go"):
        training.e2e_ft_loss(unet, vae, batch, text, "depth", noise_type=None, noise=_noise())


def _old_zeros_path(unet, vae, batch, text, modality):
    """the micro-step as it was before `noise_type` existed, composed from the same public pieces: zeros concatenated behind the rgb latent, x0 by the one scale"""
    from diffusion_e2e_ft_amd import autograd as F
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    dev, dt = unet.device, unet.dtype
    with torch.no_grad():
        rgb_latents = training.encode_image(vae, batch["rgb"].to(device=dev, dtype=dt)) * vae.config.scaling_factor
    b = rgb_latents.shape[0]
    unet_input = torch.cat((rgb_latents, torch.zeros_like(rgb_latents)), dim=1).contiguous(memory_format=torch.channels_last)
    model_pred = unet(unet_input, torch.full((b,), 999, device=dev, dtype=torch.long), text.to(device=dev, dtype=dt).repeat(b, 1, 1), return_dict=False)[0]
    x0 = model_pred * (DDIMScheduler().zero_latent_x0_scale(999) / vae.config.scaling_factor)
    est = vae.decoder(vae.post_quant_conv(x0)).permute(0, 2, 3, 1)
    if modality == "depth":
        return F.ssi_loss(F.depth_head(est, to_unit=False), batch["metric"].to(dev), batch["val_mask"].bool().to(dev))
    return F.angular_loss(F.normal_head(est, clamp=True), batch["normals"].to(dev), batch["val_mask"].bool().to(dev))


@pytest.mark.parametrize("modality", ["depth", "normals"])
def test_zeros_default_is_bit_identical_to_the_old_path(dev, modality):
    from diffusion_e2e_ft_amd import _lib, training
    unet, vae = _models(dev)
    batch, text = gc.train_batch()
    _old_zeros_path(unet, vae, batch, text, modality).backward()          # warm the packed-weight caches (forward and backward): both counted runs issue the same library calls
    unet.zero_grad(set_to_none=True)
    c0 = _lib.CALLS[0]
    old = _old_zeros_path(unet, vae, batch, text, modality)
    old.backward()
    n_old = _lib.CALLS[0] - c0
    g_old = {k: p.grad.clone() for k, p in unet.named_parameters()}
    unet.zero_grad(set_to_none=True)
    c0 = _lib.CALLS[0]
    new = training.e2e_ft_loss(unet, vae, batch, text, modality)          # every new argument at its default
    new.backward()
    assert _lib.CALLS[0] - c0 == n_old          # the same number of library calls: no extra copy / scale / noise launch on the default path
    assert torch.equal(new, old)
    for k, p in unet.named_parameters():
        assert torch.equal(p.grad, g_old[k]), k
    # explicit zeros through the NEW route (input buffer written in place, x0 = c_x * 0 + c_v * v by latent_x0): the same bits again
    unet.zero_grad(set_to_none=True)
    via_new = training.e2e_ft_loss(unet, vae, batch, text, modality, noise=torch.zeros(2, 4, 8, 8))
    assert torch.equal(via_new, old)


def test_pipeline_device_pyramid_noise_equals_explicit_latent(dev):
    from diffusion_e2e_ft_amd.noise import DeviceNoise, pyramid_noise_into
    from diffusion_e2e_ft_amd.pipeline import MarigoldPipeline
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    from oracle import synth
    rgb, ctx = synth.synth_inputs(2, 64, 64, 2, 128, seed=3)
    unet, vae = _models(dev)
    pipe = MarigoldPipeline(unet.eval(), vae, DDIMScheduler())
    pipe.empty_text_embed = ctx.to(dev)
    random.seed(8)
    g = DeviceNoise(19)
    out = pipe.single_infer(rgb, 2, noise="pyramid", generator=g)
    assert g.draw == 1
    random.seed(8)
    latent = pyramid_noise_into(torch.empty(2, 8, 8, 4, device=dev), DeviceNoise(19)).permute(0, 3, 1, 2)      # the same latent, read back
    assert abs(latent.double().std().item() - 1.0) < 1e-5
    want = pipe.single_infer(rgb, 2, noise=latent.cpu())
    assert rel_err(out.float(), want.float()) <= 2e-3          # the bar of test_pipeline_multistep_matches_oracle
    # any other generator keeps torch's path: reproducible from a torch.Generator as before
    a = pipe.single_infer(rgb, 2, noise="gaussian", generator=torch.Generator(device=dev).manual_seed(1))
    b = pipe.single_infer(rgb, 2, noise="gaussian", generator=torch.Generator(device=dev).manual_seed(1))
    assert torch.equal(a, b) and not torch.equal(a, out)
    c = pipe.single_infer(rgb, 2, noise="gaussian", generator=DeviceNoise(19))
    d = pipe.single_infer(rgb, 2, noise="gaussian", generator=DeviceNoise(19))
    assert torch.equal(c, d) and not torch.equal(c, a)


@pytest.mark.parametrize("kind", ["gaussian", "pyramid"])
def test_geowizard_device_noise_equals_explicit_latent(dev, kind):
    """the joint depth + normal DDIM loop from device-drawn noise == the same loop from that latent handed in (the depth and the normal row share it)"""
    from diffusion_e2e_ft_amd.noise import DeviceNoise, noise_into
    from diffusion_e2e_ft_amd.pipeline import DepthNormalEstimationPipeline
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    rgb, emb = gc.geo_pipe_inputs()
    unet = UNet2DConditionModel(**config.TINY_GEOWIZARD_UNET)
    unet.load_state_dict(gc.tiny_geo_sd())
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(gc.tiny_vae_sd())
    pipe = DepthNormalEstimationPipeline(unet.to(dev).eval(), vae.to(dev).eval(), DDIMScheduler())
    random.seed(4)
    d, n = pipe.single_infer(rgb, img_embed=emb, num_inference_steps=2, noise=kind, generator=DeviceNoise(23))
    random.seed(4)
    B, _, H, W = rgb.shape
    latent = noise_into(kind, torch.empty(B, H // 8, W // 8, 4, device=dev), DeviceNoise(23)).permute(0, 3, 1, 2)
    d2, n2 = pipe.single_infer(rgb, img_embed=emb, num_inference_steps=2, noise=latent.cpu())
    assert rel_err(d, d2) <= 2e-3 and rel_err(n, n2) <= 2e-3
    assert torch.isfinite(d).all() and torch.isfinite(n).all()


def test_pipeline_call_passes_the_generator_through(dev):
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    from diffusion_e2e_ft_amd.pipeline import MarigoldPipeline
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    from oracle import synth
    rgb, ctx = synth.synth_inputs(1, 64, 64, 2, 128, seed=3)
    unet, vae = _models(dev)
    pipe = MarigoldPipeline(unet.eval(), vae, DDIMScheduler())
    pipe.empty_text_embed = ctx.to(dev)
    img = (rgb[0] + 1) / 2 * 255
    kw = dict(denoising_steps=2, ensemble_size=2, batch_size=1, processing_res=0, show_progress_bar=False, noise="gaussian", color_map=None)
    g = DeviceNoise(5)
    a = pipe(img, generator=g, **kw).depth_np
    assert g.draw == 2                                                  # one draw per ensemble batch
    b = pipe(img, generator=DeviceNoise(5), **kw).depth_np
    c = pipe(img, generator=DeviceNoise(6), **kw).depth_np
    assert (a == b).all() and (a != c).any()
