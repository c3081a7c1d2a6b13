"""`training.CapturedTrainStepAt`: the captured optimizer step with what `CapturedTrainStep` refuses — pyramid noise over host-drawn level sizes,
the diffusion objective's per-step timesteps, the EMA — each fed through device words the host fills before a replay.

Two identical model / optimizer twins on the tiny synthetic models, 64 x 64 micro-batches of 2; one twin steps eagerly, the other through the captured step.  Per
step the host streams (Python's `random`, numpy's global stream) are saved, the eager step runs, the streams are put back, the captured step runs: both must leave
both streams and both generators' `draw` counters where the eager step left them.  Call 1 of a key is the eager warm-up, call 2 captures and replays, calls 3 and 4
only replay.  A replay repeats the same kernels in fixed-order reductions: every comparison is `torch.equal`, no tolerance anywhere."""
import random

import numpy as np
import pytest
import torch

import diffusion_objective_ref as oref
import golden_cases as gc
from oracle import config
from test_train_graph_gpu import _batch, _eager_step, _embed, _same_optimizer, _same_state_dict, _twin

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _grouped_twin(dev, cdt=torch.float32, ckpt=False, lr=1e-3):
    """the tiny GeoWizard UNet under GeoWizard's own optimizer: two parameter groups, the class embedding at ten times the rate"""
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    unet = UNet2DConditionModel(**config.TINY_GEOWIZARD_UNET)
    unet.load_state_dict(gc.tiny_geo_sd())
    unet = unet.to(dev).train()
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(gc.tiny_vae_sd())
    vae = vae.to(dev).eval()
    vae.requires_grad_(False)
    if cdt != torch.float32:
        unet.set_compute_dtype(cdt)
        vae = vae.to(cdt)
    if ckpt:
        unet.enable_gradient_checkpointing()
        vae.enable_gradient_checkpointing()
    opt = training.GroupedFlatAdamW(training.geowizard_param_groups(unet, lr), betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=1.0)
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["params"] and opt.param_groups[1]["lr"] == 10 * lr
    return unet, vae, opt


def _diffusion_batch(seed, dev):
    """`_batch` with the diffusion objective's fields: a 3-channel `depth`, and a mask that leaves whole latent cells valid (a 5 % random mask leaves none)"""
    batch = _batch(seed, dev)[0]
    batch["depth"] = batch["metric"].repeat(1, 3, 1, 1)
    batch["val_mask"] = oref.objective_mask().to(dev)
    return batch


def _host_streams():
    return random.getstate(), np.random.get_state()


def _restore(streams):
    random.setstate(streams[0])
    np.random.set_state(streams[1])


def _same_streams(a, b):
    assert a[0] == b[0], "Python's random ended elsewhere"
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:], "numpy's global stream ended elsewhere"


def _drive(dev, what, eager, captured, step, eager_loss, batch_of, gens=None, emas=None, geo=True, steps=4, acc=2, spoil=None):
    """the common scheme.  eager / captured: (unet, vae, optimizer); eager_loss(i, batch, embed) the eager twin's micro-step loss; gens / emas: (eager's, captured's).
    spoil: the step whose first micro-batch gets a NaN (the guard skips that update).  -> the losses of the captured twin"""
    from diffusion_e2e_ft_amd import training
    (eu, ev, eo), (cu, cv, co) = eager, captured
    scheds = [torch.optim.lr_scheduler.LambdaLR(o, training.IterExponential(total_iter_length=6, final_ratio=0.01)) for o in (eo, co)]
    losses, lrs = [], []
    for s in range(steps):
        batches = [batch_of(300 + 10 * s + i) for i in range(acc)]
        if spoil == s:
            batches[0]["rgb"][1, 0, 5, 7] = float("nan")
        embeds = [_embed(400 + 10 * s + i) for i in range(acc)] if geo else [None] * acc
        lr_scale = 1.0 if s != 2 else 0.5
        before = _host_streams()
        want = _eager_step(eu, ev, eo, batches, lambda i, b: eager_loss(i, b, embeds[i]), lr_scale)
        if emas is not None:
            emas[0].step(eo.params)
        after = _host_streams()
        _restore(before)
        got = step(batches, lr_scale, imgs_embed=embeds) if geo else step(batches, lr_scale)
        _same_streams(_host_streams(), after)
        if gens is not None:
            assert gens[0].draw == gens[1].draw, (what, s, gens[0].draw, gens[1].draw)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (what, s, got.item(), want.item())       # (bit patterns: equal also if both are NaN)
        assert spoil == s or bool(torch.isfinite(want).all()), (what, s)
        _same_optimizer(co, eo, (what, s))
        _same_state_dict(co.state_dict(), eo.state_dict())
        assert all(p.grad is None for p in co.params) and not any(co._claimed)
        if emas is not None:
            assert torch.equal(emas[1]._shadow_flat, emas[0]._shadow_flat), (what, s)
            assert emas[1].optimization_step == emas[0].optimization_step == s + 1 and emas[1].cur_decay_value == emas[0].cur_decay_value, (what, s)
        losses.append(got.item())
        lrs.append(eo.param_groups[0]["lr"])
        for sc in scheds:
            sc.step()
    ent, = step._entries.values()
    assert ent["graphs"] is not None and ent["graphs"]["later"] is not None
    assert len(set(lrs)) == steps
    return losses


# ---- (a) E2E-FT depth, noise_type="pyramid" ------------------------------------------------------------------------------------------------------------------
def test_pyramid_e2e_ft_steps_equal_eager_steps(dev):
    from diffusion_e2e_ft_amd import noise, training
    eager, captured = _twin(dev), _twin(dev)
    egen, cgen = noise.DeviceNoise(7), noise.DeviceNoise(7)
    text = _batch(0, dev)[1]
    step = training.CapturedTrainStepAt(*captured, text, "depth", noise_type="pyramid", generator=cgen, accumulation=2)
    random.seed(4)          # level 1 of the eight draws at 8 x 8 latents: 3, 3, 2, 2, 3, 2, 3, 2 rows (checked on the host)
    tables = []

    def loss(i, b, _):
        st = random.getstate()
        tables.append(tuple(noise.pyramid_level_sizes(8, 8)))      # what this micro-step is about to draw (the stream is put back)
        random.setstate(st)
        return training.e2e_ft_loss(eager[0], eager[1], b, text, "depth", noise_type="pyramid", generator=egen)

    losses = _drive(dev, "pyramid", eager, captured, step, loss, lambda seed: _batch(seed, dev)[0], gens=(egen, cgen), geo=False)
    assert egen.draw == 8 and len(set(losses)) == 4
    # (8 x 8 latents always give three levels here — 8 x 8, then 2 .. 4, then 1 — so it is the sizes that vary, not the count; case (d) varies the count)
    assert len(tables) == 8 and all(len(t) == 3 for t in tables) and len(set(tables[4:])) >= 2, tables          # (also among the pure replays)


# ---- (b) GeoWizard E2E-FT, "geowizard_pyramid" -----------------------------------------------------------------------------------------------------------------
def test_geowizard_pyramid_e2e_ft_steps_equal_eager_steps(dev):
    from diffusion_e2e_ft_amd import noise, training
    eager, captured = _twin(dev, geo=True), _twin(dev, geo=True)
    egen, cgen = noise.DeviceNoise(11), noise.DeviceNoise(11)
    step = training.CapturedTrainStepAt.geowizard(*captured, "indoor", 0.5, 1.0, noise_type="geowizard_pyramid", generator=cgen, accumulation=2)
    np.random.seed(1)

    def loss(i, b, e):
        return training.geowizard_e2e_ft_loss(eager[0], eager[1], b, e, "indoor", 0.5, 1.0, noise_type="geowizard_pyramid", generator=egen)

    _drive(dev, "geowizard_pyramid", eager, captured, step, loss, lambda seed: _batch(seed, dev)[0], gens=(egen, cgen))
    assert egen.draw == 8


# ---- (c) the diffusion objective, "gaussian", epsilon --------------------------------------------------------------------------------------------------------------
def test_diffusion_objective_steps_equal_eager_steps(dev):
    from diffusion_e2e_ft_amd import noise, training
    from diffusion_e2e_ft_amd.scheduler import DDPMScheduler
    eager, captured = _twin(dev, geo=True), _twin(dev, geo=True)
    egen, cgen = noise.DeviceNoise(13), noise.DeviceNoise(13)
    sched = DDPMScheduler()
    step = training.CapturedTrainStepAt.diffusion(*captured, "indoor", sched, "epsilon", "gaussian", generator=cgen, accumulation=2)

    def loss(i, b, e):
        return training.geowizard_diffusion_loss(eager[0], eager[1], b, e, "indoor", sched, "gaussian", egen, timesteps=egen, prediction_type="epsilon")

    losses = _drive(dev, "diffusion", eager, captured, step, loss, lambda seed: _diffusion_batch(seed, dev), gens=(egen, cgen))
    assert egen.draw == 16 and all(v > 0 for v in losses)                # two draws per micro-step; a selected cell in every batch


# ---- (d), (e) GeoWizard's default step -----------------------------------------------------------------------------------------------------------------------------
def _default_step(dev, cdt, ckpt, spoil=None):
    from diffusion_e2e_ft_amd import noise, training
    from diffusion_e2e_ft_amd.scheduler import DDPMScheduler
    eager, captured = _grouped_twin(dev, cdt, ckpt), _grouped_twin(dev, cdt, ckpt)
    egen, cgen = noise.DeviceNoise(17), noise.DeviceNoise(17)
    emas = [training.EMAModel(o.params, decay=0.999) for o in (eager[2], captured[2])]
    assert all(e._shadow_flat is not None for e in emas)
    sched = DDPMScheduler()
    step = training.CapturedTrainStepAt.diffusion(*captured, "indoor", sched, "v_prediction", "geowizard_pyramid", generator=cgen, accumulation=2, ema=emas[1])
    np.random.seed(1)
    counts = []

    def loss(i, b, e):
        st = np.random.get_state()
        counts.append(len(noise.geowizard_pyramid_level_sizes(8, 8)))      # what this micro-step is about to draw (the stream is put back)
        np.random.set_state(st)
        return training.geowizard_diffusion_loss(eager[0], eager[1], b, e, "indoor", sched, "geowizard_pyramid", egen, timesteps=egen,
                                                 prediction_type="v_prediction")

    losses = _drive(dev, "default", eager, captured, step, loss, lambda seed: _diffusion_batch(seed, dev), gens=(egen, cgen), emas=emas, spoil=spoil)
    assert egen.draw == 16
    return eager, captured, emas, counts, losses


def test_geowizard_default_step_equals_eager_steps(dev):
    """diffusion objective, geowizard_pyramid noise, v_prediction, two parameter groups, EMA.  Under np.random.seed(1) the eight size draws at 8 x 8 latents hold
    4, 4, 3, 3, 3, 4, 3, 5 levels (checked on the host), so the captured graphs are replayed over tables of different level counts."""
    eager, captured, emas, counts, losses = _default_step(dev, torch.float32, False)
    assert counts == [4, 4, 3, 3, 3, 4, 3, 5] and len(set(counts)) >= 2
    assert all(v > 0 for v in losses) and captured[2].step_count == 4 and captured[2].skipped_steps() == 0
    assert not torch.equal(emas[1]._shadow_flat, captured[2].flat_param)          # a shadow that trails the parameters, not a copy of them


def test_geowizard_default_step_bf16_recompute_equals_eager_steps(dev):
    _, captured, _, counts, _ = _default_step(dev, BF16, True)
    assert len(set(counts)) >= 2 and captured[2].step_count == 4


# ---- (f) the EMA after a skipped step -------------------------------------------------------------------------------------------------------------------------------
def test_the_ema_steps_after_a_skipped_optimizer_step(dev):
    """a NaN in step 2 (a replayed one): the guard skips the update on the device, the EMA launch — the update graph's last node — still runs, as the eager pair
    `optimizer.step(); ema.step()` does"""
    eager, captured, emas, _, losses = _default_step(dev, torch.float32, False, spoil=2)
    assert captured[2].skipped_steps() == eager[2].skipped_steps() == 1 and captured[2].step_count == eager[2].step_count == 3
    assert emas[1].optimization_step == 4


# ---- (g) refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_new_class_come_before_any_entry(dev):
    from diffusion_e2e_ft_amd import noise, training
    cu, cv, co = _twin(dev, geo=True)
    gen = noise.DeviceNoise(1)
    At = training.CapturedTrainStepAt
    with pytest.raises(ValueError, match="t / 1000"):
        At.geowizard(cu, cv, co, noise_type="pyramid", generator=gen)
    with pytest.raises(ValueError, match="t / 1000"):
        At.diffusion(cu, cv, co, noise_type="pyramid", generator=gen)
    with pytest.raises(ValueError, match="Unknown noise type"):
        At(cu, cv, co, torch.zeros(1, 2, 96), "depth", noise_type="geowizard_pyramid", generator=gen)
    with pytest.raises(TypeError, match="DeviceNoise"):
        At.diffusion(cu, cv, co, noise_type="zeros")                             # the timesteps need a generator even without noise
    with pytest.raises(TypeError, match="DeviceNoise"):
        At.geowizard(cu, cv, co, noise_type="geowizard_pyramid", generator=torch.Generator())
    with pytest.raises(TypeError, match="DeviceNoise"):
        At.diffusion(cu, cv, co, generator=noise.DrawAt(1, torch.zeros(1, dtype=torch.int64, device=dev)))
    with pytest.raises(ValueError, match="prediction type"):
        At.diffusion(cu, cv, co, prediction_type="sample", generator=gen)
    with pytest.raises(NotImplementedError, match="gather_loss"):
        At.diffusion(cu, cv, co, generator=gen, gather_loss=True)
    with pytest.raises(ValueError, match="loss must be"):
        At(cu, cv, co, None, loss="perceptual")
    loose = training.EMAModel([p.detach().clone().requires_grad_(True) for p in co.params])      # a per-tensor shadow, not over the flat buffer
    with pytest.raises(NotImplementedError, match="flat one-launch form"):
        At.diffusion(cu, cv, co, generator=gen, ema=loose)
    with pytest.raises(TypeError, match="EMAModel"):
        At.diffusion(cu, cv, co, generator=gen, ema=object())
    ou, ov, oo = _twin(dev, geo=True)
    with pytest.raises(NotImplementedError, match="THIS optimizer"):
        At.diffusion(cu, cv, co, generator=gen, ema=training.EMAModel(oo.params))                 # flat, but over another optimizer's buffer
    step = At.diffusion(cu, cv, co, generator=gen, accumulation=2, ema=training.EMAModel(co.params))
    batch = _diffusion_batch(3, dev)
    with pytest.raises(ValueError, match="accumulation is 2"):
        step([batch], imgs_embed=[_embed(1)])
    with pytest.raises(ValueError, match="imgs_embed"):
        step([batch, batch])
    assert not step._entries and gen.draw == 0 and step.ema.optimization_step == 0
    co.world = 2
    try:
        with pytest.raises(NotImplementedError, match="world size 2"):
            At.diffusion(cu, cv, co, generator=gen)
        with pytest.raises(NotImplementedError, match="world size 2"):
            step([batch, batch], imgs_embed=[_embed(1), _embed(2)])
        assert not step._entries
    finally:
        co.world = 1
    # and the base class refuses what it refused
    with pytest.raises(ValueError, match="host draws"):
        training.CapturedTrainStep(cu, cv, co, torch.zeros(1, 2, 96), "depth", noise_type="pyramid", generator=gen)
    with pytest.raises(NotImplementedError, match="diffusion"):
        training.CapturedTrainStep(cu, cv, co, None, loss="diffusion")
    with pytest.raises(NotImplementedError, match="EMA"):
        training.CapturedTrainStep(cu, cv, co, torch.zeros(1, 2, 96), "depth", ema=training.EMAModel(co.params))
