"""`training.CapturedTrainStep`: the optimizer step of `train_step` replayed from hipGraphs — first / later micro-step and update graphs over
one pool, static input buffers, lr and grad_scale read on the device (`e2eft_adamw_step_guarded_at`), Gaussian noise redrawn through `noise.randn_at`.

Two identical model / optimizer twins on the tiny synthetic models, 64 x 64 micro-batches of 2 unless stated; one twin steps eagerly, the other through the
captured step.  Call 1 of a key is the eager warm-up, call 2 captures and replays, later calls only replay.  A replay issues the same kernels on the same data in
the same order and every reduction of the library has a fixed order, so every comparison is `torch.equal`: no tolerance anywhere."""
import ctypes
import gc as _pygc

import pytest
import torch

import golden_cases as gc
from oracle import config

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _twin(dev, cdt=torch.float32, ckpt=False, geo=False, lr=1e-3):
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    unet = UNet2DConditionModel(**(config.TINY_GEOWIZARD_UNET if geo else config.TINY_UNET))
    unet.load_state_dict(gc.tiny_geo_sd() if geo else gc.tiny_unet_sd())
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
    return unet, vae, training.FlatAdamW(unet.parameters(), lr=lr, max_grad_norm=1.0)


def _batch(seed, dev, B=2, H=64, W=64, on_device=True):
    batch, text = gc.train_batch(seed, B=B, H=H, W=W)
    if on_device:
        batch = {k: v.to(dev) for k, v in batch.items()}
    return batch, text


def _embed(seed):
    return 0.5 * torch.randn(2, 1, config.TINY_GEOWIZARD_UNET["cross_attention_dim"], generator=torch.Generator().manual_seed(seed))


def _eager_step(unet, vae, opt, batches, loss_of, lr_scale=1.0):
    """`train_step` with the loss as an argument (the GeoWizard loss, a noise type): its loop, line for line"""
    n, total = len(batches), None
    for i, batch in enumerate(batches):
        opt.sync_grads = i == n - 1
        loss = loss_of(i, batch)
        (loss / n).backward()
        total = loss.detach() if total is None else total + loss.detach()
    opt.step(lr_scale=lr_scale)
    opt.zero_grad()
    return total / n


def _same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"] and a["flat_adamw"] == b["flat_adamw"] and a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a["state"][k][name], b["state"][k][name]), (k, name)


def _same_optimizer(a, b, what):
    for name in ("flat_param", "exp_avg", "exp_avg_sq", "_steps"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)


# ---- 2. captured equals eager ------------------------------------------------------------------------------------------------------------------------
CASES = [("fp32_depth", torch.float32, "depth", False, False, 2), ("bf16_normals", BF16, "normals", False, False, 2),
         ("fp32_depth_recompute", torch.float32, "depth", True, False, 2), ("geowizard", torch.float32, None, False, True, 2),
         ("fp32_depth_accumulation1", torch.float32, "depth", False, False, 1)]


@pytest.mark.parametrize("what,cdt,modality,ckpt,geo,acc", CASES, ids=[c[0] for c in CASES])
def test_captured_steps_equal_eager_steps(dev, what, cdt, modality, ckpt, geo, acc):
    """4 optimizer steps, a different micro-batch every micro-step, a LambdaLR that changes lr after every step: losses, parameters, both moments, the device
    step words and `state_dict()` of the captured twin equal the eager twin's after every step"""
    from diffusion_e2e_ft_amd import training
    eu, ev, eo = _twin(dev, cdt, ckpt, geo)
    cu, cv, co = _twin(dev, cdt, ckpt, geo)
    scheds = [torch.optim.lr_scheduler.LambdaLR(o, training.IterExponential(total_iter_length=6, final_ratio=0.01)) for o in (eo, co)]
    text = _batch(0, dev)[1]
    if geo:
        step = training.CapturedTrainStep.geowizard(cu, cv, co, "indoor", 0.5, 1.0, accumulation=acc)
    else:
        step = training.CapturedTrainStep(cu, cv, co, text, modality, accumulation=acc)
    lrs = []
    for s in range(4):
        # host tensors on odd steps, device tensors on even ones: the static buffers take both
        batches = [_batch(100 + 10 * s + i, dev, on_device=s % 2 == 0)[0] for i in range(acc)]
        embeds = [_embed(200 + 10 * s + i) for i in range(acc)]
        lr_scale = 1.0 if s != 2 else 0.5
        if geo:
            want = _eager_step(eu, ev, eo, batches, lambda i, b: training.geowizard_e2e_ft_loss(eu, ev, b, embeds[i], "indoor", 0.5, 1.0), lr_scale)
            got = step(batches, lr_scale, imgs_embed=embeds)
        else:
            want = training.train_step(eu, ev, eo, batches, text, modality, lr_scale=lr_scale)
            got = step(batches, lr_scale)
        assert torch.isfinite(want).all() and torch.equal(got, want), (what, s, got.item(), want.item())
        _same_optimizer(co, eo, (what, s))
        assert all(p.grad is None for p in co.params) and not any(co._claimed)
        lrs.append(eo.param_groups[0]["lr"])
        for sc in scheds:
            sc.step()
    ent, = step._entries.values()
    assert ent["graphs"] is not None and (ent["graphs"]["later"] is None) == (acc == 1)
    assert len(set(lrs)) == 4 and eo.step_count == 4 and co.step_count == 4 and co.skipped_steps() == 0
    _same_state_dict(co.state_dict(), eo.state_dict())


# ---- 3. Gaussian noise ---------------------------------------------------------------------------------------------------------------------------------
def test_gaussian_noise_is_redrawn_by_every_replay(dev):
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    eu, ev, eo = _twin(dev)
    cu, cv, co = _twin(dev)
    egen, cgen = DeviceNoise(7), DeviceNoise(7)
    batch, text = _batch(41, dev)
    step = training.CapturedTrainStep(cu, cv, co, text, "depth", noise_type="gaussian", generator=cgen, accumulation=2)
    losses = []
    for s in range(3):
        want = _eager_step(eu, ev, eo, [batch, batch], lambda i, b: training.e2e_ft_loss(eu, ev, b, text, "depth", noise_type="gaussian", generator=egen))
        got = step([batch, batch])
        assert torch.equal(got, want), (s, got.item(), want.item())
        _same_optimizer(co, eo, s)
        losses.append(got.item())
    assert losses[1] != losses[2]                 # the same batch, replayed twice: only the noise (and the step before) can tell them apart
    assert cgen.draw == egen.draw == 6


# ---- 4. a non-finite step ------------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_step_is_skipped_under_replay(dev):
    from diffusion_e2e_ft_amd import training
    eu, ev, eo = _twin(dev)
    cu, cv, co = _twin(dev)
    text = _batch(0, dev)[1]
    step = training.CapturedTrainStep(cu, cv, co, text, "depth", accumulation=1)
    for s in range(4):
        batch = _batch(60 + s, dev)[0]
        if s == 2:
            batch["rgb"][1, 0, 5, 7] = float("nan")
        before = co.flat_param.clone()
        want = training.train_step(eu, ev, eo, [batch], text, "depth")
        got = step([batch])
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (s, got.item(), want.item())      # (bit patterns: equal also if both were NaN)
        _same_optimizer(co, eo, s)
        assert torch.equal(co.flat_param, before) == (s == 2), s
    assert co.skipped_steps() == eo.skipped_steps() == 1 and co.step_count == eo.step_count == 3


# ---- 5. an eager forward between replays sees the new weights ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdt", [torch.float32, BF16], ids=["fp32", "bf16"])
def test_an_eager_forward_between_replays_reads_current_weights(dev, cdt):
    from diffusion_e2e_ft_amd import training
    eu, ev, eo = _twin(dev, cdt)
    cu, cv, co = _twin(dev, cdt)
    text = _batch(0, dev)[1]
    val = _batch(77, dev)[0]
    step = training.CapturedTrainStep(cu, cv, co, text, "depth", accumulation=2)
    for s in range(4):
        batches = [_batch(80 + 2 * s + i, dev)[0] for i in range(2)]
        assert torch.equal(step(batches), training.train_step(eu, ev, eo, batches, text, "depth")), s
        if s >= 1:          # (after the capturing step and after both pure replays)
            with torch.no_grad():
                got, want = training.e2e_ft_loss(cu, cv, val, text, "depth"), training.e2e_ft_loss(eu, ev, val, text, "depth")
            assert torch.equal(got, want), (s, got.item(), want.item())
    _same_optimizer(co, eo, "end")


# ---- 6. a replayed step issues no library launch from the host -----------------------------------------------------------------------------------------
COUNTERS = ("e2eft_debug_patch_launches", "e2eft_debug_persistent_launches", "e2eft_debug_thin_launches")


def _counts():
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    out = []
    for n in COUNTERS:
        fn = getattr(lib, n)
        fn.restype = ctypes.c_long
        out.append(fn())
    return out + [_lib.CALLS[0]]      # (+ every library call the host layer made)


def test_a_replayed_step_issues_no_library_launch_from_the_host(dev):
    """128 x 128 here: at 64 x 64 the tiny models reach none of the three counted kernels (tests/test_multistep_graph_gpu.py), and a zero that cannot be anything
    else shows nothing — so the same test asks the eager step for a non-zero count"""
    from diffusion_e2e_ft_amd import training
    cu, cv, co = _twin(dev)
    batches = [_batch(90 + i, dev, H=128, W=128)[0] for i in range(2)]
    text = _batch(0, dev)[1]
    step = training.CapturedTrainStep(cu, cv, co, text, "depth", accumulation=2)
    step(batches)
    step(batches)               # captures
    torch.cuda.synchronize()
    c0 = _counts()
    loss = step(batches)
    torch.cuda.synchronize()
    assert [b - a for a, b in zip(c0, _counts())] == [0, 0, 0, 0]
    assert torch.isfinite(loss).all()
    c0 = _counts()
    training.train_step(cu, cv, co, batches, text, "depth")
    torch.cuda.synchronize()
    delta = [b - a for a, b in zip(c0, _counts())]
    assert sum(delta[:3]) > 0 and delta[3] > 0, delta


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_capture(dev):
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    cu, cv, co = _twin(dev)
    batch, text = _batch(3, dev)
    for nt in ("pyramid", "geowizard_pyramid"):
        with pytest.raises(ValueError, match="host draws"):
            training.CapturedTrainStep(cu, cv, co, text, "depth", noise_type=nt, generator=DeviceNoise(1))
    with pytest.raises(TypeError, match="DeviceNoise"):
        training.CapturedTrainStep(cu, cv, co, text, "depth", noise_type="gaussian", generator=torch.Generator())
    with pytest.raises(NotImplementedError, match="gather_loss"):
        training.CapturedTrainStep(cu, cv, co, text, "depth", gather_loss=True)
    with pytest.raises(NotImplementedError, match="EMA"):
        training.CapturedTrainStep(cu, cv, co, text, "depth", ema=object())
    with pytest.raises(NotImplementedError, match="diffusion"):
        training.CapturedTrainStep(cu, cv, co, text, loss="diffusion")
    step = training.CapturedTrainStep(cu, cv, co, text, "depth", accumulation=2)
    with pytest.raises(ValueError, match="accumulation is 2"):
        step([batch])
    assert not step._entries
    co.world = 2                # a second rank, as far as the step can tell
    try:
        with pytest.raises(NotImplementedError, match="world size 2"):
            training.CapturedTrainStep(cu, cv, co, text, "depth")
        with pytest.raises(NotImplementedError, match="world size 2"):
            step([batch, batch])
        assert not step._entries
    finally:
        co.world = 1


# ---- 8. cache hygiene ----------------------------------------------------------------------------------------------------------------------------------
def test_a_second_shape_is_a_second_entry_and_dropping_the_step_frees_its_graphs(dev):
    from diffusion_e2e_ft_amd import training
    eu, ev, eo = _twin(dev)
    cu, cv, co = _twin(dev)
    text = _batch(0, dev)[1]
    step = training.CapturedTrainStep(cu, cv, co, text, "depth", accumulation=1)
    shapes = {"a": dict(B=2, H=64, W=64), "b": dict(B=1, H=64, W=72)}
    for s, which in enumerate("aabbabab"):          # each key: eager, capture, then replays interleaved with the other key's
        batch = _batch(120 + s, dev, **shapes[which])[0]
        assert torch.equal(step([batch]), training.train_step(eu, ev, eo, [batch], text, "depth")), (s, which)
        _same_optimizer(co, eo, (s, which))
    assert len(step._entries) == 2 and all(e["graphs"] is not None for e in step._entries.values())
    # no cycle: dropping the last reference frees the step, its entries and their graphs at once, collector off (a graph destroyed by the cyclic collector
    # inside a later capture aborts the process, tests/test_multistep_graph_gpu.py)
    import weakref
    ent = next(iter(step._entries.values()))
    refs = [weakref.ref(step), weakref.ref(ent["total"]), weakref.ref(ent["batch"]["rgb"])]      # (the entry's buffers: freed with the entry and its graphs)
    del ent
    _pygc.collect()
    _pygc.disable()
    try:
        del step
        assert all(r() is None for r in refs)
    finally:
        _pygc.enable()
    # and the models step on eagerly afterwards
    batch = _batch(140, dev)[0]
    assert torch.equal(training.train_step(cu, cv, co, [batch], text, "depth"), training.train_step(eu, ev, eo, [batch], text, "depth"))
    _same_optimizer(co, eo, "after")
