"""Multi-step inference through `_LatentPipeline._denoise`: head / step / tail hipGraphs over static buffers, the DDIM update fused into the step
graph (`ops.ddim_step_`), Gaussian noise a captured graph redraws (`ops.randn_fill_at_`), one VAE encode per ensemble batch.

Tiny synthetic models, 64x64 images (8x8 latents), fp32 unless stated.  Three kinds of statement:
  exact     captured == the same launches issued eagerly (`captured=False`), bit for bit; graphs on == graphs off where `_denoise` must not be taken;
  measured  the fused loop against the host-driven loop of `single_infer` with graphs off (the path this work leaves unchanged).  The two differ only by the rounding
            order of the update (one fused fp32 expression from float64-derived coefficients, against half a dozen torch operations in the storage dtype), carried
            through the UNet: not derivable, so the bars are 4x the values measured on an MI355X (the convention of tests/test_noise_gpu.py), listed at FUSED_BARS;
  counted   a warmed captured call issues no library launch from the host."""
import ctypes
import functools
import random

import pytest
import torch

import golden_cases as gc
from oracle import config, synth

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _models(kind, dtype, dev):
    """(unet, vae[, clip tower]) of one kind / dtype on the device: built once, shared by the tests, never modified"""
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    unet = UNet2DConditionModel(**(config.TINY_UNET if kind == "marigold" else config.TINY_GEOWIZARD_UNET))
    unet.load_state_dict(gc.tiny_unet_sd() if kind == "marigold" else gc.tiny_geo_sd())
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(gc.tiny_vae_sd())
    out = [unet.to(dev, dtype).eval(), vae.to(dev, dtype).eval()]
    if kind == "geowizard":
        from diffusion_e2e_ft_amd.clip import CLIPVisionModelWithProjection
        from test_clip_cpu import TINY, tiny_clip_sd
        cfg = dict(TINY, projection_dim=gc.geo_pipe_inputs()[1].shape[-1])
        enc = CLIPVisionModelWithProjection(**cfg)
        enc.load_state_dict(tiny_clip_sd(cfg=cfg))
        out.append(enc.to(dev, dtype).eval())
    return tuple(out)


def _marigold(dev, dtype=torch.float32, graphs=False):
    from diffusion_e2e_ft_amd.pipeline import MarigoldPipeline
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    unet, vae = _models("marigold", dtype, dev)
    pipe = MarigoldPipeline(unet, vae, DDIMScheduler())
    pipe.empty_text_embed = synth.synth_inputs(1, 64, 64, 2, 128, seed=3)[1][:1].to(dev, dtype)
    return pipe.enable_hip_graphs(graphs)


def _geowizard(dev, dtype=torch.float32, graphs=False):
    from diffusion_e2e_ft_amd.pipeline import DepthNormalEstimationPipeline
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    unet, vae, enc = _models("geowizard", dtype, dev)
    return DepthNormalEstimationPipeline(unet, vae, DDIMScheduler(), image_encoder=enc).enable_hip_graphs(graphs)


def _rgb(batch, seed=3, hw=(64, 64)):
    return synth.synth_inputs(batch, hw[0], hw[1], 2, 128, seed=seed)[0]


def _tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(_tuple(a), _tuple(b)))


# ---- exact: the capture adds nothing and loses nothing -------------------------------------------------------------------------------------------------
def test_marigold_capture_is_exact(dev):
    """B = 2, 3 steps, gaussian from DeviceNoise(19), two consecutive calls: captured == eager launches on both; the calls differ (the replayed graph draws fresh
    noise); a fresh pipeline and generator reproduce both; `single_infer` with graphs on is that path"""
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    rgb = _rgb(2).to(dev)

    def two_calls(captured):
        pipe, gen = _marigold(dev, graphs=captured), DeviceNoise(19)
        return [pipe._denoise(rgb, 3, "gaussian", gen, captured=captured, normals=False) for _ in range(2)], gen

    cap, gen = two_calls(True)
    eag, _ = two_calls(False)
    again, _ = two_calls(True)
    assert gen.draw == 2
    for i in range(2):
        assert torch.isfinite(cap[i]).all() and tuple(cap[i].shape) == (2, 1, 64, 64)
        assert torch.equal(cap[i], eag[i]), i
        assert torch.equal(cap[i], again[i]), i
    assert not torch.equal(cap[0], cap[1])
    pipe, gen = _marigold(dev, graphs=True), DeviceNoise(19)
    assert torch.equal(pipe.single_infer(rgb, 3, noise="gaussian", generator=gen), cap[0])
    # eager and captured calls interleave on one generator: the host counter is the single source of truth
    off = _marigold(dev, graphs=False)
    assert torch.equal(off._denoise(rgb, 3, "gaussian", gen, captured=False, normals=False), cap[1])
    assert gen.draw == 2


def test_geowizard_capture_is_exact(dev):
    """B = 1, 2 steps, the CLIP embedding computed inside the head graph; in addition the captured Gaussian result == the captured result for the explicit latent
    `noise.randn_into` reads back for the same seed (the same noise in the depth and the normal row block, geowizard_pipeline.py:271)"""
    from diffusion_e2e_ft_amd import noise as N
    rgb = gc.geo_pipe_inputs()[0][:1].to(dev)
    assert tuple(rgb.shape[-2:]) == (64, 64)

    def two_calls(captured):
        pipe, gen = _geowizard(dev, graphs=captured), N.DeviceNoise(19)
        return [pipe._denoise(rgb, 2, "gaussian", gen, captured=captured, domain="indoor") for _ in range(2)]

    cap, eag, again = two_calls(True), two_calls(False), two_calls(True)
    for i in range(2):
        assert all(torch.isfinite(t).all() for t in cap[i])
        assert tuple(cap[i][0].shape) == (1, 1, 64, 64) and tuple(cap[i][1].shape) == (1, 3, 64, 64)
        assert _same(cap[i], eag[i]) and _same(cap[i], again[i]), i
    assert not torch.equal(cap[0][0], cap[1][0]) and not torch.equal(cap[0][1], cap[1][1])
    pipe, gen = _geowizard(dev, graphs=True), N.DeviceNoise(19)
    for i in range(2):
        latent = N.randn_into(torch.empty(1, 8, 8, 4, device=dev), gen).permute(0, 3, 1, 2)
        assert _same(pipe._denoise(rgb, 2, latent, captured=True, domain="indoor"), cap[i]), i
    assert _same(pipe.single_infer(rgb, 2, noise="gaussian", generator=N.DeviceNoise(19)), cap[0])


def test_another_seed_recaptures_the_entry_in_place(dev):
    """the seed is a launch argument of the head graph: a generator with another seed must not replay the old one's noise, and must not grow the cache"""
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    rgb = _rgb(2).to(dev)
    pipe, off = _marigold(dev, graphs=True), _marigold(dev, graphs=False)
    for seed in (19, 20, 19):
        got = pipe._denoise(rgb, 2, "gaussian", DeviceNoise(seed), normals=False)
        assert torch.equal(got, off._denoise(rgb, 2, "gaussian", DeviceNoise(seed), captured=False, normals=False)), seed
        assert len(pipe._graphs) == 1


def test_cache_entries_do_not_refer_back_to_the_pipeline(dev):
    """an entry that referred to its pipeline (a closure over `self`) would make pipeline -> cache -> entry -> pipeline a cycle: the graphs would then be destroyed
    whenever the cyclic collector runs, possibly inside a later stream capture.  Dropping the last reference must free the pipeline at once, collector off."""
    import gc
    import weakref
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    rgb = _rgb(2).to(dev)
    pipe = _marigold(dev, graphs=True)
    pipe._denoise(rgb, 2, "gaussian", DeviceNoise(3), normals=False)
    ref, entry = weakref.ref(pipe), weakref.ref(next(iter(pipe._graphs.values()))["xin"])      # (the entry's buffer: freed with the entry and its graphs)
    gc.collect()
    gc.disable()
    try:
        del pipe
        assert ref() is None and entry() is None
    finally:
        gc.enable()


# ---- counted ------------------------------------------------------------------------------------------------------------------------------------------
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


def test_replay_issues_no_library_launch_from_the_host(dev):
    """128 x 128 images here: at 64 x 64 no launch of the tiny models reaches one of the three counted kernels (measured: deltas 0, 0, 0 with graphs off), and a
    zero that cannot be anything else shows nothing.  `_lib.CALLS` counts every call into the library on top."""
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    rgb = _rgb(2, hw=(128, 128)).to(dev)
    pipe, gen = _marigold(dev, graphs=True), DeviceNoise(5)
    pipe.single_infer(rgb, 3, noise="gaussian", generator=gen)          # captures
    keys = set(pipe._graphs)
    assert len(keys) == 1
    c0 = _counts()
    out = pipe.single_infer(rgb, 3, noise="gaussian", generator=gen)
    torch.cuda.synchronize()
    assert [b - a for a, b in zip(c0, _counts())] == [0, 0, 0, 0]
    assert torch.isfinite(out).all()
    pipe.single_infer(rgb, 4, noise="gaussian", generator=gen)          # the key leaves the step count out
    assert set(pipe._graphs) == keys
    pipe.enable_hip_graphs(False)
    gen.draw = 1
    c0 = _counts()
    want = pipe.single_infer(rgb, 3, noise="gaussian", generator=gen)
    delta = [b - a for a, b in zip(c0, _counts())]
    assert sum(delta[:3]) > 0 and delta[3] > 0, delta
    assert want.shape == out.shape


# ---- measured: fused against the host-driven loop -----------------------------------------------------------------------------------------------------------
# max |fused - eager| / max |eager| on an MI355X, per output:        measured        bar = 4x
FUSED_BARS = {
    "marigold_fp32": 4.6e-6,          # 1.13e-6  (depth, B = 2, 3 steps)
    "geowizard_fp32": 9.7e-5,         # 2.42e-5  (the normals; the depth: 1.19e-6; B = 1, 2 steps)
    "call_ensemble3_fp32": 7.9e-6,    # 1.97e-6  (the ensembled depth of `__call__`, 3 members, 2 steps)
    "marigold_fp16": 5.9e-3,          # 1.46e-3  (the host-driven loop rounds every operation of the update to fp16, the fused one rounds once)
}


def _gap(fused, eager, what):
    gaps = []
    for f, e in zip(_tuple(fused), _tuple(eager)):
        f, e = torch.as_tensor(f).double(), torch.as_tensor(e).double()
        assert f.shape == e.shape and torch.isfinite(f).all()
        gaps.append(((f - e).abs().max() / e.abs().max()).item())
    print("fused vs eager %s: %s (bar %.3e)" % (what, " ".join("%.3e" % g for g in gaps), FUSED_BARS[what]))
    return max(gaps)


@pytest.mark.parametrize("what,dtype", [("marigold_fp32", torch.float32), ("marigold_fp16", torch.float16)])
def test_marigold_fused_against_eager_loop(dev, what, dtype):
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    rgb = _rgb(2).to(dev)
    fused = _marigold(dev, dtype, graphs=True).single_infer(rgb, 3, noise="gaussian", generator=DeviceNoise(19))
    eager = _marigold(dev, dtype, graphs=False).single_infer(rgb, 3, noise="gaussian", generator=DeviceNoise(19))
    assert _gap(fused, eager, what) <= FUSED_BARS[what]


def test_geowizard_fused_against_eager_loop(dev):
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    rgb = gc.geo_pipe_inputs()[0][:1].to(dev)
    fused = _geowizard(dev, graphs=True).single_infer(rgb, 2, noise="gaussian", generator=DeviceNoise(19))
    eager = _geowizard(dev, graphs=False).single_infer(rgb, 2, noise="gaussian", generator=DeviceNoise(19))
    assert _gap(fused, eager, "geowizard_fp32") <= FUSED_BARS["geowizard_fp32"]


def test_call_ensemble_fused_against_eager_loop(dev):
    """`__call__`, ensemble_size = 3, 2 steps: ONE encode broadcast into three rows against three stacked copies through the encoder, then the ensembling"""
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    img = ((_rgb(1)[0] + 1) * 127.5).round().clamp(0, 255).to(torch.uint8)
    kw = dict(denoising_steps=2, ensemble_size=3, processing_res=0, color_map=None, show_progress_bar=False, noise="gaussian")
    pipe = _marigold(dev, graphs=True)
    fused = pipe(img, generator=DeviceNoise(19), **kw)
    assert [k[2] for k in pipe._graphs] == [3] and [k[1][0] for k in pipe._graphs] == [1]      # one image encoded, three rows denoised
    eager = _marigold(dev, graphs=False)(img, generator=DeviceNoise(19), **kw)
    assert fused.depth_np.shape == (64, 64)
    assert _gap(fused.depth_np, eager.depth_np, "call_ensemble3_fp32") <= FUSED_BARS["call_ensemble3_fp32"]


# ---- what the ensemble's single encode rests on -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(64, 64), (72, 104)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_encoder_is_batch_invariant(dev, hw, dtype):
    pipe = _marigold(dev, dtype)
    x = _rgb(1, seed=11, hw=hw).to(dev, dtype)
    one = pipe.encode_rgb(x)[0]
    three = pipe.encode_rgb(torch.stack([x[0]] * 3))
    assert tuple(three.shape) == (3, 4, hw[0] // 8, hw[1] // 8)
    for r in range(3):
        assert torch.equal(three[r], one), (hw, dtype, r)


# ---- exact: what `_denoise` must not take -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["pyramid", "pyramid_host", "gaussian_torch"])
def test_host_driven_starts_are_unchanged_with_graphs_on(dev, noise):
    """"pyramid" (its level sizes are host draws per call) and a `torch.Generator` keep the host-driven loop: graphs on == graphs off under the same seeds"""
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    rgb = _rgb(2).to(dev)

    def run(graphs):
        pipe = _marigold(dev, graphs=graphs)
        random.seed(23)
        torch.manual_seed(29)
        if noise == "pyramid":
            out = pipe.single_infer(rgb, 2, noise="pyramid", generator=DeviceNoise(19))
        elif noise == "pyramid_host":
            out = pipe.single_infer(rgb, 2, noise="pyramid")
        else:
            out = pipe.single_infer(rgb, 2, noise="gaussian", generator=torch.Generator(device=dev).manual_seed(31))
        return out, pipe

    on, pipe = run(True)
    off, _ = run(False)
    assert torch.isfinite(on).all() and torch.equal(on, off)
    assert len(pipe._graphs) == 0
