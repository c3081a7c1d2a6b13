"""e2eft_pyramid_noise_weighted (the GeoWizard trainer's `pyramid_noise_like(x, timesteps)`, train_depth_normal.py:286-296) on the GPU against the float64
restatement tests/geowizard_pyramid_ref.py, its ties to the kernels that exist, and the two GeoWizard trainers with noise_type="geowizard_pyramid".

Error bar of the fp32 cases: computed here, per case — 4 x the largest absolute error of `geowizard_pyramid_ref.weighted_pyramid_fp32` (the same formula rounded
to fp32 step by step in numpy: an independent rounding) against the float64 evaluation of the same case.  The factor 4 covers the device's logf / sinf / cosf
being a few ulp from numpy's.  The measured figures stand in the docstring of test_weighted_pyramid_fp32 and in DESIGN.md §3.23a."""
import functools

import numpy as np
import pytest
import torch

import containment
import diffusion_objective_ref as oref
import geowizard_pyramid_ref as gref
import golden_cases as gc
from oracle import config

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
DRAW = 9
TEN_LEVELS = ((12, 10), (8, 7), (6, 5), (4, 6), (3, 3), (1, 5), (2, 2), (3, 1), (2, 3), (1, 1))      # full size first; (4,6) wider than (6,5); three with a dimension of 1
CASES = {
    "whole_pixel_strided": ((3, 4, 9, 12), ((9, 12), (4, 6), (2, 3), (1, 1)), (0, 999, 500), True),
    "scalar": ((2, 3, 5, 7), ((5, 7), (2, 3), (1, 1)), (1, 999), True),
    "ten_levels": ((4, 4, 12, 10), TEN_LEVELS, (0, 1, 500, 999), False),
}


@functools.lru_cache(maxsize=None)
def _ref64(shape, sizes, timesteps):
    return gref.weighted_pyramid(SEED, DRAW, shape, list(sizes), list(timesteps))          # float64 [B,C,H,W]; shared, never modified


@functools.lru_cache(maxsize=None)
def _fp32_error(shape, sizes, timesteps):
    lo = gref.weighted_pyramid_fp32(SEED, DRAW, shape, list(sizes), list(timesteps))
    return float(np.abs(lo.astype(np.float64) - _ref64(shape, sizes, timesteps).numpy()).max())


def _buffer(shape, dtype, dev, col0=None):
    """NHWC destination view [B,H,W,C] and the whole buffer: dense (col0 None), or channels col0:col0+C of an 8-channel sentinel-filled buffer"""
    B, C, H, W = shape
    if col0 is None:
        buf = torch.full((B, H, W, C), 7.0, dtype=dtype, device=dev)
        return buf, buf
    buf = torch.arange(B * H * W * 8, device=dev, dtype=torch.float32).reshape(B, H, W, 8).remainder(251.0).sub(125.0).to(dtype)
    return buf[..., col0:col0 + C], buf


def _t(timesteps, dev):
    return torch.tensor(timesteps, dtype=torch.int64, device=dev)


def _ordinal(t):
    """16-bit floats -> integers that count representable values in order (distance 1 = one ulp)"""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


# ---- 4. fp32 against the float64 restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_weighted_pyramid_fp32(dev, case):
    """Measured on an MI355X (device max abs error against float64 / error of the numpy fp32 evaluation / bar = 4 x that):
    whole_pixel_strided 5.2e-7 / 5.7e-7 / 2.3e-6,  scalar 3.6e-7 / 3.6e-7 / 1.4e-6,  ten_levels 1.1e-6 / 1.7e-6 / 6.9e-6."""
    from diffusion_e2e_ft_amd import ops
    shape, sizes, timesteps, strided = CASES[case]
    dst, buf = _buffer(shape, torch.float32, dev, 4 if strided else None)
    before = buf.clone()
    ops.pyramid_noise_weighted_(dst, SEED, DRAW, sizes, _t(timesteps, dev))
    got = dst.permute(0, 3, 1, 2).double().cpu()
    err = (got - _ref64(shape, sizes, timesteps)).abs().max().item()
    host = _fp32_error(shape, sizes, timesteps)
    print("weighted pyramid fp32 %s %s: max abs err %.3e; numpy fp32 evaluation %.3e; bar (4 x) %.3e" % (case, shape, err, host, 4 * host))
    assert 0.0 < host < 1e-5                    # the bar itself is an fp32 rounding error, not a defect-sized number
    assert err <= 4 * host, (err, host)
    assert abs(got.std().item() - 1.0) <= 1e-5
    if strided:
        C = shape[1]
        assert torch.equal(buf[..., :4], before[..., :4]) and torch.equal(buf[..., 4 + C:], before[..., 4 + C:])      # the other channels: bit-unchanged
    again, _ = _buffer(shape, torch.float32, dev, 4 if strided else None)
    assert torch.equal(ops.pyramid_noise_weighted_(again, SEED, DRAW, sizes, _t(timesteps, dev)), dst)               # bit-equal run to run
    assert not torch.equal(ops.pyramid_noise_weighted_(again, SEED, DRAW + 1, sizes, _t(timesteps, dev)), dst)


# ---- 5. ties to what exists ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_weight_one_is_the_unweighted_kernel_bit_for_bit(dev, case):
    from diffusion_e2e_ft_amd import ops
    shape, sizes, _, strided = CASES[case]
    a, _ = _buffer(shape, torch.float32, dev, 4 if strided else None)
    b, _ = _buffer(shape, torch.float32, dev, 4 if strided else None)
    ops.pyramid_noise_weighted_(a, SEED, DRAW, sizes, _t([1000] * shape[0], dev))          # tw == 1.0f
    ops.pyramid_noise_(b, SEED, DRAW, sizes)
    assert torch.equal(a, b)
    ops.pyramid_noise_weighted_(a, SEED, DRAW, sizes, _t([250] * shape[0], dev), timestep_div=250.0)
    assert torch.equal(a, b)
    ops.pyramid_noise_weighted_(a, SEED, DRAW, sizes, _t([999] * shape[0], dev))
    assert not torch.equal(a, b)


@pytest.mark.parametrize("case", sorted(CASES))
def test_weight_zero_is_the_base_grid_over_its_std(dev, case):
    """all timesteps 0: randn_fill_ of the same seed and draw (slot 0) divided by its unbiased std.  The reference side divides in float64 by the float64 std of the
    fp32 grid; the kernel rounds the std and the quotient to fp32: 2^-23 relative."""
    from diffusion_e2e_ft_amd import ops
    shape, sizes, _, _ = CASES[case]
    B, C, H, W = shape
    got = ops.pyramid_noise_weighted_(torch.empty((B, H, W, C), device=dev), SEED, DRAW, sizes, _t([0] * B, dev)).double().cpu()
    base = ops.randn_fill_(torch.empty((B, H, W, C), device=dev), SEED, DRAW, slot=0).double().cpu()
    want = base / base.std()
    rel = ((got - want).abs() / want.abs()).max().item()
    print("weight 0 %s: max relative error against randn_fill_ / std %.3e (bar 2^-23 = %.3e)" % (case, rel, 2.0 ** -23))
    assert rel <= 2.0 ** -23


# ---- 6. 16-bit strided, containment ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_weighted_pyramid_16bit_strided_and_contained(dev, dtype):
    from diffusion_e2e_ft_amd import ops
    shape, sizes, timesteps, _ = CASES["whole_pixel_strided"]
    B, C, H, W = shape
    want = _ref64(shape, sizes, timesteps).to(dtype)

    def run(fill):
        buffer, view = containment.guarded((B, H, W, 8), dtype, dev, fill)      # the 8-channel UNet input inside guard bands; the noise goes to channels 4:8
        ops.pyramid_noise_weighted_(view[..., 4:], SEED, DRAW, sizes, _t(timesteps, dev))
        kept = view[..., :4].contiguous().view(torch.uint8)
        assert bool((kept == fill).all()), "channels 0:4 were written"
        return {"noise": view[..., 4:].permute(0, 3, 1, 2).contiguous()}, [(buffer, view)]

    def check(name, t):
        assert int((_ordinal(t.cpu()) - _ordinal(want)).abs().max()) <= 1      # within one ulp of the rounded restatement

    containment.check_two_fills(run, check, what="pyramid_noise_weighted_ %s" % dtype)


def test_scalar_path_is_contained(dev):
    from diffusion_e2e_ft_amd import ops
    shape, sizes, timesteps, _ = CASES["scalar"]
    B, C, H, W = shape
    want = _ref64(shape, sizes, timesteps)
    bar = 4 * _fp32_error(shape, sizes, timesteps)

    def run(fill):
        buffer, view = containment.guarded((B, H, W, 8), torch.float32, dev, fill)
        ops.pyramid_noise_weighted_(view[..., 4:4 + C], SEED, DRAW, sizes, _t(timesteps, dev))
        for kept in (view[..., :4], view[..., 4 + C:]):
            assert bool((kept.contiguous().view(torch.uint8) == fill).all()), "a channel outside the slice was written"
        return {"noise": view[..., 4:4 + C].permute(0, 3, 1, 2).contiguous()}, [(buffer, view)]

    def check(name, t):
        assert (t.double().cpu() - want).abs().max().item() <= bar

    containment.check_two_fills(run, check, what="pyramid_noise_weighted_ scalar path")


# ---- 7. launch-geometry / layout independence ---------------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_layout_or_store_path(dev):
    """one logical tensor written dense (whole-pixel stores), into channels 4:8 of an 8-channel buffer (whole-pixel, strided) and into channels 1:5 (misaligned: the
    element-wise scale pass); and a tensor large enough that the first pass's threads loop (more than 1024 x 256 elements), dense against strided"""
    from diffusion_e2e_ft_amd import ops
    shape, sizes, timesteps, _ = CASES["ten_levels"]
    t = _t(timesteps, dev)
    outs = [ops.pyramid_noise_weighted_(_buffer(shape, torch.float32, dev, col0)[0], SEED, DRAW, sizes, t) for col0 in (None, 4, 1)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    big, big_sizes = (4, 4, 136, 132), ((136, 132), (51, 47), (9, 13), (1, 2))
    assert big[0] * big[1] * big[2] * big[3] > 1024 * 256
    outs = [ops.pyramid_noise_weighted_(_buffer(big, torch.float32, dev, col0)[0], SEED, DRAW, big_sizes, t) for col0 in (None, 4, 1)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert bool(torch.isfinite(outs[0]).all()) and abs(outs[0].double().std().item() - 1.0) <= 1e-5
    # rows differ by their weight only where a level enters: row 0 (t = 0) is its base grid over the common std
    base = ops.randn_fill_(torch.empty_like(outs[0]), SEED, DRAW, slot=0)
    ratio = (outs[0][0] / base[0]).double()
    assert float((ratio / ratio.flatten()[0] - 1).abs().max()) <= 2.0 ** -22


# ---- 8. timesteps are read on the device ----------------------------------------------------------------------------------------------------------------------------
def test_captured_call_reads_the_timesteps_at_replay(dev):
    from diffusion_e2e_ft_amd import ops
    shape, sizes, timesteps, _ = CASES["ten_levels"]
    B, C, H, W = shape
    t = _t(timesteps, dev)
    xin = torch.zeros((B, H, W, 8), device=dev)
    ops.pyramid_noise_weighted_(xin[..., 4:], SEED, DRAW, sizes, t)          # code objects loaded before the capture
    first = xin.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                            # one stream, no parallel branches
        ops.pyramid_noise_weighted_(xin[..., 4:], SEED, DRAW, sizes, t)
    t.copy_(torch.tensor([731, 0, 999, 17]))                                 # new contents, in place
    graph.replay()
    torch.cuda.synchronize()
    got = xin.clone()
    want = ops.pyramid_noise_weighted_(torch.zeros((B, H, W, 4), device=dev), SEED, DRAW, sizes, _t([731, 0, 999, 17], dev))
    assert torch.equal(got[..., 4:], want) and not torch.equal(got, first)
    assert bool((got[..., :4] == 0).all())


# ---- 9. the trainers ---------------------------------------------------------------------------------------------------------------------------------------------------
def _models(dev):
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    unet = UNet2DConditionModel(**config.TINY_GEOWIZARD_UNET)
    unet.load_state_dict(gc.tiny_geo_sd())
    unet = unet.to(dev).train()
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(gc.tiny_vae_sd())
    vae = vae.to(dev).eval()
    vae.requires_grad_(False)
    return unet, vae


def test_geowizard_diffusion_loss_with_the_weighted_pyramid(dev):
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.noise import DeviceNoise, geowizard_pyramid_noise_into, geowizard_pyramid_level_sizes
    unet, vae = _models(dev)
    batch, emb, timesteps, _ = oref.objective_inputs()
    kw = dict(timesteps=timesteps, prediction_type="epsilon", return_parts=True)
    runs = []
    with torch.no_grad():
        for _ in range(2):
            np.random.seed(5)
            gen = DeviceNoise(9)
            runs.append(training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_type="geowizard_pyramid", generator=gen, **kw))
            assert gen.draw == 1
        (l0, n0, tg0, xt0), (l1, n1, tg1, xt1) = runs
        assert torch.equal(l0, l1) and torch.equal(n0, n1) and torch.equal(tg0, tg1) and torch.equal(xt0, xt1)            # two runs are bit-equal
        # the explicit form: the same draw made by hand under the same numpy seed, generator and doubled timesteps
        np.random.seed(5)
        sizes = geowizard_pyramid_level_sizes(8, 8)
        np.random.seed(5)
        nz = geowizard_pyramid_noise_into(torch.empty((4, 8, 8, 4), device=dev), DeviceNoise(9), timesteps.to(dev).repeat(2))
        assert float(np.random.random()) == _next_random_after(5, 8, 8) and len(sizes) >= 2
        l2, n2, tg2, xt2 = training.geowizard_diffusion_loss(unet, vae, batch, emb, noise=nz.permute(0, 3, 1, 2), **kw)
        assert torch.equal(tg0, tg2) and torch.equal(xt0, xt2) and torch.equal(l0, l2) and torch.equal(n0, n2)
        assert torch.equal(tg0, nz.permute(0, 3, 1, 2))                      # the epsilon target IS the noise
        # rows 0 and 2 carry t = 0: their noise is the base grid over the common std; rows 1 and 3 (t = 731) hold the levels
        assert oref.TIMESTEPS == (0, 731)
        want = gref.weighted_pyramid(9, 0, (4, 4, 8, 8), sizes, [0, 731, 0, 731])
        assert (tg0.double().cpu() - want).abs().max().item() <= 1e-5
    loss = training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_type="geowizard_pyramid", generator=DeviceNoise(9), timesteps=timesteps,
                                             prediction_type="epsilon")
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in unet.parameters())
    with pytest.raises(TypeError, match="DeviceNoise"):
        training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_type="geowizard_pyramid", timesteps=timesteps)
    with pytest.raises(ValueError, match="t / 1000"):
        training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_type="pyramid", generator=DeviceNoise(9))
    # drawn timesteps (no `timesteps=`): runs, finite, and reproducible under torch's and numpy's seeds
    with torch.no_grad():
        outs = []
        for _ in range(2):
            torch.manual_seed(1234)
            np.random.seed(5)
            outs.append(training.geowizard_diffusion_loss(unet, vae, batch, emb, noise_type="geowizard_pyramid", generator=DeviceNoise(9)))
        assert torch.equal(outs[0], outs[1]) and bool(torch.isfinite(outs[0]))


def _next_random_after(seed, rows, cols):
    from diffusion_e2e_ft_amd.noise import geowizard_pyramid_level_sizes
    rng = np.random.RandomState(seed)
    geowizard_pyramid_level_sizes(rows, cols, rng=rng)
    return float(rng.random_sample())


def test_geowizard_e2e_ft_loss_with_the_weighted_pyramid(dev):
    from diffusion_e2e_ft_amd import training
    from diffusion_e2e_ft_amd.noise import DeviceNoise, geowizard_pyramid_noise_into
    unet, vae = _models(dev)
    batch, emb, _, _ = oref.objective_inputs()
    with torch.no_grad():
        runs = []
        for _ in range(2):
            np.random.seed(5)
            runs.append(training.geowizard_e2e_ft_loss(unet, vae, batch, emb, return_parts=True, noise_type="geowizard_pyramid", generator=DeviceNoise(9)))
        assert all(torch.equal(a, b) for a, b in zip(*runs))
        np.random.seed(5)
        nz = geowizard_pyramid_noise_into(torch.empty((4, 8, 8, 4), device=dev), DeviceNoise(9), torch.full((4,), 999, dtype=torch.int64, device=dev))
        explicit = training.geowizard_e2e_ft_loss(unet, vae, batch, emb, return_parts=True, noise=nz.permute(0, 3, 1, 2))
        assert all(torch.equal(a, b) for a, b in zip(runs[0], explicit))
        zeros = training.geowizard_e2e_ft_loss(unet, vae, batch, emb)
        assert zeros.item() != runs[0][0].item()
    np.random.seed(5)
    loss = training.geowizard_e2e_ft_loss(unet, vae, batch, emb, noise_type="geowizard_pyramid", generator=DeviceNoise(9))
    assert torch.equal(loss.detach(), runs[0][0])
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in unet.parameters())
    with pytest.raises(TypeError, match="DeviceNoise"):
        training.geowizard_e2e_ft_loss(unet, vae, batch, emb, noise_type="geowizard_pyramid")
    with pytest.raises(ValueError, match="t / 1000"):
        training.geowizard_e2e_ft_loss(unet, vae, batch, emb, noise_type="pyramid", generator=DeviceNoise(9))
