"""csrc/denoise.hip (`ops.ddim_step_`) and the capture-safe Gaussian fill (`ops.randn_fill_at_`) on the GPU.

ddim_step_: fp32 against a float64 evaluation with the float64 coefficient table; bit equality with `ops.latent_x0` (whose arithmetic it restates) in every dtype;
memory containment with the guard bands of tests/containment.py.  randn_fill_at_: bit equality with `randn_fill_` for the same draw.

The fp32 bar is derived, not measured: the kernel sees each coefficient rounded once to fp32 (2^-24 relative on its term) and rounds the fused result once
(2^-24 of |c_x x + c_v v| <= |c_x x| + |c_v v|):  |err| <= 2^-23 (|c_x x| + |c_v v|)."""
import functools

import pytest
import torch

import containment as cm

pytestmark = pytest.mark.gpu

BAR = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _table(n=3, prediction_type="v_prediction"):
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    return DDIMScheduler(prediction_type=prediction_type).step_coefficients_f64(n)      # float64 [n, 2]; shared, never modified


def _operands(shape, seed):
    g = torch.Generator().manual_seed(seed)
    B, C, H, W = shape
    return torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, C, generator=g)      # NHWC x, v (fp32 values)


def _views(kind, x, v, dtype, dev):
    """x as the kernel sees it -> (whole buffer, view): "ld8": channels 4:4+C of a [B,H,W,8] buffer (the UNet input; 16-byte aligned when C == 4);
    "odd": channels 1:1+C of a [B,H,W,9] buffer (odd element offset, ld no multiple of 4: element path); "dense": the tensor itself"""
    B, H, W, C = x.shape
    if kind == "dense":
        buf = x.to(dev, dtype).contiguous()
        return buf, buf
    width, c0 = (8, 4) if kind == "ld8" else (9, 1)
    buf = torch.arange(B * H * W * width, dtype=torch.float32).reshape(B, H, W, width).remainder(251.0).sub(125.0).to(dev, dtype)
    view = buf[..., c0:c0 + C]
    view.copy_(x.to(dev, dtype))
    return buf, view


# (shape NCHW, layout of x, row of the 3-step table): the whole-pixel path (c == 4, aligned), its block tail (35 pixels), the element path (c == 3; c == 4 at an
# odd element offset), and more items than 256 * the grid cap of 16384 blocks (the stride loop)
FP32_CASES = [((2, 4, 8, 8), "ld8", 0), ((1, 4, 5, 7), "ld8", 1), ((3, 3, 9, 12), "ld8", 2), ((2, 4, 5, 7), "odd", 0), ((1, 3, 1200, 1200), "dense", 1)]


@pytest.mark.parametrize("shape,layout,row", FP32_CASES)
def test_ddim_step_fp32_against_float64(dev, shape, layout, row):
    from diffusion_e2e_ft_amd import ops
    x, v = _operands(shape, seed=sum(shape) + row)
    tab = _table()
    coef = tab[row].to(torch.float32).to(dev)
    buf, view = _views(layout, x, v, torch.float32, dev)
    before = buf.clone()
    vd = v.to(dev)
    if shape[1] == 4 and layout == "ld8":
        assert view.data_ptr() % 16 == 0 and vd.data_ptr() % 16 == 0          # the whole-pixel path's condition
    if layout == "dense":
        assert x.numel() > 256 * 16384                                         # one element per item: every thread of the capped grid loops
    out = ops.ddim_step_(view, vd, coef)
    assert out is view
    c_x, c_v = tab[row, 0].item(), tab[row, 1].item()
    want = c_x * x.double() + c_v * v.double()
    scale = (c_x * x.double()).abs() + (c_v * v.double()).abs()
    ratio = ((view.cpu().double() - want).abs() / scale).max().item()
    print("ddim_step fp32 %s %s row %d: max |err| / (|c_x x| + |c_v v|) = %.3f * 2^-23" % (shape, layout, row, ratio / BAR))
    assert ratio <= BAR, ratio / BAR
    # channels outside the view keep their bits, v is not written
    if layout != "dense":
        c0 = 4 if layout == "ld8" else 1
        keep = torch.ones(buf.shape[-1], dtype=torch.bool)
        keep[c0:c0 + shape[1]] = False
        assert torch.equal(buf[..., keep.to(dev)], before[..., keep.to(dev)])
    assert torch.equal(vd.cpu(), v)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape,layout", [((2, 4, 8, 8), "ld8"), ((1, 4, 5, 7), "ld8"), ((3, 3, 9, 12), "ld8"), ((2, 4, 5, 7), "odd"), ((2, 8, 6, 6), "dense")])
def test_ddim_step_is_latent_x0_bit_for_bit(dev, dtype, shape, layout):
    """in place with coefficients from device memory == `ops.latent_x0` out of place with the same fp32 coefficients by value"""
    from diffusion_e2e_ft_amd import ops
    x, v = _operands(shape, seed=7 + sum(shape))
    for row in range(3):
        coef = _table()[row].to(torch.float32)
        _, view = _views(layout, x, v, dtype, dev)
        vd = v.to(dev, dtype)
        want = ops.latent_x0(view, vd, coef[0].item(), coef[1].item())
        ops.ddim_step_(view, vd, coef.to(dev))
        assert torch.equal(view, want), (dtype, shape, layout, row)
        assert torch.isfinite(view.float()).all() and not torch.equal(view.cpu().float(), x.to(dtype).float())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("shape,col0", [((2, 8, 8, 4), None), ((1, 5, 7, 4), None), ((3, 9, 12, 3), None), ((2, 5, 7, 4), "odd")])
def test_ddim_step_containment(dev, dtype, shape, col0):
    """x and v as interior views of guarded allocations: after the call every byte outside x's logical extent (channels in front of and behind the view, the rows
    before and after) still holds the fill, v's allocation is untouched, and the result does not depend on the fill"""
    from diffusion_e2e_ft_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    x, v = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    coef = _table()[0].to(torch.float32)
    unit = 16 // (4 if dtype == torch.float32 else 2)
    want = coef[0] * x.to(dtype).float() + coef[1] * v.to(dtype).float()
    bits = torch.int32 if dtype == torch.float32 else torch.int16      # (the 0xFF fill is a NaN: compare bits)

    def run(fill):
        xb, xv = cm.guarded(shape, dtype, dev, fill, data=x, col0=None if col0 is None else unit + 1)
        vb, vv = cm.guarded(shape, dtype, dev, fill, data=v)
        v_before = vb.clone()
        ops.ddim_step_(xv, vv, coef.to(dev))
        assert torch.equal(vb.view(bits), v_before.view(bits))
        return {"x": xv.clone()}, [(xb, xv), (vb, vv)]

    def check(name, t):
        tol = 2e-6 if dtype == torch.float32 else 2e-3
        assert (t.float().cpu() - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())

    cm.check_two_fills(run, check, what="ddim_step %s %s" % (dtype, shape))


DRAWS = [0, 1, 2 ** 31, 2 ** 32 - 1]
SEED = 0x5EED0123456789AB


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape,strided", [((2, 4, 8, 8), False), ((2, 4, 8, 8), True), ((2, 3, 5, 7), False), ((1, 4, 5, 7), True), ((2, 3, 5, 7), True)])
def test_randn_fill_at_is_randn_fill_bit_for_bit(dev, dtype, shape, strided):
    """the draw read from a one-element int64 device tensor (its low 32 bits) == the draw by value, dense and strided, on the whole-pixel path ((2,4,8,8)) and the
    element path (c != 4, hw % 4 != 0); channels outside the view untouched"""
    from diffusion_e2e_ft_amd import ops
    B, C, H, W = shape

    def dest():
        if not strided:
            buf = torch.full((B, H, W, C), 7.0, dtype=dtype, device=dev)
            return buf, buf
        buf = torch.arange(B * H * W * 8, device=dev, dtype=torch.float32).reshape(B, H, W, 8).remainder(251.0).sub(125.0).to(dtype)
        return buf, buf[..., 4:4 + C]

    draw_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    seen = []
    for draw in DRAWS:
        wb, want = dest()
        ops.randn_fill_(want, SEED, draw, slot=0)
        gb, got = dest()
        draw_dev.fill_(draw)
        assert ops.randn_fill_at_(got, SEED, draw_dev, slot=0) is got
        assert torch.equal(gb, wb), (draw, dtype, shape, strided)          # the whole buffers: the noise AND the channels around it
        seen.append(got.clone())
    # only the low 32 bits count; another slot is another grid
    gb, got = dest()
    draw_dev.fill_(2 ** 32 + 1)
    ops.randn_fill_at_(got, SEED, draw_dev, slot=0)
    assert torch.equal(got, seen[1])
    assert not any(torch.equal(seen[i], seen[j]) for i in range(4) for j in range(i))
    with pytest.raises(TypeError):
        ops.randn_fill_at_(got, SEED, torch.zeros(1, dtype=torch.int32, device=dev))
