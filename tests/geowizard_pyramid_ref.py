"""Host restatement of e2eft_pyramid_noise_weighted, written from the contract in include/e2eft.h ("The GeoWizard trainer's timestep-weighted multi-resolution
noise") over the generator restatement of tests/noise_ref.py.  TEST INFRASTRUCTURE ONLY.

  weighted_pyramid(seed, draw, shape, sizes, timesteps, ...)       float64 torch tensor [B,C,H,W]: the definition, bilinear by torch's own interpolate
  weighted_pyramid_fp32(seed, draw, shape, sizes, timesteps, ...)  the same formula rounded to fp32 at every step the kernel rounds at, in numpy: an INDEPENDENT
                                                                    rounding (numpy's logf / sinf / cosf, products and sums rounded apart where the kernel fuses)
  level_grids(seed, draw, shape, sizes)                             the float64 grids of slot 0 and slots 1 + i, in the order the reference's function asks for them

The weight of level i of sample b is  tw_b * discount^i  with  tw_b = (float)timesteps[b] / timestep_div, an fp32 number — also in the float64 evaluation, because the
reference's own `timesteps[..., None, None, None] / 1000` is an fp32 tensor (torch divides an int64 tensor into the default dtype).  The kernel's
w_i = (float)discount^i and its single product w_i * tw_b are roundings that only the fp32 evaluation makes; the float64 one takes the float64 power."""
import numpy as np

import noise_ref

F32 = np.float32


def timestep_weights(timesteps, timestep_div=1000.0):
    """tw_b as fp32 numbers (numpy float32 array [B])"""
    return np.asarray(timesteps, dtype=np.int64).astype(F32) / F32(timestep_div)


def level_weights(n, discount=0.9):
    """w_i = (float)discount^i: the double power (by repeated products, as the library's host code) rounded once"""
    out, w = [], 1.0
    for _ in range(n):
        out.append(F32(w))
        w *= float(F32(discount))
    return out


def level_grids(seed, draw, shape, sizes):
    B, C, H, W = shape
    return [noise_ref.normal_grid(seed, draw, 0, shape)] + [noise_ref.normal_grid(seed, draw, 1 + i, (B, C, r, c)) for i, (r, c) in enumerate(sizes)]


def weighted_pyramid(seed, draw, shape, sizes, timesteps, discount=0.9, timestep_div=1000.0):
    """float64 [B,C,H,W]: base + sum_i tw_b * discount^i * bilinear_up(level_i), over the unbiased std of the whole tensor.  discount^i is the float64 power here
    (the fp32 w_i of the kernel is one of the roundings the fp32 evaluation below makes); tw_b is the fp32 number, the reference's own"""
    import torch
    B, C, H, W = shape
    grids = level_grids(seed, draw, shape, sizes)
    tw = torch.from_numpy(timestep_weights(timesteps, timestep_div).astype(np.float64)).reshape(B, 1, 1, 1)
    total = grids[0]
    for i in range(len(sizes)):
        up = torch.nn.functional.interpolate(grids[1 + i], size=(H, W), mode="bilinear", align_corners=False)
        total = total + up * tw * discount ** i
    return total / total.std()


# ---- the fp32 evaluation ---------------------------------------------------------------------------------------------------------------------------------
def _half_unit(x):
    return (x.astype(F32) + F32(0.5)) * F32(2.0 ** -24)


def normals_fp32(seed, draw, slot, n):
    """the generator in fp32, step by step as the contract words it: u or 1 - u, whichever is an fp32 number; ln by log / log1p; theta = 2 pi u; r cos / r sin"""
    w, e = noise_ref.words(seed, draw, slot, n)
    e = e.astype(np.int64)
    pair = e & 2
    x = (w >> np.uint32(8)).astype(np.int64)
    xa, xb = x[e, pair], x[e, pair + 1]
    lo = xa < (1 << 23)
    lnu = np.where(lo, np.log(_half_unit(np.where(lo, xa, 0))), np.log1p(-_half_unit(np.where(lo, 0, 0xFFFFFF - xa)))).astype(F32)
    r = np.sqrt(F32(-2.0) * lnu)
    fold = xb >= (1 << 23)
    th = F32(6.283185307179586) * _half_unit(np.where(fold, 0xFFFFFF - xb, xb))
    zc, zs = r * np.cos(th), r * np.sin(th)
    zs = np.where(fold, -zs, zs)
    out = np.where(e & 1, zs, zc)
    assert out.dtype == F32
    return out


def _taps_fp32(n_in, n_out):
    """nn.Upsample(mode="bilinear"), align_corners=False, in fp32: src = (in / out) * (dst + 0.5) - 0.5 clamped below at 0, i1 = min(i0 + 1, in - 1)"""
    dst = np.arange(n_out).astype(F32)
    src = (F32(n_in) / F32(n_out)) * (dst + F32(0.5)) - F32(0.5)
    src = np.where(src < 0, F32(0), src).astype(F32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, (src - i0.astype(F32)).astype(F32)


def weighted_pyramid_fp32(seed, draw, shape, sizes, timesteps, discount=0.9, timestep_div=1000.0):
    """fp32 numpy array [B,C,H,W]: every product and sum of the definition rounded to fp32 in the kernel's order (corner weights wy * wx, the four corners summed in
    order, then acc + (w_i * tw_b) * up); the std from float64 sums of the fp32 totals, rounded to fp32; one fp32 division"""
    B, C, H, W = shape
    acc = normals_fp32(seed, draw, 0, B * C * H * W).reshape(shape)
    tw = timestep_weights(timesteps, timestep_div).reshape(B, 1, 1, 1)
    for i, ((r, c), w) in enumerate(zip(sizes, level_weights(len(sizes), discount))):
        lvl = normals_fp32(seed, draw, 1 + i, B * C * r * c).reshape(B, C, r, c)
        y0, y1, ly = _taps_fp32(r, H)
        x0, x1, lx = _taps_fp32(c, W)
        wy = ((F32(1) - ly)[:, None], ly[:, None])
        wx = ((F32(1) - lx)[None, :], lx[None, :])
        up = np.zeros(shape, dtype=F32)
        for a, ys in enumerate((y0, y1)):
            for d, xs in enumerate((x0, x1)):
                up = up + (wy[a] * wx[d]) * lvl[:, :, ys[:, None], xs[None, :]]
        acc = acc + (w * tw) * up
        assert acc.dtype == F32 and up.dtype == F32
    t64 = acc.astype(np.float64)
    n = t64.size
    s1, s2 = t64.sum(), (acc * acc).astype(np.float64).sum()
    sd = F32(np.sqrt((s2 - s1 * s1 / n) / (n - 1)))
    return acc / sd
