"""Shared helpers for the parity tests."""
import torch

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
# max |out - ref| / max |ref| tolerances for a single op with fp32 accumulation and output rounding to dtype
TOL = {torch.float32: 3e-5, torch.float16: 3e-3, torch.bfloat16: 2e-2}


def rel_err(out, ref):
    out = out.detach().double().cpu()
    ref = ref.detach().double().cpu()
    denom = ref.abs().max().clamp_min(1e-30)
    return ((out - ref).abs().max() / denom).item()


def assert_close(out, ref, dtype, what="", scale=1.0):
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert torch.isfinite(out.float()).all(), "%s: non-finite output" % what
    e = rel_err(out, ref)
    assert e <= TOL[dtype] * scale, "%s: rel err %.3e > %.3e (%s)" % (what, e, TOL[dtype] * scale, dtype)
    return e


def q(t, dtype):
    """quantize a fp32 CPU tensor to dtype and back (so reference and kernel see identical inputs)"""
    return t.to(dtype).float()


def nhwc(t, dtype, dev):
    """NCHW fp32 cpu -> NHWC dtype device"""
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).to(dev)


def to_nchw(t):
    return t.permute(0, 3, 1, 2).float().cpu()


def pack_conv_weight(w, dtype, dev, cin_pad=None):
    """[Co,Ci,kh,kw] -> [Co, kh*kw*Ci(_pad)] OHWI"""
    Co, Ci, kh, kw = w.shape
    w = w.permute(0, 2, 3, 1)
    if cin_pad is not None and cin_pad != Ci:
        w = torch.nn.functional.pad(w, (0, cin_pad - Ci))
    return w.reshape(Co, -1).contiguous().to(dtype).to(dev)


def chan_err_wgrad(got, ref, dy, x, taps):
    """Channel-aware error of a weight gradient: max over entries of |got - ref| / (||dY[..., co]||_2 * ||X[..., ci]||_2).  got, ref: [cout, taps * cin] in OHWI
    order; dy [..., cout] and x [..., cin] channels-last, norms in float64 over all pixels.  The normaliser is invariant to any per-channel rescaling of either
    operand and, unlike |ref| itself, never tiny through cancellation; all-zero channels are left out of the maximum."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    dy, x = dy.detach().double().cpu(), x.detach().double().cpu()
    cout, cin = dy.shape[-1], x.shape[-1]
    assert tuple(got.shape) == tuple(ref.shape) == (cout, taps * cin), (got.shape, ref.shape, cout, taps, cin)
    ny = dy.reshape(-1, cout).square().sum(0).sqrt()
    nx = x.reshape(-1, cin).square().sum(0).sqrt()
    den = ny[:, None, None] * nx[None, None, :]
    err = (got - ref).abs().view(cout, taps, cin)
    live = (den > 0).expand_as(err)
    if not live.any():
        return 0.0
    return (err[live] / den.expand_as(err)[live]).max().item()


def chan_err_rows(got, ref):
    """max over output channels (the LAST dimension) of max|err| in the channel / max|ref| in the channel: forward and data-gradient outputs, channels-last.
    Channels whose reference is all zero are left out."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    c = ref.shape[-1]
    e = (got - ref).abs().reshape(-1, c).max(0).values
    m = ref.abs().reshape(-1, c).max(0).values
    live = m > 0
    return (e[live] / m[live]).max().item() if live.any() else 0.0
