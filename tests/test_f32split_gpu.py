"""fp32 3x3 convolutions on the f16 matrix pipe (csrc/f32split.hip, igemm6_kernel<..., F32O>; include/e2eft.h e2eft_f32_split2 / e2eft_conv2d_fwd_f32split).
The claim under test: the two-term f16 split is an fp32-class route — against a float64 convolution its error is no larger than the fp32 matrix instruction's
(igemm2<float>) on the same inputs, on well-scaled data, on data that spans nine decades, with bias / residual / GroupNorm statistics, and through autograd (the data
gradient is the same call on dY).  The split itself is checked for exactness: x * s - (x0 + x1) <= 2^-22 |x s| wherever x1 is a normal f16, s a power of two with the
maximum in [2^14, 2^15).  Subprocess + 8-workgroup grid as tests/test_patch_conv_gpu.py (small shapes must reach the persistent kernel)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SCRIPT = r'''
import sys, os, math
sys.path.insert(0, os.path.join(%r, ".."))
sys.path.insert(0, %r)
import ctypes
import torch
import torch.nn.functional as F
from diffusion_e2e_ft_amd import ops, _lib, autograd as ag
from util import nhwc, to_nchw, pack_conv_weight, rel_err
dev = torch.device("cuda:0")
lib = _lib.load()
_lib.set_option(_lib.OPT_PERSISTENT_GRID, 8)
lib.e2eft_debug_last_kernel.restype = ctypes.c_char_p

# ---- the split: exact to 2^-22, scale from the maximum
g = torch.Generator().manual_seed(1)
x = torch.randn(2, 16, 32, 64, generator=g) * torch.exp(torch.randn(2, 16, 32, 64, generator=g) * 3.0)     # log-normal magnitudes: ~9 decades
xd = x.to(dev)
planes, scale = ops.f32_split2(xd)
torch.cuda.synchronize()
s, inv = scale[1].item(), scale[2].item()
amax = x.abs().max().item()
assert s * inv == 1.0 and math.frexp(s)[0] == 0.5, (s, inv)
assert 2.0 ** 14 <= amax * s < 2.0 ** 15, (amax, s)
x0, x1 = planes[..., :64].double().cpu(), planes[..., 64:].double().cpu()
xs = x.double() * s
err = (xs - (x0 + x1)).abs()
normal = (xs.abs() >= 2.0 ** -3)          # x1 = f16 of a value >= 2^-14: a normal half
assert (err[normal] <= xs.abs()[normal] * 2.0 ** -22).all(), (err[normal] / xs.abs()[normal]).max()
assert (err <= 2.0 ** -25).logical_or(normal).all()           # elsewhere: half a subnormal step, 2^-39 of the maximum
print("split exact: max rel err %%.3e (bound %%.3e); scale 2^%%d" %% ((err[normal] / xs.abs()[normal]).max().item(), 2.0 ** -22, int(math.log2(s))), flush=True)
# zeros and a huge tensor: the scale stays a finite power of two
z, zs = ops.f32_split2(torch.zeros(1, 8, 32, 64, device=dev))
assert zs[1].item() == 1.0 and float(z.abs().max()) == 0.0
hp, hs = ops.f32_split2(torch.full((1, 8, 32, 64), 3.0e30, device=dev))
assert torch.isfinite(hp.float()).all() and 2.0 ** 14 <= 3.0e30 * hs[1].item() < 2.0 ** 15

# ---- the convolution against float64, beside the fp32 matrix instruction on the same inputs
worst = 0.0
# B, H, W, C, Co, bias, residual, wide-range input, (kh, kw, stride, pad), kernel
cases = [
    (2, 32, 64, 128, 128, True, True, False, (3, 3, 1, 1), "igemm6"),
    (1, 16, 64, 64, 128, True, False, False, (3, 3, 1, 1), "igemm6"),      # one plane = one 64-channel chunk: every chunk changes block
    (5, 8, 32, 192, 64, False, True, True, (3, 3, 1, 1), "igemm6"),        # three chunks per plane, cout 64, input over 6 decades
    (2, 16, 32, 192, 256, True, False, True, (3, 3, 1, 1), "igemm6"),      # two N tiles (K = 1728: below the split-K plan of small problems)
    (2, 16, 48, 128, 128, True, True, False, (3, 3, 1, 1), "igemm5"),      # width 48: not the halo-patch kernel's grid -> igemm5 (tap-major K, 256-row tiles)
    (8, 8, 24, 128, 64, True, False, True, (3, 3, 1, 1), "igemm5"),        # 192 pixels per image: tiles straddle images, no statistics from the epilogue
    (2, 32, 64, 128, 128, True, False, False, (4, 4, 2, 1), "igemm5"),     # 4x4 / stride 2 / pad 1: the data gradient of an upsampler convolution (autograd.upconv_dgrad_weight)
    (2, 32, 64, 64, 192, False, False, False, (3, 3, 2, 1), "igemm5"),     # a stride-2 downsampler, ragged N tile
    (2, 32, 32, 256, 128, True, False, False, (1, 1, 1, 0), "igemm5"),     # a 1x1 shortcut convolution (K = 3 C: three k-tiles per 64 channels)
    (5, 18, 18, 128, 128, True, True, False, (3, 3, 1, 1), "igemm5"),      # 1620 output pixels = 6.33 tiles: the ragged last tile's rows beyond M are zeroed on the way in and masked on the way out
    (10, 9, 9, 192, 64, False, False, True, (3, 3, 1, 1), "igemm5"),       # 810 pixels: 3.16 tiles, 81 pixels per image
]
for (B, H, W, Cc, Co, hb, rs, wide, (kh, kw, st, pd), kern) in cases:
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + Cc + Co + W + kh)
    x = torch.randn(B, Cc, H, W, generator=g) * 1.5 + 0.3
    if wide:
        x = x * torch.exp(torch.randn(B, Cc, H, W, generator=g) * 2.0)
    w = torch.randn(Co, Cc, kh, kw, generator=g) / (Cc * kh * kw) ** 0.5
    b = torch.randn(Co, generator=g) if hb else None
    ref = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=st, padding=pd)
    Ho, Wo = ref.shape[2], ref.shape[3]
    r = torch.randn(B, Co, Ho, Wo, generator=g) if rs else None
    xd, wd = nhwc(x, torch.float32, dev), pack_conv_weight(w, torch.float32, dev)
    bd = None if b is None else b.to(dev)
    rd = None if r is None else nhwc(r, torch.float32, dev)
    if r is not None:
        ref = ref + r.double()
    _lib.set_option(_lib.OPT_F32_SPLIT, 1)
    y1 = ops.conv2d(xd, wd, bd, Co, kh, kw, st, (pd, pd, pd, pd), residual=rd, gn_stats=True)
    torch.cuda.synchronize()
    k1 = lib.e2eft_debug_last_kernel().decode()
    assert "f32split" in k1 and kern in k1, k1
    _lib.set_option(_lib.OPT_F32_SPLIT, 0)
    y2 = ops.conv2d(xd, wd, bd, Co, kh, kw, st, (pd, pd, pd, pd), residual=rd, gn_stats=True)
    torch.cuda.synchronize()
    k2 = lib.e2eft_debug_last_kernel().decode()
    assert "float" in k2 and "f32split" not in k2, k2
    _lib.set_option(_lib.OPT_F32_SPLIT, 1)
    e1, e2 = rel_err(to_nchw(y1).double(), ref), rel_err(to_nchw(y2).double(), ref)
    rms1 = ((to_nchw(y1).double() - ref) ** 2).mean().sqrt().item() / ref.abs().max().item()
    rms2 = ((to_nchw(y2).double() - ref) ** 2).mean().sqrt().item() / ref.abs().max().item()
    # GroupNorm statistics of the output (n, mean, M2 per slab and channel) where the epilogue emits them: they describe the tensor that was written
    st1 = getattr(y1, "_e2eft_gn", None)
    assert st1 is not None or (Ho * Wo) %% 256 != 0, "statistics missing"
    if st1 is not None:
        p = st1.partial.view(B, st1.nslabs, Co, 3).double().cpu()
        n1 = p[..., 0].sum(1)
        m1 = (p[..., 0] * p[..., 1]).sum(1) / n1
        v1 = (p[..., 2] + p[..., 0] * (p[..., 1] - m1[:, None]) ** 2).sum(1)
        yy = to_nchw(y1).double()
        assert (n1 == Ho * Wo).all()
        assert (m1 - yy.mean((2, 3))).abs().max() <= 1e-5 * yy.abs().max(), "statistics: mean"
        assert ((v1 / (Ho * Wo)) - yy.var((2, 3), unbiased=False)).abs().max() <= 1e-4 * yy.var((2, 3), unbiased=False).max(), "statistics: variance"
    print("f32split conv %%s: max err %%.3e (fp32 MFMA %%.3e), rms %%.3e (%%.3e)  [%%s]" %% ((B, H, W, Cc, Co, hb, rs, wide, kh, st), e1, e2, rms1, rms2, k1), flush=True)
    assert e1 <= max(1.5 * e2, 4e-7), (e1, e2)
    assert rms1 <= max(1.5 * rms2, 5e-8), (rms1, rms2)
    worst = max(worst, e1 / max(e2, 1e-12))

# ---- two sources (the UNet's up blocks: conv(cat(h, skip))): one pair of planes under one scale (e2eft_f32_split2_cat); forward and weight gradient
g = torch.Generator().manual_seed(23)
B, H, W, C1, C2, Co = 2, 16, 32, 128, 64, 128
xa = torch.randn(B, C1, H, W, generator=g) * 2.0
xb = torch.randn(B, C2, H, W, generator=g) * 0.01           # a skip tensor three decades below its partner: the common scale must not cost it its bits
w = torch.randn(Co, C1 + C2, 3, 3, generator=g) / ((C1 + C2) * 9) ** 0.5
gy = torch.randn(B, Co, H, W, generator=g)
xcat = torch.cat([xa, xb], 1).double()
w64 = w.double().requires_grad_(True)
y64 = F.conv2d(xcat, w64, None, padding=1)
y64.backward(gy.double())
refw = w64.grad.permute(0, 2, 3, 1).reshape(Co, -1)
xad, xbd, wd, gd = nhwc(xa, torch.float32, dev), nhwc(xb, torch.float32, dev), pack_conv_weight(w, torch.float32, dev), nhwc(gy, torch.float32, dev)
res2 = {}
for on in (True, False):
    _lib.set_option(_lib.OPT_F32_SPLIT, int(on))
    y = ops.conv2d(xad, wd, None, Co, 3, 3, 1, (1, 1, 1, 1), x2=xbd)
    torch.cuda.synchronize()
    assert ("f32split" in lib.e2eft_debug_last_kernel().decode()) == on, lib.e2eft_debug_last_kernel()
    dw = ops.conv2d_wgrad(gd, xad, xbd, Co, 3, 3, 1, (1, 1, 1, 1), 1.0)
    torch.cuda.synchronize()
    res2[on] = (to_nchw(y).double(), dw.double().cpu())
_lib.set_option(_lib.OPT_F32_SPLIT, 1)
e1, e2 = rel_err(res2[True][0], y64.detach()), rel_err(res2[False][0], y64.detach())
w1, w2 = rel_err(res2[True][1], refw), rel_err(res2[False][1], refw)
# the small source's own contribution: the columns of dW that multiply xb
s1, s2 = rel_err(res2[True][1].view(Co, 9, C1 + C2)[..., C1:], refw.view(Co, 9, C1 + C2)[..., C1:]), rel_err(res2[False][1].view(Co, 9, C1 + C2)[..., C1:], refw.view(Co, 9, C1 + C2)[..., C1:])
print("two sources: forward %%.3e (fp32 MFMA %%.3e), weight gradient %%.3e (%%.3e), its columns of the small source %%.3e (%%.3e)" %% (e1, e2, w1, w2, s1, s2), flush=True)
assert e1 <= max(1.5 * e2, 4e-7) and w1 <= max(1.5 * w2, 4e-7) and s1 <= max(1.5 * s2, 6e-7), (e1, e2, w1, w2, s1, s2)

# ---- nn.Linear (e2eft_gemm_f32split, igemm5's GEMM mode): x W^T + b + residual against float64, beside the fp32 matrix instruction
for (Mr, N, K, hb, rs) in [(1024, 320, 320, True, True), (2048, 1280, 64, False, False), (512, 640, 2560, True, False), (1100, 320, 320, True, True), (1296, 1280, 1280, False, True)]:
    g = torch.Generator().manual_seed(Mr + N + K)
    a = torch.randn(Mr, K, generator=g) * torch.exp(torch.randn(Mr, K, generator=g))
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if hb else None
    r = torch.randn(Mr, N, generator=g) if rs else None
    ref = a.double() @ w.double().t()
    if b is not None:
        ref = ref + b.double()
    if r is not None:
        ref = ref + r.double()
    ad, wd = a.to(dev), w.to(dev)
    ys = {}
    for on in (True, False):
        _lib.set_option(_lib.OPT_F32_SPLIT, int(on))
        ys[on] = ops.gemm(ad, wd, None if b is None else b.to(dev), None if r is None else r.to(dev))
        torch.cuda.synchronize()
        assert ("f32split" in lib.e2eft_debug_last_kernel().decode()) == on, lib.e2eft_debug_last_kernel()
    _lib.set_option(_lib.OPT_F32_SPLIT, 1)
    e1, e2 = rel_err(ys[True].double().cpu(), ref), rel_err(ys[False].double().cpu(), ref)
    print("f32split gemm M%%d N%%d K%%d: max err %%.3e (fp32 MFMA %%.3e)" %% (Mr, N, K, e1, e2), flush=True)
    assert e1 <= max(1.5 * e2, 4e-7), (e1, e2)

# ---- nearest-2x upsample + conv3x3 as four 2x2 phases of the split planes (e2eft_upconv2x_fwd_f32split): both kernels
for (B, H, W, Cc, Co, kern) in [(2, 16, 32, 128, 128, "igemm6"), (4, 16, 16, 128, 64, "igemm5")]:
    g = torch.Generator().manual_seed(B + H + W + Cc + Co)
    x = torch.randn(B, Cc, H, W, generator=g) * 1.3
    w = torch.randn(Co, Cc, 3, 3, generator=g) / (Cc * 9) ** 0.5
    b = torch.randn(Co, generator=g)
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest"), w.double(), b.double(), padding=1)
    up = torch.nn.Conv2d(Cc, Co, 3, padding=1).to(dev)
    with torch.no_grad():
        up.weight.copy_(w); up.bias.copy_(b)
    ys = {}
    for on in (True, False):
        _lib.set_option(_lib.OPT_F32_SPLIT, int(on))
        with torch.no_grad():
            ys[on] = ag.conv(up, nhwc(x, torch.float32, dev), up_to=(2 * H, 2 * W))
        torch.cuda.synchronize()
        kk = lib.e2eft_debug_last_kernel().decode()
        assert ("f32split" in kk) == on and (not on or kern in kk), kk
    _lib.set_option(_lib.OPT_F32_SPLIT, 1)
    e1, e2 = rel_err(to_nchw(ys[True]).double(), ref), rel_err(to_nchw(ys[False]).double(), ref)
    print("f32split upconv2x %%s: max err %%.3e (fp32 MFMA %%.3e)" %% ((B, H, W, Cc, Co), e1, e2), flush=True)
    assert e1 <= max(1.5 * e2, 4e-7), (e1, e2)

# ---- weight gradients: three launches of the 16-bit kernel on the split planes of dY and X against float64, beside wgrad32_kernel
for (B, H, W, Cc, Co, k) in [(2, 24, 24, 320, 320, 3), (4, 16, 32, 64, 128, 1), (2, 18, 18, 640, 640, 3)]:
    g = torch.Generator().manual_seed(B + H + Cc + Co + k)
    x = torch.randn(B, Cc, H, W, generator=g) * torch.exp(torch.randn(B, Cc, H, W, generator=g))
    gy = torch.randn(B, Co, H, W, generator=g) * 1e-3 * torch.exp(torch.randn(B, Co, H, W, generator=g))
    w64 = torch.zeros(Co, Cc, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w64, None, padding=k // 2).backward(gy.double())
    ref = w64.grad.permute(0, 2, 3, 1).reshape(Co, -1)
    xd, gd = nhwc(x, torch.float32, dev), nhwc(gy, torch.float32, dev)
    rs = {}
    for on in (True, False):
        _lib.set_option(_lib.OPT_F32_SPLIT, int(on))
        rs[on] = ops.conv2d_wgrad(gd, xd, None, Co, k, k, 1, (k // 2,) * 4, 1.0)
        torch.cuda.synchronize()
        assert rs[on] is not None
    _lib.set_option(_lib.OPT_F32_SPLIT, 1)
    e1, e2 = rel_err(rs[True].double().cpu(), ref), rel_err(rs[False].double().cpu(), ref)
    print("f32split wgrad %%s: max err %%.3e (fp32 MFMA %%.3e)" %% ((B, H, W, Cc, Co, k), e1, e2), flush=True)
    assert e1 <= max(1.5 * e2, 4e-7), (e1, e2)

# ---- GroupNorm + SiLU whose apply pass writes the planes (e2eft_groupnorm_fwd_split), without a gradient: ops.conv2d(norm=) against float64
g = torch.Generator().manual_seed(11)
B, H, W, Cc, Co = 2, 32, 64, 128, 128
x = torch.randn(B, Cc, H, W, generator=g) * 3.0 - 1.0
gamma, beta = torch.randn(Cc, generator=g) * 0.3 + 1.0, torch.randn(Cc, generator=g) * 0.5
w = torch.randn(Co, Cc, 3, 3, generator=g) / (Cc * 9) ** 0.5
b = torch.randn(Co, generator=g)
ref = F.conv2d(F.silu(F.group_norm(x.double(), 32, gamma.double(), beta.double(), 1e-5)), w.double(), b.double(), padding=1)
xd, wd = nhwc(x, torch.float32, dev), pack_conv_weight(w, torch.float32, dev)
yn = {}
for on in (True, False):
    _lib.set_option(_lib.OPT_F32_SPLIT, int(on))
    yn[on] = ops.conv2d(xd, wd, b.to(dev), Co, 3, 3, 1, (1, 1, 1, 1), norm=(gamma.to(dev), beta.to(dev), 32, 1e-5, True))
    torch.cuda.synchronize()
    assert ("f32split" in lib.e2eft_debug_last_kernel().decode()) == on
_lib.set_option(_lib.OPT_F32_SPLIT, 1)
en1, en2 = rel_err(to_nchw(yn[True]).double(), ref), rel_err(to_nchw(yn[False]).double(), ref)
print("norm -> planes -> conv: max err %%.3e (fp32 GroupNorm pass + fp32 MFMA %%.3e)" %% (en1, en2), flush=True)
assert en1 <= max(1.5 * en2, 6e-7), (en1, en2)

# ---- autograd: forward + data gradient through the split route against float64 autograd
from types import SimpleNamespace
g = torch.Generator().manual_seed(7)
B, H, W, Cc, Co = 2, 16, 64, 128, 128
x = torch.randn(B, Cc, H, W, generator=g)
w = torch.randn(Co, Cc, 3, 3, generator=g) / (Cc * 9) ** 0.5
b = torch.randn(Co, generator=g)
gy = torch.randn(B, Co, H, W, generator=g)
conv = torch.nn.Conv2d(Cc, Co, 3, padding=1).to(dev)
with torch.no_grad():
    conv.weight.copy_(w); conv.bias.copy_(b)
conv.weight.requires_grad_(False); conv.bias.requires_grad_(False)       # the frozen VAE: only the data gradient
res = {}
for on in (True, False):
    _lib.set_option(_lib.OPT_F32_SPLIT, int(on))
    xd = nhwc(x, torch.float32, dev).requires_grad_(True)
    y = ag.conv(conv, xd)
    y.backward(nhwc(gy, torch.float32, dev))
    torch.cuda.synchronize()
    res[on] = (to_nchw(y.detach()).double(), to_nchw(xd.grad).double(), lib.e2eft_debug_last_kernel().decode())
_lib.set_option(_lib.OPT_F32_SPLIT, 1)
x64 = x.double().requires_grad_(True)
y64 = F.conv2d(x64, w.double(), b.double(), padding=1)
y64.backward(gy.double())
assert "f32split" in res[True][2] and "f32split" not in res[False][2], (res[True][2], res[False][2])
ef1, ef2 = rel_err(res[True][0], y64.detach()), rel_err(res[False][0], y64.detach())
eg1, eg2 = rel_err(res[True][1], x64.grad), rel_err(res[False][1], x64.grad)
print("autograd: forward %%.3e (fp32 MFMA %%.3e), data gradient %%.3e (%%.3e)" %% (ef1, ef2, eg1, eg2), flush=True)
assert ef1 <= max(1.5 * ef2, 4e-7) and eg1 <= max(1.5 * eg2, 4e-7)

# ---- a frozen fp32 ResnetBlock2D under autograd (the VAE decoder of the fp32 recipe): _NormConvSplitFn twice, the skip gradient folded into the first norm's backward
from diffusion_e2e_ft_amd import modules as M
blk = M.ResnetBlock2D(128, 128, None).to(dev)
with torch.no_grad():
    for prm in blk.parameters():
        prm.copy_(torch.randn(prm.shape, generator=g) * (0.05 if prm.dim() > 1 else 0.3) + (1.0 if prm.dim() == 1 else 0.0))
blk.requires_grad_(False)
x = torch.randn(2, 128, 16, 64, generator=g) * 2.0
gy = torch.randn(2, 128, 16, 64, generator=g)
out = {}
for on in (True, False):
    _lib.set_option(_lib.OPT_F32_SPLIT, int(on))
    xd = nhwc(x, torch.float32, dev).requires_grad_(True)
    y = blk.nhwc(xd)
    y.backward(nhwc(gy, torch.float32, dev))
    torch.cuda.synchronize()
    out[on] = (to_nchw(y.detach()).double(), to_nchw(xd.grad).double())
_lib.set_option(_lib.OPT_F32_SPLIT, 1)
b64 = torch.nn.Module()
x64 = x.double().requires_grad_(True)
sd = {k: v.detach().double().cpu() for k, v in blk.state_dict().items()}
h = F.conv2d(F.silu(F.group_norm(x64, 32, sd["norm1.weight"], sd["norm1.bias"], 1e-5)), sd["conv1.weight"], sd["conv1.bias"], padding=1)
h = F.conv2d(F.silu(F.group_norm(h, 32, sd["norm2.weight"], sd["norm2.bias"], 1e-5)), sd["conv2.weight"], sd["conv2.bias"], padding=1)
y64 = x64 + h
y64.backward(gy.double())
eb1, eb2 = rel_err(out[True][0], y64.detach()), rel_err(out[False][0], y64.detach())
egb1, egb2 = rel_err(out[True][1], x64.grad), rel_err(out[False][1], x64.grad)
print("frozen ResnetBlock2D under autograd: forward %%.3e (unfused fp32 %%.3e), input gradient %%.3e (%%.3e)" %% (eb1, eb2, egb1, egb2), flush=True)
assert eb1 <= max(1.5 * eb2, 6e-7) and egb1 <= max(1.5 * egb2, 6e-7)

# ---- nothing on the route reads the device back: a ResnetBlock2D forward (norm -> planes -> conv twice: maximum / bound, scales, weight splits all on the
#      device) is captured in a hipGraph and replayed on new input — any host synchronisation inside would fail the capture
blk2 = M.ResnetBlock2D(128, 128, None).to(dev)
with torch.no_grad():
    for prm in blk2.parameters():
        prm.copy_(torch.randn(prm.shape, generator=g) * (0.05 if prm.dim() > 1 else 0.3) + (1.0 if prm.dim() == 1 else 0.0))
xs = nhwc(torch.randn(2, 128, 16, 64, generator=g), torch.float32, dev)
with torch.no_grad():
    for _ in range(2):                      # warm-up on a side stream, as torch asks before a capture
        s_ = torch.cuda.Stream()
        s_.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s_):
            blk2.nhwc(xs)
        torch.cuda.current_stream().wait_stream(s_)
    for prm in blk2.parameters():           # fresh weight versions: the capture has to contain the weight splits as well
        prm.mul_(1.0)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        yg = blk2.nhwc(xs)
    assert "f32split" in lib.e2eft_debug_last_kernel().decode()
    xs.copy_(nhwc(torch.randn(2, 128, 16, 64, generator=g) * 3.0, torch.float32, dev))
    gr.replay()
    torch.cuda.synchronize()
    ye = blk2.nhwc(xs)
    torch.cuda.synchronize()
assert torch.equal(yg, ye), (yg - ye).abs().max().item()
print("hipGraph capture + replay of the split route: bit-equal to the eager launches", flush=True)

# ---- the option switches the route off; shapes the kernel does not take fall back (width not a multiple of 32)
_lib.set_option(_lib.OPT_F32_SPLIT, 0)
xd, wd = nhwc(x, torch.float32, dev), pack_conv_weight(w, torch.float32, dev)
ops.conv2d(xd, wd, None, Co, 3, 3, 1, (1, 1, 1, 1))
assert "f32split" not in lib.e2eft_debug_last_kernel().decode()
_lib.set_option(_lib.OPT_F32_SPLIT, 1)
x72 = nhwc(torch.randn(1, 128, 8, 72), torch.float32, dev)
y72 = ops.conv2d(x72, wd, None, Co, 3, 3, 1, (1, 1, 1, 1))
assert "f32split" not in lib.e2eft_debug_last_kernel().decode()
print("F32SPLIT CASES PASSED worst ratio to the fp32 matrix instruction %%.2f" %% worst)
''' % (HERE, HERE)


def test_f32split_conv(dev):
    r = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, env=dict(os.environ), timeout=900)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and "F32SPLIT CASES PASSED" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
