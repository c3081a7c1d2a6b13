"""igemm6.hip in its v_mfma_f32_16x16x32 form (E2EFT_OPT_PATCH_MFMA = 2: 4 x 4 accumulators of four registers per wave, two k-steps of 32 channels per k-tile,
the patch swizzle chunk ^ (((row >> 1) & 3) << 1), the epilogues in the 16x16 accumulator layout) against torch CPU float64 on the quantised inputs — the cases of
tests/test_patch_conv_gpu.py at which this form can go wrong by itself:
  (1) random data: 2 / 3 / 5 chunks, concat, ragged N tile, one tile row, one tile per image, fused 2x upsample, every epilogue option, both dtypes;
  (2) impulse responses with weights that depend on output channel, input channel AND tap, exact in fp16: a k-slot or swizzle mapping that differs between the
      A and the B operand moves products between channels, which the one-stencil impulse test of the other file cannot see;
  (3) the 2x2-tap variant on one upsampler convolution;
  (4) the fused-GroupNorm variants are NOT instantiated in this form (they spill): under option 2 a fused launch must still run, on the 32x32x16 form;
  (5) the GroupNorm partials, reduced on the host in float64, against mean and variance of the output tensor;
  (6) the same launch under option 1 and option 2: each within tolerance of float64, each bit-equal to itself run twice (output and partials);
  (7) the planner's invariant under the default option: the fused launch and the plain launch of one problem name the same form.
Runs as a subprocess so that the options never leak; E2EFT_OPT_PERSISTENT_GRID = 8 and E2EFT_OPT_PERSISTENT_MIN_QROUNDS = 8 send small problems through the
persistent kernel; e2eft_debug_patch_launches and e2eft_debug_last_kernel prove which kernel and which form ran."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SCRIPT = r'''
import sys, os
sys.path.insert(0, os.path.join(%r, ".."))
sys.path.insert(0, %r)
import ctypes
import torch
import torch.nn.functional as F
from diffusion_e2e_ft_amd import ops, _lib
from diffusion_e2e_ft_amd import autograd as AG
from util import nhwc, to_nchw, pack_conv_weight, q, rel_err, TOL
dev = torch.device("cuda:0")
lib = _lib.load()
_lib.set_option(_lib.OPT_PERSISTENT_GRID, 8)
_lib.set_option(_lib.OPT_PERSISTENT_MIN_QROUNDS, 8)
_lib.set_option(_lib.OPT_PATCH_MFMA, 2)
lib.e2eft_debug_patch_launches.restype = ctypes.c_long
lib.e2eft_debug_last_kernel.restype = ctypes.c_char_p
def launches():
    return lib.e2eft_debug_patch_launches()
def tag():
    return lib.e2eft_debug_last_kernel().decode()
def is16(t):
    return t.startswith("igemm6_kernel<") and ", m16, " in t
worst = 0.0

# ---- (1) random data.  B, H, W, C1, C2, Co, rowadd, residual, alpha[, fused nearest upsample to]
cases = [
    (2, 32, 64, 128, 0, 128, False, False, 1.0),
    (1, 64, 64, 192, 0, 128, True, True, 0.7),           # 3 chunks, rowadd + residual + alpha
    (1, 96, 96, 64, 64, 320, False, True, 1.0),          # ragged last N tile, concat switch on the chunk boundary
    (10, 32, 32, 320, 0, 136, False, False, 1.0),        # 5 chunks, 8 columns in the second N tile
    (1, 8, 512, 128, 0, 128, False, True, 1.0),          # one tile row: padding on every tile
    (17, 8, 32, 128, 0, 128, True, False, 1.0),          # one tile = one image
    (2, 16, 32, 128, 0, 128, False, False, 1.0, (32, 64)),   # fused 2x nearest upsample
]
for dtype in (torch.float16, torch.bfloat16):
    for case in cases:
        (B, H, W, C1, C2, Co, ra, rs, alpha), up = case[:9], (case[9] if len(case) > 9 else None)
        g = torch.Generator().manual_seed(B * 1000 + H * 10 + C1 + Co + W)
        x = q(torch.randn(B, C1, H, W, generator=g), dtype)
        x2 = q(torch.randn(B, C2, H, W, generator=g), dtype) if C2 else None
        w = q(torch.randn(Co, C1 + C2, 3, 3, generator=g) / ((C1 + C2) * 9) ** 0.5, dtype)
        b = q(torch.randn(Co, generator=g), dtype)
        xin = x if x2 is None else torch.cat([x, x2], dim=1)
        if up is not None:
            xin = F.interpolate(xin, size=up, mode="nearest")
        ref = F.conv2d(xin.double(), w.double(), b.double(), stride=1, padding=1).float()
        rav = q(torch.randn(B, Co, generator=g), dtype) if ra else None
        rsv = q(torch.randn(ref.shape, generator=g), dtype) if rs else None
        if rav is not None:
            ref = ref + rav[:, :, None, None]
        ref = ref * alpha
        if rsv is not None:
            ref = ref + rsv
        n0 = launches()
        out = ops.conv2d(nhwc(x, dtype, dev), pack_conv_weight(w, dtype, dev), b.to(dtype).to(dev), Co, 3, 3, 1, (1, 1, 1, 1),
                         x2=None if x2 is None else nhwc(x2, dtype, dev), up_to=up, rowadd=None if rav is None else rav.to(dtype).to(dev),
                         residual=None if rsv is None else nhwc(rsv, dtype, dev), alpha=alpha)
        torch.cuda.synchronize()
        took, t = launches() - n0, tag()
        e = rel_err(to_nchw(out), ref)
        print("%%s conv %%s rel err %%.2e patch=%%d %%s" %% (str(dtype)[6:], (B, H, W, C1, C2, Co, up), e, took, t), flush=True)
        worst = max(worst, e / TOL[dtype])
        assert took == 1 and is16(t), (took, t)
        assert t.endswith(", %%s, false>" %% ("true" if rs else "false")), t
        assert e <= TOL[dtype] and bool(torch.isfinite(out.float()).all()), e

# ---- (2) impulse responses, weights ((3 co + 5 ci + 7 tap) mod 17 - 8) / 16: every value and every output exact in fp16
co, ci, tp = torch.arange(128).view(128, 1, 1), torch.arange(128).view(1, 128, 1), torch.arange(9).view(1, 1, 9)
w = (((3 * co + 5 * ci + 7 * tp) %% 17 - 8).float() / 16.0).reshape(128, 128, 3, 3)
wd = pack_conv_weight(w, torch.float16, dev)
for (py, px) in [(0, 0), (7, 31), (8, 32), (15, 63), (31, 0), (16, 33)]:
    x = torch.zeros(2, 128, 32, 64)
    x[1, 5, py, px] = 1.0
    x[0, 77, 31 - py, 63 - px] = -2.0
    ref = F.conv2d(x.double(), w.double(), None, padding=1).float()
    n0 = launches()
    out = ops.conv2d(nhwc(x, torch.float16, dev), wd, None, 128, 3, 3, 1, (1, 1, 1, 1))
    torch.cuda.synchronize()
    assert launches() - n0 == 1 and is16(tag()), tag()
    assert torch.equal(to_nchw(out).float().cpu(), ref), (py, px)
print("impulse responses exact", flush=True)

# ---- (3) the 2x2-tap variant: the upsampler convolution (1, 16, 32) -> (32, 64), 128 -> 128 as its four parity phases — phase (py, px) is the 2x2 convolution of the
# low-resolution input with pads (1 - py, py, 1 - px, px) whose output is pixel (2 Y + py, 2 X + px); a phase of this problem is two tiles, fewer than e2eft_upconv2x_fwd
# takes by itself, so the phases are launched one by one — against the float64 upsample + 3x3 convolution
_lib.set_option(_lib.OPT_PERSISTENT_MIN_QROUNDS, 1)
for dtype in (torch.float16, torch.bfloat16):
    g = torch.Generator().manual_seed(16 * 7 + 32 + 128)
    conv = torch.nn.Conv2d(128, 128, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(q(torch.randn(conv.weight.shape, generator=g) / (9 * 128) ** 0.5, dtype))
        conv.bias.copy_(q(torch.randn(128, generator=g), dtype))
    x = q(torch.randn(1, 128, 16, 32, generator=g), dtype)
    ref = conv.double()(F.interpolate(x.double(), scale_factor=2.0, mode="nearest")).float()
    conv = conv.float().to(dev)
    wph, bd, xd = AG.phase_conv_weight(conv, dtype), conv.bias.detach().to(dtype), nhwc(x, dtype, dev)
    y = torch.empty((1, 32, 64, 128), dtype=dtype, device=dev)
    for py in range(2):
        for px in range(2):
            n0 = launches()
            yp = ops.conv2d(xd, wph[2 * py + px].contiguous(), bd, 128, 2, 2, 1, (1 - py, py, 1 - px, px))
            t = tag()
            assert launches() - n0 == 1 and is16(t) and t.endswith(", false, false, 2>"), t
            y[:, py::2, px::2, :] = yp
    torch.cuda.synchronize()
    e = rel_err(to_nchw(y), ref)
    print("%%s upconv2x as four 2x2 phases rel err %%.2e %%s" %% (str(dtype)[6:], e, t), flush=True)
    assert e <= TOL[dtype], e
    worst = max(worst, e / TOL[dtype])
_lib.set_option(_lib.OPT_PERSISTENT_MIN_QROUNDS, 8)

# ---- (4) no fused-GroupNorm variant in this form: the fused launch runs, on the 32x32x16 form, and equals GroupNorm + the 32x32x16 plain launch bit for bit
x = nhwc(q(torch.randn(2, 128, 32, 64) * 2.0 + 0.7, torch.float16), torch.float16, dev)
wn = pack_conv_weight(q(torch.randn(128, 128, 3, 3) / 34.0, torch.float16), torch.float16, dev)
ga, be = torch.ones(128, device=dev).half(), torch.zeros(128, device=dev).half()
n0 = launches()
y1 = ops.conv2d(x, wn, None, 128, 3, 3, 1, (1, 1, 1, 1), gn_stats=True, norm=(ga, be, 32, 1e-5, True))
torch.cuda.synchronize()
t = tag()
assert launches() - n0 == 1 and getattr(y1, "_e2eft_keep", None) is not None and t.startswith("igemm6_kernel<") and t.endswith(", true>") and not is16(t), t
_lib.set_option(_lib.OPT_PATCH_MFMA, 1)
y2 = ops.conv2d(ops.groupnorm(x, ga, be, 32, 1e-5, silu=True), wn, None, 128, 3, 3, 1, (1, 1, 1, 1), gn_stats=True)
_lib.set_option(_lib.OPT_PATCH_MFMA, 2)
assert torch.equal(y1, y2) and torch.equal(y1._e2eft_gn.partial, y2._e2eft_gn.partial)
print("fused norm under option 2: %%s" %% t, flush=True)

# ---- (5) statistics: the partials [images, slabs, C, 3] = (n, mean, M2), merged on the host in float64, against the output tensor
def merged(st, B, Co):
    p = st.partial.double().cpu().view(B, st.nslabs, Co, 3)
    n, m, m2 = p[..., 0], p[..., 1], p[..., 2]
    N = n.sum(1)
    mean = (n * m).sum(1) / N
    var = (m2 + n * (m - mean[:, None]) ** 2).sum(1) / N
    return mean, var
for (B, H, W, C1, C2, Co, res) in [(2, 32, 64, 128, 0, 128, False), (1, 96, 96, 64, 64, 320, True)]:
    g = torch.Generator().manual_seed(B + H + Co)
    x = q(torch.randn(B, C1, H, W, generator=g) * 3.0 + 1.5, torch.float16)
    x2 = q(torch.randn(B, C2, H, W, generator=g), torch.float16) if C2 else None
    w = q(torch.randn(Co, C1 + C2, 3, 3, generator=g) / ((C1 + C2) * 9) ** 0.5, torch.float16)
    bb = q(torch.randn(Co, generator=g) * 4.0, torch.float16)
    r = nhwc(q(torch.randn(B, Co, H, W, generator=g) * 2.0 - 5.0, torch.float16), torch.float16, dev) if res else None
    n0 = launches()
    y = ops.conv2d(nhwc(x, torch.float16, dev), pack_conv_weight(w, torch.float16, dev), bb.half().to(dev), Co, 3, 3, 1, (1, 1, 1, 1),
                   x2=None if x2 is None else nhwc(x2, torch.float16, dev), residual=r, gn_stats=True)
    torch.cuda.synchronize()
    assert launches() - n0 == 1 and is16(tag()), tag()
    assert getattr(y, "_e2eft_gn", None) is not None, "no GroupNorm statistics emitted"
    yd = to_nchw(y).double().cpu()
    mean, var = merged(y._e2eft_gn, B, Co)
    mref, vref = yd.mean((2, 3)), yd.var((2, 3), unbiased=False)
    em = ((mean - mref).abs() / vref.sqrt()).max().item()
    ev = ((var - vref).abs() / vref).max().item()
    ga, be = torch.ones(Co, device=dev).half(), torch.zeros(Co, device=dev).half()
    a = ops.groupnorm(y, ga, be, 32, 1e-5, True)
    e1 = rel_err(to_nchw(a), F.silu(F.group_norm(yd, 32, eps=1e-5)).float())
    print("gn partials %%s: mean err %%.2e sigma, var rel err %%.2e, groupnorm on them %%.2e" %% ((B, H, W, C1 + C2, Co, res), em, ev, e1), flush=True)
    assert em < 2e-3 and ev < 2e-3 and e1 < 2e-3      # (the bar of the statistics case in tests/test_patch_conv_gpu.py)

# ---- (6) the two forms against each other
g = torch.Generator().manual_seed(6)
x = q(torch.randn(2, 192, 32, 64, generator=g), torch.float16)
w = q(torch.randn(256, 192, 3, 3, generator=g) / (192 * 9) ** 0.5, torch.float16)
rs = q(torch.randn(2, 256, 32, 64, generator=g), torch.float16)
ref = F.conv2d(x.double(), w.double(), None, padding=1).float()
xd, wd2, rd = nhwc(x, torch.float16, dev), pack_conv_weight(w, torch.float16, dev), nhwc(rs, torch.float16, dev)
for res in (None, rd):
    ys = {}
    for form in (1, 2):
        _lib.set_option(_lib.OPT_PATCH_MFMA, form)
        ya = ops.conv2d(xd, wd2, None, 256, 3, 3, 1, (1, 1, 1, 1), residual=res, gn_stats=True)
        ta = tag()
        yb = ops.conv2d(xd, wd2, None, 256, 3, 3, 1, (1, 1, 1, 1), residual=res, gn_stats=True)
        torch.cuda.synchronize()
        assert ta.startswith("igemm6_kernel<") and is16(ta) == (form == 2), ta
        assert torch.equal(ya, yb) and torch.equal(ya._e2eft_gn.partial, yb._e2eft_gn.partial), "form %%d is not deterministic" %% form
        e = rel_err(to_nchw(ya), ref if res is None else ref + rs)
        assert e <= TOL[torch.float16], (form, e)
        ys[form] = ya
    print("forms 1 / 2 (residual %%d): bit-equal to each other = %%d, rel diff %%.2e" %% (res is not None, torch.equal(ys[1], ys[2]), rel_err(to_nchw(ys[1]), to_nchw(ys[2]).float())), flush=True)

# ---- (7) the planner's invariant under the default option: fused and plain launch of one problem name the same form
_lib.set_option(_lib.OPT_PATCH_MFMA, 0)
for (B, H, W, Cc, Co) in [(2, 32, 64, 128, 128), (4, 32, 32, 192, 128), (17, 8, 32, 128, 64), (5, 8, 512, 320, 128), (2, 32, 64, 128, 256)]:
    g = torch.Generator().manual_seed(B + H + Cc + Co)
    xd = nhwc(q(torch.randn(B, Cc, H, W, generator=g), torch.float16), torch.float16, dev)
    wd3 = pack_conv_weight(q(torch.randn(Co, Cc, 3, 3, generator=g) / (Cc * 9) ** 0.5, torch.float16), torch.float16, dev)
    ga, be = torch.ones(Cc, device=dev).half(), torch.zeros(Cc, device=dev).half()
    n0 = launches()
    yp = ops.conv2d(xd, wd3, None, Co, 3, 3, 1, (1, 1, 1, 1), gn_stats=True)
    tp_ = tag()
    yf = ops.conv2d(xd, wd3, None, Co, 3, 3, 1, (1, 1, 1, 1), gn_stats=True, norm=(ga, be, 32, 1e-5, True))
    tf_ = tag()
    torch.cuda.synchronize()
    assert launches() - n0 == 2 and tp_.startswith("igemm6_kernel<") and tf_.startswith("igemm6_kernel<"), (tp_, tf_)
    print("default forms %%s: plain %%s | through the norm %%s" %% ((B, H, W, Cc, Co), tp_, tf_), flush=True)
    assert is16(tp_) == is16(tf_), (tp_, tf_)
print("MFMA16 CASES PASSED worst %%.2f of tolerance" %% worst)
''' % (HERE, HERE)


def test_patch_kernel_16x16x32_form(dev):
    r = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, env=dict(os.environ), timeout=600)
    print(r.stdout[-8000:])
    assert r.returncode == 0 and "MFMA16 CASES PASSED" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
