"""The fp32 split route (csrc/f32split.hip) where the magnitudes of the channels differ: what tests/test_f32split_gpu.py cannot see, because its inputs have channels of
one magnitude and util.rel_err divides by the largest entry of the whole tensor.

Weight gradients: dW[co, tap, ci] = sum dY[., co] X[., ci] separates per channel, and AdamW divides every element by its own second moment, so the measure is
util.chan_err_wgrad — the error of every entry against the norms of ITS two columns.  Every case runs on the split route, on the fp32 matrix instruction and in
float64 on the same inputs; the bar is E_split <= max(1.5 E_fp32, E_fp32 of the same shape at r = 0), and today's global bar on top.
Forward and data gradient: the channel is the reduction index there, no rescaling of the result can help, and the per-tensor scale stays; asserted is what the header
of f32split.hip promises per output element: err <= 2^-37 amax(X) sum|w| + 2^-20 sum|x w| + 1.5 err_fp32[channel] (the f16-subnormal absolute term 2^-39 amax with a
factor 4 of slack; 3 * 2^-22 per product rounded up; the accumulation error the fp32 instruction shows on the same inputs).  The per-output-channel relative error of
outputs that are small beside an outlier (util.chan_err_rows) is printed, not asserted: it documents the per-tensor scale's limit.
Stale planes: ops.f32_split2(keep=True) must not return the planes of a buffer that a library kernel has refilled through its raw pointer since.
Subprocess + 8-workgroup grid as tests/test_f32split_gpu.py."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SCRIPT = r'''
import sys, os
HERE = sys.argv[1]
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import ctypes
import torch
import torch.nn.functional as F
from diffusion_e2e_ft_amd import ops, _lib, autograd as ag
from util import nhwc, to_nchw, pack_conv_weight, rel_err, chan_err_wgrad, chan_err_rows
dev = torch.device("cuda:0")
lib = _lib.load()
_lib.set_option(_lib.OPT_PERSISTENT_GRID, 8)
lib.e2eft_debug_last_kernel.restype = ctypes.c_char_p
RS = (0, 12, 20, 24, 30)
failures = []

def last_kernel():
    return lib.e2eft_debug_last_kernel().decode()

def both_routes(fn):
    """fn() on the split route and on the fp32 matrix instruction -> {True: ..., False: ...}"""
    res = {}
    for on in (True, False):
        _lib.set_option(_lib.OPT_F32_SPLIT, int(on))
        res[on] = fn(on)
    _lib.set_option(_lib.OPT_F32_SPLIT, 1)
    return res

# ---- weight gradients per channel.  All tensors NHWC on the host; x is the channel concatenation where there are two sources.
def wgrad_inputs(fam, r, dy0, x0, c1, two):
    dy, x = dy0.clone(), x0.clone()
    if fam in "ac":
        dy[..., 1::2] *= 2.0 ** -r
    if fam in "bc":
        x[..., 3::4] *= 2.0 ** -r
    if fam == "d":
        dy[0, 5, 7, 1] *= 2.0 ** r
    if fam == "e":
        x[-1, 3, 9, 2] *= 2.0 ** r
    if fam == "f":                                   # true dW of the small blocks ~ 2^-70: a normal fp32 value
        dy[..., : dy.shape[-1] // 2] *= 2.0 ** -40
        x[..., : c1 // 2] *= 2.0 ** -30
    if fam == "g":
        dy[..., 3] = 0.0
        x[..., 5] = 0.0
    if two:                                          # the second source 2^-r below the first (f, g: 2^-20)
        x[..., c1:] *= 2.0 ** -(r if fam in "abcde" else 20)
    return dy, x

calls = []
orig_cols = ops.f32_split2_cols
ops.f32_split2_cols = lambda *a, **k: (calls.append(1), orig_cols(*a, **k))[1]
# name, B, H, W, c1, c2, cout, k, stride, pad
shapes = [("3x3 s1", 2, 16, 16, 64, 0, 128, 3, 1, 1), ("1x1", 2, 16, 16, 128, 0, 64, 1, 1, 0), ("3x3 two sources", 2, 16, 16, 64, 64, 64, 3, 1, 1), ("3x3 s2", 1, 16, 32, 64, 0, 64, 3, 2, 1)]
for (name, B, H, W, c1, c2, Co, k, st, pd) in shapes:
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + c1 + c2 + Co + k + st)
    cin = c1 + c2
    Ho, Wo = (H + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
    x0 = torch.randn(B, H, W, cin, generator=g)
    dy0 = torch.randn(B, Ho, Wo, Co, generator=g)
    # which route serves this shape?  conv2d_wgrad asks the 16-bit kernel before it splits anything (ops._wgrad_split_serves); the per-channel split pass is what
    # only the split route launches, so counting its calls shows what a call did
    del calls[:]
    takes = ops._wgrad_split_serves(dy0.to(dev), x0.to(dev), cin, Co, k, k, st, (pd,) * 4)
    if st == 1:
        assert takes, "the split route must take " + name
    if not takes:
        t = ops.conv2d_wgrad(dy0.to(dev), x0[..., :c1].contiguous().to(dev), None, Co, k, k, st, (pd,) * 4, 1.0)
        torch.cuda.synchronize()
        assert t is not None and not calls, "the split route took a shape its own rule refuses"
        print("wgrad %s: the split route does not take this shape (the fp32 instruction served it): no comparison" % name, flush=True)
        continue
    floor = None
    for fam, r in [("a", 0)] + [(f, r) for f in "abcde" for r in RS[1:]] + [("f", 0), ("g", 0)]:
        dy, x = wgrad_inputs(fam, r, dy0, x0, c1, c2 > 0)
        w64 = torch.zeros(Co, cin, k, k, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double().permute(0, 3, 1, 2), w64, None, stride=st, padding=pd).backward(dy.double().permute(0, 3, 1, 2))
        ref = w64.grad.permute(0, 2, 3, 1).reshape(Co, -1)
        dyd, xd = dy.to(dev), x.to(dev)
        xa, xb = (xd[..., :c1].contiguous(), xd[..., c1:].contiguous()) if c2 else (xd, None)
        def run(on):
            t = ops.conv2d_wgrad(dyd, xa, xb, Co, k, k, st, (pd,) * 4, 1.0)
            torch.cuda.synchronize()
            assert t is not None
            return t.double().cpu()
        del calls[:]
        rs = both_routes(run)
        assert len(calls) == 2, "split route: one per-channel split of dY and one of X, none on the fp32 instruction (%d)" % len(calls)
        E1, E2 = chan_err_wgrad(rs[True], ref, dy, x, k * k), chan_err_wgrad(rs[False], ref, dy, x, k * k)
        e1, e2 = rel_err(rs[True], ref), rel_err(rs[False], ref)
        if floor is None:
            floor = E2                               # the fp32 instruction's own error on this shape at r = 0
        ok = torch.isfinite(rs[True]).all().item() and E1 <= max(1.5 * E2, floor) and e1 <= max(1.5 * e2, 4e-7)
        if fam == "g":
            got = rs[True].view(Co, k * k, cin)
            ok = ok and float(got[3].abs().max()) == 0.0 and float(got[:, :, 5].abs().max()) == 0.0
        if fam == "f":                               # the small block is there: not flushed, not overflowed
            blk = rs[True].view(Co, k * k, cin)[: Co // 2, :, : c1 // 2]
            ok = ok and float(blk.abs().max()) > 0.0
        print("wgrad %s (%s) r=%d: per channel %.3e (fp32 MFMA %.3e, floor %.3e), global %.3e (%.3e)  %s" % (name, fam, r, E1, E2, floor, e1, e2, "ok" if ok else "FAIL"), flush=True)
        if not ok:
            failures.append("wgrad %s (%s) r=%d" % (name, fam, r))

ops.f32_split2_cols = orig_cols

# ---- forward and data gradient: the per-tensor scale's promise, per output element
def promise(what, got_s, got_f, ref, amax, W1, A):
    """got_s / got_f / ref / A channels-last, W1 per output channel"""
    es, ef = (got_s - ref).abs(), (got_f - ref).abs()
    c = ref.shape[-1]
    bound = 2.0 ** -37 * amax * W1 + 2.0 ** -20 * A + 1.5 * ef.reshape(-1, c).max(0).values
    ok = torch.isfinite(got_s).all().item() and (es <= bound).all().item()
    print("%s: worst err / bound %.3f; per output channel %.3e (fp32 MFMA %.3e), global %.3e (%.3e)  %s" % (
        what, (es / bound.clamp_min(1e-300)).max().item(), chan_err_rows(got_s, ref), chan_err_rows(got_f, ref), rel_err(got_s, ref), rel_err(got_f, ref), "ok" if ok else "FAIL"), flush=True)
    if not ok:
        failures.append(what)

def outliers(t, fam, r):
    """t channels-last: (b) every fourth channel shrunk, (e) one element raised"""
    t = t.clone()
    if fam == "b":
        t[..., 3::4] *= 2.0 ** -r
    else:
        t[-1, 3, 9, 2] *= 2.0 ** r
    return t

g = torch.Generator().manual_seed(77)
B, H, W, Cc, Co = 2, 16, 32, 128, 128
x0 = torch.randn(B, H, W, Cc, generator=g)
gy0 = torch.randn(B, H, W, Co, generator=g)
w0 = torch.randn(Co, Cc, 3, 3, generator=g) / (Cc * 9) ** 0.5
for zero_w in (False, True):
    for fam in "be":
        for r in RS:
            if zero_w and r < 20:
                continue
            w = w0.clone()
            if zero_w:                               # the second half of the outputs does not see the large input channels: those outputs are small
                big = torch.ones(Cc, dtype=torch.bool)
                if fam == "b":
                    big[3::4] = False
                else:
                    big[:] = False
                    big[2] = True
                w[Co // 2:, big] = 0.0
            # forward
            x = outliers(x0, fam, r)
            ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), None, padding=1).permute(0, 2, 3, 1)
            A = F.conv2d(x.double().abs().permute(0, 3, 1, 2), w.double().abs(), None, padding=1).permute(0, 2, 3, 1)
            xd, wd = x.to(dev), pack_conv_weight(w, torch.float32, dev)
            def fwd(on):
                y = ops.conv2d(xd, wd, None, Co, 3, 3, 1, (1, 1, 1, 1))
                torch.cuda.synchronize()
                kk = last_kernel()
                assert ("f32split" in kk and "igemm6" in kk) if on else ("float" in kk and "f32split" not in kk), kk
                return y.double().cpu()
            ys = both_routes(fwd)
            promise("conv3x3 forward%s (%s) r=%d" % (" zero weights" if zero_w else "", fam, r), ys[True], ys[False], ref, x.abs().max().item(), w.double().abs().sum((1, 2, 3)), A)
            if zero_w:
                continue
            # data gradient through autograd with frozen weights: the same families on dY
            gy = outliers(gy0, fam, r)
            conv = torch.nn.Conv2d(Cc, Co, 3, padding=1).to(dev)
            with torch.no_grad():
                conv.weight.copy_(w)
            conv.weight.requires_grad_(False); conv.bias.requires_grad_(False)
            x64 = x0.double().permute(0, 3, 1, 2).requires_grad_(True)
            F.conv2d(x64, w.double(), None, padding=1).backward(gy.double().permute(0, 3, 1, 2))
            refg = x64.grad.permute(0, 2, 3, 1)
            Ag = F.conv_transpose2d(gy.double().abs().permute(0, 3, 1, 2), w.double().abs(), None, padding=1).permute(0, 2, 3, 1)
            def bwd(on):
                xq = x0.to(dev).requires_grad_(True)
                ag.conv(conv, xq).backward(gy.to(dev))
                torch.cuda.synchronize()
                assert ("f32split" in last_kernel()) == on, last_kernel()
                return xq.grad.double().cpu()
            gs = both_routes(bwd)
            promise("conv3x3 data gradient (%s) r=%d" % (fam, r), gs[True], gs[False], refg, gy.abs().max().item(), w.double().abs().sum((0, 2, 3)), Ag)

Mr, K, N = 512, 128, 64
_lib.set_option(_lib.OPT_PERSISTENT_MIN_QROUNDS, 1)      # two 256-row tiles on the 8-workgroup grid: a quarter round (the default asks for half a round before igemm5 takes a launch)
a0 = torch.randn(Mr, K, generator=g)
wl0 = torch.randn(N, K, generator=g) / K ** 0.5
for zero_w in (False, True):
    for fam in "be":
        for r in RS:
            if zero_w and r < 20:
                continue
            a, wl = a0.clone(), wl0.clone()
            if fam == "b":
                a[:, 3::4] *= 2.0 ** -r
            else:
                a[37, 2] *= 2.0 ** r
            if zero_w:
                big = torch.ones(K, dtype=torch.bool)
                if fam == "b":
                    big[3::4] = False
                else:
                    big[:] = False
                    big[2] = True
                wl[N // 2:, big] = 0.0
            ref = a.double() @ wl.double().t()
            A = a.double().abs() @ wl.double().abs().t()
            ad, wld = a.to(dev), wl.to(dev)
            def lin(on):
                y = ops.gemm(ad, wld)
                torch.cuda.synchronize()
                assert ("f32split" in last_kernel()) == on, last_kernel()
                return y.double().cpu()
            ys = both_routes(lin)
            promise("gemm M%d K%d N%d%s (%s) r=%d" % (Mr, K, N, " zero weights" if zero_w else "", fam, r), ys[True], ys[False], ref, a.abs().max().item(), wl.double().abs().sum(1), A)

_lib.set_option(_lib.OPT_PERSISTENT_MIN_QROUNDS, 2)

# ---- planes parked on a tensor (keep=True) against writes the tensor's version counter does not see
def refills():
    yield "copy_scale", lambda x, y: ops.copy_scale(y, x, mul=1.0)
    yield "add(out=)", lambda x, y: ops.add(y, torch.zeros_like(y), out=x)
    yield "cast_", lambda x, y: ops.cast_(y.contiguous().view(-1), x.view(-1))
for what, refill in refills():
    x = torch.randn(1, 8, 32, 64, generator=g).to(dev)
    y = (torch.randn(1, 8, 32, 64, generator=g) * 37.0).to(dev)          # another maximum: another scale
    p1, s1 = ops.f32_split2(x, keep=True)
    p1b, s1b = ops.f32_split2(x, keep=True)
    shared = p1b is p1 and s1b is s1                                     # nothing was written: the planes are shared
    refill(x, y)
    p2, s2 = ops.f32_split2(x, keep=True)
    p3, s3 = ops.f32_split2(x.clone())
    torch.cuda.synchronize()
    ok = shared and torch.equal(x, y) and torch.equal(p2, p3) and s2[1].item() == s3[1].item()
    print("planes kept on a tensor refilled by %s: shared while unwritten %s, fresh afterwards %s  %s" % (what, shared, torch.equal(p2, p3) and s2[1].item() == s3[1].item(), "ok" if ok else "FAIL"), flush=True)
    if not ok:
        failures.append("stale planes after " + what)

assert not failures, "%d FAILED: %s" % (len(failures), "; ".join(failures))
print("F32SPLIT RANGE CASES PASSED")
'''


def test_f32split_range(dev):
    r = subprocess.run([sys.executable, "-c", SCRIPT, HERE], capture_output=True, text=True, env=dict(os.environ), timeout=900)
    print(r.stdout[-30000:])
    assert r.returncode == 0 and "F32SPLIT RANGE CASES PASSED" in r.stdout, (r.stdout[-6000:], r.stderr[-3000:])
