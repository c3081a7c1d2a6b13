"""The cases of tests/test_bwd_scale_gpu.py: inputs (the unit-normal, dtype-quantised inputs of tests/test_bwd_gpu.py, same seeds), the float autograd reference of
each case on the CPU, and the runner that sends the case through the public functions of autograd.py the way the model calls them.  No GPU is needed to import
this module or to evaluate a reference: tests/test_scale_harness_cpu.py checks with it that every reference gradient meets the harness's non-vacuity bound.

A case is a Case(dy, outputs, block, zero, reference, runner):
  dy          the incoming gradient (fp32 CPU tensor holding values of the case's dtype, in the layout the device op receives), or a tuple scaled together
  outputs     names of the gradients compared;  zero: those that are analytically zero;  block: see util.assert_backward_scales
  reference() {name: float CPU gradient} from torch autograd of the same op on the same inputs (layout free: only counted)
  runner(F, dev) -> run(dy on the device) -> {name: gradient}"""
import collections
import math

import torch
import torch.nn.functional as TF

from util import q

Case = collections.namedtuple("Case", "dy outputs block zero reference runner")

DTYPES = [torch.bfloat16, torch.float32]          # fp16 packs P and dS to f16, whose subnormals make scaling inexact by construction


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _leaf(t, dtype, dev):
    return t.to(dtype).to(dev).requires_grad_(True)


def _ref(t):
    return t.clone().requires_grad_(True)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _axes(n):
    return tuple(range(n))


# ------------------------------------------------------------------------------------------------ convolution
class _Conv(torch.nn.Conv2d):
    pass


CONV_NAMES = ["3x3 wide", "3x3", "s2 odd", "up2", "up forced", "concat", "conv_out"]


def conv_case(c, dtype):
    """c: an entry of test_bwd_gpu.CONV_CASES"""
    g = _g(len(c["name"]) * 13 + c["c1"])
    cin = c["c1"] + c["c2"]
    B, H, W, co, c1 = c["B"], c["H"], c["W"], c["co"], c["c1"]
    w = q(torch.randn(co, cin, c["k"], c["k"], generator=g) / math.sqrt(cin * c["k"] ** 2), dtype)
    b = q(torch.randn(co, generator=g), dtype)
    x = q(torch.randn(B, cin, H, W, generator=g), dtype)
    hl, wl = c["up"] if c["up"] else (H, W)
    ho = (hl + 2 * c["p"] - c["k"]) // c["s"] + 1
    wo = (wl + 2 * c["p"] - c["k"]) // c["s"] + 1
    rowadd = q(torch.randn(B, co, generator=g), dtype)
    res = q(torch.randn(B, co, ho, wo, generator=g), dtype)
    dy = q(torch.randn(B, co, ho, wo, generator=g), dtype)
    alpha = 0.5

    def reference():
        xr, rr, ar, wr, br = _ref(x), _ref(res), _ref(rowadd), _ref(w), _ref(b)
        xi = TF.interpolate(xr, size=c["up"], mode="nearest") if c["up"] else xr
        (alpha * (TF.conv2d(xi, wr, br, c["s"], c["p"]) + ar[:, :, None, None]) + rr).backward(dy)
        out = dict(dx=xr.grad[:, :c1], dW=wr.grad, dbias=br.grad, drowadd=ar.grad, dres=rr.grad)
        if c["c2"]:
            out["dx2"] = xr.grad[:, c1:]
        return out

    def runner(F, dev):
        xn = _nhwc(x)

        def run(dyd):
            conv = _Conv(cin, co, c["k"], c["s"], c["p"]).to(dev).to(dtype)
            with torch.no_grad():
                conv.weight.copy_(w)
                conv.bias.copy_(b)
            x1 = _leaf(xn[..., :c1].contiguous(), dtype, dev)
            x2 = _leaf(xn[..., c1:].contiguous(), dtype, dev) if c["c2"] else None
            rd, ad = _leaf(_nhwc(res), dtype, dev), _leaf(rowadd, dtype, dev)
            F.conv(conv, x1, x2=x2, up_to=c["up"], rowadd=ad, residual=rd, alpha=alpha).backward(dyd)
            return dict(dx=x1.grad, dx2=None if x2 is None else x2.grad, dW=conv.weight.grad, dbias=conv.bias.grad, drowadd=ad.grad, dres=rd.grad)

        return run

    outputs = ["dx", "dW", "dbias", "drowadd", "dres"] + (["dx2"] if c["c2"] else [])
    block = dict(dx=((0,), (0,)), dx2=((0,), (0,)), dW=((3,), (0,)), dbias=((3,), (0,)), drowadd=((0, 3), (0, 1)), dres=(_axes(4), _axes(4)))
    return Case(_nhwc(dy), outputs, {n: block[n] for n in outputs}, (), reference, runner)


# ------------------------------------------------------------------------------------------------ linear
LINEAR_CASES = [((3, 33), 128, (64, 64, 64)),      # fused q | k | v, transposes + split-K GEMM weight gradient
                ((2,), 10, (128,)),                # K padded to a 16-byte multiple
                ((600,), 320, (200,))]             # M >= 512: the direct weight gradient; N is not a multiple of 64 (dy is zero-extended for dx)


def linear_case(M, K, Ns, dtype):
    g = _g(K + sum(Ns))
    N = sum(Ns)
    ws = [q(torch.randn(n, K, generator=g) / math.sqrt(K), dtype) for n in Ns]
    bias = q(torch.randn(N, generator=g), dtype)
    x = q(torch.randn(*M, K, generator=g), dtype)
    res = q(torch.randn(*M, N, generator=g), dtype)
    dy = q(torch.randn(*M, N, generator=g), dtype)

    def reference():
        xr, rr, br, wr = _ref(x), _ref(res), _ref(bias), _ref(torch.cat(ws, 0))
        (TF.linear(xr, wr, br) + rr).backward(dy)
        return dict(dx=xr.grad, dW=wr.grad, dbias=br.grad, dres=rr.grad)

    def runner(F, dev):
        def run(dyd):
            owner = torch.nn.Module()
            wd = [torch.nn.Parameter(w.to(dtype).to(dev)) for w in ws]
            bd, xd, rd = _leaf(bias, dtype, dev), _leaf(x, dtype, dev), _leaf(res, dtype, dev)
            F.linear(xd, tuple(wd), bd, residual=rd, owner=owner, name="wcat").backward(dyd)
            return dict(dx=xd.grad, dW=torch.cat([p.grad for p in wd], 0), dbias=bd.grad, dres=rd.grad)

        return run

    lead, n = _axes(len(M)), len(M) + 1
    block = dict(dx=(lead, lead), dW=((-1,), (0,)), dbias=((-1,), (0,)), dres=(_axes(n), _axes(n)))
    return Case(dy, list(block), block, (), reference, runner)


# ------------------------------------------------------------------------------------------------ GroupNorm
GROUPNORM_CASES = [(2, 9, 7, 64, 0, 32, True, False),
                   (2, 8, 8, 24, 40, 32, True, False),         # channel concat of two sources
                   (1, 40, 40, 320, 0, 32, True, False),       # several slabs per image
                   (2, 9, 7, 64, 0, 32, True, True)]           # split=True: the skip path's gradient is added inside the backward apply kernel


def groupnorm_case(B, H, W, c1, c2, G, silu, split, dtype):
    g = _g(c1 + c2 + H)
    C = c1 + c2
    x = q(torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3, dtype)
    ga, be = q(1 + 0.2 * torch.randn(C, generator=g), dtype), q(0.2 * torch.randn(C, generator=g), dtype)
    dy = q(torch.randn(B, C, H, W, generator=g), dtype)
    dskip = q(torch.randn(B, C, H, W, generator=g), dtype) if split else None

    def reference():
        xr, gr, br = _ref(x), _ref(ga), _ref(be)
        yr = TF.group_norm(xr, G, gr, br, 1e-5)
        (TF.silu(yr) if silu else yr).backward(dy)
        return dict(dx=xr.grad + dskip if split else xr.grad, dgamma=gr.grad, dbeta=br.grad)

    def runner(F, dev):
        xn = _nhwc(x)

        def run(dyd):
            x1 = _leaf(xn[..., :c1].contiguous(), dtype, dev)
            x2 = _leaf(xn[..., c1:].contiguous(), dtype, dev) if c2 else None
            gd, bd = _leaf(ga, dtype, dev), _leaf(be, dtype, dev)
            if split:
                y, skip = F.groupnorm(x1, gd, bd, G, 1e-5, silu=silu, split=True)
                torch.autograd.backward([y, skip], [dyd[0], dyd[1]])
            else:
                F.groupnorm(x1, gd, bd, G, 1e-5, silu=silu, x2=x2).backward(dyd)
            # the two sources of a concat as one tensor: the blocks are the groups of all C channels
            dx = x1.grad if x2 is None else torch.cat([x1.grad, x2.grad], dim=-1)
            return dict(dx=dx, dgamma=gd.grad, dbeta=bd.grad)

        return run

    per_group = ((0, (3, C // G)), (0, (3, C // G)))
    block = dict(dx=per_group, dgamma=((3,), (0,)), dbeta=((3,), (0,)))
    return Case((_nhwc(dy), _nhwc(dskip)) if split else _nhwc(dy), list(block), block, (), reference, runner)


# ------------------------------------------------------------------------------------------------ LayerNorm / GEGLU / SiLU
ROW_CASES = [((2, 37), 320), ((3, 9), 1280)]
ROW_OPS = ["layernorm", "geglu", "silu"]


def row_case(op, rows, C, dtype):
    g = _g(C)
    x = q(torch.randn(*rows, C, generator=g) * 2 + 0.5, dtype)
    ga, be = q(1 + 0.2 * torch.randn(C, generator=g), dtype), q(0.2 * torch.randn(C, generator=g), dtype)
    dy = q(torch.randn(*rows, C, generator=g), dtype)
    h = q(torch.randn(*rows, 2 * C, generator=g), dtype)
    lead = _axes(len(rows))
    block = dict(dx=(lead, lead))
    if op == "layernorm":
        block.update(dgamma=((-1,), (0,)), dbeta=((-1,), (0,)))

    def reference():
        if op == "layernorm":
            xr, gr, br = _ref(x), _ref(ga), _ref(be)
            TF.layer_norm(xr, (C,), gr, br, 1e-5).backward(dy)
            return dict(dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)
        if op == "geglu":
            hr = _ref(h)
            (hr[..., :C] * TF.gelu(hr[..., C:])).backward(dy)
            return dict(dx=hr.grad)
        xr = _ref(x)
        TF.silu(xr).backward(dy)
        return dict(dx=xr.grad)

    def runner(F, dev):
        def run(dyd):
            if op == "layernorm":
                xd, gd, bd = _leaf(x, dtype, dev), _leaf(ga, dtype, dev), _leaf(be, dtype, dev)
                F.layernorm(xd, gd, bd, 1e-5).backward(dyd)
                return dict(dx=xd.grad, dgamma=gd.grad, dbeta=bd.grad)
            xd = _leaf(h if op == "geglu" else x, dtype, dev)
            (F.geglu(xd) if op == "geglu" else F.silu(xd)).backward(dyd)
            return dict(dx=xd.grad)

        return run

    return Case(dy, list(block), block, (), reference, runner)


# ------------------------------------------------------------------------------------------------ attention
def _attn_ref(q_, k_, v_, heads, scale):
    B, N, C = q_.shape
    d = C // heads
    sp = lambda t: t.view(B, -1, heads, d).transpose(1, 2)
    s = (sp(q_) @ sp(k_).transpose(-1, -2)) * scale
    return (torch.softmax(s, -1) @ sp(v_)).transpose(1, 2).reshape(B, N, C)


# (B, N, L or None for self-attention, heads, d) per dtype: the route each reaches is the default one for that dtype and head dim
ATTENTION_CASES = {
    torch.bfloat16: [(1, 321, None, 2, 64), (2, 100, 77, 2, 64), (1, 129, 257, 3, 64), (1, 50, 1, 1, 64),      # csrc/attn_bwd.hip
                     (2, 64, None, 1, 128), (1, 144, None, 1, 512)],                                           # softmax_bwd_rows + batched GEMMs
    torch.float32: [(1, 130, None, 2, 64), (1, 96, 77, 2, 64),                                                 # csrc/attn32.hip
                    (2, 64, None, 1, 128), (1, 144, None, 1, 512)],
}


def attention_case(B, N, L, heads, d, dtype):
    C = heads * d
    if L is None:
        g = _g(N + d)
        qkv = q(torch.randn(B, N, 3 * C, generator=g), dtype)
        kv = None
    else:
        g = _g(N + L)
        qkv = q(torch.randn(B, N, C, generator=g), dtype)
        kv = q(torch.randn(B, L, 2 * C, generator=g), dtype)
    do = q(torch.randn(B, N, C, generator=g), dtype)

    def reference():
        r = _ref(qkv)
        if kv is None:
            _attn_ref(r[..., :C], r[..., C:2 * C], r[..., 2 * C:], heads, d ** -0.5).backward(do)
            return dict(dq=r.grad[..., :C], dk=r.grad[..., C:2 * C], dv=r.grad[..., 2 * C:])
        kr = _ref(kv)
        _attn_ref(r, kr[..., :C], kr[..., C:], heads, d ** -0.5).backward(do)
        return dict(dq=r.grad, dk=kr.grad[..., :C], dv=kr.grad[..., C:])

    def runner(F, dev):
        def run(dyd):
            x = _leaf(qkv, dtype, dev)
            if kv is None:
                F.attention(x, None, heads, d ** -0.5).backward(dyd)
                return dict(dq=x.grad[..., :C], dk=x.grad[..., C:2 * C], dv=x.grad[..., 2 * C:])
            kd = _leaf(kv, dtype, dev)
            F.attention(x, kd, heads, d ** -0.5).backward(dyd)
            return dict(dq=x.grad, dk=kd.grad[..., :C], dv=kd.grad[..., C:])

        return run

    per_head = ((0, (2, d)), (0, (2, d)))
    block = dict(dq=((0, 1, (2, d)), (0, 1, (2, d))), dk=per_head, dv=per_head)
    zero = ("dq", "dk") if L == 1 else ()      # softmax over one key: P = 1, dS = P (dP - D) = 0 analytically
    return Case(do, list(block), block, zero, reference, runner)


# ------------------------------------------------------------------------------------------------ heads, layout
HEAD_OPS = ["depth_head", "normal_head", "nchw_to_nhwc"]


def head_case(op, dtype):
    g = _g(12)
    x = q(torch.randn(2, 3, 20, 24, generator=g) * 0.8, dtype)
    dy1 = q(torch.randn(2, 1, 20, 24, generator=g), dtype)
    dy3 = q(torch.randn(2, 3, 20, 24, generator=g), dtype)
    pix_nchw, pix_nhwc = (0, 2, 3), (0, 1, 2)

    def reference():
        xr = _ref(x)
        if op == "depth_head":
            torch.clamp(xr.mean(dim=1, keepdim=True), -1, 1).backward(dy1)
        elif op == "normal_head":
            torch.clamp(xr / (torch.norm(xr, p=2, dim=1, keepdim=True) + 1e-5), -1, 1).backward(dy3)
        else:
            xr.permute(0, 2, 3, 1).backward(_nhwc(dy3))
        return dict(dx=xr.grad)

    def runner(F, dev):
        def run(dyd):
            if op == "nchw_to_nhwc":
                xd = _leaf(x, dtype, dev)
                F.nchw_to_nhwc(xd, cpad=xd.shape[1]).backward(dyd)
            else:
                xd = _leaf(_nhwc(x), dtype, dev)
                (F.depth_head(xd) if op == "depth_head" else F.normal_head(xd, clamp=True)).backward(dyd)
            return dict(dx=xd.grad)

        return run

    if op == "nchw_to_nhwc":
        return Case(_nhwc(dy3), ["dx"], dict(dx=(pix_nhwc, pix_nchw)), (), reference, runner)
    return Case(dy1 if op == "depth_head" else dy3, ["dx"], dict(dx=(pix_nchw, pix_nhwc)), (), reference, runner)


def all_cases(conv_cases):
    """(id, dtype, builder) of every case: what the GPU test parametrises over and the CPU pre-check of the references walks"""
    out = []
    for dtype in DTYPES:
        t = str(dtype).split(".")[1]
        by_name = {c["name"]: c for c in conv_cases}
        for name in CONV_NAMES:
            out.append(("conv %s %s" % (name, t), dtype, lambda c=by_name[name], dt=dtype: conv_case(c, dt)))
        for M, K, Ns in LINEAR_CASES:
            out.append(("linear %s %d %s %s" % (M, K, Ns, t), dtype, lambda a=(M, K, Ns), dt=dtype: linear_case(*a, dt)))
        for gc_ in GROUPNORM_CASES:
            out.append(("groupnorm %s %s" % (gc_, t), dtype, lambda a=gc_, dt=dtype: groupnorm_case(*a, dt)))
        for op in ROW_OPS:
            for rows, C in ROW_CASES:
                out.append(("%s %s %d %s" % (op, rows, C, t), dtype, lambda a=(op, rows, C), dt=dtype: row_case(*a, dt)))
        for ac in ATTENTION_CASES[dtype]:
            out.append(("attention %s %s" % (ac, t), dtype, lambda a=ac, dt=dtype: attention_case(*a, dt)))
        for op in HEAD_OPS:
            out.append(("%s %s" % (op, t), dtype, lambda o=op, dt=dtype: head_case(o, dt)))
    return out
