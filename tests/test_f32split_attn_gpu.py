"""fp32 fused attention from two-term f16 splits (csrc/attn_f32split.hip, E2EFT_OPT_F32_SPLIT_ATTN = 1) beside the strict fp32 route (csrc/attn32.hip, the default)
on the same inputs, both against float64: forward + base-2 lse, backward, a 2^10 range spread, strided q|k|v views, GeoWizard's joint keys (declined: they stay on
attn32), the autograd function, determinism / graph capture, zeros and extremes.  The per-case bars are tests/test_attn32_gpu.py's (the project's bars for this
operation); the pooled bar — worst error over all cases <= 2 x attn32's worst over the same cases, measured in the same run — has margin 2 because a CPU emulation of
the scheme puts the pooled ratio at 0.8 - 1.4 from rounding noise alone; case-by-case ratios are noise (up to 4.7 x in either direction) and are not asserted."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as TF

from util import chan_err_rows, rel_err

pytestmark = pytest.mark.gpu
TOL_FWD, TOL_LSE, TOL_BWD = 2e-5, 2e-5, 1e-4
FWD_SHAPES = [(2, 5, 144, 144), (1, 2, 300, 300), (3, 1, 128, 129), (2, 3, 576, 2), (1, 5, 200, 77), (2, 2, 96, 193), (1, 4, 64, 1280), (1, 1, 1, 1)]
BWD_SHAPES = [(2, 5, 144, 144), (1, 2, 300, 300), (2, 1, 130, 65), (1, 3, 64, 2), (1, 2, 96, 77), (1, 1, 257, 448)]


@contextlib.contextmanager
def route(on):
    from diffusion_e2e_ft_amd import _lib
    _lib.set_option(_lib.OPT_F32_SPLIT_ATTN, int(on))
    try:
        yield
    finally:
        _lib.set_option(_lib.OPT_F32_SPLIT_ATTN, 0)


def _tag():
    from diffusion_e2e_ft_amd import ops
    return ops._last_kernel()


def _sp(t, heads):
    return t.reshape(t.shape[0], t.shape[1], heads, 64).transpose(1, 2)


def _ref(q, k, v, heads, scale):
    o = TF.scaled_dot_product_attention(_sp(q.double(), heads), _sp(k.double(), heads), _sp(v.double(), heads), scale=scale)
    return o.transpose(1, 2).reshape(q.shape)


def _ref_lse2(q, k, heads, scale):
    s = torch.einsum("bhqd,bhkd->bhqk", _sp(q.double(), heads), _sp(k.double(), heads)) * scale
    return torch.logsumexp(s, dim=-1) / math.log(2.0)


def _fwd_both(dev, q, k, v, heads, scale):
    """{route: (out, lse, tag)} on the same device tensors"""
    from diffusion_e2e_ft_amd import ops
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    res = {}
    for on in (True, False):
        with route(on):
            o, lse = ops.attention(qd, kd, vd, heads, scale, return_lse=True)
            tag = _tag()
        torch.cuda.synchronize()
        res[on] = (o, lse, tag)
    return res


def _bwd_both(dev, q, k, v, do, heads, scale):
    """{route: (dq, dk, dv, tag, out)}: each route's backward from its own forward"""
    from diffusion_e2e_ft_amd import ops
    qd, kd, vd, dod = q.to(dev), k.to(dev), v.to(dev), do.to(dev)
    res = {}
    for on in (True, False):
        with route(on):
            o, lse = ops.attention(qd, kd, vd, heads, scale, return_lse=True)
            gq, gk, gv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
            ops.attention_bwd(qd, kd, vd, o, dod, lse, heads, scale, gq, gk, gv)
            tag = _tag()
        torch.cuda.synchronize()
        res[on] = (gq, gk, gv, tag, o)
    return res


@pytest.fixture(scope="module")
def forward_runs(dev):
    """every forward case once, both routes: {shape: {route: (err O, err lse, tag)}}"""
    runs = {}
    scale = 64 ** -0.5
    for B, heads, N, Nk in FWD_SHAPES:
        g = torch.Generator().manual_seed(N * 3 + Nk)
        C = heads * 64
        q, k, v = (torch.randn(B, n, C, generator=g) for n in (N, Nk, Nk))
        q[0, 0] *= 4.0                                   # a sharp row: the running maximum moves late
        want, want_lse = _ref(q, k, v, heads, scale), _ref_lse2(q, k, heads, scale)
        res = _fwd_both(dev, q, k, v, heads, scale)
        runs[(B, heads, N, Nk)] = {on: (rel_err(o, want), (lse.double().cpu() - want_lse).abs().max().item(), tag) for on, (o, lse, tag) in res.items()}
        print("fwd %s: O split %.3e attn32 %.3e | lse split %.3e attn32 %.3e" % ((B, heads, N, Nk), runs[(B, heads, N, Nk)][True][0], runs[(B, heads, N, Nk)][False][0],
                                                                                   runs[(B, heads, N, Nk)][True][1], runs[(B, heads, N, Nk)][False][1]))
    return runs


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_forward_and_lse_against_float64(forward_runs, shape):
    split, strict = forward_runs[shape][True], forward_runs[shape][False]
    assert "f32split" in split[2] and "attn32" not in split[2], split[2]
    assert "attn32" in strict[2] and "f32split" not in strict[2], strict[2]
    assert split[0] <= TOL_FWD, split
    assert split[1] <= TOL_LSE, split


def test_forward_pooled_error_against_attn32(forward_runs):
    for i, what in ((0, "O"), (1, "lse")):
        split = max(r[True][i] for r in forward_runs.values())
        strict = max(r[False][i] for r in forward_runs.values())
        print("fwd pooled %s: split %.3e attn32 %.3e ratio %.2f" % (what, split, strict, split / strict))
        assert split <= 2.0 * strict, (what, split, strict)


@pytest.fixture(scope="module")
def backward_runs(dev):
    runs = {}
    scale = 64 ** -0.5
    for B, heads, N, Nk in BWD_SHAPES:
        g = torch.Generator().manual_seed(N + 7 * Nk)
        C = heads * 64
        q, k, v = (torch.randn(B, n, C, generator=g) for n in (N, Nk, Nk))
        do = torch.randn(B, N, C, generator=g)
        qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
        _ref(qd, kd, vd, heads, scale).backward(do.double())
        res = _bwd_both(dev, q, k, v, do, heads, scale)
        runs[(B, heads, N, Nk)] = {on: (rel_err(r[0], qd.grad), rel_err(r[1], kd.grad), rel_err(r[2], vd.grad), r[3]) for on, r in res.items()}
        print("bwd %s: dq/dk/dv split %.3e %.3e %.3e | attn32 %.3e %.3e %.3e" % (((B, heads, N, Nk),) + runs[(B, heads, N, Nk)][True][:3] + runs[(B, heads, N, Nk)][False][:3]))
    return runs


@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_backward_against_float64_autograd(backward_runs, shape):
    split, strict = backward_runs[shape][True], backward_runs[shape][False]
    assert "f32split" in split[3] and "attn32" not in split[3], split[3]
    assert "attn32" in strict[3] and "f32split" not in strict[3], strict[3]
    for i, name in enumerate(("dq", "dk", "dv")):
        assert split[i] <= TOL_BWD, (name, split[i])


def test_backward_pooled_error_against_attn32(backward_runs):
    for i, name in enumerate(("dq", "dk", "dv")):
        split = max(r[True][i] for r in backward_runs.values())
        strict = max(r[False][i] for r in backward_runs.values())
        print("bwd pooled %s: split %.3e attn32 %.3e ratio %.2f" % (name, split, strict, split / strict))
        assert split <= 2.0 * strict, (name, split, strict)


def test_range_per_channel(dev):
    """one query row and one key row 2^10 above the rest, the channels of V and dO spread geometrically over 2^10: errors of O, dV and dK per head channel, relative
    to that channel's own maximum.  2^10 lies inside the 2^17 window in which every scale of the route keeps 22 bits."""
    g = torch.Generator().manual_seed(21)
    N, heads, scale = 300, 1, 0.125
    q, k, v, do = (torch.randn(1, N, 64, generator=g) for _ in range(4))
    q[0, 17] *= 1024.0
    k[0, 201] *= 1024.0
    spread = torch.pow(2.0, torch.linspace(0.0, 10.0, 64))
    v *= spread
    do *= spread.flip(0)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    want = _ref(qd, kd, vd, heads, scale)
    want.backward(do.double())
    res = _bwd_both(dev, q, k, v, do, heads, scale)
    err = {on: {"O": chan_err_rows(r[4], want), "dV": chan_err_rows(r[2], vd.grad), "dK": chan_err_rows(r[1], kd.grad)} for on, r in res.items()}
    print("range: split %s | attn32 %s" % (err[True], err[False]))
    assert "f32split" in res[True][3] and "attn32" in res[False][3]
    for name in ("O", "dV", "dK"):
        assert err[True][name] <= 2.0 * err[False][name], (name, err[True][name], err[False][name])
    assert max(err[True].values()) <= 2.0 * max(err[False].values())


def test_strided_views_leave_the_other_columns_alone(dev):
    """q, k, v as column slices of one [B, N, 3C] projection (two of the projection's three heads are attended to), dq, dk, dv and out written into slices of buffers of
    the same shape: the columns outside the slices keep their bytes"""
    from diffusion_e2e_ft_amd import ops
    g = torch.Generator().manual_seed(5)
    B, heads, N, C = 2, 2, 320, 192
    W = heads * 64
    qkv = torch.randn(B, N, 3 * C, generator=g)
    do = torch.randn(B, N, W, generator=g)
    sl = [slice(i * C, i * C + W) for i in range(3)]
    d = qkv.to(dev)
    dqkv = torch.full((B, N, 3 * C), -7.25, device=dev)
    obuf = torch.full((B, N, 3 * C), -7.25, device=dev)
    with route(True):
        o, lse = ops.attention(d[..., sl[0]], d[..., sl[1]], d[..., sl[2]], heads, 0.125, out=obuf[..., sl[1]], return_lse=True)
        assert "f32split" in _tag()
        ops.attention_bwd(d[..., sl[0]], d[..., sl[1]], d[..., sl[2]], o, do.to(dev), lse, heads, 0.125, dqkv[..., sl[0]], dqkv[..., sl[1]], dqkv[..., sl[2]])
        assert "f32split" in _tag()
    torch.cuda.synchronize()
    qd, kd, vd = (qkv[..., s].double().requires_grad_(True) for s in sl)
    want = _ref(qd, kd, vd, heads, 0.125)
    want.backward(do.double())
    assert rel_err(obuf[..., sl[1]], want) <= TOL_FWD
    for s, t in zip(sl, (qd, kd, vd)):
        assert rel_err(dqkv[..., s], t.grad) <= TOL_BWD
    keep = torch.ones(3 * C, dtype=torch.bool)
    for s in sl:
        keep[s] = False
    assert (dqkv[..., keep.to(dev)] == -7.25).all()
    keep[:] = True
    keep[sl[1]] = False
    assert (obuf[..., keep.to(dev)] == -7.25).all()


def test_joint_keys_stay_on_attn32(dev):
    """GeoWizard's joint attention (kv_nseg = 2; 200 keys per segment, tiles span the boundary) is declined: with the option on the launch goes to
    attn32 and the result is the option-off result bit for bit"""
    import ctypes as C_
    from diffusion_e2e_ft_amd import _lib, ops
    g = torch.Generator().manual_seed(6)
    Bh, Nj, heads = 2, 200, 2
    C = heads * 64
    q, k, v = (torch.randn(2 * Bh, Nj, C, generator=g).to(dev) for _ in range(3))
    with route(True):
        dsc = ops._attn_desc(q, k, v, q, heads, 0.125, 2, Bh)
        took = _lib.load().e2eft_attn_f32split_supported(C_.byref(dsc), 0)
        on = ops.attention(q, k, v, heads, 0.125, kv_nseg=2, kv_bmod=Bh)
        tag = _tag()
    off = ops.attention(q, k, v, heads, 0.125, kv_nseg=2, kv_bmod=Bh)
    torch.cuda.synchronize()
    kj = torch.cat([torch.cat([k[:Bh], k[Bh:]], dim=1)] * 2, dim=0)
    vj = torch.cat([torch.cat([v[:Bh], v[Bh:]], dim=1)] * 2, dim=0)
    assert rel_err(on, _ref(q.cpu(), kj.cpu(), vj.cpu(), heads, 0.125)) <= TOL_FWD
    if took == 1:
        assert "f32split" in tag
    else:
        assert "attn32" in tag and "f32split" not in tag, tag
        assert torch.equal(on, off)


def test_autograd_function_takes_the_route(dev):
    """autograd.attention on packed self-attention qkv and on cross-attention q + kv with the option on: fused families only, the split kernels' tags, output and all
    gradients within 1e-5 of the tensor maximum of the option-off run"""
    from diffusion_e2e_ft_amd import autograd as F, ops
    g = torch.Generator().manual_seed(11)
    B, heads, N, L = 2, 5, 200, 77
    C = heads * 64
    for kv_len in (None, L):
        qkv0 = torch.randn(B, N, 3 * C if kv_len is None else C, generator=g).to(dev)
        kv0 = None if kv_len is None else torch.randn(B, kv_len, 2 * C, generator=g).to(dev)
        do = torch.randn(B, N, C, generator=g).to(dev)
        res = {}
        for on in (True, False):
            with route(on):
                try:
                    qkv = qkv0.clone().requires_grad_(True)
                    kv = None if kv0 is None else kv0.clone().requires_grad_(True)
                    timer = ops.KernelTimer()
                    ops.TIMER = timer
                    o = F.attention(qkv, kv, heads, 0.125)
                    tag_f = _tag()
                    o.backward(do)
                    tag_b = _tag()
                    torch.cuda.synchronize()
                finally:
                    ops.TIMER = None
                fams = set(k for k, v_ in timer.summary().items() if v_["launches"])
                res[on] = (o.detach(), qkv.grad, None if kv is None else kv.grad, fams, tag_f, tag_b)
        for on in (True, False):
            assert "attn" in res[on][3] and "attn_bwd" in res[on][3] and "igemm" not in res[on][3], res[on][3]
        assert "f32split" in res[True][4] and "f32split" in res[True][5], res[True][4:]
        assert "attn32" in res[False][4] and "attn32" in res[False][5], res[False][4:]
        for a, b_ in zip(res[True][:3], res[False][:3]):
            if a is not None:
                assert rel_err(a, b_) <= 1e-5, rel_err(a, b_)


def test_deterministic_and_graph_capturable(dev):
    from diffusion_e2e_ft_amd import ops
    g = torch.Generator().manual_seed(31)
    B, heads, N = 1, 2, 300
    C = heads * 64
    q, k, v, do = (torch.randn(B, N, C, generator=g).to(dev) for _ in range(4))

    def step():
        o, lse = ops.attention(q, k, v, heads, 0.125, return_lse=True)
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ops.attention_bwd(q, k, v, o, do, lse, heads, 0.125, gq, gk, gv)
        return o, lse, gq, gk, gv

    with route(True):
        first = step()
        assert "f32split" in _tag()
        second = step()
        torch.cuda.synchronize()
        for a, b_ in zip(first, second):
            assert torch.equal(a, b_)
        s_ = torch.cuda.Stream()                 # warm-up on a side stream, as torch asks before a capture
        s_.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s_):
            step()
        torch.cuda.current_stream().wait_stream(s_)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            captured = step()
        assert "f32split" in _tag()
        for t in captured:
            t.fill_(float("nan"))
        gr.replay()
        torch.cuda.synchronize()
        for a, b_ in zip(first, captured):
            assert torch.equal(a, b_)


def test_zeros_and_extremes_stay_finite(dev):
    from diffusion_e2e_ft_amd import ops
    B, heads, N, Nk = 1, 2, 70, 130
    C = heads * 64
    g = torch.Generator().manual_seed(41)
    do = torch.randn(B, N, C, generator=g).to(dev)
    with route(True):
        for fill, dout in ((0.0, torch.zeros_like(do)), (3.0e30 * 2.0 ** -64, do), (1.0e-30, do)):
            q = torch.full((B, N, C), fill, device=dev)
            k = torch.full((B, Nk, C), fill, device=dev)
            v = torch.full((B, Nk, C), fill, device=dev)
            o, lse = ops.attention(q, k, v, heads, 0.125, return_lse=True)
            assert "f32split" in _tag()
            gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
            ops.attention_bwd(q, k, v, o, dout, lse, heads, 0.125, gq, gk, gv)
            torch.cuda.synchronize()
            for t in (o, lse, gq, gk, gv):
                assert torch.isfinite(t).all(), fill
            # every key of a row scores the same: a uniform row, O = v (sum_i p_i) / l.  p and v each carry a split error <= 2^-22, the fp32 row sum of 130
            # terms at most 130 x 2^-24: 2 x 2^-22 + 130 x 2^-24 = 8.2e-6 in the worst case
            assert (o.double() - fill).abs().max().item() <= 1e-5 * abs(fill), fill
            if fill == 0.0:
                assert (o == 0).all() and (gq == 0).all() and (gk == 0).all() and (gv == 0).all()
                assert (lse.double() - math.log2(Nk)).abs().max().item() <= 2e-5
