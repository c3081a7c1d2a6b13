"""The d = 64 attention kernels (csrc/attn.hip forward in both K / V deliveries, csrc/attn_bwd.hip, and the fp32 routes csrc/attn32.hip / csrc/attn_f32split.hip)
per ROW against float64, on inputs that drive the deferred rescale of the reference maximum and on logits of standard deviation 1 ... 16 nats.

References, metric and bars are tests/attn_model.py's (read its docstring): truth = float64 softmax attention of the T-rounded inputs; E_T = error of the plain
same-dtype form on the same inputs; row_err = max over (image, head, row) of max_d |x - truth| / max_d |truth|.
    outputs and gradients   row_err(kernel) <= 2 E_T
    base-2 lse              |lse - truth| <= log2(1 + u) + 2^-17 max_{q,k} sum_d |c q_d k_d|, per (image, head)
The inputs are shown on the CPU to fail a kernel whose rescale is wrong (tests/test_attn_model_cpu.py: a model of the kernel with alpha = 1 for O or for l misses
the output bar by more than 10 x on every input here that moves the reference), and the model of the kernels' arithmetic measures <= 1.2 E_T for O and <= 1.6 E_T
for every gradient, in either of its two metrics, on exactly these inputs.  Both deliveries (E2EFT_OPT_ATTN_DMA = 0 / 1) run every 16-bit case and must agree bit for bit."""
import pytest
import torch

import attn_model as am

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
_ids = lambda d: str(d).replace("torch.", "")


def _route(on):
    from diffusion_e2e_ft_amd import _lib
    return _lib.option(_lib.OPT_F32_SPLIT_ATTN, int(on))


@pytest.fixture(scope="module")
def fwd_cases():
    """{dtype: {name: (heads, truth O, truth lse2, E_T, lse bars)}}: every reference once"""
    return {dt: {name: (heads,) + am.forward_refs(heads, dt) for name, heads in am.forward_cases(dt).items()} for dt in DTYPES}


def _both_deliveries(fn):
    from diffusion_e2e_ft_amd import _lib
    with _lib.option(_lib.OPT_ATTN_DMA, 0):
        o0, l0 = fn()
    with _lib.option(_lib.OPT_ATTN_DMA, 1):
        o1, l1 = fn()
    torch.cuda.synchronize()
    assert torch.equal(o0, o1) and torch.equal(l0, l1), ((o0.float() - o1.float()).abs().max().item(), (l0 - l1).abs().max().item())
    return o1, l1


def _check_forward(what, o, lse, truth_o, truth_lse, e_t, bars):
    """o [B, N, H * 64], lse [B, H, N] from the kernel"""
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all(), what
    err = am.row_err(am.unpack(o), truth_o)
    lerr = (lse.double().cpu().reshape(truth_lse.shape) - truth_lse).abs().max(dim=1).values
    print("%s: O row err %.3e = %.2f E_T (E_T %.3e) | lse err / bar per head %s" % (what, err, err / e_t, e_t, " ".join("%.2f" % r for r in (lerr / bars).tolist())))
    assert err <= 2.0 * e_t, (what, err, e_t)
    assert bool((lerr <= bars).all()), (what, lerr.tolist(), bars.tolist())


def _dev3(heads, dtype, dev):
    return (am.pack([h[i] for h in heads]).to(dtype).to(dev) for i in range(3))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", list(am.RESCALE_FAMILIES) + ["spread_%d" % s for s in am.SPREADS])
def test_forward_per_row(dev, fwd_cases, dtype, name):
    """families 1 - 4: a late key with a moderate lead (as the issue builds it, with leads that also move wave 1 and move wave 0 twice, and in a partial
    last tile), scores creeping up by 3.0 / 5.9 / 6.1 per tile, a strongly negative first
    tile (about -6.5 and about -160 in the exponent domain), the logit-spread sweep"""
    from diffusion_e2e_ft_amd import ops
    heads, *refs = fwd_cases[dtype][name]
    q, k, v = _dev3(heads, dtype, dev)
    o, lse = _both_deliveries(lambda: ops.attention(q, k, v, am.H, am.SCALE, return_lse=True))
    _check_forward("%s %s" % (name, _ids(dtype)), o, lse, *refs)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", ["late_key_partial_tile", "spread_8"])
def test_forward_per_row_joint_keys(dev, fwd_cases, dtype, name):
    """the same keys as the two segments of a joint call (kv_nseg = 2, kv_bmod = 1: 150 / 224 keys per segment, the late key 290 in segment 1): both images
    attend to image 0's keys"""
    from diffusion_e2e_ft_amd import ops
    heads = fwd_cases[dtype][name][0]
    heads = [(q, heads[i % am.H][1], heads[i % am.H][2]) for i, (q, _, _) in enumerate(heads)]      # image 1: its own queries on image 0's keys
    refs = am.forward_refs(heads, dtype)
    q, k, v = _dev3(heads, dtype, dev)
    half = k.shape[1] // 2
    kj, vj = (torch.cat([t[:1, :half], t[:1, half:]], dim=0).contiguous() for t in (k, v))
    o, lse = _both_deliveries(lambda: ops.attention(q, kj, vj, am.H, am.SCALE, kv_nseg=2, kv_bmod=1, return_lse=True))
    _check_forward("joint %s %s" % (name, _ids(dtype)), o, lse, *refs)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_forward_per_row_fused_qkv_views(dev, dtype):
    """spread 8 through column views of one fused q|k|v projection (N = Nk = 192)"""
    from diffusion_e2e_ft_amd import ops
    heads = am.heads_of(lambda seed, dt: am.spread(seed, dt, 8, N=192, Nk=192), dtype, seed0=10)
    refs = am.forward_refs(heads, dtype)
    C = am.H * 64
    qkv = torch.cat([am.pack([h[i] for h in heads]) for i in range(3)], dim=2).to(dtype).to(dev)
    o, lse = _both_deliveries(lambda: ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], am.H, am.SCALE, return_lse=True))
    _check_forward("fused views spread_8 %s" % _ids(dtype), o, lse, *refs)


@pytest.mark.parametrize("split", [False, True], ids=["attn32", "f32split"])
@pytest.mark.parametrize("sigma", am.SPREADS)
def test_forward_per_row_fp32_routes(dev, split, sigma):
    """family 5: the sweep in fp32 on the strict route and on the split route (E2EFT_OPT_F32_SPLIT_ATTN), E_T from the plain form in fp32, u = 2^-24"""
    from diffusion_e2e_ft_amd import ops
    heads = am.heads_of(lambda seed, dt: am.spread(seed, dt, sigma), torch.float32)
    refs = am.forward_refs(heads, torch.float32)
    q, k, v = _dev3(heads, torch.float32, dev)
    with _route(split):
        o, lse = ops.attention(q, k, v, am.H, am.SCALE, return_lse=True)
        tag = ops._last_kernel()
    torch.cuda.synchronize()
    assert ("f32split" in tag) == split and ("attn32" in tag) != split, tag
    _check_forward("fp32 %s spread_%d" % ("split" if split else "strict", sigma), o, lse, *refs)


@pytest.fixture(scope="module")
def bwd_cases():
    return {dt: {name: (heads, dos, self_attn) + am.backward_refs(heads, dos, dt) for name, (heads, dos, self_attn) in am.backward_cases(dt).items()} for dt in DTYPES}


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", am.BACKWARD_NAMES)
def test_backward_per_row(dev, bwd_cases, dtype, name):
    """family 6: autograd.attention on the sweep as self-attention (fused q|k|v, N = Nk = 192) and as cross-attention (q + fused k|v, N = 128, Nk = 448) and on
    family 1 (cross, Nk = 320), dO ~ randn: dQ per query row, dK and dV per key row against float64 autograd, bar 2 E_T, in TWO metrics.
    row_err (a row's error over that row's own maximum) is a check at spread 1 and on family 1 (E_T 7e-4 ... 5e-2) and for dV in bf16; at spread >= 4 the
    float64 dQ / dK of near-one-hot rows is about 0 and E_T in this metric is 0.03 ... 2e6: there its bar passes a zero gradient.  head_err (a row's error
    over the largest row maximum of its (image, head)) has E_T 3e-4 ... 1.4e-3 in fp16 and 3e-3 ... 1e-2 in bf16 in EVERY case, asserted <= 0.05 here; a zero
    gradient scores 1.0 in it, and the single-rounded backward 3 - 18 E_T at spread 16 (tests/test_attn_model_cpu.py pins both).  The CPU model of the kernels'
    arithmetic (c applied to the fp32 score, forward and backward) measures at most 1.29 / 1.24 / 1.47 E_T (dQ / dK / dV) in row_err and 1.32 / 1.24 / 1.54 E_T
    in head_err over these cases in both dtypes (asserted <= 2 there), so no gradient needs the wider model-derived bar."""
    from diffusion_e2e_ft_amd import autograd as F
    heads, dos, self_attn, truth, e_t, e_t_head = bwd_cases[dtype][name]
    q, k, v = _dev3(heads, dtype, dev)
    do = am.pack(dos).to(dtype).to(dev)
    C = am.H * 64
    if self_attn:
        qkv = torch.cat([q, k, v], dim=2).requires_grad_(True)
        F.attention(qkv, None, am.H, am.SCALE).backward(do)
        grads = (qkv.grad[..., :C], qkv.grad[..., C:2 * C], qkv.grad[..., 2 * C:])
    else:
        qq, kv = q.clone().requires_grad_(True), torch.cat([k, v], dim=2).requires_grad_(True)
        F.attention(qq, kv, am.H, am.SCALE).backward(do)
        grads = (qq.grad, kv.grad[..., :C], kv.grad[..., C:])
    torch.cuda.synchronize()
    errs = [am.row_err(am.unpack(g), t) for g, t in zip(grads, truth)]
    herrs = [am.head_err(am.unpack(g), t) for g, t in zip(grads, truth)]
    print("%s %s: dq dk dv row err / E_T %s (E_T %s) | head err / E_T %s (E_T %s)" % (name, _ids(dtype), " ".join("%.2f" % (e / t) for e, t in zip(errs, e_t)),
          " ".join("%.2e" % t for t in e_t), " ".join("%.2f" % (e / t) for e, t in zip(herrs, e_t_head)), " ".join("%.2e" % t for t in e_t_head)))
    for what, e, t, he, ht, g in zip(("dq", "dk", "dv"), errs, e_t, herrs, e_t_head, grads):
        assert torch.isfinite(g.float()).all(), what
        assert ht <= 0.05, (what, ht)               # the bar below is a real one
        assert he <= 2.0 * ht, (what, he, ht)
        assert e <= 2.0 * t, (what, e, t)
