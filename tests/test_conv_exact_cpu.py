"""tests/conv_exact_cases.py against a plain fp32 CPU convolution evaluated in two summation orders — the whole K in one call, and 64-channel chunks summed in
reverse — for every variant (base, large-sum, one-rounding, the split-K contract, the split-plane construction): both orders must pass, and each injected fault (one
dropped 8-channel chunk, one border row that reads the pixel beyond the pad, a bias shifted by one column in the last N tile, a 16-bit accumulator on the large-sum
variant) must fail with the channel, row and tile counts of the entries it really touches."""
import re

import pytest
import torch
import torch.nn.functional as F

import conv_exact_cases as X

DTYPES = [torch.float16, torch.bfloat16, torch.float32]
GEOM = dict(B=2, H=16, W=16, c1=128, cout=136)          # M = 512: two 256-row tiles; K = 1152; two N tiles of 128, the last one 8 wide


def _case(dtype, variant, **kw):
    args = dict(GEOM, bias=True, rowadd=True, residual=True, alpha=0.5, variant=variant)
    args.update(kw)
    c = X.exact_conv_case(dtype, **args)
    assert c is not None
    return c


def _acc32(c, order, x=None, w=None, acc_dtype=torch.float32, pad_from_neighbour=None):
    """fp32 accumulators [B, cout, Ho, Wo] of the case: order "whole" (one F.conv2d over all of K) or "chunks" (64-channel chunks, last chunk first, summed one by one in
    acc_dtype).  pad_from_neighbour = b: image b's top padding row holds image b - 1's last row (what a flat row index one short of the pad check reads)."""
    x = (c.x if c.x2 is None else torch.cat([c.x, c.x2], 1)) if x is None else x
    w = c.w if w is None else w
    if c.up_to is not None:
        x = F.interpolate(x, size=tuple(c.up_to), mode="nearest")
    p = c.pad
    xin = F.pad(x, (p[2], p[3], p[0], p[1])).float()
    if pad_from_neighbour is not None:
        b = pad_from_neighbour
        xin[b, :, 0, p[2]: xin.shape[3] - p[3]] = x[b - 1, :, -1, :].float()
    w = w.float()
    if order == "whole":
        return F.conv2d(xin, w, stride=c.stride)
    acc = None
    for c0 in reversed(range(0, x.shape[1], 64)):
        part = F.conv2d(xin[:, c0: c0 + 64], w[:, c0: c0 + 64], stride=c.stride).to(acc_dtype)
        acc = part if acc is None else (acc + part).to(acc_dtype)
    return acc.float()


def _epilogue32(c, acc, bias=None):
    """out = alpha (acc + bias + rowadd) + residual in fp32, one operation at a time, rounded to the output type; NHWC"""
    bias = c.bias if bias is None else bias
    t = acc
    if bias is not None:
        t = t + bias.float().view(1, -1, 1, 1)
    if c.rowadd is not None:
        t = t + c.rowadd.float().view(t.shape[0], -1, 1, 1)
    t = t * torch.tensor(c.alpha, dtype=torch.float32)
    if c.residual is not None:
        t = t + c.residual.float()
    return t.to(c.dtype).permute(0, 2, 3, 1).contiguous()


def _counts(msg):
    m = re.search(r"(\d+) entries in (\d+) of \d+ output channels, (\d+) of \d+ image rows, (\d+) of \d+ 256-row tiles", msg)
    assert m, msg
    return dict(zip(("entries", "channels", "rows", "tiles"), map(int, m.groups())))


def _footprint(got, want):
    """the same counts, taken directly from the two tensors"""
    bad = got != want
    pix = bad.any(3).reshape(-1).nonzero().reshape(-1)
    return dict(entries=int(bad.sum()), channels=int(bad.any(0).any(0).any(0).sum()), rows=int(bad.any(3).any(2).sum()), tiles=len(set((pix // 256).tolist())))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ["whole", "chunks"])
@pytest.mark.parametrize("variant", X.VARIANTS)
def test_both_summation_orders_pass_every_variant(dtype, order, variant):
    c = _case(dtype, variant)
    X.check(c.name, _epilogue32(c, _acc32(c, order)), c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("order", ["whole", "chunks"])
@pytest.mark.parametrize("geom", [dict(stride=2), dict(pad=(0, 1, 0, 1), stride=2), dict(up_to=(32, 32), B=1), dict(up_to=(24, 40), B=1), dict(c1=64, c2=64), dict(k=1, c1=192),
                                  dict(k=2, pad=(1, 0, 0, 1))])
def test_every_geometry_is_exact_in_both_orders(dtype, order, geom):
    c = _case(dtype, "base", **geom)
    X.check(c.name, _epilogue32(c, _acc32(c, order)), c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", X.VARIANTS)
def test_split_k_contract(dtype, variant):
    """partials per row of filter taps, rounded to the output type, summed in fp32: equal to the plain expectation while the partials are small integers (base), a
    different — and for 16-bit types inexact — number on the large-sum variant, where it is the model that must be met"""
    c = _case(dtype, variant, c1=256, cout=128, B=2, H=12, W=12)
    model = X.splitk_expect(c)
    if variant == "base":
        X.assert_exact(c.name, model, c.expect)
    elif variant == "round1":
        X.assert_one_rounding(c.name, model, c)
    elif dtype == torch.float32:
        X.assert_exact(c.name, model, c.expect)
    else:
        assert not torch.equal(model, c.expect), "rounded partials must show on the large-sum variant"
        err = (model.double() - c.expect.double()).abs() / X.ulp(c.expect.double(), dtype)
        assert err.max().item() <= 4        # three partials rounded at 64 x the output's magnitude-per-ulp ... still only a few output ulp


@pytest.mark.parametrize("order", ["whole", "chunks"])
def test_split_plane_construction(order):
    """x = a + b 2^-13, w = c + d 2^-13: the planes are (a s, b 2^-13 s) exactly, the route's three-block sum is sum ac + 2^-13 sum (ad + bc), and fp32 convolutions of the
    planes give it bit for bit in either order; the plain product would add the b d 2^-26 terms the route drops"""
    c = _case(torch.float32, "base", planes=True, rowadd=False, alpha=1.0)
    x0, x1, sx = X.split_planes(c.x)
    a = c.x.round()
    assert sx == 2.0 ** 14 and torch.equal(x0, a * sx) and torch.equal(x1, (c.x - a) * sx)
    assert torch.equal(c.acc, c.acc_formula)
    w0, w1, sw = X.split_planes(c.w)
    acc = (_acc32(c, order, x0, w0) + _acc32(c, order, x0, w1) + _acc32(c, order, x1, w0)) * torch.tensor(1.0 / (sx * sw), dtype=torch.float32)
    X.check(c.name, _epilogue32(c, acc), c)
    assert not torch.equal(F.conv2d(F.pad(c.x, (1, 1, 1, 1)), c.w), c.acc)


def test_fused_norm_operand_is_a_small_integer():
    c = _case(torch.float16, "base", norm=True, cout=128)
    assert c.operand.abs().max().item() <= 4 and torch.equal(c.operand, c.operand.round())
    a, mean = c.coeff[..., 0], c.coeff[..., 1]
    k = c.beta.view(1, -1) - mean * a
    assert set(k.abs().unique().tolist()) <= {0.0, 1.0, 2.0} and set(a.unique().tolist()) == {1.0, 2.0}
    assert len(mean.unique()) > 2 and not torch.equal(mean[0], mean[1])          # the coefficients differ between the images


# ---- injected faults ----------------------------------------------------------------------------------------------------------------------------------------
def _expect_failure(c, got):
    with pytest.raises(AssertionError) as e:
        X.check(c.name, got, c)
    return str(e.value)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_dropped_8_channel_chunk_is_found(dtype):
    """channels 40..47 of tap (0, 2) are left out of the second 256-row tile (image 1): 8 of the 1152 terms"""
    c = _case(dtype, "base")
    acc = _acc32(c, "whole")
    x_only = torch.zeros_like(c.x)
    x_only[1, 40:48] = c.x[1, 40:48]
    w_only = torch.zeros_like(c.w)
    w_only[:, :, 0, 2] = c.w[:, :, 0, 2]
    got = _epilogue32(c, acc - _acc32(c, "whole", x_only, w_only))
    msg = _expect_failure(c, got)
    n, want = _counts(msg), _footprint(got, c.expect)
    assert n == want, (n, want)
    assert n["tiles"] == 1 and "tiles [1]" in msg and n["rows"] <= 16 and n["channels"] > 64


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_border_row_that_reads_beyond_the_pad_is_found(dtype):
    """the top padding row of image 1 holds the last row of image 0: exactly one image row of outputs, the first of the second tile, is wrong"""
    c = _case(dtype, "base")
    got = _epilogue32(c, _acc32(c, "chunks", pad_from_neighbour=1))
    msg = _expect_failure(c, got)
    n = _counts(msg)
    assert n == _footprint(got, c.expect)
    assert n["rows"] == 1 and n["tiles"] == 1 and "tiles [1]" in msg and "first (b, y, x, co): [(1, 0, " in msg and n["channels"] > 100


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_bias_shifted_by_one_column_in_the_last_n_tile_is_found(dtype):
    """columns 128..135 (the ragged second N tile) take bias[n - 1]: only those channels differ, in every row and tile"""
    c = _case(dtype, "base")
    bias = c.bias.clone()
    bias[128:] = c.bias[127:-1]
    changed = int((bias != c.bias).sum())
    assert 0 < changed <= 8
    got = _epilogue32(c, _acc32(c, "whole"), bias=bias)
    msg = _expect_failure(c, got)
    n = _counts(msg)
    assert n == _footprint(got, c.expect)
    assert n["channels"] == changed and n["rows"] == 32 and n["tiles"] == 2 and n["entries"] == changed * 512
    first = re.search(r"first \(b, y, x, co\): \[\(0, 0, 0, (\d+)\)", msg)
    assert first and int(first.group(1)) >= 128, msg


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_a_16_bit_accumulator_fails_the_large_sum_variant(dtype):
    c = _case(dtype, "large")
    ok = _epilogue32(c, _acc32(c, "chunks"))
    X.check(c.name, ok, c)
    if dtype == torch.float16:
        # fp16 cannot hold 2^16: keep the accumulator in range by summing alpha-scaled chunks — still a 16-bit running sum
        w = c.w * c.alpha
        acc = _acc32(c, "chunks", w=w, acc_dtype=dtype) / c.alpha
    else:
        acc = _acc32(c, "chunks", acc_dtype=dtype)
    got = _epilogue32(c, acc)
    msg = _expect_failure(c, got)
    n = _counts(msg)
    assert n == _footprint(got, c.expect) and n["tiles"] == 2 and n["channels"] == 136
    # ... and a T-rounded intermediate fails the one-rounding variant while the fp32 epilogue passes it
    r = _case(dtype, "round1")
    acc = _acc32(r, "whole")
    t = ((acc + r.bias.float().view(1, -1, 1, 1) + r.rowadd.float().view(2, -1, 1, 1)) * torch.tensor(r.alpha, dtype=torch.float32)).to(dtype).float() + r.residual.float()
    with pytest.raises(AssertionError, match="beyond one rounding"):
        X.check(r.name, t.to(dtype).permute(0, 2, 3, 1).contiguous(), r)


def test_large_variant_declines_short_reductions_and_ulp_is_right():
    assert X.exact_conv_case(torch.float16, 2, 16, 16, 8, 128, variant="large") is None            # K = 72
    assert X.exact_gemm_case(torch.float16, 129, 129, 72, variant="large") is None
    assert X.exact_gemm_case(torch.float16, 64, 64, 256, variant="large") is None and X.exact_gemm_case(torch.float16, 64, 64, 320, variant="large") is not None
    t = torch.tensor([1.0, 1.5, 2.0, 0.75, 100.0, 0.0, 2.0 ** -20], dtype=torch.float64)
    assert X.ulp(t, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -4, 2.0 ** -24, 2.0 ** -24]
    assert X.ulp(t, torch.bfloat16)[:5].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -1]
    assert X.ulp(t, torch.float32)[:2].tolist() == [2.0 ** -23, 2.0 ** -23]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", X.VARIANTS)
def test_gemm_and_dgrad_cases(dtype, variant):
    c = X.exact_gemm_case(dtype, 129, 129, 512, bias=True, residual=True, alpha=0.5, variant=variant)
    out = (c.a.float() @ c.w.float().t())
    if c.bias is not None:
        out = out + c.bias.float()
    out = out * torch.tensor(c.alpha, dtype=torch.float32)
    if c.residual is not None:
        out = out + c.residual.float()
    X.check(c.name, out.to(dtype), c)
    d = X.exact_dgrad_case(dtype, 2, 16, 16, 64, 128, variant=variant)
    if variant == "large":
        assert d is None            # some input pixels of a stride-2 3x3 receive one tap only
        return
    x = torch.zeros(2, 64, 16, 16, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, d.w, None, stride=2, padding=1).backward(d.dy)
    assert torch.equal(x.grad, d.acc)
    # the flipped, transposed packing: a stride-1 convolution of the zero-inserted dy
    dyz = torch.zeros(2, 128, 16, 16, dtype=torch.float64)
    dyz[:, :, ::2, ::2] = d.dy
    wf = d.w_dgrad.view(64, 3, 3, 128).permute(0, 3, 1, 2)
    assert torch.equal(F.conv2d(F.pad(dyz, (1, 1, 1, 1)), wf)[:, :, :16, :16], d.acc)
