"""Integer-valued convolution / GEMM cases whose result does not depend on the order of summation (tests/test_conv_exact_cpu.py, tests/test_conv_exact_gpu.py).

With operands that are small integers every product and every partial sum of the contraction is an integer below 2^24: fp32 accumulation is exact whatever the tile
shape, the k order, the MFMA form or the split of K, and the output of ANY correct kernel equals the float64 reference bit for bit.  No tolerance is chosen anywhere.

  base      x, x2, w in {-1, 0, +1} (density 1/4 for K >= 1152, 1/2 below), bias and rowadd integers in [-8, 8], residual integers in [-16, 16], alpha 1 or 0.5.
            Checked here, on the reference: max |accumulator| and max |output| <= 128 (half-integers are then exact in bf16, and so is a split-K partial rounded to
            the output type) and at least util.NON_VACUOUS of the outputs are non-zero.
  large     x in {lo..3}, w in {lo..7}, no bias / rowadd / residual, alpha = 2^-6: every accumulator lies in [2^12, 2^16] (checked here) — exact in fp32, in no 16-bit
            accumulator.  Expected: acc * alpha rounded ONCE to the output type.  The lower ends `lo` rise with the shortest reduction of the case (a corner pixel of a
            padded 3x3 sees 4/9 of K) until that pixel stays above 2^12 by six standard deviations; a case whose shortest reduction cannot (K_min < 320) has no large variant.
  round1    integer operands, alpha = 0.7 (as the fp32 value the C ABI carries), residual in multiples of 1/8: only the epilogue rounds.  Per element
                |out - ref| <= ulp_T(ref) / 2 + 4 * 2^-24 * (|acc alpha| + |bias alpha| + |rowadd alpha| + |res|)
            — one rounding to T plus up to four fp32 roundings of the epilogue's terms; an epilogue that rounds an intermediate through T (2^-11 / 2^-8) breaks it.

Split-K (e2eft_conv2d_fwd_splitk) has an arithmetic contract of its own: one partial per row of filter taps rounded to T, summed in fp32 by splitk_finish_kernel, then
the epilogue and one more rounding: splitk_expect() models that.  The fp32 split-plane route (csrc/f32split.hip) sums x0 w0 + x0 w1 + x1 w0 of the two-term f16 planes
and drops x1 w1 by design: split_planes() / the `planes` cases model that; with x = a + b 2^-13, w = c + d 2^-13 (a, c in {-1, 0, 1}; b, d in {-1, 0, 1} where a, c are not
zero) the planes are x0 = a s, x1 = b 2^-13 s exactly and the expected sum is  sum a c + 2^-13 sum (a d + b c).

Tensors are float64 on the CPU, activations NCHW, weights OIHW; `expect` is NHWC in the output type."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import util

MAX_MAG = 128.0
LARGE_ALPHA, LARGE_LO, LARGE_HI = 2.0 ** -6, 2.0 ** 12, 2.0 ** 16
ROUND1_ALPHA = torch.tensor(0.7, dtype=torch.float32).item()      # 0.7 as the C ABI's float carries it
VARIANTS = ("base", "large", "round1")
PLANE_EPS = 2.0 ** -13
_LARGE_LADDER = ((0, 0), (1, 0), (1, 2), (2, 4), (2, 5))         # (lowest x, lowest w): mean product 5.25, 7, 9, 13.75, 15 — never a constant operand
_MANT = {torch.float16: 11, torch.bfloat16: 8, torch.float32: 24}
_EMIN = {torch.float16: -14, torch.bfloat16: -126, torch.float32: -126}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ternary(shape, density, g):
    """entries in {-1, 0, +1}: non-zero with probability `density`, either sign equally likely"""
    shape = tuple(shape)
    on = torch.rand(shape, generator=g) < density
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (on * sign).double()


def integers(shape, lo, hi, g, step=1.0):
    """uniform integers in [lo, hi] times `step`"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double() * step


def ulp(ref, dtype):
    """spacing of `dtype` at the magnitude of every entry of the float64 tensor `ref` (the subnormal spacing below the smallest normal)"""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -140))            # |ref| = m 2^e, m in [0.5, 1)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 1).clamp_min(_EMIN[dtype]).double() - (_MANT[dtype] - 1))


def _round_to(t64, dtype):
    """float64 -> dtype through fp32 (every value rounded here is exact in fp32, so this is ONE rounding)"""
    return t64.to(torch.float32).to(dtype)


def _logical_input(x, x2, up_to):
    xin = x if x2 is None else torch.cat([x, x2], dim=1)
    if up_to is not None:
        xin = F.interpolate(xin, size=tuple(up_to), mode="nearest")
    return xin


def _draw(variant, shapes_x, shape_w, kfull, kmin, g, density):
    """operands of one variant -> (list of x tensors, w), or None when the large variant cannot reach 2^12 on the shortest reduction"""
    if variant == "large":
        for lx, lw in _LARGE_LADDER:
            # mean and variance of one product x w, x uniform on {lx..3}, w on {lw..7}: the shortest reduction must stay above 2^12 by six standard deviations
            ex, ex2 = (lx + 3) / 2.0, sum(v * v for v in range(lx, 4)) / (4.0 - lx)
            ew, ew2 = (lw + 7) / 2.0, sum(v * v for v in range(lw, 8)) / (8.0 - lw)
            if kmin * ex * ew - 6.0 * (kmin * (ex2 * ew2 - (ex * ew) ** 2)) ** 0.5 >= LARGE_LO:
                break
        else:
            return None
        return [integers(s, lx, 3, g) for s in shapes_x], integers(shape_w, lw, 7, g)
    if density is None:
        density = 0.25 if kfull >= 1152 else 0.5
    return [ternary(s, density, g) for s in shapes_x], ternary(shape_w, density, g)


def _finish(c, acc, bias_b, rowadd_b, res):
    """c: the case so far (variant, dtype, alpha); acc float64; bias_b / rowadd_b broadcast against acc, or None; res like acc, or None.  Fills ref, expect (or
    bound) and asserts the conditions that make the case exact and non-vacuous on the reference itself."""
    zero = torch.zeros((), dtype=torch.float64)
    b, r, s = (bias_b if bias_b is not None else zero), (rowadd_b if rowadd_b is not None else zero), (res if res is not None else zero)
    c.acc = acc
    c.ref = c.alpha * (acc + b + r) + s
    c.bound = None
    if c.variant == "large":
        assert bias_b is None and rowadd_b is None and res is None and c.alpha == LARGE_ALPHA
        lo, hi = acc.min().item(), acc.max().item()
        assert LARGE_LO <= lo and hi <= LARGE_HI, "%s: large-sum accumulators span [%g, %g], wanted [2^12, 2^16]" % (c.name, lo, hi)
    else:
        m = acc.abs().max().item()
        assert m <= MAX_MAG, "%s: max |accumulator| %g > 128" % (c.name, m)
    if c.variant == "round1":
        c.bound = ulp(c.ref, c.dtype) / 2 + 4 * 2.0 ** -24 * ((acc * c.alpha).abs() + (b * c.alpha).abs() + (r * c.alpha).abs() + s.abs()).expand_as(c.ref)
        c.expect = None
    else:
        c.expect = _round_to(c.ref, c.dtype)
        if c.variant == "base":
            m = c.ref.abs().max().item()
            assert m <= MAX_MAG, "%s: max |output| %g > 128" % (c.name, m)
            assert torch.equal(c.expect.double(), c.ref), "%s: the reference is not representable in %s" % (c.name, c.dtype)
    f = util.nonzero_fraction(c.ref)
    assert f >= util.NON_VACUOUS, "%s: only %.1f %% of the reference outputs are non-zero" % (c.name, 100 * f)
    return c


def _epilogue_operands(c, B, cout, out_shape, g, bias, rowadd, residual):
    """the variant's bias [cout], rowadd [B, cout] and residual (NCHW, out_shape): None where the variant or the caller has none"""
    if c.variant == "large":
        c.bias = c.rowadd = c.residual = None
        return
    c.bias = integers((cout,), -8, 8, g) if bias else None
    c.rowadd = integers((B, cout), -8, 8, g) if rowadd else None
    if not residual:
        c.residual = None
    elif c.variant == "round1":
        c.residual = integers(out_shape, -128, 128, g, step=0.125)          # multiples of 1/8 in [-16, 16]: exact in bf16
    else:
        c.residual = integers(out_shape, -16, 16, g)


def _alpha(variant, alpha):
    assert alpha in (1.0, 0.5)
    return {"base": alpha, "large": LARGE_ALPHA, "round1": ROUND1_ALPHA}[variant]


def exact_conv_case(dtype, B, H, W, c1, cout, k=3, stride=1, pad=None, c2=0, up_to=None, bias=True, rowadd=False, residual=False, alpha=1.0, variant="base",
                    seed=0, density=None, planes=False, norm=False, w_density=None, name=None):
    """A forward convolution of [B, c1 (+ c2), H, W] (read through a nearest upsample to up_to = (hl, wl)) with k x k taps, pad = (top, bottom, left, right) -> the
    case, or None when the variant does not exist for this geometry (see the module's text).  planes (fp32): the two-plane construction of the split route; the
    reference is then the route's three-block sum."""
    pad = tuple(pad) if pad is not None else (k // 2,) * 4
    g = gen(seed * 7919 + B * 1000 + H * 10 + W + c1 * 3 + c2 + cout + k)
    c = SimpleNamespace(name=name or "conv B%d %dx%d %d+%d->%d k%d s%d %s" % (B, H, W, c1, c2, cout, k, stride, variant), variant=variant, dtype=dtype,
                        alpha=_alpha(variant, alpha), k=k, stride=stride, pad=pad, up_to=up_to, cout=cout, planes=planes, nchw=True)
    cin = c1 + c2
    hl, wl = (H, W) if up_to is None else up_to
    taps = F.conv2d(F.pad(torch.ones(1, 1, hl, wl, dtype=torch.float64), (pad[2], pad[3], pad[0], pad[1])), torch.ones(1, 1, k, k, dtype=torch.float64), stride=stride)
    ops_ = _draw(variant, [(B, c1, H, W)] + ([(B, c2, H, W)] if c2 else []), (cout, cin, k, k), k * k * cin, int(taps.min().item()) * cin, g, density)
    if ops_ is None:
        return None
    xs, c.w = ops_
    c.x, c.x2 = xs[0], (xs[1] if c2 else None)

    def conv(xa, xb, w):
        return F.conv2d(F.pad(_logical_input(xa, xb, up_to), (pad[2], pad[3], pad[0], pad[1])), w, stride=stride)

    c.coeff = c.beta = None
    if norm:
        # The operand is read through GroupNorm's affine map n = (x - mean) a + beta with hand-made coefficients: a in {1, 2} and an integer mean per (image, channel),
        # integer beta per channel, no SiLU — n = x a + k is again a small integer, |n| <= 4.  k = beta - mean a is kept in {0, +-1, +-2}: the kernels evaluate
        # fma(x, a log2e, k log2e) * ln2 (common.h), which is an exact zero where n = 0 only if k log2e needs no rounding, i.e. k is zero or a power of two; every
        # other n comes out as n (1 + O(2^-23)) and rounds to n in the 16-bit operand type.
        assert c2 == 0 and variant != "large"
        c.beta = integers((c1,), -2, 2, g)
        a = integers((B, c1), 1, 2, g)
        odd = (c.beta % 2 != 0).expand(B, c1)
        k2 = torch.where(odd, integers((B, c1), 0, 1, g) * 2 - 1, integers((B, c1), -1, 1, g) * 2)
        kk = torch.where(a == 1, integers((B, c1), -1, 1, g), k2)
        mean = (c.beta.view(1, -1) - kk) / a
        assert torch.equal(mean, mean.round())
        c.coeff = torch.stack([a, mean], dim=2)                              # [B][C][(a, mean)]
        c.operand = (c.x - mean.view(B, c1, 1, 1)) * a.view(B, c1, 1, 1) + c.beta.view(1, c1, 1, 1)
        assert c.operand.abs().max().item() <= 4
        c.w = ternary(c.w.shape, 0.125 if w_density is None else w_density, g)
        acc = conv(c.operand, None, c.w)
    elif planes:
        assert dtype == torch.float32 and variant != "large"
        a_x, a_x2, a_w = c.x, c.x2, c.w
        c.x = a_x + (a_x != 0) * integers(a_x.shape, -1, 1, g) * PLANE_EPS
        c.x2 = None if a_x2 is None else a_x2 + (a_x2 != 0) * integers(a_x2.shape, -1, 1, g) * PLANE_EPS
        c.w = a_w + (a_w != 0) * integers(a_w.shape, -1, 1, g) * PLANE_EPS
        acc = split_conv_model(c, conv)
        # exact in fp32 in any order: every partial sum is a multiple of 2^-13 bounded by the sum of the terms' magnitudes
        mag = conv(a_x.abs(), None if a_x2 is None else a_x2.abs(), a_w.abs()).max().item() * (1 + 2 * PLANE_EPS)
        assert mag / PLANE_EPS < 2.0 ** 24, "%s: partial sums may need more than 24 bits (%g)" % (c.name, mag)
        c.acc_formula = conv(a_x, a_x2, a_w) + (conv(a_x, a_x2, c.w - a_w) + conv(c.x - a_x, None if a_x2 is None else c.x2 - a_x2, a_w))
    else:
        acc = conv(c.x, c.x2, c.w)
    _epilogue_operands(c, B, cout, acc.shape, g, bias, rowadd, residual)
    _finish(c, acc, None if c.bias is None else c.bias.view(1, -1, 1, 1), None if c.rowadd is None else c.rowadd.view(B, cout, 1, 1), c.residual)
    if c.expect is not None:
        c.expect = c.expect.permute(0, 2, 3, 1).contiguous()
    return c


def split_planes(t):
    """the two-term f16 split of e2eft_f32_split2 / e2eft_f32_split_weight: (t0, t1, s) with s the power of two that brings max |t| into [2^14, 2^15), t0 = f16(t s),
    t1 = f16(t s - t0), as float64"""
    m = t.abs().max().item()
    if m == 0:
        return t.clone(), t.clone(), 1.0
    _, e = torch.frexp(torch.tensor(m, dtype=torch.float64))
    s = 2.0 ** (15 - int(e.item()))
    t0 = (t * s).to(torch.float16).double()
    t1 = (t * s - t0).to(torch.float16).double()
    return t0, t1, s


def split_conv_model(c, conv):
    """the split route's contract on the case's operands: (x0 w0 + x0 w1 + x1 w0) / (s_x s_w); the two sources share one scale"""
    xcat = c.x if c.x2 is None else torch.cat([c.x, c.x2], dim=1)
    x0, x1, sx = split_planes(xcat)
    w0, w1, sw = split_planes(c.w)
    n1 = c.x.shape[1]
    cut = (lambda t: (t[:, :n1], t[:, n1:])) if c.x2 is not None else (lambda t: (t, None))
    return (conv(*cut(x0), w0) + conv(*cut(x0), w1) + conv(*cut(x1), w0)) / (sx * sw)


def splitk_expect(c):
    """e2eft_conv2d_fwd_splitk's contract on a stride-s k x k case: one partial per ROW of filter taps rounded to T (the first pass writes its partials in the output
    type), the partials summed in fp32 in row order, bias and rowadd added in fp32, then fma(sum, alpha, residual) rounded to T -> NHWC tensor in the output type"""
    pad, k, st = c.pad, c.k, c.stride
    xin = F.pad(_logical_input(c.x, c.x2, c.up_to), (pad[2], pad[3], pad[0], pad[1]))
    hout = (xin.shape[2] - k) // st + 1
    acc = None
    for ky in range(k):
        part = F.conv2d(xin[:, :, ky: ky + (hout - 1) * st + 1, :], c.w[:, :, ky: ky + 1, :], stride=st)
        part = _round_to(part, c.dtype).to(torch.float32)
        acc = part if acc is None else acc + part
    if c.bias is not None:
        acc = acc + c.bias.float().view(1, -1, 1, 1)
    if c.rowadd is not None:
        acc = acc + c.rowadd.float().view(acc.shape[0], -1, 1, 1)
    out = acc.double() * c.alpha                                           # (fp32 x fp32: exact in float64)
    if c.residual is not None:
        out = out + c.residual
    return _round_to(out, c.dtype).permute(0, 2, 3, 1).contiguous()


def exact_dgrad_case(dtype, B, H, W, cin, cout, k=3, stride=2, pad=1, variant="base", alpha=1.0, seed=0):
    """The data gradient of a k x k / stride / pad convolution [B, cin, H, W] -> cout (H, W multiples of the stride), i.e. the zero-insertion route of
    e2eft_conv2d_dgrad: dy ternary [B, cout, H / stride, W / stride], w ternary; reference: conv_transpose2d in float64.  c.w_dgrad: [cin, (ky, kx, co)] with flipped
    taps, as ops.conv2d_dgrad takes it."""
    g = gen(seed * 7919 + B * 1000 + H * 10 + W + cin * 3 + cout + k + stride)
    c = SimpleNamespace(name="dgrad B%d %dx%d %d<-%d k%d s%d %s" % (B, H, W, cin, cout, k, stride, variant), variant=variant, dtype=dtype, alpha=_alpha(variant, alpha),
                        k=k, stride=stride, pad=(pad,) * 4, cout=cin, nchw=True)
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    opad = (H - ((ho - 1) * stride - 2 * pad + k), W - ((wo - 1) * stride - 2 * pad + k))

    def tconv(dy, w):
        return F.conv_transpose2d(dy, w, stride=stride, padding=pad, output_padding=opad)

    taps = tconv(torch.ones(1, 1, ho, wo, dtype=torch.float64), torch.ones(1, 1, k, k, dtype=torch.float64))
    # (through the zero-insertion grid a pixel's reduction holds 1 to 4 of the k x k taps: 3/4 of the entries are non-zero so that the shortest still rarely sums to zero)
    ops_ = _draw(variant, [(B, cout, ho, wo)], (cout, cin, k, k), k * k * cout, int(taps.min().item()) * cout, g, 0.75 if stride > 1 else None)
    if ops_ is None:
        return None
    (c.dy,), c.w = ops_
    c.w_dgrad = c.w.permute(1, 2, 3, 0).flip(1, 2).reshape(cin, k * k * cout).contiguous()
    c.bias = c.rowadd = c.residual = None
    _finish(c, tconv(c.dy, c.w), None, None, None)
    if c.expect is not None:
        c.expect = c.expect.permute(0, 2, 3, 1).contiguous()
    return c


def exact_gemm_case(dtype, M, N, K, bias=True, bias_along_m=False, residual=False, alpha=1.0, variant="base", seed=0, batch=(), planes=False, density=None):
    """out[.., m, n] = alpha (sum_k a[.., m, k] w[.., n, k] + bias) + residual; batch: leading dims shared by a, w and out (no bias / residual broadcast over them is
    needed by any caller: batched cases carry neither)."""
    g = gen(seed * 7919 + M * 7 + N * 3 + K + len(batch))
    c = SimpleNamespace(name="gemm %s%dx%dx%d %s" % ("%s x " % (tuple(batch),) if batch else "", M, N, K, variant), variant=variant, dtype=dtype, alpha=_alpha(variant, alpha),
                        planes=planes)
    ops_ = _draw(variant, [tuple(batch) + (M, K)], tuple(batch) + (N, K), K, K, g, density)
    if ops_ is None:
        return None
    (c.a,), c.w = ops_
    if planes:
        assert dtype == torch.float32 and variant != "large" and not batch
        ia, iw = c.a, c.w
        c.a = ia + (ia != 0) * integers(ia.shape, -1, 1, g) * PLANE_EPS
        c.w = iw + (iw != 0) * integers(iw.shape, -1, 1, g) * PLANE_EPS
        a0, a1, sa = split_planes(c.a)
        w0, w1, sw = split_planes(c.w)
        acc = (a0 @ w0.t() + a0 @ w1.t() + a1 @ w0.t()) / (sa * sw)
        assert (ia.abs() @ iw.abs().t()).max().item() * (1 + 2 * PLANE_EPS) / PLANE_EPS < 2.0 ** 24
        c.acc_formula = ia @ iw.t() + (ia @ (c.w - iw).t() + (c.a - ia) @ iw.t())
    else:
        acc = c.a @ c.w.transpose(-1, -2)
    c.rowadd = None
    if variant == "large" or not bias:
        c.bias = None
    else:
        c.bias = integers((M if bias_along_m else N,), -8, 8, g)
    c.bias_along_m = bias_along_m
    if variant == "large" or not residual:
        c.residual = None
    else:
        c.residual = integers(acc.shape, -128, 128, g, step=0.125) if variant == "round1" else integers(acc.shape, -16, 16, g)
    _finish(c, acc, None if c.bias is None else (c.bias.view(-1, 1) if bias_along_m else c.bias.view(1, -1)), None, c.residual)
    return c


# ---- comparison -------------------------------------------------------------------------------------------------------------------------------------------------
def _as_bhwc(t):
    """[M, N] -> [1, M, 1, N]; [.., M, N] of a batched GEMM -> [z, M, 1, N]; NHWC stays"""
    if t.dim() == 4:
        return t
    return t.reshape(-1, t.shape[-2], 1, t.shape[-1])


def _where(bad):
    """(text, counts) describing the True entries of a [B, Y, X, C] mask: how many output channels, image rows and 256-row tiles hold one, and the first few indices"""
    B, Y, X, Cc = bad.shape
    idx = bad.nonzero()
    chans = int(bad.any(0).any(0).any(0).sum())
    rows = int(bad.any(3).any(2).sum())
    pix = bad.any(3).reshape(-1).nonzero().reshape(-1)
    tiles = sorted(set((pix // 256).tolist()))
    first = [tuple(i) for i in idx[:6].tolist()]
    counts = dict(entries=int(bad.sum()), channels=chans, rows=rows, tiles=len(tiles))
    text = ("%d entries in %d of %d output channels, %d of %d image rows, %d of %d 256-row tiles (tiles %s%s); first (b, y, x, co): %s"
            % (counts["entries"], chans, Cc, rows, B * Y, len(tiles), -(-(B * Y * X) // 256), tiles[:8], " ..." if len(tiles) > 8 else "", first))
    return text, counts


def assert_exact(name, got, ref):
    """util.assert_same_bits on a channels-last output ([B, Y, X, C], or [.., M, N] of a GEMM) with, on a mismatch, the location of the differing entries: a
    failure points at a tile border or a chunk"""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype, "%s: %s %s vs %s %s" % (name, tuple(got.shape), got.dtype, tuple(ref.shape), ref.dtype)
    if torch.equal(got, ref):
        return
    text, _ = _where(_as_bhwc(got != ref) | _as_bhwc(torch.isnan(got.float())))
    util.assert_same_bits(name, got, ref, "not bit-exact: " + text)


def assert_one_rounding(name, got, c):
    """the round1 variant: |got - ref| <= c.bound per element (got channels-last in the output type; c.ref / c.bound float64, NCHW for c.nchw cases, else [.., M, N])"""
    got = got.detach().cpu().double()
    ref, bound = (c.ref.permute(0, 2, 3, 1), c.bound.permute(0, 2, 3, 1)) if getattr(c, "nchw", False) else (c.ref, c.bound)
    assert got.shape == ref.shape, "%s: %s vs %s" % (name, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if not bad.any():
        return
    text, _ = _where(_as_bhwc(bad))
    worst = (err / bound)[bad].max().item() if torch.isfinite(err[bad]).all() else float("inf")
    raise AssertionError("%s: beyond one rounding of %s: %s; worst error %.2f x the bound" % (name, c.dtype, text, worst))


def check(name, got, c, expect=None):
    """the comparison a variant asks for (expect: a route's own contract, such as splitk_expect(c), in place of c.expect)"""
    if c.variant == "round1":
        assert_one_rounding(name, got, c)
    else:
        assert_exact(name, got, c.expect if expect is None else expect)
