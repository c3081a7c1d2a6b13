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


# ---- exact power-of-two scaling of backward passes ------------------------------------------------------------------------------------------------------
# Every backward op is linear in the incoming gradient dy, and every rounding inside it (fp32 accumulation, bf16 packing, output rounding) commutes with a
# multiplication by a power of two while nothing leaves the normal range: bwd(2^k dy) == 2^k bwd(dy) BIT FOR BIT, and block by block wherever an output block
# depends on one block of dy alone.  No tolerance is involved, so an absolute threshold, an epsilon on a dy term, an f16 intermediate, stale pad / workspace
# contents or a neighbour's row show at training-scale gradients (2^-24 and below) where the unit-scale parity tests cannot see them.
SCALE_UNIFORM_K = (-24, -40)          # ~ 1 / (pixels of one benchmark micro-batch); room for accumulation and small losses, every product still above 2^-100
SCALE_BLOCK_K = (-27, 0, -40, -13)    # exponent of block i: SCALE_BLOCK_K[i % 4]
NON_VACUOUS = 0.9                     # a compared output is finite and non-zero in at least this fraction of its entries


def _ulp_index(t):
    """monotone integer index of every float of t (consecutive representable values differ by one): |index(a) - index(b)| = distance in units in the last place"""
    t = t.detach().contiguous()
    nbits = 8 * t.element_size()
    bits = t.view({16: torch.int16, 32: torch.int32, 64: torch.int64}[nbits]).to(torch.int64)
    mag = bits & ((1 << (nbits - 1)) - 1)
    return torch.where(bits < 0, -mag, mag)


def assert_same_bits(name, got, want, what):
    """torch.equal(got, want), with a message that names the output, how many entries differ, the largest difference in ulp and the first differing index"""
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s: %s %s vs %s %s" % (name, what, tuple(got.shape), got.dtype, tuple(want.shape), want.dtype)
    if torch.equal(got, want):
        return
    ne = got != want
    ulps = (_ulp_index(got) - _ulp_index(want)).abs()
    first = tuple(ne.nonzero()[0].tolist())
    raise AssertionError("%s: %s: %d of %d entries differ, largest difference %d ulp, first at index %s (got %r, want %r)"
                         % (name, what, int(ne.sum()), ne.numel(), int(ulps.max()), first, got[first].item(), want[first].item()))


def nonzero_fraction(t):
    t = t.detach()
    return (torch.isfinite(t) & (t != 0)).double().mean().item() if t.numel() else 1.0


def block_ids(shape, axes):
    """Block number of every entry of a tensor of `shape` cut into blocks along `axes`, as an int64 tensor that broadcasts against it.  An axis is an int (one
    block per index) or (axis, chunk) (one block per `chunk` consecutive indices: the heads of a [.., heads * d] axis).  With several axes the number is the SUM of
    the block coordinates — neighbours along every axis get different exponents from a period-4 table, which a row-major number would not give along an outer
    axis whenever the inner extent is a multiple of four."""
    ids = torch.zeros([1] * len(shape), dtype=torch.int64)
    for a in axes:
        ax, chunk = a if isinstance(a, (tuple, list)) else (a, 1)
        view = [1] * len(shape)
        view[ax % len(shape)] = -1
        ids = ids + (torch.arange(shape[ax % len(shape)]) // chunk).view(view)
    return ids


def _block_counts(shape, axes):
    return [-(-shape[(a[0] if isinstance(a, (tuple, list)) else a) % len(shape)] // (a[1] if isinstance(a, (tuple, list)) else 1)) for a in axes]


def _block_factor(shape, axes, like):
    k = torch.tensor(SCALE_BLOCK_K, dtype=torch.float64)[block_ids(shape, axes) % len(SCALE_BLOCK_K)]
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), k).to(like.dtype).to(like.device)      # powers of two within bf16's / fp32's exponent range: exact


def assert_backward_scales(run, dy, outputs, block=None, zero=()):
    """run(dy) -> {name: gradient tensor}: builds fresh leaves, runs forward and backward, returns the gradients.  dy: the incoming gradient in the op's dtype, or a
    tuple of equally shaped gradients that are scaled together (a skip gradient next to dy); run receives what it was given.  outputs: the names to compare.
    Checked, in this order:
      repeatability   two runs on dy are torch.equal for every output;
      non-vacuity     every output is finite and non-zero in >= 90 % of its entries; the outputs named in `zero` (analytically zero) are only required to be finite;
      uniform         run(dy * 2^k)[name] is torch.equal to run(dy)[name] * 2^k (formed in the output's own dtype, where it is exact) for k = -24, -40;
      blocks          block = {name: (axes of dy, axes of the output)}: the output's blocks along its axes depend on the matching blocks of dy alone (axis specs as in
                      block_ids; the i-th axis of one side pairs with the i-th of the other).  Block i of dy is multiplied by 2^SCALE_BLOCK_K[i % 4] and the matching
                      block of the output must equal the unscaled one times that factor.  Outputs sharing their dy axes share a run; the others are not compared in it."""
    many = isinstance(dy, (tuple, list))
    dys = tuple(dy) if many else (dy,)
    assert all(t.shape == dys[0].shape for t in dys)

    def call(ts):
        out = run(tuple(ts) if many else ts[0])
        lack = [n for n in outputs if out.get(n) is None]
        assert not lack, "run() returned no %s" % lack
        return out

    base = {n: t.detach().clone() for n, t in call(dys).items() if n in outputs}
    again = call(dys)
    for n in outputs:
        assert_same_bits(n, again[n].detach(), base[n], "second run on the same dy")
    for n in outputs:
        assert torch.isfinite(base[n]).all() or n not in zero, "%s: non-finite entries" % n
        if n not in zero:
            f = nonzero_fraction(base[n])
            assert f >= NON_VACUOUS, "%s: only %.1f %% of the entries are finite and non-zero" % (n, 100 * f)
    for k in SCALE_UNIFORM_K:
        got = call([t * 2.0 ** k for t in dys])
        for n in outputs:
            assert_same_bits(n, got[n].detach(), base[n] * 2.0 ** k, "dy * 2^%d" % k)
    if not block:
        return
    unknown = [n for n in block if n not in outputs]
    assert not unknown, unknown
    variants = {}
    for n in outputs:
        if n in block:
            dax, oax = block[n]
            assert _block_counts(dys[0].shape, dax) == _block_counts(base[n].shape, oax), "%s: blocks of dy %s and of the output %s do not pair" % (n, dax, oax)
            variants.setdefault(tuple(tuple(a) if isinstance(a, (tuple, list)) else a for a in dax), []).append(n)
    for dax, names in variants.items():
        got = call([t * _block_factor(t.shape, dax, t) for t in dys])
        for n in names:
            assert_same_bits(n, got[n].detach(), base[n] * _block_factor(base[n].shape, block[n][1], base[n]),
                             "block scaling, blocks of dy along %s scaled by 2^%s in turn" % (list(dax), list(SCALE_BLOCK_K)))
