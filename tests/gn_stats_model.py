"""Reference, inputs and bars for the GroupNorm statistics every producer writes: one (n, mean, M2) triple per image, pixel slab and channel.  CPU only; imports
nothing of the library.  tests/test_gn_stats_model_cpu.py proves the bars on these inputs with emulated fp32 arithmetic, tests/test_gn_statistics_gpu.py holds the
kernels to them.

Exact inputs.  Activations are integers in [-3, 3], weights are in {-1, 0, 1} / 8, alpha is 1 or 0.5, bias / rowadd / residual are dyadic numbers that fp16 AND bf16
hold exactly.  Every partial sum of a convolution is then a multiple of 2^-3 far below 2^24 of them: exact in fp32 in any summation order, and so is
    pre = alpha * (acc + bias + rowadd[image]) + residual                                   (a multiple of 2^-4 below 2^12)
the value an epilogue holds BEFORE it rounds to the output type; written = pre rounded to nearest-even in that type (= pre in fp32).  conv_case() asserts all of it:
the fp32 CPU convolution equals the fp64 one bit for bit, every operand survives a round trip through fp16 and bf16, and rounding changes at least half of `pre`.

Channels that cannot be confused.  Output channel c of an N tile (128 columns) sits on its own rung of a ladder: bias = 32 * rung + a few fractional bits, rungs
-64 .. 63 handed out by an odd multiplier, so neighbouring columns are 37 rungs apart, and the rungs of the next N tile are shifted by 11.  With a per-channel sigma
below 4 every channel is more than 8 of its own sigma from all others of its tile (asserted).  One channel per N tile has no weights at all: it is constant over an
image and its triple must be EXACTLY (n, c, 0).
Slabs and images that cannot be confused.  Eight input channels carry no noise but v = (slab + 3 * image) mod 7 - 3 at the pixel the centre tap reads, with weight 1/8
in every output channel: each slab of an image and the same slab of the next image are shifted against each other by a whole number.  Where the launch has them the
residual adds a ramp over the rows and rowadd an offset per image.  (The four phases of an upsampler convolution share their low-resolution pixels: they differ
by their summed weights and their borders only, which test_gn_stats_model_cpu.py shows to be far above the bars as well.)

Bars, from fp32 arithmetic alone (u = 2^-23), for shifted sums about any pivot taken from the slab and for Welford / Chan merges of such sums, with R = max |x - mean|:
    n exact,    |mean' - mean| <= u (n R + |mean|),    |M2' - M2| <= u n (M2 + n R^2)
The emulations below (sequential, eight strided lanes, Welford about a pivot, 64-row blocks merged by Chan's formula, the stand-alone pass's per-lane pivots merged
relative to one pivot) stay below 1.0 of both on every generator (at most 0.47 / 0.20); a column swap, a slab swap and a pivot taken from the wrong column exceed them on every slab and channel."""
import torch
import torch.nn.functional as F

U = 2.0 ** -23
NTILE = 128          # columns of one N tile in every producer
LADDER = 32.0        # distance of two rungs
NPAT = 8             # input channels that carry the slab / image pattern
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}

# what the statistics of each producer describe: "pre" = the exact fp32 value before rounding to the output type, "written" = the rounded tensor.  Read from the code:
# every vector epilogue accumulates x - pivot from the fp32 value it is about to round; only the stand-alone pass (which reads the tensor back) describes the rounded
# tensor.  (The generic branch of igemm_epilogue_rows emits none: its hosts decline statistics off the full-tile path, see test_gn_statistics_gpu.py.)
TARGET = {
    "gn_partial_kernel": "written",
    "igemm_epilogue_rows/full (igemm2: conv and GEMM)": "pre",
    "epilogue_packed (igemm5, convin, igemm6; 32x32 and 16x16x32)": "pre",
    "epilogue, fp32 window (igemm5, igemm6; 32x32 and 16x16x32)": "pre",
    "epilogue_f32 (f32split: igemm5, igemm6)": "pre",
    "upconv2x phases (igemm5 / igemm6 2x2)": "pre",
}


def round_to(t, dtype):
    """fp64 -> nearest-even in dtype -> fp64 (values here are exact in fp32, so the detour through fp32 rounds once)"""
    return t.to(torch.float32).to(dtype).to(torch.float64)


def representable(t, *dtypes):
    return all(bool((round_to(t, d) == t).all()) for d in dtypes)


# ---- slab maps: the slab of every output pixel (row-major y, x) of one image ---------------------------------------------------------------------------------------
def rowrun_slabs(hw, rows):
    """igemm2 / igemm5 / GEMM: slab s = the `rows` consecutive GEMM rows (pixels in row-major order) of M tile s of the image"""
    assert hw % rows == 0
    return torch.arange(hw) // rows, hw // rows


def patch_slabs(H, W):
    """igemm6 / convin: slab ty * (W / 32) + tx = the 8 x 32-pixel block at (8 ty, 32 tx)"""
    assert H % 8 == 0 and W % 32 == 0
    y, x = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    return ((y // 8) * (W // 32) + x // 32).reshape(-1), (H // 8) * (W // 32)


def phase_slabs(H, W):
    """the four-phase upsampler of a low-resolution H x W image: the statistics buffer of an image is [4 phases][H W / 256 runs]; slab ph * runs + r holds the output pixels
    (2 Y + py, 2 X + px), ph = 2 py + px, of the low-resolution pixels Y * W + X in [256 r, 256 r + 256).  (igemm6's 2x2 form takes 8 x 32 blocks of the low-resolution
    image instead: the same sets when W = 32.)"""
    assert (H * W) % 256 == 0
    runs = H * W // 256
    y, x = torch.arange(2 * H).view(2 * H, 1), torch.arange(2 * W).view(1, 2 * W)
    ph = 2 * (y % 2) + x % 2
    return (ph * runs + ((y // 2) * W + x // 2) // 256).reshape(-1), 4 * runs


def standalone_geometry(hw, C, elem_bytes):
    """gn_geom of csrc/norm.hip: a workgroup of 256 threads = cpb 16-byte channel chunks x pl pixel lanes; slabs of `slab` consecutive pixels, lane q of a slab reads
    pixels q, q + pl, ... and keeps shifted sums about ITS first pixel; the lanes are merged in order with Chan's formula -> (nslabs, slab, pl)"""
    nchunks = C // (16 // elem_bytes)
    nb = 1
    while nchunks % nb != 0 or nchunks // nb > 256:
        nb += 1
    pl = 256 // (nchunks // nb)
    ns = min(max((hw + pl * 16 - 1) // (pl * 16), 1), 1024)
    slab = (hw + ns - 1) // ns
    return (hw + slab - 1) // slab, slab, pl


def standalone_slabs(hw, C, elem_bytes):
    nslabs, slab, _ = standalone_geometry(hw, C, elem_bytes)
    return torch.arange(hw) // slab, nslabs


# ---- reference -------------------------------------------------------------------------------------------------------------------------------------------------
def triple(x):
    """x [n, ...] fp64 -> (n, mean, M2, R = max |x - mean|) over the first axis"""
    n = x.shape[0]
    mu = x.mean(0)
    d = x - mu
    return n, mu, (d * d).sum(0), d.abs().max(0).values


def slab_triples(t, slab_id, nslabs):
    """t [B, P, C] fp64, slab_id [P] -> n [S], mean / M2 / R [B, S, C]"""
    B, P, C = t.shape
    n = torch.zeros(nslabs, dtype=torch.float64)
    mu, m2, R = (torch.zeros(B, nslabs, C, dtype=torch.float64) for _ in range(3))
    for s in range(nslabs):
        sel = (slab_id == s).nonzero().flatten()
        n[s], mu[:, s], m2[:, s], R[:, s] = triple(t[:, sel].transpose(0, 1))
    return n, mu, m2, R


def chan_merge(n, mu, m2, axis):
    """fp64 merge of triples along `axis` of mu / m2 (n broadcastable): -> (N, mean, M2)"""
    n = n.expand_as(mu) if isinstance(n, torch.Tensor) else torch.full_like(mu, float(n))
    N = n.sum(axis)
    mean = (n * mu).sum(axis) / N
    M2 = (m2 + n * (mu - mean.unsqueeze(axis)) ** 2).sum(axis)
    return N, mean, M2


def bars(n, mu, m2, R):
    """-> (mean bar, M2 bar) of a set of n values with fp64 statistics (mu, M2) and largest deviation R"""
    return U * (n * R + mu.abs()), U * n * (m2 + n * R * R)


def entry_ratios(got_mu, got_m2, n, mu, m2, R):
    """|error| / bar of every entry -> (mean ratios, M2 ratios); where the bar is 0 (a constant channel) the ratio is 0 when the entry is exact and inf otherwise"""
    bm, b2 = bars(n, mu, m2, R)

    def div(err, bar):
        return torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))

    return div((got_mu.double() - mu).abs(), bm), div((got_m2.double() - m2).abs(), b2)


def ratios(got_mu, got_m2, n, mu, m2, R):
    """worst |error| / bar over all entries -> (mean ratio, M2 ratio)"""
    rm, r2 = entry_ratios(got_mu, got_m2, n, mu, m2, R)
    return rm.max().item(), r2.max().item()


def slab_columns(t, slab_id, nslabs):
    """t [B, P, C] with slabs of one size -> [n, B, S, C]: the n values of every (image, slab, channel), in the order of the pixels"""
    B, P, C = t.shape
    order = torch.argsort(slab_id, stable=True)
    assert P % nslabs == 0 and bool((torch.bincount(slab_id, minlength=nslabs) == P // nslabs).all())
    return t[:, order].view(B, nslabs, P // nslabs, C).permute(2, 0, 1, 3).contiguous()


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------------------
def ladder(C, frac=True, step=LADDER):
    """bias of channel c: step * rung + fractional bits (step = 32 / alpha, so that the rungs of `pre` are 32 apart); rung = (37 c + 11 tile) mod 128 - 64 inside
    its N tile.  The fraction is one step of the bf16 grid at that magnitude (one to three steps of at most 1 below 256; sixteenths on rung 0), away from zero: the value stays exact in fp16 and bf16, is no whole number where
    the grid allows it, and two rungs stay at least 29 apart."""
    c = torch.arange(C)
    rung = ((37 * (c % NTILE) + 11 * (c // NTILE)) % NTILE - 64).double()
    base = step * rung
    if not frac:
        return base
    mag = base.abs().clamp_min(8.0)
    ulp = 2.0 ** (torch.floor(torch.log2(mag)) - 7)
    b = base + torch.sign(base + 0.5) * ulp * torch.where(ulp <= 1.0, (1 + c % 3).double(), torch.ones_like(ulp))
    assert representable(b, torch.float16, torch.bfloat16)
    return b


def const_channels(C):
    return [t * NTILE + 5 for t in range((C + NTILE - 1) // NTILE) if t * NTILE + 5 < C]


def _pattern(slab_id, B):
    """v [B, P] = (slab + 3 image) mod 7 - 3"""
    return ((slab_id.view(1, -1) + 3 * torch.arange(B).view(B, 1)) % 7 - 3).double()


def conv_case(B, H, W, cin, cout, k=3, stride=1, residual=False, rowadd=False, alpha=1.0, up=False, slabs=None, pattern=True, xvals=3, nnz=16, seed=0,
              hostile=False, balanced=0, bias=None):
    """One exact convolution.  slabs: (slab_id [Ho Wo], nslabs) of the producer under test (places the pattern).  xvals: activations are integers in [-xvals, xvals];
    nnz: non-zero weights per output channel (sigma of the noise = sqrt(nnz * E x^2) / 8: 1.0 for (3, 16) and for (1, 64)).  hostile: fp32 only — bias 1000 + 32 rung'
    (|mean| / sigma >= 1000), no pattern, and 80 further input channels that are 3 at the first pixel of every slab and 0 elsewhere with weight 1/8: a 30 sigma
    outlier exactly where the row epilogue and lane 0 of the stand-alone pass take their pivot.  balanced = G: activations are +-1, as many of each in every (image,
    group of cin / G channels) — mean 0 and variance 1 per group, so GroupNorm(G groups, gamma 1, beta 0) of them rounds back to +-1 in fp16 and bf16 and a convolution
    that reads its input through that norm is as exact as one that reads it directly.  bias: a [cout] tensor instead of the ladder (the finalize cases).
    -> dict of fp64 CPU tensors: x [B, cin, H, W], w [cout, cin, k, k], bias [cout], rowadd [B, cout] / residual [B, Ho, Wo, cout] or None, pre and written-per-dtype
    [B, Ho Wo, cout], geometry."""
    g = torch.Generator().manual_seed(1000 * seed + B * 100 + H + W + cin + cout + k)
    custom_bias = bias
    pad = k // 2
    Hl, Wl = (2 * H, 2 * W) if up else (H, W)
    Ho, Wo = (Hl + 2 * pad - k) // stride + 1, (Wl + 2 * pad - k) // stride + 1
    slab_id, nslabs = slabs if slabs is not None else rowrun_slabs(Ho * Wo, Ho * Wo)
    assert slab_id.numel() == Ho * Wo
    nspecial = 0 if not pattern else NPAT
    nout = 80 if hostile else 0
    assert cin >= nspecial + nout + 8
    x = torch.randint(-xvals, xvals + 1, (B, cin, H, W), generator=g).double()
    if balanced:
        assert not pattern and not hostile and cin % balanced == 0 and (cin // balanced * H * W) % 2 == 0
        m = cin // balanced * H * W
        half = torch.cat([torch.ones(m // 2), -torch.ones(m // 2)]).double()
        x = torch.stack([half[torch.randperm(m, generator=g)] for _ in range(B * balanced)]).view(B, cin, H, W)
    w = torch.zeros(cout, cin, k, k, dtype=torch.float64)
    nfree = (cin - nspecial - nout) * k * k
    for co in range(cout):
        idx = torch.randperm(nfree, generator=g)[:nnz]
        sign = (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1).double() / 8.0
        w[co, nspecial + nout:].view(-1)[idx] = sign
    if pattern:
        # the centre tap of output pixel (oy, ox) reads logical pixel (oy * stride, ox * stride); with the fused upsample that is source pixel (.. // 2, .. // 2)
        v = _pattern(slab_id, B).view(B, Ho, Wo)
        x[:, :NPAT] = 0.0
        if up:
            x[:, :NPAT] = v[:, ::2, ::2].unsqueeze(1)        # (the phases of a low-resolution pixel share its value: phase_slabs gives them the same run)
        else:
            x[:, :NPAT, ::stride, ::stride] = v.unsqueeze(1)
        w[:, :NPAT, pad, pad] = 1.0 / 8.0
    if hostile:
        first = torch.zeros(nslabs, dtype=torch.long)
        for s in range(nslabs):
            first[s] = (slab_id == s).nonzero()[0, 0]
        assert stride == 1 and not up
        xo = torch.zeros(B, nout, H * W, dtype=torch.float64)
        xo[:, :, first] = 3.0
        x[:, nspecial:nspecial + nout] = xo.view(B, nout, H, W)
        w[:, nspecial:nspecial + nout, pad, pad] = 1.0 / 8.0
    consts = const_channels(cout)
    w[consts] = 0.0
    if bias is not None:
        bias = bias.double()
    else:
        bias = ladder(cout, step=LADDER / alpha) if not hostile else 1000.0 + LADDER * (ladder(cout, frac=False) / LADDER + 64.0)
    ra = rs = None
    if rowadd:
        ra = 8.0 * (torch.arange(B) % 3).double().view(B, 1) + torch.randint(-4, 5, (B, cout), generator=g).double() / 4.0
    if residual:
        rs = 0.25 * (torch.arange(Ho) % 16).double().view(1, Ho, 1, 1) + torch.randint(-4, 5, (B, Ho, Wo, cout), generator=g).double() / 4.0
        rs[..., consts] = 1.5
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    acc = F.conv2d(xin, w, None, stride=stride, padding=pad)
    acc32 = F.conv2d(xin.float(), w.float(), None, stride=stride, padding=pad)
    assert torch.equal(acc32.double(), acc), "the convolution is not exact in fp32: the case is not representable"
    assert bool((acc * 8 == (acc * 8).round()).all()) and acc.abs().max() < 2.0 ** 12
    pre = acc.permute(0, 2, 3, 1) + bias
    if ra is not None:
        pre = pre + ra.view(B, 1, 1, cout)
    pre = pre * alpha
    if rs is not None:
        pre = pre + rs
    assert torch.equal(pre.float().double(), pre) and bool((pre * 16 == (pre * 16).round()).all())
    # the same value in the epilogues' association, in fp32: fma(acc, alpha, bias * alpha), fma(rowadd, alpha, .), + residual
    e32 = acc32.permute(0, 2, 3, 1) * alpha + (bias.float() * alpha)
    if ra is not None:
        e32 = ra.float().view(B, 1, 1, cout) * alpha + e32
    if rs is not None:
        e32 = e32 + rs.float()
    assert torch.equal(e32.double(), pre), "the epilogue's fp32 association is not exact"
    ops16 = [x, w, bias] + ([ra] if ra is not None else []) + ([rs] if rs is not None else [])
    if not hostile:
        assert all(representable(t, torch.float16, torch.bfloat16) for t in ops16), "an operand is not exact in fp16 and bf16"
    pre = pre.reshape(B, Ho * Wo, cout).contiguous()
    written = {name: round_to(pre, dt) for name, dt in DTYPES.items()}
    if not hostile and custom_bias is None:
        for name in ("fp16", "bf16"):
            changed = (written[name] != pre).double().mean().item()
            assert changed >= 0.5, "rounding to %s changes only %.2f of the entries" % (name, changed)
    return dict(x=x, w=w, bias=bias, rowadd=ra, residual=rs, alpha=alpha, pre=pre, written=written, consts=consts, slab_id=slab_id, nslabs=nslabs,
                geom=(B, H, W, cin, cout, k, stride, Ho, Wo), up=up, hostile=hostile)


def geometric_ladder(C):
    """mean of channel c of a stand-alone tensor: +-0.5 * 1.19^r, r = 0 .. 63 (0.5 .. 29000), sign and r from the channel's rung.  A floating-point type resolves a
    channel's noise only relative to its mean, so the ladder is geometric and sigma is about mean / 60: the next rung towards zero is 0.16 |mean| = 9.6 sigma away."""
    c = torch.arange(C)
    rung = (37 * (c % NTILE) + 11 * (c // NTILE)) % NTILE
    return torch.where(rung % 2 == 0, 1.0, -1.0).double() * 0.5 * 1.19 ** (rung // 2).double()


def standalone_case(B, H, W, C, dtype_name, seed=0, hostile=False):
    """A tensor for the stand-alone pass, rounded to the type (`written` IS the input): mean_c * (1 + e / 64) on the geometric ladder, e = noise in sixteenths (sigma
    0.3) + the slab / image pattern v / 2 (at least one step of the bf16 grid) + a ramp over the rows.  hostile (fp32): mean 1000 + 32 rung', sigma 1, first pixel of every slab + 30."""
    dt = DTYPES[dtype_name]
    g = torch.Generator().manual_seed(77 + 1000 * seed + B + H * W + C)
    slab_id, nslabs = standalone_slabs(H * W, C, 4 if dtype_name == "fp32" else 2)
    y = (torch.arange(H * W) // W).double()
    consts = const_channels(C)
    if hostile:
        t = 1000.0 + LADDER * (ladder(C, frac=False) / LADDER + 64.0) + torch.randint(-14, 15, (B, H * W, C), generator=g).double() / 8.0      # sigma 1.01
        for s in range(nslabs):
            t[:, (slab_id == s).nonzero()[0, 0]] += 30.0
        t[..., consts] = (1000.0 + LADDER * (ladder(C, frac=False) / LADDER + 64.0))[consts]
    else:
        e = torch.randint(-8, 9, (B, H * W, C), generator=g).double() / 16.0 + _pattern(slab_id, B).unsqueeze(2) / 2.0 + ((y % 16) / 32.0).view(1, -1, 1)
        e[..., consts] = 0.0
        t = geometric_ladder(C) * (1.0 + e / 64.0)
    t = round_to(t, dt)
    return dict(t=t, consts=consts, slab_id=slab_id, nslabs=nslabs, geom=(B, H, W, C), hostile=hostile)


def assert_separated(t, consts):
    """t [B, P, C]: per image, every channel is >= 8 of its OWN sigma away in mean from every other channel of its N tile, or their sigmas differ by a factor >= 2"""
    mu, sd = t.mean(1), t.var(1, unbiased=False).sqrt()
    C = t.shape[2]
    for t0 in range(0, C, NTILE):
        m, s = mu[:, t0:t0 + NTILE], sd[:, t0:t0 + NTILE]
        gap = (m.unsqueeze(2) - m.unsqueeze(1)).abs()                      # [B, i, j]
        far = gap >= 8.0 * s.unsqueeze(2)
        ratio = s.unsqueeze(2) / s.unsqueeze(1).clamp_min(1e-300)
        other = (ratio >= 2.0) | (ratio <= 0.5)
        eye = torch.eye(m.shape[1], dtype=torch.bool).unsqueeze(0)
        assert bool((far | other | eye).all()), "channels of N tile %d are not separated" % (t0 // NTILE)


# ---- fp32 emulations of the producers' summation orders: x [n, K] fp64 (exact in fp32) -> (mean, M2) fp32 [K] ----------------------------------------------------
def _f(x):
    return x.to(torch.float32)


def _finish(piv, s, ss, n):
    n = torch.tensor(float(n), dtype=torch.float32)
    return piv + s / n, (ss - s * s / n).clamp_min(0.0)


def emu_shifted(x, piv):
    """one accumulator, rows in order"""
    x, piv = _f(x), _f(piv)
    s, ss = torch.zeros_like(piv), torch.zeros_like(piv)
    for i in range(x.shape[0]):
        d = x[i] - piv
        s = s + d
        ss = ss + d * d
    return _finish(piv, s, ss, x.shape[0])


def emu_lanes(x, piv, lanes=8):
    """`lanes` strided accumulators about one pivot, added as a butterfly (the row passes of igemm_epilogue_rows, the slices of the persistent epilogues)"""
    x, piv = _f(x), _f(piv)
    n = x.shape[0]
    assert n % lanes == 0
    d = x.view(n // lanes, lanes, -1) - piv
    s, ss = torch.zeros_like(d[0]), torch.zeros_like(d[0])
    for i in range(n // lanes):
        s = s + d[i]
        ss = ss + d[i] * d[i]
    while s.shape[0] > 1:
        h = s.shape[0] // 2
        s, ss = s[:h] + s[h:], ss[:h] + ss[h:]
    return _finish(piv, s[0], ss[0], n)


def emu_welford(x, piv=None):
    """Welford's update row by row, on x - piv (piv = None: on x itself, from zero — the form the generic branch of igemm_epilogue_rows once had; its mean picks up a
    rounding of |mean| u / 2 per row, which the mean bar does not allow when |mean| >> n R: test_gn_stats_model_cpu.py pins that)"""
    x = _f(x)
    piv = torch.zeros_like(x[0]) if piv is None else _f(piv)
    mean, m2 = torch.zeros_like(x[0]), torch.zeros_like(x[0])
    for i in range(x.shape[0]):
        v = x[i] - piv
        d = v - mean
        mean = mean + d * torch.tensor(1.0 / (i + 1), dtype=torch.float32)
        m2 = m2 + d * (v - mean)
    return piv + mean, m2


def _chan32(na, ma, m2a, nb, mb, m2b):
    nt = na + nb
    dl = mb - ma
    f = torch.tensor(nb / nt, dtype=torch.float32)
    return nt, ma + dl * f, m2a + m2b + dl * dl * torch.tensor(float(na), dtype=torch.float32) * f


def emu_blocks(x, block=64):
    """blocks of `block` rows, each shifted sums about its own first row (eight lanes), merged in order by Chan's formula (combine() of the persistent epilogues)"""
    n = x.shape[0]
    assert n % block == 0
    acc = None
    for b0 in range(0, n, block):
        m, m2 = emu_lanes(x[b0:b0 + block], x[b0])
        acc = (block, m, m2) if acc is None else _chan32(acc[0], acc[1], acc[2], block, m, m2)
    return acc[1], acc[2]


def emu_standalone(x, pl, relative=True):
    """gn_partial_kernel: lane q takes rows q, q + pl, ... about its own first row; the lanes are merged in order by Chan's formula — their means relative to lane
    0's pivot, which is added back at the end.  relative = False: the lanes' ABSOLUTE means are merged, every step rounding at the size of the mean (the kernel before
    this model existed: above the bars on short slabs of 16-bit data, test_gn_stats_model_cpu.py pins it)"""
    acc = None
    p0 = _f(x[0])
    for q in range(min(pl, x.shape[0])):
        rows = x[q::pl]
        piv = _f(rows[0])
        m, m2 = emu_shifted(rows, rows[0])
        if relative:      # (mean - pivot) as the kernel holds it: s / n, before the pivot is added
            s = torch.zeros_like(piv)
            for i in range(rows.shape[0]):
                s = s + (_f(rows[i]) - piv)
            m = (piv - p0) + s / torch.tensor(float(rows.shape[0]), dtype=torch.float32)
        acc = (rows.shape[0], m, m2) if acc is None else _chan32(acc[0], acc[1], acc[2], rows.shape[0], m, m2)
    return (p0 + acc[1] if relative else acc[1]), acc[2]


def emulations(x, pl=None):
    """name -> (mean, M2) of every order, pivots: first row, the column minimum, and (shifted sums only) the column's value 100 sigma away is covered by the hostile cases"""
    n = x.shape[0]
    out = {"sequential, pivot = first row": emu_shifted(x, x[0]), "sequential, pivot = minimum": emu_shifted(x, x.min(0).values), "welford about the first row": emu_welford(x, x[0])}
    if n % 8 == 0:
        out["eight lanes + butterfly"] = emu_lanes(x, x[0])
    if n % 64 == 0 and n > 64:
        out["64-row blocks + Chan"] = emu_blocks(x)
    if pl is not None:
        out["per-lane pivots + Chan (%d lanes)" % pl] = emu_standalone(x, pl)
    return out


def emu_wrong_pivot(x):
    """the mutant: sums about the pivot of the NEXT column, mean rebuilt with the column's own pivot"""
    x32 = _f(x)
    piv = x32[0]
    other = torch.roll(piv, -1)
    s, ss = torch.zeros_like(piv), torch.zeros_like(piv)
    for i in range(x.shape[0]):
        d = x32[i] - other
        s = s + d
        ss = ss + d * d
    return _finish(piv, s, ss, x.shape[0])


# ---- the cases of tests/test_gn_statistics_gpu.py (shapes; the routing lives there).  slab = how the producer cuts an image: ("rows", r) / ("patch",) / ("phase",) -----
def _slabs_of(kind, Ho, Wo, H, W):
    if kind[0] == "rows":
        return rowrun_slabs(Ho * Wo, kind[1])
    if kind[0] == "patch":
        return patch_slabs(Ho, Wo)
    return phase_slabs(H, W)


CONV_CASES = {
    # name: (B, H, W, cin, cout, k, stride, residual, rowadd, alpha, up, slab kind, extra keywords)
    "rows_3x3": (3, 16, 16, 64, 128, 3, 1, False, False, 1.0, False, ("rows", 128), {}),
    "rows_3x3_bm256": (3, 16, 16, 64, 128, 3, 1, True, True, 0.5, False, ("rows", 256), {}),
    "rows_1x1": (3, 16, 32, 128, 64, 1, 1, False, False, 1.0, False, ("rows", 128), {}),
    "rows_1x1_res_ra_alpha": (3, 16, 32, 128, 64, 1, 1, True, True, 0.5, False, ("rows", 128), {}),
    "rows_hostile": (3, 16, 16, 128, 128, 3, 1, False, False, 1.0, False, ("rows", 128), {"hostile": True, "pattern": False}),
    "linear": (3, 16, 16, 64, 128, 1, 1, False, False, 1.0, False, ("rows", 128), {}),
    "igemm5_packed": (1, 64, 64, 64, 128, 3, 1, False, False, 1.0, False, ("rows", 256), {}),
    "igemm5_window": (1, 64, 64, 64, 128, 3, 1, True, True, 0.5, False, ("rows", 256), {}),
    "igemm5_ragged_n": (1, 96, 96, 64, 320, 3, 1, True, False, 1.0, False, ("rows", 256), {}),
    "igemm5_image_per_tile": (16, 16, 16, 64, 128, 3, 1, True, False, 1.0, False, ("rows", 256), {}),
    "igemm5_images_per_tile": (64, 8, 8, 64, 128, 3, 1, True, False, 1.0, False, ("rows", 64), {}),
    "igemm5_stride2": (4, 64, 64, 64, 256, 3, 2, False, True, 1.0, False, ("rows", 256), {}),
    "convin": (4, 32, 32, 8, 128, 3, 1, False, False, 1.0, False, ("patch",), {"pattern": False, "nnz": 16}),
    "igemm6": (2, 32, 64, 128, 128, 3, 1, False, False, 1.0, False, ("patch",), {}),
    "igemm6_res": (2, 32, 64, 128, 128, 3, 1, True, True, 0.5, False, ("patch",), {}),
    "igemm6_normed": (2, 32, 64, 128, 128, 3, 1, True, False, 1.0, False, ("patch",), {"pattern": False, "balanced": 32, "nnz": 64}),
    "upconv_phases": (2, 32, 32, 64, 256, 3, 1, False, False, 1.0, True, ("phase",), {}),
    "f32split_igemm6": (2, 32, 64, 128, 128, 3, 1, True, False, 1.0, False, ("patch",), {}),
    "f32split_igemm5": (2, 16, 48, 128, 128, 3, 1, True, False, 1.0, False, ("rows", 256), {}),
    "f32split_upconv_igemm6": (2, 16, 32, 128, 128, 3, 1, False, False, 1.0, True, ("phase",), {}),
    "f32split_upconv_igemm5": (4, 16, 16, 128, 64, 3, 1, False, False, 1.0, True, ("phase",), {}),
}
STANDALONE_SHAPES = [(2, 40, 36, 128), (2, 5, 5, 320), (2, 6, 6, 960)]
STANDALONE_HOSTILE = (2, 40, 36, 128)

_cache = {}


def get_conv_case(name):
    """built once per process and shared (never modified by the tests)"""
    if name not in _cache:
        B, H, W, cin, cout, k, stride, res, ra, alpha, up, kind, kw = CONV_CASES[name]
        pad = k // 2
        Hl, Wl = (2 * H, 2 * W) if up else (H, W)
        Ho, Wo = (Hl + 2 * pad - k) // stride + 1, (Wl + 2 * pad - k) // stride + 1
        kw = dict(kw)
        if name == "convin":      # eight input channels in all: 3x3 x 8 = 72 weights per output channel, no room for the pattern channels
            _cache[name] = _convin_case(B, H, W, cout, patch_slabs(Ho, Wo))
        else:
            _cache[name] = conv_case(B, H, W, cin, cout, k, stride, res, ra, alpha, up, _slabs_of(kind, Ho, Wo, H, W), seed=len(_cache), **kw)
    return _cache[name]


def _convin_case(B, H, W, cout, slabs):
    """conv_in has eight input channels in all (72 weights per output channel): two of them carry the slab / image pattern, a shift of v / 4 — neighbouring slabs
    differ by at least 0.25 against bars of ~1e-4 — and 16 of the other 54 weights are non-zero: sigma 1."""
    g = torch.Generator().manual_seed(4242)
    slab_id, nslabs = slabs
    x = torch.randint(-3, 4, (B, 8, H, W), generator=g).double()
    v = _pattern(slab_id, B).view(B, H, W)
    x[:, :2] = v.unsqueeze(1)
    w = torch.zeros(cout, 8, 3, 3, dtype=torch.float64)
    for co in range(cout):
        idx = torch.randperm(54, generator=g)[:16]
        w[co, 2:].view(-1)[idx] = (torch.randint(0, 2, (16,), generator=g) * 2 - 1).double() / 8.0
    w[:, :2, 1, 1] = 1.0 / 8.0
    consts = const_channels(cout)
    w[consts] = 0.0
    bias = ladder(cout)
    acc = F.conv2d(x, w, None, padding=1)
    assert torch.equal(F.conv2d(x.float(), w.float(), None, padding=1).double(), acc)
    pre = (acc.permute(0, 2, 3, 1) + bias).reshape(B, H * W, cout).contiguous()
    assert torch.equal(pre.float().double(), pre)
    assert all(representable(t, torch.float16, torch.bfloat16) for t in (x, w, bias))
    written = {name: round_to(pre, dt) for name, dt in DTYPES.items()}
    for name in ("fp16", "bf16"):
        assert (written[name] != pre).double().mean().item() >= 0.5
    return dict(x=x, w=w, bias=bias, rowadd=None, residual=None, alpha=1.0, pre=pre, written=written, consts=consts, slab_id=slab_id, nslabs=nslabs,
                geom=(B, H, W, 8, cout, 3, 1, H, W), up=False, hostile=False)


# ---- finalize: inputs whose groups are tight (R of a group is a few sigma, so the bars of a group mean something) ---------------------------------------------------
CONST_GROUP = 3


def finalize_means(C, groups, c0=0, c1=None):
    """base value of channels c0 .. c1 of a C-channel norm: 8 * (group mod 8 - 4) + (c mod 4) / 2 — exact in fp16 and bf16"""
    c = torch.arange(c0, C if c1 is None else c1)
    g = c // (C // groups)
    return 8.0 * (g % 8 - 4).double() + 0.5 * (c % 4).double()


def finalize_tensor(B, P, C, groups, dtype_name, c0=0, c1=None, seed=0):
    """channels c0 .. c1 of the input of a C-channel GroupNorm: base + image + noise in eighths (sigma 0.9), rounded to the type; group CONST_GROUP is built from
    per-channel constants base + (c mod cpg) / 2: all of its variance comes from the delta term of Chan's formula"""
    c1 = C if c1 is None else c1
    g = torch.Generator().manual_seed(5 + seed + C + P + c0)
    t = finalize_means(C, groups, c0, c1) + torch.arange(B).double().view(B, 1, 1) + torch.randint(-12, 13, (B, P, c1 - c0), generator=g).double() / 8.0
    c = torch.arange(c0, c1)
    cpg = C // groups
    cg = (c // cpg) == CONST_GROUP
    t[..., cg] = (finalize_means(C, groups, c0, c1) + 0.5 * (c % cpg).double())[cg]
    return round_to(t, DTYPES[dtype_name])


# ---- finalize: (a, mean) pairs and rstd per (image, group) ----------------------------------------------------------------------------------------------------------
def group_reference(t, groups, eps):
    """t [B, P, C] fp64 -> per (image, group): n, mean, M2, R, rstd"""
    B, P, C = t.shape
    cpg = C // groups
    x = t.view(B, P, groups, cpg).permute(0, 2, 1, 3).reshape(B, groups, P * cpg)
    n = P * cpg
    mu = x.mean(2)
    d = x - mu.unsqueeze(2)
    m2 = (d * d).sum(2)
    return n, mu, m2, d.abs().max(2).values, 1.0 / torch.sqrt(m2 / n + eps)


def rstd_bar(n, m2, R, eps):
    """|rstd' / rstd - 1| <= (M2 bar) / (2 (M2 + n eps)) + 2^-21   (the last term: rsqrtf and the division)"""
    return 0.5 * (U * n * (m2 + n * R * R)) / (m2 + n * eps) + 2.0 ** -21
