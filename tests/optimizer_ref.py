"""Float64 reference of one flat-optimizer step (csrc/bwd.hip: adamw_kernel, adamw_guarded_kernel) with per-element error bounds, the test cases the CPU and
the GPU tests share, and the exactly rounded sum the accumulate form of `cast_` is compared with.  Plain torch on the CPU.

torch.optim.AdamW (decoupled decay) after clip_grad_norm_, the gradient pre-multiplied by grad_scale:
    clip  = grad_scale * min(1, max_norm / (sqrt(sumsq) * grad_scale + 1e-6))      (max_norm > 0, else grad_scale)
    g^    = g * clip
    p     = p (1 - lr wd)
    m'    = b1 m + (1 - b1) g^
    v'    = b2 v + (1 - b2) g^2
    denom = sqrt(v') / sqrt(1 - b2^t) + eps
    p'    = p - lr / (1 - b1^t) * m' / denom

Bounds, u = 2^-24, S = |b1 m| + |(1 - b1) g^|:
    |dv| <= K u v'          |dm| <= K u S          |dp| <= K u (|p| + |upd|) + (lr / bc1) K u S / denom
K = 20 from counting the kernel's fp32 roundings to first order: the clip chain has 5 (sqrt -> float, * grad_scale, + 1e-6, the division, * grad_scale) and g^ one
more, so v' carries 2 * 6 + 3 = 15, m' at most 8 in units of S, and the update about 16.5 next to the m' term.  20 leaves room for the second-order terms; FMA
contraction only removes roundings.  K is a property of the operation count, not of any run: a kernel above it has a defect to be explained."""
import math

import torch

U = 2.0 ** -24
K = 20
N = 100003
STEPS = (1, 2, 3, 10, 100, 1000, 20000)
B1, B2, EPS = 0.9, 0.999, 1e-8

# name: (lowest and highest exponent e of |g| = 2^e (1 + rand), grad_scale, max_norm, lr, wd, fraction of g that is exactly zero)
CASES = {
    "unit_clipped": (-3, 3, 1.0, 1.0, 3e-5, 1e-2, 0.0),
    "unit_averaged_8_ranks": (-3, 3, 0.125, 1.0, 3e-5, 1e-2, 0.0),
    "scale_not_power_of_two": (-3, 3, 1.0 / 3.0, 1.0, 3e-3, 0.0, 0.0),
    "training_scale": (-40, -24, 0.125, 1.0, 3e-5, 1e-2, 0.0),          # clip idle, eps dominates the denominator
    "around_eps": (-28, -25, 1.0, 0.0, 3e-5, 1e-2, 0.0),
    "wide": (-30, 10, 1.0, 1.0, 3e-5, 1e-2, 0.0),
    "quarter_zero": (-3, 3, 1.0, 1.0, 3e-5, 1e-2, 0.25),
}


def f32(x):
    """the double nearest to x after rounding to float32: what a float argument of the C ABI carries"""
    return torch.tensor(float(x), dtype=torch.float64).float().double().item()


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1000003 + k + 1
    return torch.Generator().manual_seed(seed)


def zero_mask(n):
    """the elements whose gradient is exactly zero on EVERY step of a case with a zero fraction: one index in four of each of the four blocks of p"""
    return (torch.arange(n) // 4) % 4 == 0


def make_params(n, seed=0):
    """fp32 p in four interleaved blocks: exactly 0 (p' is the update itself: its relative error shows at any lr), about 2^-20, 0.05 randn, +-8"""
    g = _gen(seed, 17)
    sign = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()
    p = torch.zeros(n, dtype=torch.float64)
    i = torch.arange(n) % 4
    small = 2.0 ** -20 * (1 + torch.rand(n, generator=g, dtype=torch.float64)) * sign
    mid = 0.05 * torch.randn(n, generator=g, dtype=torch.float64)
    p = torch.where(i == 1, small, p)
    p = torch.where(i == 2, mid, p)
    p = torch.where(i == 3, 8.0 * sign, p)
    return p.float()


def make_grad(case, k, n, seed=0):
    """the fp32 gradient of step number k (0-based) of a case: 2^e (1 + rand), random sign, e a uniform integer of the case's range"""
    lo, hi, _, _, _, _, zero = CASES[case]
    g = _gen(seed, sorted(CASES).index(case), k)
    e = torch.randint(lo, hi + 1, (n,), generator=g).double()
    mag = torch.pow(torch.tensor(2.0, dtype=torch.float64), e) * (1 + torch.rand(n, generator=g, dtype=torch.float64))
    sign = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()
    out = (mag * sign).float()
    if zero:
        out[zero_mask(n)] = 0.0
    return out


def clip_ref(sumsq, grad_scale, max_norm, hyper="fp32"):
    r = f32 if hyper == "fp32" else float
    gs, mn, tiny = r(grad_scale), r(max_norm), r(1e-6)
    return gs * min(1.0, mn / (math.sqrt(sumsq) * gs + tiny)) if mn > 0 else gs


def bias_corrections(b1, b2, step, hyper="fp32"):
    """1 - b1^t and sqrt(1 - b2^t) in Python doubles"""
    r = f32 if hyper == "fp32" else float
    return 1.0 - r(b1) ** step, math.sqrt(1.0 - r(b2) ** step)


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, step, sumsq, grad_scale, max_norm, hyper="fp32"):
    """-> p', m', v' (float64) and the bounds on |dp|, |dm|, |dv|.  hyper="fp32": every scalar is rounded to float32 first and then used as a double (what the C
    ABI carries, so what a kernel can be held to); hyper="exact": Python doubles, as torch uses them."""
    assert hyper in ("fp32", "exact")
    r = f32 if hyper == "fp32" else float
    lr, b1, b2, eps, wd = r(lr), r(b1), r(b2), r(eps), r(wd)
    p, g, m, v = (t.detach().double().cpu() for t in (p, g, m, v))
    clip = clip_ref(float(sumsq), grad_scale, max_norm, hyper)
    gh = g * clip
    pd = p * (1.0 - lr * wd)
    m1 = b1 * m + (1.0 - b1) * gh
    v1 = b2 * v + (1.0 - b2) * gh * gh
    bc1, bc2s = 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)
    denom = v1.sqrt() / bc2s + eps
    upd = (lr / bc1) * m1 / denom
    p1 = pd - upd
    s = (b1 * m).abs() + ((1.0 - b1) * gh).abs()
    bound_v = K * U * v1
    bound_m = K * U * s
    bound_p = K * U * (pd.abs() + upd.abs()) + (lr / bc1) * K * U * s / denom
    return p1, m1, v1, bound_p, bound_m, bound_v


def smallest_v_term(g, sumsq, grad_scale, max_norm, b2=B2):
    """the smallest non-zero (1 - b2) g^2 of a step (non-vacuity: at least 2^-120, so everything stays in fp32's normal range)"""
    gh = g.double() * clip_ref(float(sumsq), grad_scale, max_norm)
    t = (1.0 - f32(b2)) * gh * gh
    return t[t > 0].min().item()


def _worst(name, got, ref, bound, inputs):
    """(ratio of the worst element to its bound, a description of it).  A zero bound (zero state, zero gradient) admits a zero error only."""
    err = (got.detach().double().cpu() - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    i = int(ratio.argmax())
    what = "%s[%d]: got %.9e want %.17e, |err| %.3e = %.3f of the bound %.3e (%.2f units of 2^-24); inputs %s" % (
        name, i, got[i].item(), ref[i].item(), err[i].item(), ratio[i].item(), bound[i].item(), ratio[i].item() * K,
        ", ".join("%s=%.9e" % (k, t[i].item()) for k, t in inputs.items()))
    return ratio[i].item(), what


def check_step(what, got, ref, inputs):
    """got = (p', m', v') of a kernel or an emulation, ref = adamw_ref(...) on the same inputs, inputs = {name: tensor} for the message.
    -> {"p": ratio, "m": ratio, "v": ratio}: the largest |error| / bound of each output; AssertionError naming the worst element where one exceeds 1."""
    ratios, bad = {}, []
    for k, name in enumerate(("p", "m", "v")):
        ratios[name], msg = _worst(name, got[k], ref[k], ref[3 + k], inputs)
        if not ratios[name] <= 1.0:
            bad.append(msg)
    assert not bad, "%s: outside the bound\n  %s" % (what, "\n  ".join(bad))
    return ratios


def check_zero_gradient(what, p0, got, m0, v0, g, lr, wd):
    """An element with zero moments and a zero gradient: m' and v' are exactly 0 and p' is p (1 - lr wd) as fp32 rounds it — p - fl(lr wd) p with one rounding
    (contracted to an FMA) or with two.  -> the number of such elements."""
    z = ((g == 0) & (m0 == 0) & (v0 == 0)).cpu()
    gp, gm, gv = (t.detach().cpu() for t in got)
    assert (gm[z] == 0).all() and (gv[z] == 0).all(), "%s: a moment of an element with zero state and zero gradient is not 0" % what
    lw = torch.tensor(lr, dtype=torch.float32) * torch.tensor(wd, dtype=torch.float32)
    pz = p0.detach().cpu()[z]
    fused = (pz.double() - lw.double() * pz.double()).float()        # 24 x 24 bit product: exact in double; the difference rounds once
    unfused = pz - lw * pz
    ok = (gp[z] == fused) | (gp[z] == unfused)
    assert ok.all(), "%s: p' of %d elements with zero state and zero gradient is not p (1 - lr wd) as rounded, first: p %.9e -> %.9e, want %.9e" % (
        what, int((~ok).sum()), pz[~ok][0].item(), gp[z][~ok][0].item(), fused[~ok][0].item())
    return int(z.sum())


# ---- cast_ ------------------------------------------------------------------------------------------------------------------------------------------
CAST_LOW16 = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def fp32_edge_patterns():
    """every fp32 whose upper 16 bits run over all 65 536 values and whose lower 16 bits are one of CAST_LOW16: every tie of a 16-bit rounding and its two
    neighbours, every NaN class, +-inf, +-0, the subnormals and everything that overflows fp16 — 393 216 values"""
    hi = torch.arange(65536, dtype=torch.int64)[:, None] << 16
    lo = torch.tensor(CAST_LOW16, dtype=torch.int64)[None, :]
    bits = (hi | lo).reshape(-1)
    return torch.where(bits >= 1 << 31, bits - (1 << 32), bits).to(torch.int32).view(torch.float32)


def all_16bit_patterns(dtype):
    return (torch.arange(65536, dtype=torch.int32) - 32768).to(torch.int16).view(dtype)


def sum_rounded_once(a, b):
    """float32(a + b) of float64 a, b with ONE rounding.  The float64 sum of two numbers whose exponents lie far apart is itself rounded, and rounding that to
    float32 can land on the other side of a tie; so the float64 sum is rounded to odd first (TwoSum gives the sign of what was lost), after which the rounding to
    24 bits equals the rounding of the exact sum."""
    s = a + b
    bb = s - a
    e = (a - (s - bb)) + (b - bb)
    fix = torch.isfinite(s) & torch.isfinite(e) & (e != 0) & ((s.view(torch.int64) & 1) == 0)
    toward = torch.where(e > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    return torch.where(fix, torch.nextafter(s, toward), s).float()


def assert_same_bits_or_both_nan(what, got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    it = {2: torch.int16, 4: torch.int32}[got.element_size()]
    bad = (got.view(it) != want.view(it)) & ~(torch.isnan(got) & torch.isnan(want))
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError("%s: %d of %d differ, first at %d: got %r (0x%x) want %r (0x%x)" % (
            what, int(bad.sum()), bad.numel(), i, got[i].item(), got.view(it)[i].item() & (2 ** (8 * got.element_size()) - 1), want[i].item(),
            want.view(it)[i].item() & (2 ** (8 * got.element_size()) - 1)))
