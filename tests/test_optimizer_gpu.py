"""The flat optimizer's kernels (csrc/bwd.hip: e2eft_adamw_step, e2eft_adamw_step_guarded, e2eft_ema_step, e2eft_cast) element by element against float64:
every p', m' and v' of one AdamW step inside the bounds of tests/optimizer_ref.py (K = 20 units of 2^-24, from the operation count) at the project's learning
rate, at training-scale gradients where eps dominates the denominator, with grad_scale != 1 and at step counts up to 20 000; buffers that need a second
grid-stride trip; and `cast_` bit for bit on every tie, NaN, infinity, subnormal and fp16 overflow.  tests/test_optimizer_ref_cpu.py shows that eight plausible
defects leave these bounds.

Measured on an MI355X, both AdamW kernels alike: at most 0.131 of the bound for p, 0.175 for m and 0.321 for v (2.6, 3.5 and 6.4 units of 2^-24), the figures of
the float32 emulation to the last digit.  Before e2eft_adamw_step took its bias corrections in double, its p' left the bound at steps 2 and 3 of six of the seven
cases (1.04 to 1.53 of it; at training scale eps hides bc2: 0.80); before the accumulate form of e2eft_cast became one FMA, y + 2 x was inf or NaN where 2 x alone
overflows and the sum does not, y + x / 8 lost the bits of a subnormal product, and x / 3 - fl(x / 3) was 0."""
import math

import pytest
import torch

import optimizer_ref as R

pytestmark = pytest.mark.gpu

KERNELS = ("guarded", "unguarded")
N_ADAMW_LARGE = 16384 * 256 + 5 * 256 + 3          # grid_for caps at 16384 blocks of 256: a second trip of 5 blocks and a tail of 3
N_EMA_LARGE = 4 * 16384 * 256 + 4 * 300 + 3        # the EMA kernel moves 4 elements per thread


@pytest.fixture(scope="module")
def ops(dev):
    from diffusion_e2e_ft_amd import ops as _ops
    return _ops


def _ulp32(x):
    return abs(x) * 2.0 ** -23


def _step(ops, dev, kernel, p, g, m, v, t, lr, wd, gs, mn, ss=None):
    """one step of `kernel` in place on device tensors; -> (sumsq as a Python float, state, coef) with state / coef None for the unguarded kernel"""
    if ss is None:
        ss = ops.sumsq(g)
    if kernel == "guarded":
        state = torch.tensor([t - 1, 0], dtype=torch.int64, device=dev)
        coef = torch.full((4,), -7.0, device=dev)
        ops.adamw_step_guarded_(p, g, m, v, lr, R.B1, R.B2, R.EPS, wd, state, coef, ss, grad_scale=gs, max_norm=mn)
        return ss.item(), state.cpu(), coef.cpu()
    ops.adamw_step_(p, g, m, v, lr, R.B1, R.B2, R.EPS, wd, t, grad_sumsq=ss, grad_scale=gs, max_norm=mn)
    return ss.item(), None, None


def _check_coef(what, state, coef, t, ss, gs, mn):
    assert state.tolist() == [t, 0], (what, state.tolist())
    assert coef[3].item() == 1.0, (what, coef.tolist())
    bc1, bc2s = R.bias_corrections(R.B1, R.B2, t)
    for k, want in ((1, R.f32(bc1)), (2, R.f32(bc2s))):
        assert abs(coef[k].item() - want) <= _ulp32(want), "%s: coef[%d] = %.9e, want %.9e within one fp32 ulp" % (what, k, coef[k].item(), want)
    clip = R.clip_ref(ss, gs, mn)
    assert abs(coef[0].item() - clip) <= 6 * R.U * clip, "%s: clip %.9e, want %.9e within 6 * 2^-24" % (what, coef[0].item(), clip)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_adamw_step_per_element(ops, dev, case, kernel):
    """Teacher-forced: the reference of every step starts from the device's own p, m, v of the step before, so no drift bound is needed.  The guarded kernel reads
    the step from state[0] = t - 1, the unguarded one from its argument; a fresh gradient per step."""
    _, _, gs, mn, lr, wd, zero = R.CASES[case]
    p, m, v = R.make_params(R.N).to(dev), torch.zeros(R.N, device=dev), torch.zeros(R.N, device=dev)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for k, t in enumerate(R.STEPS):
        g = R.make_grad(case, k, R.N)
        p0, m0, v0 = p.cpu(), m.cpu(), v.cpu()
        ss, state, coef = _step(ops, dev, kernel, p, g.to(dev), m, v, t, lr, wd, gs, mn)
        what = "%s, %s kernel, step %d" % (case, kernel, t)
        exact = float((g.double() ** 2).sum())
        assert abs(ss - exact) <= 1e-12 * exact, (what, ss, exact)
        if kernel == "guarded":
            _check_coef(what, state, coef, t, ss, gs, mn)
        ref = R.adamw_ref(p0, g, m0, v0, lr, R.B1, R.B2, R.EPS, wd, t, ss, gs, mn, "fp32")
        got = (p.cpu(), m.cpu(), v.cpu())
        r = R.check_step(what, got, ref, {"p": p0, "g": g, "m": m0, "v": v0})
        if zero:
            assert R.check_zero_gradient(what, p0, got, m0, v0, g, lr, wd) >= R.N // 4
        print("%s: ratio to the bound p %.3f m %.3f v %.3f" % (what, r["p"], r["m"], r["v"]))
        worst = {n: max(worst[n], r[n]) for n in worst}
    print("WORST %s %s: p %.3f m %.3f v %.3f of the bound" % (case, kernel, worst["p"], worst["m"], worst["v"]))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("bad", ("inf", "nan", "nan_in_g"))
def test_adamw_skipped_step(ops, dev, bad, kernel):
    """a non-finite sum of squares: p, m, v keep their bits; the guarded kernel counts the skip and does not advance the bias-correction step"""
    case, t = "unit_clipped", 3
    _, _, gs, mn, lr, wd, _ = R.CASES[case]
    g = R.make_grad(case, 0, R.N)
    if bad == "nan_in_g":
        g[R.N // 2] = float("nan")
    p0, m0, v0 = R.make_params(R.N), 0.1 * R.make_grad(case, 1, R.N), R.make_grad(case, 2, R.N) ** 2
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    ss = torch.tensor([float("inf") if bad == "inf" else float("nan")], dtype=torch.float64, device=dev)
    if bad == "nan_in_g":
        ss = ops.sumsq(g.to(dev))
        assert math.isnan(ss.item())
    _, state, coef = _step(ops, dev, kernel, p, g.to(dev), m, v, t, lr, wd, gs, mn, ss=ss)
    for name, got, want in (("p", p, p0), ("m", m, m0), ("v", v, v0)):
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), "%s changed on a skipped step" % name
    if kernel == "guarded":
        assert state.tolist() == [t - 1, 1] and coef.tolist() == [0.0, 1.0, 1.0, 0.0], (state.tolist(), coef.tolist())


# ---- large buffers: the second grid-stride trip and the tails ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_adamw_beyond_the_grid_cap(ops, dev, kernel):
    case, t, n = "unit_averaged_8_ranks", 3, N_ADAMW_LARGE
    _, _, gs, mn, lr, wd, _ = R.CASES[case]
    p0, g = R.make_params(n), R.make_grad(case, 0, n)
    m0, v0 = 0.1 * R.make_grad(case, 1, n), R.make_grad(case, 2, n) ** 2
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    ss, state, coef = _step(ops, dev, kernel, p, g.to(dev), m, v, t, lr, wd, gs, mn)
    what = "%s, %s kernel, n = %d" % (case, kernel, n)
    if kernel == "guarded":
        _check_coef(what, state, coef, t, ss, gs, mn)
    got = (p.cpu(), m.cpu(), v.cpu())
    r = R.check_step(what, got, R.adamw_ref(p0, g, m0, v0, lr, R.B1, R.B2, R.EPS, wd, t, ss, gs, mn, "fp32"), {"p": p0, "g": g, "m": m0, "v": v0})
    print("WORST large %s: p %.3f m %.3f v %.3f of the bound" % (kernel, r["p"], r["m"], r["v"]))
    # the last 2000 elements, and on their own the 5 * 256 + 3 of them beyond 16384 * 256 that only a second trip reaches
    for tail in (slice(n - 2000, n), slice(16384 * 256, n)):
        for name, a, b in (("p", got[0], p0), ("m", got[1], m0), ("v", got[2], v0)):
            assert (a[tail] != b[tail]).double().mean().item() >= 0.9, "%s: elements %d..%d were not updated" % (name, tail.start, tail.stop)


@pytest.mark.parametrize("omd", (0.1, 1 - 0.9999, 1.0))
def test_ema_beyond_the_grid_cap(ops, dev, omd):
    """bit-equal to torch's fp32 s - omd * (s - p) on the CPU (sub, mul, sub: no contraction), over four-element vectors, a second trip and a tail of 3"""
    gen = torch.Generator().manual_seed(41)
    s0 = torch.randn(N_EMA_LARGE, generator=gen)
    p = torch.randn(N_EMA_LARGE, generator=gen)
    s = s0.to(dev)
    ops.ema_step_(s, p.to(dev), omd)
    want = s0 - omd * (s0 - p)
    R.assert_same_bits_or_both_nan("ema, 1 - decay = %r" % omd, s.cpu(), want)
    if omd == 1.0:
        assert (want[-2000:] != s0[-2000:]).all()


def test_cast_beyond_the_grid_cap(ops, dev):
    gen = torch.Generator().manual_seed(42)
    x = torch.randn(N_ADAMW_LARGE, generator=gen)
    y = torch.zeros(N_ADAMW_LARGE, dtype=torch.bfloat16, device=dev)
    ops.cast_(x.to(dev), y)
    R.assert_same_bits_or_both_nan("fp32 -> bf16", y.cpu(), x.to(torch.bfloat16))
    assert (y.cpu()[-2000:] != 0).all()
    acc0 = torch.randn(N_ADAMW_LARGE, generator=gen)
    acc = acc0.to(dev)
    ops.cast_(x.to(dev), acc, mul=2.0, accumulate=True)
    R.assert_same_bits_or_both_nan("fp32 += 2 fp32", acc.cpu(), R.sum_rounded_once(acc0.double(), 2.0 * x.double()))


# ---- cast_, exhaustively at the edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16))
def test_cast_from_fp32_every_edge(ops, dev, dtype):
    x = R.fp32_edge_patterns()
    y = torch.zeros(x.numel(), dtype=dtype, device=dev)
    ops.cast_(x.to(dev), y)
    R.assert_same_bits_or_both_nan("fp32 -> %s" % dtype, y.cpu(), x.to(dtype))


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float16))
def test_cast_to_fp32_every_pattern(ops, dev, dtype):
    x = R.all_16bit_patterns(dtype)
    y = torch.zeros(x.numel(), dtype=torch.float32, device=dev)
    ops.cast_(x.to(dev), y)
    R.assert_same_bits_or_both_nan("%s -> fp32" % dtype, y.cpu(), x.float())


def _accumulate_inputs(out_dtype, mul):
    """x: the fp32 edge patterns.  y, by index modulo 4: an unrelated pattern (the same set, or every 16-bit pattern six times over, shifted); -fl(x * mul), so that
    the sum is what a separately rounded product loses; -x (2 x overflows where 2 x - x does not); x itself (carries, sums that overflow)."""
    x = R.fp32_edge_patterns()
    y = torch.roll(x if out_dtype == torch.float32 else R.all_16bit_patterns(out_dtype).repeat(6).float(), 100003)
    i = torch.arange(x.numel()) % 4
    y = torch.where(i == 1, -(x * torch.tensor(mul, dtype=torch.float32)), torch.where(i == 2, -x, torch.where(i == 3, x, y)))
    return x, y.to(out_dtype).contiguous()


@pytest.mark.parametrize("out_dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("mul", (1.0, 2.0, 0.125))
def test_cast_accumulate_power_of_two(ops, dev, mul, out_dtype):
    """y + x * mul: the float64 sum rounded once to fp32 and then to the output type.  The product by a power of two is exact (fused; and unfused wherever it
    stays in the normal range)."""
    x, y0 = _accumulate_inputs(out_dtype, mul)
    y = y0.to(dev)
    ops.cast_(x.to(dev), y, mul=mul, accumulate=True)
    want = R.sum_rounded_once(y0.double(), x.double() * mul).to(out_dtype)
    R.assert_same_bits_or_both_nan("%s += %r * fp32" % (out_dtype, mul), y.cpu(), want)


@pytest.mark.parametrize("out_dtype", (torch.float32, torch.bfloat16))
def test_cast_accumulate_one_third(ops, dev, out_dtype):
    """mul = 1/3 is no power of two: a separately rounded product is half an ulp of x / 3 off, which is everything where y cancels it.  The one FMA of the kernel
    leaves the rounding of the exact sum; held to one ulp of the output type."""
    from util import _ulp_index
    x, y0 = _accumulate_inputs(out_dtype, 1.0 / 3.0)
    y = y0.to(dev)
    ops.cast_(x.to(dev), y, mul=1.0 / 3.0, accumulate=True)
    want = R.sum_rounded_once(y0.double(), x.double() * R.f32(1.0 / 3.0)).to(out_dtype)
    got = y.cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    d = (_ulp_index(got) - _ulp_index(want)).abs()[~nan]
    assert d.max().item() <= 1, "%d elements more than one ulp off, largest %d" % (int((d > 1).sum()), int(d.max()))
