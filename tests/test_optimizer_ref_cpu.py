"""The float64 AdamW reference of tests/optimizer_ref.py against torch.optim.AdamW, and its bounds against a float32 emulation of the kernel's operation order:
the emulation stays inside every bound on every case of test_optimizer_gpu.py, and each of eight plausible defects, switched on in the emulation, leaves one —
so the device tests can fail for those defects without any device code being touched here."""
import math

import pytest
import torch

import optimizer_ref as R

F = torch.float32
MUTATIONS = ("no_eps", "eps_inside_bias_correction", "bc2_without_sqrt", "clip_from_unscaled_norm", "m_from_unclipped_gradient", "one_minus_beta2_literal",
             "no_weight_decay", "fp32_pow")


def _t(x):
    return torch.tensor(float(x), dtype=F)


def emulate(p, g, m, v, lr, b1, b2, eps, wd, step, sumsq, grad_scale, max_norm, mutate=None):
    """adamw_prepare_kernel + adamw_guarded_kernel (csrc/bwd.hip) in torch float32, one rounding per operation (no FMA); `mutate` switches one defect on"""
    assert mutate is None or mutate in MUTATIONS, mutate
    lr, b1, b2, eps, wd, gs, mn = (_t(x) for x in (lr, b1, b2, eps, wd, grad_scale, max_norm))
    clip = gs
    if mn.item() > 0:
        nrm = _t(math.sqrt(sumsq))
        if mutate != "clip_from_unscaled_norm":
            nrm = nrm * gs
        clip = clip * torch.minimum(_t(1.0), mn / (nrm + _t(1e-6)))
    if mutate == "fp32_pow":
        bc1 = _t(1.0) - torch.pow(b1, _t(step))
        bc2 = _t(1.0) - torch.pow(b2, _t(step))
        bc2s = bc2.sqrt()
    else:
        bc1 = _t(1.0 - b1.double().item() ** step)
        bc2 = _t(1.0 - b2.double().item() ** step)
        bc2s = _t(math.sqrt(1.0 - b2.double().item() ** step))
    gi = g * clip
    pi = p if mutate == "no_weight_decay" else p - (lr * wd) * p
    mi = b1 * m + (_t(1.0) - b1) * (g if mutate == "m_from_unclipped_gradient" else gi)
    omb2 = _t(0.001) if mutate == "one_minus_beta2_literal" else _t(1.0) - b2
    vi = b2 * v + omb2 * gi * gi
    if mutate == "no_eps":
        denom = vi.sqrt() / bc2s
    elif mutate == "eps_inside_bias_correction":
        denom = (vi.sqrt() + eps) / bc2s
    elif mutate == "bc2_without_sqrt":
        denom = vi.sqrt() / bc2 + eps
    else:
        denom = vi.sqrt() / bc2s + eps
    return pi - (lr / bc1) * (mi / denom), mi, vi


def run_case(case, mutate=None):
    """the seven teacher-forced steps of a case through the emulation -> the largest ratio to the bound of p, m, v; AssertionError from the first step outside"""
    _, _, gs, mn, lr, wd, zero = R.CASES[case]
    p, m, v = R.make_params(R.N), torch.zeros(R.N), torch.zeros(R.N)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for k, t in enumerate(R.STEPS):
        g = R.make_grad(case, k, R.N)
        ss = float((g.double() ** 2).sum())
        ref = R.adamw_ref(p, g, m, v, lr, R.B1, R.B2, R.EPS, wd, t, ss, gs, mn, "fp32")
        got = emulate(p, g, m, v, lr, R.B1, R.B2, R.EPS, wd, t, ss, gs, mn, mutate)
        what = "%s, step %d%s" % (case, t, ", " + mutate if mutate else "")
        r = R.check_step(what, got, ref, {"p": p, "g": g, "m": m, "v": v})
        if zero:
            assert R.check_zero_gradient(what, p, got, m, v, g, lr, wd) >= R.N // 4
        worst = {n: max(worst[n], r[n]) for n in worst}
        p, m, v = got
    return worst


def test_reference_equals_torch_adamw_after_clip_grad_norm():
    """teacher-forced for 20 steps: adamw_ref(hyper="exact") on torch's own p, m, v of the step before equals clip_grad_norm_ + torch.optim.AdamW in float64"""
    gen = torch.Generator().manual_seed(3)
    n, lr, wd, mn = 4099, 3e-3, 1e-2, 1.0
    ref = torch.nn.Parameter(torch.randn(n, generator=gen, dtype=torch.float64))
    opt = torch.optim.AdamW([ref], lr=lr, betas=(R.B1, R.B2), eps=R.EPS, weight_decay=wd)
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 21):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * (5.0 if t % 3 == 2 else 0.003)      # clipped steps and idle ones
        p0 = ref.detach().clone()
        p1, m1, v1 = R.adamw_ref(p0, g, m, v, lr, R.B1, R.B2, R.EPS, wd, t, float((g * g).sum()), 1.0, mn, "exact")[:3]
        ref.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([ref], mn)
        opt.step()
        m, v = opt.state[ref]["exp_avg"].clone(), opt.state[ref]["exp_avg_sq"].clone()
        for name, got, want in (("p", p1, ref.detach()), ("m", m1, m), ("v", v1, v)):
            err = ((got - want).abs().max() / want.abs().max()).item()
            assert err <= 1e-12, (t, name, err)
        assert int(opt.state[ref]["step"]) == t


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_emulation_stays_inside_the_bounds(case):
    worst = run_case(case)
    print("%s: largest ratio to the bound p %.3f m %.3f v %.3f (units of 2^-24: %.2f %.2f %.2f)" % (
        case, worst["p"], worst["m"], worst["v"], worst["p"] * R.K, worst["m"] * R.K, worst["v"] * R.K))


@pytest.mark.parametrize("mutate", MUTATIONS)
def test_a_defect_breaks_a_bound(mutate):
    """Each defect leaves a bound on at least one case.  Seven of them leave the per-element bounds of p, m or v; the omitted weight decay moves p by
    lr wd = 3e-7 of itself, 5 units of 2^-24 and so inside K = 20, and is caught by the exact p' of the elements with zero state and zero gradient."""
    broken = []
    for case in sorted(R.CASES):
        try:
            run_case(case, mutate)
        except AssertionError as e:
            broken.append((case, str(e).splitlines()[0]))
    print(mutate, "breaks", [c for c, _ in broken])
    assert broken, "%s passes every case: the bounds cannot see it" % mutate


def test_every_case_keeps_v_in_the_normal_range():
    """non-vacuity: the smallest non-zero (1 - b2) g^2 of every step of every case is at least 2^-120, so flush-to-zero behaviour is not what is being tested"""
    for case, (_, _, gs, mn, _, _, _) in R.CASES.items():
        for k in range(len(R.STEPS)):
            g = R.make_grad(case, k, R.N)
            assert R.smallest_v_term(g, float((g.double() ** 2).sum()), gs, mn) >= 2.0 ** -120, (case, k)


def test_cases_are_what_they_claim():
    p = R.make_params(R.N)
    assert (p[0::4] == 0).all() and (p[3::4].abs() == 8).all() and (p[1::4].abs() >= 2.0 ** -20).all() and (p[1::4].abs() < 2.0 ** -19).all()
    for case, (lo, hi, gs, mn, _, _, zero) in R.CASES.items():
        g = R.make_grad(case, 0, R.N)
        nz = g[g != 0].abs()
        assert nz.min() >= 2.0 ** lo and nz.max() < 2.0 ** (hi + 1) and (g < 0).any() and (g > 0).any()
        assert abs((g == 0).double().mean().item() - zero) < 1e-3
        clip = R.clip_ref(float((g.double() ** 2).sum()), gs, mn)
        assert (clip < gs) == (case not in ("training_scale", "around_eps")), case     # the clip is active exactly where the case says so
    g = R.make_grad("around_eps", 0, R.N).double().abs()       # sqrt(v') = sqrt(1 - b2) |g| / sqrt(bc2) = |g| at step 1: on both sides of eps
    assert (g < R.EPS).any() and (g > R.EPS).any()


def test_fp32_hyperparameters_lower_v_by_1_29e_5():
    """The C ABI carries beta2 as float32(0.999), which is 1.29e-5 (1 - beta2) above 0.999: v' is that much, relatively, below torch's and by no more
    (the update then about 6.4e-6 above).  Documented next to the entry points in include/e2eft.h."""
    shift = (1.0 - R.f32(R.B2)) / (1.0 - R.B2) - 1.0
    assert -1.30e-5 < shift < -1.28e-5
    case = "unit_clipped"
    _, _, gs, mn, lr, wd, _ = R.CASES[case]
    p, g = R.make_params(R.N), R.make_grad(case, 0, R.N)
    ss = float((g.double() ** 2).sum())
    zeros = torch.zeros(R.N)
    a = R.adamw_ref(p, g, zeros, zeros, lr, R.B1, R.B2, R.EPS, wd, 1, ss, gs, mn, "fp32")
    b = R.adamw_ref(p, g, zeros, zeros, lr, R.B1, R.B2, R.EPS, wd, 1, ss, gs, mn, "exact")
    rel = (a[2] - b[2]) / b[2]
    assert (rel - shift).abs().max().item() < 1e-9, (rel.min().item(), rel.max().item(), shift)
    v0 = b[2]                                                   # with a state: b2 v is 1.3e-8 above, (1 - b2) g^2 1.29e-5 below: never beyond the latter
    g1 = R.make_grad(case, 1, R.N)
    ss1 = float((g1.double() ** 2).sum())
    a = R.adamw_ref(p, g1, zeros, v0, lr, R.B1, R.B2, R.EPS, wd, 2, ss1, gs, mn, "fp32")
    b = R.adamw_ref(p, g1, zeros, v0, lr, R.B1, R.B2, R.EPS, wd, 2, ss1, gs, mn, "exact")
    rel = (a[2] - b[2]) / b[2]
    assert rel.max().item() <= 1.3e-8 and rel.min().item() >= shift - 1e-9, (rel.min().item(), rel.max().item())


def test_sum_rounded_once():
    """1 + (2^-24 + 2^-60) lies above the tie between 1 and 1 + 2^-23; the plain float64 sum loses the 2^-60 and rounds to even, i.e. down"""
    a = torch.tensor([1.0, 1.0, -1.0, 1.0, float("inf"), 3.0e38], dtype=torch.float64)
    b = torch.tensor([2.0 ** -24 + 2.0 ** -60, 2.0 ** -24, -(2.0 ** -24 + 2.0 ** -60), 2.0 ** -24 - 2.0 ** -70, -float("inf"), 3.0e38], dtype=torch.float64)
    got = R.sum_rounded_once(a, b)
    assert got[0].item() == 1.0 + 2.0 ** -23 and got[1].item() == 1.0 and got[2].item() == -(1.0 + 2.0 ** -23) and got[3].item() == 1.0
    assert math.isnan(got[4].item()) and got[5].item() == float("inf")
    assert (a + b).float()[0].item() == 1.0          # what the helper is for
    x = R.fp32_edge_patterns()
    assert x.numel() == 393216 and torch.isnan(x).any() and torch.isinf(x).any() and (x == 0).sum().item() == 2
