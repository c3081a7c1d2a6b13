"""The grouped flat-optimizer kernels (csrc/bwd.hip: e2eft_adamw_step_groups, e2eft_adamw_step_groups_at) on about 1e5 elements:
  1. same hyper-parameters in every group, groups covering the buffer: the bits of `adamw_step_guarded_` (parameters, moments, counters, clip factor);
  2. different hyper-parameters per group: every group's range holds the bits `adamw_step_guarded_` writes there with that group's hyper-parameters, and
     whatever lies in no group keeps its bits;
  3. per element against float64 inside the bounds of tests/optimizer_ref.py (K = 20), one group with betas (0.8, 0.99) — a shared bias correction leaves them;
  4. a non-finite sum of squares skips every group and does not advance the bias-correction step;
  5. the `_at` form, captured once and replayed with other learning-rate words, equals eager by-value steps bit for bit;
  6. containment: both entry points on the interior of guarded buffers under both fills (tests/containment.py).
Group ranges hit the edges: 8 elements, 264 (one 256-thread block and 8 more), a large one, an empty one, a gap of 8 nobody owns, a tail nobody owns, 8 groups."""
import ctypes
import math

import pytest
import torch

import optimizer_ref as R
from containment import check_two_fills, guarded

pytestmark = pytest.mark.gpu

N = R.N
# (begin, end) per group.  COVER*: every element in a group (test 1); EDGES / EIGHT: a gap [272, 280) and an unowned tail
COVER4 = ((0, 8), (8, 272), (272, 272), (272, N))
COVER8 = ((0, 8), (8, 272), (272, 272), (272, 1000), (1000, 1001), (1001, 50000), (50000, 70003), (70003, N))
EDGES = ((0, 8), (8, 272), (272, 272), (280, 90000))
EIGHT = ((0, 8), (8, 272), (272, 272), (280, 1000), (1000, 1001), (1001, 50000), (50000, 70003), (70003, 90000))
LAYOUTS = {"edges": EDGES, "eight": EIGHT}
# (lr, weight decay, beta1, beta2, eps) of group k; the large groups of both layouts (index 3 and 5) carry betas that are not the usual pair
HYPER = ((3e-5, 1e-2, 0.9, 0.999, 1e-8), (3e-4, 0.0, 0.9, 0.999, 1e-8), (1e-3, 1e-2, 0.5, 0.9, 1e-6), (1e-4, 5e-2, 0.8, 0.99, 1e-7),
         (3e-3, 0.0, 0.95, 0.98, 1e-8), (2e-5, 1e-1, 0.8, 0.99, 1e-6), (5e-4, 1e-3, 0.85, 0.9995, 1e-8), (7e-5, 0.0, 0.9, 0.95, 1e-9))


@pytest.fixture(scope="module")
def ops(dev):
    from diffusion_e2e_ft_amd import ops as _ops
    return _ops


def _table(ranges, hyper=HYPER):
    return [(b, e, hyper[k][0], hyper[k][2], hyper[k][3], hyper[k][4], hyper[k][1]) for k, (b, e) in enumerate(ranges)]


def _state(dev, applied, skipped=0):
    return torch.tensor([applied, skipped], dtype=torch.int64, device=dev)


def _coef(dev, n_groups):
    return torch.full((2 + 2 * n_groups,), -7.0, device=dev)


def _inputs(case, n=N):
    """p, m, v (a state worth reading: non-zero moments) and the gradient of a case, on the CPU"""
    return R.make_params(n), 0.1 * R.make_grad(case, 1, n), R.make_grad(case, 2, n) ** 2, R.make_grad(case, 0, n)


def _same_bits(what, got, want):
    got, want = got.cpu(), want.cpu()
    if got.is_floating_point():
        got, want = got.view(torch.int32), want.view(torch.int32)
    ne = got != want
    assert not ne.any(), "%s: %d of %d elements differ, first at %d" % (what, int(ne.sum()), ne.numel(), int(ne.nonzero()[0]))


def _owned(ranges, n=N):
    mask = torch.zeros(n, dtype=torch.bool)
    for b, e in ranges:
        mask[b:e] = True
    return mask


# ---- 1. same hyper-parameters, same bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cover", ("cover4", "cover8"))
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_same_hyper_parameters_give_the_bits_of_the_single_group_kernel(ops, dev, case, cover):
    _, _, gs, mn, lr, wd, _ = R.CASES[case]
    ranges = COVER4 if cover == "cover4" else COVER8
    assert ranges[0][0] == 0 and ranges[-1][1] == N and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    table = [(b, e, lr, R.B1, R.B2, R.EPS, wd) for b, e in ranges]
    p, m, v = R.make_params(N).to(dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    for k, t in enumerate(R.STEPS[:4]):
        g = R.make_grad(case, k, N).to(dev)
        ss = ops.sumsq(g)
        p2, m2, v2 = p.clone(), m.clone(), v.clone()
        st1, c1, st2, c2 = _state(dev, t - 1), torch.full((4,), -7.0, device=dev), _state(dev, t - 1), _coef(dev, len(ranges))
        ops.adamw_step_guarded_(p, g, m, v, lr, R.B1, R.B2, R.EPS, wd, st1, c1, ss, grad_scale=gs, max_norm=mn)
        ops.adamw_step_groups_(p2, g, m2, v2, table, st2, c2, ss, grad_scale=gs, max_norm=mn)
        what = "%s, %s, step %d" % (case, cover, t)
        for name, a, b in (("p", p2, p), ("m", m2, m), ("v", v2, v), ("state", st2, st1), ("clip", c2[0:1], c1[0:1])):
            _same_bits("%s: %s" % (what, name), a, b)
        assert st2.tolist() == [t, 0] and c2[1].item() == 1.0
        for j in range(len(ranges)):
            _same_bits("%s: bias corrections of group %d" % (what, j), c2[2 + 2 * j:4 + 2 * j], c1[1:3])
        assert not torch.equal(p2.cpu()[-2000:], R.make_params(N)[-2000:])


# ---- 2. different hyper-parameters per group -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("case", ("unit_clipped", "training_scale"))
def test_every_group_holds_what_the_single_group_kernel_writes_with_its_hyper_parameters(ops, dev, case, layout):
    _, _, gs, mn, _, _, _ = R.CASES[case]
    ranges, t = LAYOUTS[layout], 3
    p0, m0, v0, g = _inputs(case)
    gd = g.to(dev)
    ss = ops.sumsq(gd)
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    state, coef = _state(dev, t - 1), _coef(dev, len(ranges))
    ops.adamw_step_groups_(p, gd, m, v, _table(ranges), state, coef, ss, grad_scale=gs, max_norm=mn)
    assert state.tolist() == [t, 0]
    got = dict(p=p.cpu(), m=m.cpu(), v=v.cpu())
    for k, (b, e) in enumerate(ranges):
        if b == e:
            continue
        lr, wd, b1, b2, eps = HYPER[k]
        pk, mk, vk = p0.to(dev), m0.to(dev), v0.to(dev)
        ops.adamw_step_guarded_(pk, gd, mk, vk, lr, b1, b2, eps, wd, _state(dev, t - 1), torch.zeros(4, device=dev), ss, grad_scale=gs, max_norm=mn)
        for name, want in (("p", pk), ("m", mk), ("v", vk)):
            _same_bits("%s, %s, group %d [%d, %d): %s" % (case, layout, k, b, e, name), got[name][b:e], want[b:e])
        assert not torch.equal(got["p"][b:e], p0[b:e]) and not torch.equal(got["v"][b:e], v0[b:e])
    free = ~_owned(ranges)
    assert int(free.sum()) == 8 + N - 90000
    for name, before in (("p", p0), ("m", m0), ("v", v0)):
        _same_bits("%s, %s: %s outside every group" % (case, layout, name), got[name][free], before[free])


def test_a_group_beyond_the_grid_cap_takes_a_second_trip(ops, dev):
    """a group's blocks are capped at 16384: the second group here has 16384 * 256 + 5 * 256 + 3 elements and starts 8 elements into the buffer"""
    case, t = "unit_averaged_8_ranks", 3
    _, _, gs, mn, _, _, _ = R.CASES[case]
    n = 8 + 16384 * 256 + 5 * 256 + 3
    ranges = ((0, 8), (8, n))
    p0, m0, v0, g = _inputs(case, n)
    gd = g.to(dev)
    ss = ops.sumsq(gd)
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    ops.adamw_step_groups_(p, gd, m, v, _table(ranges), _state(dev, t - 1), _coef(dev, 2), ss, grad_scale=gs, max_norm=mn)
    lr, wd, b1, b2, eps = HYPER[1]
    pk, mk, vk = p0.to(dev), m0.to(dev), v0.to(dev)
    ops.adamw_step_guarded_(pk, gd, mk, vk, lr, b1, b2, eps, wd, _state(dev, t - 1), torch.zeros(4, device=dev), ss, grad_scale=gs, max_norm=mn)
    for name, a, b, before in (("p", p, pk, p0), ("m", m, mk, m0), ("v", v, vk, v0)):
        _same_bits("second trip: %s" % name, a[8:], b[8:])
        assert (a.cpu()[-1000:] != before[-1000:]).double().mean().item() >= 0.9, name


# ---- 3. float64 reference ----------------------------------------------------------------------------------------------------------------------------------
def _ulp32(x):
    return abs(x) * 2.0 ** -23


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("case", ("unit_clipped", "training_scale", "quarter_zero"))
def test_every_group_within_the_bounds_of_the_float64_reference(ops, dev, case, layout):
    """teacher-forced over steps 1, 2, 3 and 100: every group's elements against `adamw_ref` with that group's lr, weight decay, betas and eps.  Groups 3 (edges)
    and 3, 5 (eight) step with betas (0.8, 0.99): with the bias corrections of (0.9, 0.999) their p' is off by a factor of about two at step 2."""
    _, _, gs, mn, _, _, _ = R.CASES[case]
    ranges = LAYOUTS[layout]
    assert (HYPER[3][2], HYPER[3][3]) == (0.8, 0.99) and ranges[3][1] - ranges[3][0] > 256
    p, m, v = R.make_params(N).to(dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, t in enumerate((1, 2, 3, 100)):
        g = R.make_grad(case, i, N)
        p0, m0, v0 = p.cpu(), m.cpu(), v.cpu()
        ss = ops.sumsq(g.to(dev))
        state, coef = _state(dev, t - 1), _coef(dev, len(ranges))
        ops.adamw_step_groups_(p, g.to(dev), m, v, _table(ranges), state, coef, ss, grad_scale=gs, max_norm=mn)
        got, coef, ssf = (p.cpu(), m.cpu(), v.cpu()), coef.cpu(), ss.item()
        assert state.tolist() == [t, 0] and coef[1].item() == 1.0
        clip = R.clip_ref(ssf, gs, mn)
        assert abs(coef[0].item() - clip) <= 6 * R.U * clip, (coef[0].item(), clip)
        for k, (b, e) in enumerate(ranges):
            lr, wd, b1, b2, eps = HYPER[k]
            bc1, bc2s = R.bias_corrections(b1, b2, t)
            for j, want in ((2 + 2 * k, R.f32(bc1)), (3 + 2 * k, R.f32(bc2s))):
                assert abs(coef[j].item() - want) <= _ulp32(want), "group %d step %d: coef[%d] = %.9e, want %.9e within one fp32 ulp" % (k, t, j, coef[j].item(), want)
            if b == e:
                continue
            sl = slice(b, e)
            ref = R.adamw_ref(p0[sl], g[sl], m0[sl], v0[sl], lr, b1, b2, eps, wd, t, ssf, gs, mn, "fp32")
            what = "%s, %s, group %d [%d, %d), step %d" % (case, layout, k, b, e, t)
            r = R.check_step(what, tuple(x[sl] for x in got), ref, {"p": p0[sl], "g": g[sl], "m": m0[sl], "v": v0[sl]})
            worst = {n: max(worst[n], r[n]) for n in worst}
    print("WORST %s %s: p %.3f m %.3f v %.3f of the bound" % (case, layout, worst["p"], worst["m"], worst["v"]))


def test_the_reference_would_notice_a_shared_bias_correction():
    """non-vacuity of 3, on the CPU side of it: group 3's exact step 2 held against the bounds of a reference that corrects with betas (0.9, 0.999)"""
    b, e = EDGES[3]
    lr, wd, b1, b2, eps = HYPER[3]
    sl = slice(b, b + 4096)
    p0, g = R.make_params(N)[sl], R.make_grad("unit_clipped", 0, N)[sl]
    m0, v0 = 0.1 * R.make_grad("unit_clipped", 1, N)[sl], R.make_grad("unit_clipped", 2, N)[sl] ** 2
    right = R.adamw_ref(p0, g, m0, v0, lr, b1, b2, eps, wd, 2, 1.0, 1.0, 0.0, "fp32")
    bc1, bc2s = R.bias_corrections(b1, b2, 2)
    s1, s2 = R.bias_corrections(R.B1, R.B2, 2)
    pd = p0.double() * (1.0 - R.f32(lr) * R.f32(wd))
    shared = pd - (R.f32(lr) / s1) * right[1] / (right[2].sqrt() / s2 + R.f32(eps))
    with pytest.raises(AssertionError, match="outside the bound"):
        R.check_step("shared", (shared.float(), right[1].float(), right[2].float()), right, {"p": p0})
    assert bc1 != s1 and bc2s != s2


# ---- 4. a non-finite norm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("by_value", "at"))
@pytest.mark.parametrize("bad", ("inf", "nan"))
def test_a_non_finite_norm_skips_every_group(ops, dev, bad, form):
    case, applied, skipped = "unit_clipped", 5, 2
    _, _, gs, mn, _, _, _ = R.CASES[case]
    ranges = EIGHT
    p0, m0, v0, g = _inputs(case)
    gd = g.to(dev)
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    state, coef = _state(dev, applied, skipped), _coef(dev, len(ranges))
    lrs = [ctypes.c_float(h[0]).value for h in HYPER]
    hyper = torch.tensor([ctypes.c_float(gs).value] + lrs, dtype=torch.float32, device=dev)

    def step(ss, p, m, v, state, coef):
        if form == "at":
            ops.adamw_step_groups_at_(p, gd, m, v, _table(ranges), hyper, state, coef, ss, max_norm=mn)
        else:
            ops.adamw_step_groups_(p, gd, m, v, _table(ranges), state, coef, ss, grad_scale=gs, max_norm=mn)

    step(torch.tensor([float(bad)], dtype=torch.float64, device=dev), p, m, v, state, coef)
    for name, a, b in (("p", p, p0), ("m", m, m0), ("v", v, v0)):
        _same_bits("%s after a skipped step" % name, a, b)
    assert state.tolist() == [applied, skipped + 1]
    assert coef.tolist() == [0.0, 0.0] + [1.0] * (2 * len(ranges))
    # the next finite step is step applied + 1: the bits of the same update from a state that never skipped
    ss = ops.sumsq(gd)
    step(ss, p, m, v, state, coef)
    p2, m2, v2, state2, coef2 = p0.to(dev), m0.to(dev), v0.to(dev), _state(dev, applied, 0), _coef(dev, len(ranges))
    step(ss, p2, m2, v2, state2, coef2)
    assert state.tolist() == [applied + 1, skipped + 1] and state2.tolist() == [applied + 1, 0]
    for name, a, b in (("p", p, p2), ("m", m, m2), ("v", v, v2), ("coef", coef, coef2)):
        _same_bits("%s of the step after the skip" % name, a, b)
    bc1, bc2s = R.bias_corrections(HYPER[3][2], HYPER[3][3], applied + 1)
    assert abs(coef[8].item() - bc1) <= _ulp32(bc1) and abs(coef[9].item() - bc2s) <= _ulp32(bc2s)
    assert not torch.equal(p.cpu()[EIGHT[5][0]:EIGHT[5][1]], p0[EIGHT[5][0]:EIGHT[5][1]])


# ---- 5. the _at form, eagerly and replayed -------------------------------------------------------------------------------------------------------------
def test_the_at_form_replayed_with_other_learning_rates_equals_by_value_steps(ops, dev):
    """one captured update (a single chain: prepare, update), replayed three times; between replays the host writes other grad_scale / lr words, a new gradient
    and its sum of squares.  The eager twin takes the same fp32 values by value."""
    case = "unit_averaged_8_ranks"
    _, _, _, mn, _, _, _ = R.CASES[case]
    ranges = EDGES
    p0, m0, v0, _ = _inputs(case)
    table = _table(ranges)
    ignored = [(b, e, 123.0, b1, b2, eps, wd) for b, e, _, b1, b2, eps, wd in table]        # the lr fields of the table are not read by the _at form
    hyper = torch.zeros(1 + len(ranges), dtype=torch.float32, device=dev)
    g = torch.zeros(N, device=dev)
    ss = torch.zeros(1, dtype=torch.float64, device=dev)
    # everything the capture must not be the first to touch: both entry points once, eagerly, on scratch
    sp, sm, sv = p0.to(dev), m0.to(dev), v0.to(dev)
    ops.adamw_step_groups_(sp, g, sm, sv, table, _state(dev, 0), _coef(dev, len(ranges)), ss)
    ops.adamw_step_groups_at_(sp, g, sm, sv, table, hyper, _state(dev, 0), _coef(dev, len(ranges)), ss)
    p, m, v, state, coef = p0.to(dev), m0.to(dev), v0.to(dev), _state(dev, 0), _coef(dev, len(ranges))
    q, mq, vq, state_q, coef_q = p0.to(dev), m0.to(dev), v0.to(dev), _state(dev, 0), _coef(dev, len(ranges))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.adamw_step_groups_at_(p, g, m, v, ignored, hyper, state, coef, ss, max_norm=mn)
    _same_bits("a capture runs nothing", p, p0)
    for i, (gscale, mult) in enumerate(((0.125, 1.0), (1.0 / 3.0, 0.37), (1.0, 10.0))):
        words = [ctypes.c_float(gscale).value] + [ctypes.c_float(HYPER[k][0] * mult).value for k in range(len(ranges))]
        for j, w in enumerate(words):
            hyper[j:j + 1].fill_(w)
        g.copy_(R.make_grad(case, i, N))
        ops.sumsq(g, out=ss)
        graph.replay()
        by_value = [(b, e, words[1 + k], b1, b2, eps, wd) for k, (b, e, _, b1, b2, eps, wd) in enumerate(table)]
        ops.adamw_step_groups_(q, g, mq, vq, by_value, state_q, coef_q, ss, grad_scale=words[0], max_norm=mn)
        for name, a, b in (("p", p, q), ("m", m, mq), ("v", v, vq), ("state", state, state_q), ("coef", coef, coef_q)):
            _same_bits("replay %d: %s" % (i, name), a, b)
    assert state.tolist() == [3, 0] and not torch.equal(p.cpu()[280:90000], p0[280:90000])
    # and eagerly, not captured
    ops.adamw_step_groups_at_(p, g, m, v, ignored, hyper, state, coef, ss, max_norm=mn)
    ops.adamw_step_groups_(q, g, mq, vq, by_value, state_q, coef_q, ss, grad_scale=words[0], max_norm=mn)
    for name, a, b in (("p", p, q), ("m", m, mq), ("v", v, vq), ("state", state, state_q)):
        _same_bits("eager _at: %s" % name, a, b)


def test_a_wrong_hyper_length_is_a_type_error(ops, dev):
    t = torch.zeros(64, device=dev)
    ss, state = torch.ones(1, dtype=torch.float64, device=dev), _state(dev, 0)
    for bad in (torch.zeros(2, device=dev), torch.zeros(4, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)):
        with pytest.raises(TypeError, match="1 \\+ n_groups"):
            ops.adamw_step_groups_at_(t, t, t, t, [(0, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0), (8, 64, 1e-3, 0.9, 0.999, 1e-8, 0.0)], bad, state, _coef(dev, 2), ss)
    assert state.tolist() == [0, 0]


# ---- 6. containment ------------------------------------------------------------------------------------------------------------------------------------
def _flat(guards, n, dev, fill, dtype=torch.float32, misalign=False, data=None):
    unit = 16 // torch.empty(0, dtype=dtype).element_size()
    b, v = guarded((1, n), dtype, dev, fill, data=None if data is None else data.view(1, n), col0=unit + (1 if misalign else 0), rows_before=1, rows_after=1,
                   cols_after=4096)
    guards.append((b, v))
    return v.view(-1)


@pytest.mark.parametrize("misalign", (False, True), ids=("aligned", "one_element_off"))
def test_both_entry_points_write_only_their_outputs_and_read_only_their_inputs(ops, dev, misalign):
    """n = 10007; the last group ends at n exactly, so an overrun of its last block lands in the band.  Outputs of both fills equal an unguarded run bit for bit."""
    n, case, t = 10007, "unit_clipped", 3
    _, _, gs, mn, _, _, _ = R.CASES[case]
    ranges = ((0, 8), (8, 272), (272, 272), (280, n))
    table = _table(ranges)
    p0, m0, v0, g = _inputs(case, n)
    words = torch.tensor([ctypes.c_float(gs).value] + [ctypes.c_float(HYPER[k][0]).value for k in range(len(ranges))], dtype=torch.float32)
    want = dict(p=p0.to(dev), m=m0.to(dev), v=v0.to(dev), state=_state(dev, t - 1), coef=_coef(dev, len(ranges)))
    ops.adamw_step_groups_(want["p"], g.to(dev), want["m"], want["v"], table, want["state"], want["coef"], ops.sumsq(g.to(dev)), grad_scale=gs, max_norm=mn)
    want = {k: x.cpu() for k, x in want.items()}

    def run(fill):
        guards, out = [], {}
        for form in ("by_value", "at"):
            p, m, v, gd = (_flat(guards, n, dev, fill, misalign=misalign, data=x) for x in (p0, m0, v0, g))
            state = _flat(guards, 2, dev, fill, dtype=torch.int64, data=torch.tensor([t - 1, 0]))
            coef = _flat(guards, 2 + 2 * len(ranges), dev, fill, misalign=misalign)
            ss = _flat(guards, 1, dev, fill, dtype=torch.float64, data=torch.zeros(1, dtype=torch.float64))
            ops.sumsq(gd, out=ss)
            if form == "at":
                hyper = _flat(guards, words.numel(), dev, fill, misalign=misalign, data=words)
                ops.adamw_step_groups_at_(p, gd, m, v, table, hyper, state, coef, ss, max_norm=mn)
            else:
                ops.adamw_step_groups_(p, gd, m, v, table, state, coef, ss, grad_scale=gs, max_norm=mn)
            out.update({"%s_%s" % (k, form): x for k, x in (("p", p), ("m", m), ("v", v), ("state", state), ("coef", coef))})
        return out, guards

    def check(name, x):
        _same_bits(name, x, want[name.split("_")[0]])

    check_two_fills(run, check, what="adamw groups")
    assert math.isfinite(want["coef"][0].item()) and want["state"].tolist() == [t, 0]
