"""The inputs of tests/test_attn_paths_gpu.py, proven on the CPU with the model of the kernels' arithmetic (tests/attn_model.py), on exactly the calls the GPU
tests make (B x H heads, the same seeds, the pooled per-row metric):
  * the model of what the kernels do (the unscaled q contracted, c = scale log2(e) applied to the fp32 score inside the exponent, forward and backward) meets
    every bar the GPU tests set, and so does the two-term Q' = hi + lo that was the other cure;
  * a model whose rescale is wrong (alpha = 1 for O, or for l) misses the output bar by more than 10 x on every input that moves the reference after the first
    tile — and every rescale family and every spread >= 4 does move it; at spread 1 no wave moves its reference (the blind spot the families exist for), which
    is asserted so that the claim cannot go stale;
  * the single-rounded Q' = round_T(c q) the forward used to contract exceeds 2 E_T at spreads 8 and 16 in both dtypes (measured 5.5 / 7.4 / 17 x E_T in fp16 and
    3.2 / 7.9 / 11 x E_T in bf16 at spreads 4 / 8 / 16) and misses the lse bar on the creeping scores (5 - 13 x the bar): the finding that took the
    rounding out of the kernels, pinned."""
import pytest
import torch

import attn_model as am

DTYPES = [torch.float16, torch.bfloat16]
_ids = lambda d: str(d).replace("torch.", "")
FORWARD_NAMES = list(am.RESCALE_FAMILIES) + ["spread_%d" % s for s in am.SPREADS]


@pytest.fixture(scope="module")
def cases():
    return {dt: {name: (heads,) + am.forward_refs(heads, dt) for name, heads in am.forward_cases(dt).items()} for dt in DTYPES}


def _model(heads, dtype, **kw):
    r = [am.kernel_fwd(q, k, v, am.SCALE, dtype, **kw) for q, k, v in heads]
    return torch.stack([x[0] for x in r]), torch.stack([x[1] for x in r]), [x[2] for x in r]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", FORWARD_NAMES)
@pytest.mark.parametrize("form", ["fp32_scale", "two_term"])
def test_model_of_exact_scaling_meets_the_bars(cases, dtype, name, form):
    """both cures of the single rounding: c applied to the fp32 score (the kernels' form) and the two-term Q' (measured too slow)"""
    heads, truth_o, truth_lse, e_t, bars = cases[dtype][name]
    o, lse, _ = _model(heads, dtype, **{form: True})
    err = am.row_err(o, truth_o)
    lerr = (lse.double() - truth_lse).abs().max(dim=1).values
    print("%s %s: O %.2f E_T, lse / bar %.2f" % (name, _ids(dtype), err / e_t, (lerr / bars).max().item()))
    assert err <= 2.0 * e_t, (err, e_t)
    assert bool((lerr <= bars).all()), (lerr.tolist(), bars.tolist())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", FORWARD_NAMES)
def test_wrong_rescale_misses_the_output_bar_tenfold(cases, dtype, name):
    heads, truth_o, _, e_t, _ = cases[dtype][name]
    moves = _model(heads, dtype, fp32_scale=True)[2]
    if name == "spread_1":
        assert all(m == 0 for per_head in moves for m in per_head), "spread 1 moved a reference: it is no longer blind to the rescale, assert the mutants on it"
        return
    assert all(max(per_head) >= 1 for per_head in moves), moves       # every (image, head) rescales in some wave
    for mutant in am.MUTANTS:
        err = am.row_err(_model(heads, dtype, fp32_scale=True, mutant=mutant)[0], truth_o)
        print("%s %s %s: %.1f x the bar" % (name, _ids(dtype), mutant, err / (2.0 * e_t)))
        assert err >= 10.0 * 2.0 * e_t, (mutant, err, e_t)


def test_late_key_moves_the_named_waves_only():
    """family 1 as the issue builds it: only key 270 (+12 for query 3, +10 for query 70) moves a reference, waves 0 and 2 once each; the +9 / +8 of key 200 stay
    under the threshold over first-tile references of 3 - 4, so wave 1 never moves and wave 0 does not move twice: that part of the construction does not
    fire.  late_key_two_waves (14 / 13 at key 200, 22 at key 270) is the variant in which it does: waves 0 and 1 move at key 200, wave 0 again at key 270."""
    for dtype in DTYPES:
        for q, k, v in am.heads_of(am.late_key, dtype):
            moves = am.kernel_fwd(q, k, v, am.SCALE, dtype, fp32_scale=True)[2]
            assert moves == [1, 0, 1, 0], moves
        for q, k, v in am.heads_of(am.RESCALE_FAMILIES["late_key_two_waves"], dtype):
            moves = am.kernel_fwd(q, k, v, am.SCALE, dtype, fp32_scale=True)[2]
            assert moves == [2, 1, 1, 0], moves


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_single_rounded_q_exceeds_the_bar_at_large_spread(cases, dtype):
    for sigma in (8, 16):
        heads, truth_o, _, e_t, _ = cases[dtype]["spread_%d" % sigma]
        err = am.row_err(_model(heads, dtype, two_term=False)[0], truth_o)
        print("spread %d %s: single-rounded %.2f E_T" % (sigma, _ids(dtype), err / e_t))
        assert err > 2.0 * e_t, (sigma, err, e_t)
    for step in am.CREEP_STEPS:
        heads, _, truth_lse, _, bars = cases[dtype]["creep_%.1f" % step]
        lerr = (_model(heads, dtype, two_term=False)[1].double() - truth_lse).abs().max(dim=1).values
        assert bool((lerr > bars).all()), (step, lerr.tolist(), bars.tolist())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("name", am.BACKWARD_NAMES)
def test_backward_model_meets_two_e_t(dtype, name):
    """the backward's arithmetic through the model before any GPU run: every gradient within 2 E_T in both metrics, so the GPU test's bars are 2 E_T; the
    head_err bar is a real one in every case (E_T <= 0.05) and a zero gradient misses it; the single-rounded backward misses it for all three gradients at
    spread 16 (measured 2.9 - 18 E_T)"""
    heads, dos, _ = am.backward_cases(dtype)[name]
    truth, e_t, e_t_head = am.backward_refs(heads, dos, dtype)

    def model(fp32_scale):
        grads = []
        for (q, k, v), do in zip(heads, dos):
            o, lse, _ = am.kernel_fwd(q, k, v, am.SCALE, dtype, fp32_scale=fp32_scale)
            grads.append(am.kernel_bwd(q, k, v, do, o, lse, am.SCALE, dtype, fp32_scale=fp32_scale))
        return [torch.stack([g[i] for g in grads]) for i in range(3)]

    fixed, single = model(True), model(False)
    for i, what in enumerate(("dq", "dk", "dv")):
        err, herr, hsingle = am.row_err(fixed[i], truth[i]), am.head_err(fixed[i], truth[i]), am.head_err(single[i], truth[i])
        print("%s %s %s: row %.2f E_T (E_T %.1e) | head %.2f E_T (E_T %.1e), single-rounded %.2f E_T" % (name, _ids(dtype), what, err / e_t[i], e_t[i], herr / e_t_head[i],
                                                                                                          e_t_head[i], hsingle / e_t_head[i]))
        assert err <= 2.0 * e_t[i], (what, err, e_t[i])
        assert e_t_head[i] <= 0.05, (what, e_t_head[i])
        assert herr <= 2.0 * e_t_head[i], (what, herr, e_t_head[i])
        assert am.head_err(torch.zeros_like(truth[i]), truth[i]) > 10.0 * 2.0 * e_t_head[i], what            # a zero gradient: 1.0
        if name.endswith("spread_16"):
            assert hsingle > 2.0 * e_t_head[i], (what, hsingle, e_t_head[i])
