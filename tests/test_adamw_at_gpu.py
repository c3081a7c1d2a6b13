"""`e2eft_adamw_step_guarded_at` (csrc/bwd.hip) against the scalar entry point `e2eft_adamw_step_guarded`: lr and grad_scale read on the device from
`hyper = {lr, grad_scale}` instead of travelling as launch arguments.  The two entry points launch ONE kernel body behind a loader for the two values, so for the
same fp32 values every output word is equal — `torch.equal`, no tolerance: param, exp_avg, exp_avg_sq, state, coef; over two consecutive steps with `hyper`
rewritten on the device in between, with and without clipping, and across a step skipped for a NaN in the gradient."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 1e-2
SIZES = [1, 255, 256 * 1024 + 3]      # one element; one partial block; many blocks with a ragged tail
# (lr, grad_scale) of the steps: different every step, none a power of two
HYPER = [(3e-5, 1.0), (1.7e-3, 0.25), (2.9e-4, 1.0 / 3.0)]


def _f32(x):
    return ctypes.c_float(x).value


def _buffers(n, dev, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).to(dev)
    grads = [(torch.randn(n, generator=g) * (0.5 + k)).to(dev) for k in range(len(HYPER))]
    return p, grads


def _run(at, n, dev, max_norm, nan_step, seed=5):
    """len(HYPER) consecutive steps; -> the five outputs after every step"""
    from diffusion_e2e_ft_amd import ops
    p, grads = _buffers(n, dev, seed)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    state = torch.zeros(2, dtype=torch.int64, device=dev)
    coef = torch.zeros(4, dtype=torch.float32, device=dev)
    hyper = torch.zeros(2, dtype=torch.float32, device=dev)
    out = []
    for k, (lr, gs) in enumerate(HYPER):
        g = grads[k].clone()
        if k == nan_step:
            g[n // 2] = float("nan")
        ss = ops.sumsq(g)
        if at:
            hyper[0:1].fill_(_f32(lr))          # rewritten ON THE DEVICE between the steps: no new tensor, no host copy
            hyper[1:2].fill_(_f32(gs))
            ops.adamw_step_guarded_at_(p, g, m, v, hyper, B1, B2, EPS, WD, state, coef, ss, max_norm=max_norm)
        else:
            ops.adamw_step_guarded_(p, g, m, v, lr, B1, B2, EPS, WD, state, coef, ss, grad_scale=gs, max_norm=max_norm)
        out.append([t.clone() for t in (p, m, v, state, coef)])
    torch.cuda.synchronize()
    return out, [float(torch.sqrt(ops.sumsq(g_)).item()) for g_ in grads]


NAMES = ("param", "exp_avg", "exp_avg_sq", "state", "coef")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("clip", [True, False], ids=["clipped", "unclipped"])
def test_device_hyper_equals_scalar_arguments(dev, n, clip):
    # clipped: max_norm far below every step's ||g|| * grad_scale (>= 0.1 for n = 1 would not be sure, so the bar is tiny); unclipped: max_norm = 0 switches it off
    max_norm = 1e-3 if clip else 0.0
    got, norms = _run(True, n, dev, max_norm, nan_step=None)
    want, _ = _run(False, n, dev, max_norm, nan_step=None)
    for k in range(len(HYPER)):
        for name, a, b in zip(NAMES, got[k], want[k]):
            assert torch.equal(a, b), (name, k, n)
        clipf = got[k][4][0].item()
        if clip:
            assert norms[k] * HYPER[k][1] > max_norm and clipf < _f32(HYPER[k][1]), (k, norms[k], clipf)      # the clip was active
        else:
            assert clipf == _f32(HYPER[k][1])
    assert got[-1][3].tolist() == [len(HYPER), 0]
    assert not torch.equal(got[0][0], got[1][0])          # (the steps did something)


@pytest.mark.parametrize("n", SIZES)
def test_a_skipped_step_is_the_same_skip(dev, n):
    """one NaN in the gradient of step 1: state[1] += 1, parameters and moments untouched, the bias correction does not advance — in both entry points alike, and
    the following step is equal again"""
    got, _ = _run(True, n, dev, 1.0, nan_step=1)
    want, _ = _run(False, n, dev, 1.0, nan_step=1)
    for k in range(len(HYPER)):
        for name, a, b in zip(NAMES, got[k], want[k]):
            assert torch.equal(a, b), (name, k, n)
    for name, a, b in zip(NAMES[:3], got[0], got[1]):
        assert torch.equal(a, b), name                    # the skipped step changed nothing
    assert got[1][3].tolist() == [1, 1] and got[2][3].tolist() == [2, 1]
    assert got[1][4].tolist() == [0.0, 1.0, 1.0, 0.0]
    assert torch.isfinite(got[2][0]).all() and not torch.equal(got[2][0], got[1][0])


def test_hyper_is_checked(dev):
    from diffusion_e2e_ft_amd import ops
    p = torch.zeros(8, device=dev)
    state, coef = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(4, device=dev)
    ss = torch.zeros(1, dtype=torch.float64, device=dev)
    for bad in (torch.zeros(3, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)):
        with pytest.raises(TypeError):
            ops.adamw_step_guarded_at_(p, p.clone(), p.clone(), p.clone(), bad, B1, B2, EPS, WD, state, coef, ss)
