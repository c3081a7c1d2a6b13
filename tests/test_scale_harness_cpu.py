"""util.assert_backward_scales on plain torch functions (no GPU): it passes on torch's own linear and layer-norm backward, and it FAILS on three toy backward
passes that carry the defects tests/test_bwd_scale_gpu.py exists to find — the proof that those tests can fail.  Also the pre-check of that file's cases: the
float autograd reference of every case meets the non-vacuity bound the harness then asks of the kernels."""
import pytest
import torch
import torch.nn.functional as TF

import bwd_scale_cases as cases
from test_bwd_gpu import CONV_CASES
from util import NON_VACUOUS, assert_backward_scales, assert_same_bits, block_ids, nonzero_fraction

ROWS, K, N = 12, 24, 16
ROW_BLOCKS = dict(dx=((0,), (0,)))


def _inputs(seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(ROWS, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g), torch.randn(ROWS, N, generator=g))


def _leaf(t):
    return t.clone().requires_grad_(True)


def test_passes_on_torch_linear():
    x, w, b, dy = _inputs()

    def run(g):
        xl, wl, bl = _leaf(x), _leaf(w), _leaf(b)
        TF.linear(xl, wl, bl).backward(g)
        return dict(dx=xl.grad, dW=wl.grad, dbias=bl.grad)

    assert_backward_scales(run, dy, ["dx", "dW", "dbias"], block=dict(dx=((0,), (0,)), dW=((1,), (0,)), dbias=((1,), (0,))))


def test_passes_on_torch_layer_norm_and_with_a_skip_gradient_scaled_together():
    x, _, _, _ = _inputs()
    g = torch.Generator().manual_seed(6)
    x = x.view(3, 4, K) * 2 + 0.5
    ga, be, dy, dskip = 1 + 0.2 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g), torch.randn(3, 4, K, generator=g), torch.randn(3, 4, K, generator=g)
    block = dict(dx=((0, 1), (0, 1)), dgamma=((2,), (0,)), dbeta=((2,), (0,)))

    def run(gr):
        xl, gl, bl = _leaf(x), _leaf(ga), _leaf(be)
        if isinstance(gr, tuple):
            torch.autograd.backward([TF.layer_norm(xl, (K,), gl, bl, 1e-5), xl.view_as(xl)], list(gr))
        else:
            TF.layer_norm(xl, (K,), gl, bl, 1e-5).backward(gr)
        return dict(dx=xl.grad, dgamma=gl.grad, dbeta=bl.grad)

    assert_backward_scales(run, dy, list(block), block=block)
    assert_backward_scales(run, (dy, dskip), list(block), block=block)


# ---- the three defects: each is y = x * w forward, with a backward that is wrong in a way no unit-scale parity test with a relative tolerance sees
class _AddsEpsilon(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(w)
        return x * w

    @staticmethod
    def backward(ctx, dy):
        return (dy + 1e-12) * ctx.saved_tensors[0], None


class _HalfIntermediate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(w)
        return x * w

    @staticmethod
    def backward(ctx, dy):
        return (dy * ctx.saved_tensors[0]).half().float(), None


class _NeighbourRow(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(w)
        return x * w

    @staticmethod
    def backward(ctx, dy):
        below = torch.cat([dy[1:], torch.zeros_like(dy[:1])])
        return dy * ctx.saved_tensors[0] + 1e-3 * below, None


def _toy_run(fn):
    x, _, _, _ = _inputs()
    w = torch.linspace(0.5, 1.5, K)

    def run(g):
        xl = _leaf(x)
        fn.apply(xl, w).backward(g)
        return dict(dx=xl.grad)

    g = torch.Generator().manual_seed(7)
    return run, torch.randn(ROWS, K, generator=g)


@pytest.mark.parametrize("fn", [_AddsEpsilon, _HalfIntermediate], ids=["epsilon on dy", "f16 intermediate"])
def test_fails_on_an_epsilon_and_on_a_narrow_intermediate(fn):
    run, dy = _toy_run(fn)
    with pytest.raises(AssertionError, match=r"dx: dy \* 2\^-24: \d+ of %d entries differ, largest difference \d+ ulp, first at index \(\d+, \d+\)" % (ROWS * K)):
        assert_backward_scales(run, dy, ["dx"])


def test_neighbour_row_passes_uniform_scaling_and_fails_block_scaling():
    run, dy = _toy_run(_NeighbourRow)
    assert_backward_scales(run, dy, ["dx"])
    with pytest.raises(AssertionError, match=r"dx: block scaling.* entries differ, largest difference \d+ ulp, first at index \(0, 0\)"):
        assert_backward_scales(run, dy, ["dx"], block=ROW_BLOCKS)


def test_non_vacuity_repeatability_and_the_zero_exemption():
    x, _, _, dy = _inputs()
    calls = [0]

    def mostly_zero(g):
        return dict(dx=g * (torch.arange(N) < N // 2))

    with pytest.raises(AssertionError, match="dx: only 50.0 % of the entries are finite and non-zero"):
        assert_backward_scales(mostly_zero, dy, ["dx"])

    def unrepeatable(g):
        calls[0] += 1
        return dict(dx=g * (1.0 + 2.0 ** -20 * calls[0]))

    with pytest.raises(AssertionError, match="dx: second run on the same dy"):
        assert_backward_scales(unrepeatable, dy, ["dx"])
    # an analytically zero output is exempt from the 90 % bound and still has to scale exactly (zero does; rounding noise that scales does too)
    assert_backward_scales(lambda g: dict(dz=g * 0.0, dx=g * 3.0), dy, ["dz", "dx"], block=dict(dz=((0,), (0,)), dx=((0, 1), (0, 1))), zero=("dz",))
    with pytest.raises(AssertionError, match=r"dz: dy \* 2\^-24"):
        assert_backward_scales(lambda g: dict(dz=g * 0.0 + 1e-30), dy, ["dz"], zero=("dz",))


def test_message_counts_ulps_and_block_numbers_separate_neighbours():
    a = torch.tensor([1.0, -2.0, 3.0], dtype=torch.bfloat16)
    b = a.clone()
    b[1] = -2.0 - 3 * 2.0 ** -6          # three bf16 steps away from -2
    with pytest.raises(AssertionError, match=r"t: x: 1 of 3 entries differ, largest difference 3 ulp, first at index \(1,\)"):
        assert_same_bits("t", b, a, "x")
    ids = block_ids((2, 5, 8), (0, 1, (2, 4)))
    full = ids.expand(2, 5, 8) % 4
    assert (full[0, :-1] != full[0, 1:]).all() and (full[0] != full[1]).all() and (full[..., 3] != full[..., 4]).all() and (full[..., 0] == full[..., 3]).all()


ALL = cases.all_cases(CONV_CASES)


@pytest.mark.parametrize("build", [c[2] for c in ALL], ids=[c[0] for c in ALL])
def test_reference_gradient_of_every_gpu_case_is_non_vacuous(build):
    """what the 90 % bound rests on: the float autograd reference of the same inputs is finite and non-zero in >= 90 % of the entries of every compared output, and
    the outputs a case declares analytically zero are zero up to the reference's own rounding"""
    case = build()
    ref = case.reference()
    assert sorted(ref) == sorted(case.outputs)
    for n in case.outputs:
        if n in case.zero:
            assert ref[n].abs().max().item() <= 1e-5 * max(r.abs().max().item() for r in ref.values()), n
        else:
            assert nonzero_fraction(ref[n]) >= NON_VACUOUS, (n, nonzero_fraction(ref[n]))
