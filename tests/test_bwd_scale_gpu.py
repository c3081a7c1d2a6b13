"""Exact power-of-two scaling of the backward kernels at training-scale gradients (util.assert_backward_scales; the cases and their inputs: bwd_scale_cases.py).

The parity tests feed the backward kernels dy ~ N(0,1) and judge max|err| / max|ref|; training hands them gradients of order 2^-24 and below whose magnitude
differs by decades between samples, channels and query rows.  Every backward op is linear in dy and every rounding in it commutes with a power of two, so on the
default bf16 and fp32 routes, through the public functions of autograd.py as the model calls them:
  bwd(dy) twice is bit-equal;  bwd(2^k dy) == 2^k bwd(dy) bit for bit for k = -24, -40;  and with block i of dy scaled by 2^(-27, 0, -40, -13)[i % 4] every output
  block that depends on that block of dy alone carries exactly that factor:
    conv        dx, dx2 per batch item; dW, dbias per output channel; drowadd per (b, co); dres per element
    linear      dx per row; dW, dbias per output column; dres per element
    groupnorm   dx per (b, group); dgamma, dbeta per channel (split=True: dy and the skip gradient scaled together)
    layernorm   dx per row; dgamma, dbeta per channel;   geglu, silu: dx per row
    attention   dq per (b, query row, head); dk, dv per (b, head)   (fused bf16 attn_bwd.hip, fused fp32 attn32.hip, and the softmax_bwd_rows + GEMM form)
    depth_head, normal_head(clamp=True), nchw_to_nhwc: dx per pixel
The whole-model test does the same for every parameter gradient of an E2E-FT micro-step (fp32, and bf16 compute over fp32 master weights): the torch glue, the
casts, the loss kernels and every op the list leaves out.  fp16 is out of scope (P and dS are packed to f16, whose subnormals make scaling inexact)."""
import pytest
import torch

import bwd_scale_cases as cases
from test_bwd_gpu import CONV_CASES
from util import assert_backward_scales, assert_same_bits

pytestmark = pytest.mark.gpu

ALL = cases.all_cases(CONV_CASES)


@pytest.fixture(scope="module")
def F(dev):
    from diffusion_e2e_ft_amd import autograd as _F
    return _F


@pytest.mark.parametrize("dtype,build", [c[1:] for c in ALL], ids=[c[0] for c in ALL])
def test_backward_scales_exactly(F, dev, dtype, build):
    case = build()
    many = isinstance(case.dy, tuple)
    dy = tuple(t.to(dtype).to(dev) for t in case.dy) if many else case.dy.to(dtype).to(dev)
    assert_backward_scales(case.runner(F, dev), dy, case.outputs, block=case.block, zero=case.zero)


MODEL_K = (0, 0, -20)


@pytest.mark.parametrize("compute", [torch.float32, torch.bfloat16], ids=["fp32", "bf16 over fp32 master weights"])
def test_micro_step_gradients_scale_exactly_with_the_loss(dev, compute):
    """(loss * 2^k).backward() of training.e2e_ft_loss(..., "depth") on the tiny UNet + frozen VAE: two k = 0 runs give equal gradients and every parameter's
    k = -20 gradient is its k = 0 gradient times 2^-20, bit for bit.  Non-vacuity: every parameter whose golden gradient norm is above the rounding floor of the
    oracle (test_train_gpu._check_grads) has a non-zero, finite gradient here."""
    import golden_cases as gc
    from test_train_gpu import GOLD, _models
    from diffusion_e2e_ft_amd import training
    unet, vae = _models(dev)
    if compute != torch.float32:
        unet.set_compute_dtype(compute)
        vae = vae.to(compute)
    batch, text = gc.train_batch()
    grads = []
    for k in MODEL_K:
        unet.zero_grad(set_to_none=True)
        loss = training.e2e_ft_loss(unet, vae, batch, text, "depth")
        (loss * 2.0 ** k).backward()
        grads.append({n: p.grad.detach().clone() for n, p in unet.named_parameters()})
        assert all(p.grad is None for p in vae.parameters())
    norms = GOLD["depth"]["grad_norms"]
    floor = 1e-6 * max(norms.values())
    for n, g in grads[0].items():
        assert g.dtype == torch.float32 and torch.isfinite(g).all(), n
        assert norms[n] <= floor or g.abs().max().item() > 0, "%s: zero gradient" % n
    for n in grads[0]:
        assert_same_bits(n, grads[1][n], grads[0][n], "second run on the same loss")
    for n in grads[0]:
        assert_same_bits(n, grads[2][n], grads[0][n] * 2.0 ** MODEL_K[2], "loss * 2^%d" % MODEL_K[2])
