"""Host side of the fused multi-step inference (no GPU): `DDIMScheduler.step_coefficients` against `DDIMScheduler.step` (itself pinned to the reference's replayed
traces), the fp32 table, refusal of clipping configurations, argument validation of e2eft_ddim_step / e2eft_randn_fill_at, and the bindings."""
import ctypes
import inspect

import pytest
import torch

PREDICTION_TYPES = ["v_prediction", "epsilon", "sample"]
SPACINGS = ["trailing", "leading", "linspace"]


@pytest.mark.parametrize("n", [1, 2, 10, 50])
@pytest.mark.parametrize("spacing", SPACINGS)
@pytest.mark.parametrize("prediction_type", PREDICTION_TYPES)
def test_table_is_the_scheduler_step(prediction_type, spacing, n):
    """float64 table applied to float64 (x, v) == step(): both sides evaluate the same formula in float64 from the same fp32 table entries, so they differ by a few
    float64 roundings of the terms — 1e-12 relative to |c_x x| + |c_v v| is four decimal orders above that and nine below one fp32 rounding"""
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(prediction_type=prediction_type, timestep_spacing=spacing)
    tab = sch.step_coefficients_f64(n)
    assert tab.dtype == torch.float64 and tuple(tab.shape) == (n, 2)
    sch.set_timesteps(n)
    g = torch.Generator().manual_seed(1000 * n + len(spacing))
    for i, t in enumerate(sch.timesteps_host):
        x, v = torch.randn(2, 4, 5, 7, generator=g, dtype=torch.float64), torch.randn(2, 4, 5, 7, generator=g, dtype=torch.float64)
        out = sch.step(v, t, x)
        want = out.pred_original_sample if i == n - 1 else out.prev_sample
        c_x, c_v = tab[i, 0].item(), tab[i, 1].item()
        scale = (c_x * x).abs() + (c_v * v).abs()
        err = ((c_x * x + c_v * v - want).abs() / scale).max().item()
        assert err <= 1e-12, (prediction_type, spacing, n, i, err)
    # the fp32 table is the float64 table rounded once; cached per (schedule, device)
    t32 = sch.step_coefficients(n, "cpu")
    assert t32.dtype == torch.float32 and torch.equal(t32, tab.to(torch.float32))
    assert sch.step_coefficients(n, "cpu") is t32
    # the last row is x0_coefficients_for, which takes its square roots in fp32: equal to one fp32 rounding of each
    c_x, c_v = sch.x0_coefficients_for(sch.timesteps_host[-1])
    assert abs(c_x - tab[-1, 0].item()) <= 2.0 ** -22 * abs(c_x) and abs(c_v - tab[-1, 1].item()) <= 2.0 ** -22 * abs(c_v)


def test_table_follows_the_schedule_not_the_last_call():
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler()
    a = sch.step_coefficients(3, "cpu")
    sch.set_timesteps(7)
    assert sch.step_coefficients(3, "cpu") is a and tuple(sch.step_coefficients(4, "cpu").shape) == (4, 2)
    assert sch.num_inference_steps == 7          # building a table leaves the scheduler's state alone
    assert not torch.equal(DDIMScheduler(prediction_type="epsilon").step_coefficients(3, "cpu"), a)


@pytest.mark.parametrize("bad", [dict(clip_sample=True), dict(thresholding=True)])
def test_clipping_configurations_are_refused(bad):
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    with pytest.raises(NotImplementedError):
        DDIMScheduler(**bad).step_coefficients(4, "cpu")
    with pytest.raises(NotImplementedError):
        DDIMScheduler(**bad).step_coefficients_f64(4)


def test_entry_points_validate_before_launching():
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.e2eft_last_error
    # e2eft_ddim_step(dtype, pixels, c, ldx, ldv, coef, x, v, stream)
    for args in ((0, 4, 4, 8, 4, None, p, p), (0, 4, 4, 8, 4, p, None, p), (0, 4, 4, 8, 4, p, p, None)):
        assert lib.e2eft_ddim_step(*args, None) == 1 and b"null" in err(), args
    assert lib.e2eft_ddim_step(3, 4, 4, 8, 4, p, p, p, None) == 1 and b"dtype" in err()
    assert lib.e2eft_ddim_step(-1, 4, 4, 8, 4, p, p, p, None) == 1 and b"dtype" in err()
    assert lib.e2eft_ddim_step(0, 4, 4, 3, 4, p, p, p, None) == 1 and b"shape" in err()          # ldx < c
    assert lib.e2eft_ddim_step(0, 4, 4, 8, 3, p, p, p, None) == 1 and b"shape" in err()          # ldv < c
    assert lib.e2eft_ddim_step(0, 0, 4, 8, 4, p, p, p, None) == 1 and b"shape" in err()          # pixels <= 0
    assert lib.e2eft_ddim_step(0, -5, 4, 8, 4, p, p, p, None) == 1 and b"shape" in err()
    # e2eft_randn_fill_at(dtype, batch, c, hw, ldy, seed, draw, slot, y, stream): e2eft_randn_fill's checks + the draw pointer
    assert lib.e2eft_randn_fill_at(0, 1, 4, 4, 4, 1, None, 0, p, None) == 1 and b"null" in err()
    assert lib.e2eft_randn_fill_at(0, 1, 4, 4, 4, 1, p, 0, None, None) == 1 and b"null" in err()
    assert lib.e2eft_randn_fill_at(7, 1, 4, 4, 4, 1, p, 0, p, None) == 1 and b"dtype" in err()
    assert lib.e2eft_randn_fill_at(0, 1, 4, 4, 2, 1, p, 0, p, None) == 1 and b"shape" in err()     # ldy < c
    assert lib.e2eft_randn_fill_at(0, 0, 4, 4, 4, 1, p, 0, p, None) == 1 and b"shape" in err()
    assert lib.e2eft_randn_fill_at(0, 1 << 20, 4, 1 << 10, 4, 1, p, 0, p, None) == 1 and b"2^31" in err()


def test_bindings_exist():
    from diffusion_e2e_ft_amd import _lib, noise, ops
    assert list(inspect.signature(ops.ddim_step_).parameters) == ["x", "v", "coef"]
    assert list(inspect.signature(ops.randn_fill_at_).parameters) == ["dst", "seed", "draw", "slot"]
    assert {"e2eft_ddim_step", "e2eft_randn_fill_at"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert hasattr(lib, "e2eft_ddim_step") and hasattr(lib, "e2eft_randn_fill_at")
    assert lib.e2eft_version() == 119
    assert "NOT capture-safe" not in noise.__doc__ and "randn_at" in noise.__doc__
    # the header declares both (tests/test_abi.py holds the exports to the header)
    import os
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "e2eft.h")) as f:
        text = f.read()
    assert "int e2eft_ddim_step(" in text and "int e2eft_randn_fill_at(" in text
