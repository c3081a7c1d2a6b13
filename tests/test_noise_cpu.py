"""Host side of the device noise (no GPU): the Philox4x32-10 restatement against the published known answers, the pyramid level sizes against the
shapes `pipeline.pyramid_noise_like` asks torch.randn for, the x0 coefficients against `DDIMScheduler.step`, argument validation of the entry points."""
import ctypes
import random

import numpy as np
import pytest
import torch

import noise_ref

# Random123's known-answer file (kat_vectors, philox4x32 10 rounds): counter / key all zero, all ones, and the digits of pi.  A stand-alone C
# restatement (scalar 64-bit products) and the vectorised numpy one in noise_ref.py — written separately — both print exactly these words.
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def _philox_scalar(ctr, key):
    """second, scalar restatement in Python integers (independent of the numpy code path)"""
    c, k = list(ctr), list(key)
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
    return c


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = noise_ref.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert [int(v) for v in got] == want, [hex(int(v)) for v in got]
        assert _philox_scalar(ctr, key) == want
    # vectorised over a batch of counters == the scalar form, and the element -> (counter, word) mapping of the definition
    seed, draw, slot, n = 0x0123456789ABCDEF, 7, 3, 37
    w, _ = noise_ref.words(seed, draw, slot, n)
    for e in (0, 1, 5, 18, 36):
        want = _philox_scalar([e >> 2, 0, slot, draw], [seed & 0xFFFFFFFF, seed >> 32])
        assert [int(v) for v in w[e]] == want
    u = noise_ref.uniforms(seed, draw, slot, n)
    assert u.min() > 0.0 and u.max() < 1.0
    # (word >> 8) + 0.5 is an fp32 number below 2^23; above, its complement is (what the kernel computes from)
    lo = (w >> np.uint32(8)) < 2 ** 23
    exact = lambda a: np.array_equal(a.astype(np.float32).astype(np.float64), a)
    assert lo.any() and (~lo).any() and exact(u[lo]) and exact(1.0 - u[~lo])
    z = noise_ref.normals(seed, draw, slot, n)
    r = np.sqrt(-2.0 * np.log(u[4, 0]))
    assert z[4] == r * np.cos(2 * np.pi * u[4, 1]) and z[5] == r * np.sin(2 * np.pi * u[4, 1])
    r = np.sqrt(-2.0 * np.log(u[4, 2]))
    assert z[6] == r * np.cos(2 * np.pi * u[4, 3]) and z[7] == r * np.sin(2 * np.pi * u[4, 3])
    assert np.abs(z).max() <= 5.9


def test_restatement_moments_for_the_gpu_test_seed():
    """the seed tests/test_noise_gpu.py uses for its moment check passes the same bounds in the float64 restatement"""
    N = 8 * 4 * 96 * 96
    z = noise_ref.normals(1234, 0, 0, N)
    assert abs(z.mean()) <= 5 / np.sqrt(N)
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / N)


@pytest.mark.parametrize("shape", [(96, 96), (72, 72), (9, 12), (1, 7)])
@pytest.mark.parametrize("seed", [0, 1, 7, 2024])
def test_pyramid_level_sizes_match_the_host_function(monkeypatch, shape, seed):
    from diffusion_e2e_ft_amd import noise, pipeline
    x = torch.zeros(2, 4, *shape)
    asked = []
    real = torch.randn

    def spy(*size, **kw):
        asked.append(tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size))
        return real(*size, **kw)

    monkeypatch.setattr(torch, "randn", spy)
    random.seed(seed)
    pipeline.pyramid_noise_like(x)
    state_ref = random.getstate()
    monkeypatch.undo()
    random.seed(seed)
    sizes = noise.pyramid_level_sizes(*shape)
    assert random.getstate() == state_ref
    assert sizes == [s[2:] for s in asked] and all(s[:2] == (2, 4) for s in asked)
    assert 1 <= len(sizes) <= 10 and (1 in sizes[-1] or len(sizes) == 10)
    # an explicit generator object leaves the module-level state alone
    random.seed(seed)
    before = random.getstate()
    assert noise.pyramid_level_sizes(*shape, rng=random.Random(seed)) == sizes
    assert random.getstate() == before


@pytest.mark.parametrize("prediction_type", ["v_prediction", "epsilon", "sample"])
@pytest.mark.parametrize("t", [999, 500])
def test_x0_coefficients_match_scheduler_step(prediction_type, t):
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    sch = DDIMScheduler(prediction_type=prediction_type)
    sch.set_timesteps(2)                                   # timesteps 999, 499: step() needs num_inference_steps
    g = torch.Generator().manual_seed(t)
    x_t, v = torch.randn(2, 4, 5, 7, generator=g, dtype=torch.float64), torch.randn(2, 4, 5, 7, generator=g, dtype=torch.float64)
    c_x, c_v = sch.x0_coefficients_for(t)
    want = sch.step(v, t, x_t).pred_original_sample
    # the coefficients are square roots (and a quotient) taken in fp32, step() takes them in float64 from the same fp32 abar: each term is off by at most
    # two fp32 roundings (2^-23 relative) — epsilon at t = 999 multiplies by 14.6, so the bound is relative to the terms, not absolute
    bound = 2.0 ** -22 * ((c_x * x_t).abs() + (c_v * v).abs()) + 1e-12
    assert ((c_x * x_t + c_v * v - want).abs() <= bound).all()
    assert c_v == sch.zero_latent_x0_scale(t)
    for bad in (dict(clip_sample=True), dict(thresholding=True)):
        with pytest.raises(NotImplementedError):
            DDIMScheduler(prediction_type=prediction_type, **bad).x0_coefficients_for(t)


def test_device_noise_counter_is_host_side():
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    g = DeviceNoise(2 ** 64 + 5)
    assert (g.seed, g.draw) == (5, 0)
    assert [g.next_draw() for _ in range(3)] == [0, 1, 2] and g.draw == 3
    g.draw = 0xFFFFFFFF
    assert g.next_draw() == 0xFFFFFFFF and g.draw == 0


def test_noise_entry_points_validate_before_launching():
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.e2eft_randn_fill(0, 1, 4, 4, 2, 1, 0, 0, p, None) == 1 and b"shape" in lib.e2eft_last_error()          # ldy < c
    assert lib.e2eft_randn_fill(0, 1, 4, 4, 4, 1, 0, 0, None, None) == 1
    assert lib.e2eft_randn_fill(7, 1, 4, 4, 4, 1, 0, 0, p, None) == 1 and b"dtype" in lib.e2eft_last_error()
    assert lib.e2eft_pyramid_noise_workspace_bytes(0, 4, 4) == 0
    need = lib.e2eft_pyramid_noise_workspace_bytes(2, 4, 108)
    assert need >= 2 * 4 * 108 * 4
    sizes = (ctypes.c_int32 * 22)(*([1] * 22))
    assert lib.e2eft_pyramid_noise(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 11, sizes, p, p, need, None) == 1 and b"levels" in lib.e2eft_last_error()
    assert lib.e2eft_pyramid_noise(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 1, sizes, p, p, 16, None) == 2                          # workspace too small
    assert lib.e2eft_pyramid_noise(0, 1, 1, 1, 1, 1, 1, 0, 0.9, 1, sizes, p, p, need, None) == 1                          # one element has no unbiased std
    sizes[0] = 0
    assert lib.e2eft_pyramid_noise(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 1, sizes, p, p, need, None) == 1 and b"level 0" in lib.e2eft_last_error()
    assert lib.e2eft_latent_x0(0, 4, 4, 3, 4, 4, 1.0, 1.0, p, p, p, None) == 1 and b"shape" in lib.e2eft_last_error()


def test_training_rejects_bad_noise_arguments_before_touching_the_device():
    from diffusion_e2e_ft_amd import training
    with pytest.raises(ValueError, match="Unknown noise type"):
        training.e2e_ft_loss(None, None, {}, None, noise_type="perlin")
