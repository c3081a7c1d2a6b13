"""The GeoWizard trainer's timestep-weighted multi-resolution noise without a GPU: the level sizes and the float64 restatement (tests/geowizard_pyramid_ref.py)
against what the reference's own function did (tests/golden/geowizard_pyramid_golden.pt, recorded by tests/golden/make_geowizard_pyramid_golden.py), the
signatures and refusals of the host layer, and the argument validation of e2eft_pyramid_noise_weighted."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import geowizard_pyramid_ref as gref

GOLD = torch.load(os.path.join(os.path.dirname(__file__), "golden", "geowizard_pyramid_golden.pt"))


@pytest.mark.parametrize("shape", [(96, 96), (60, 80), (8, 8), (3, 200), (1, 7)])
def test_level_sizes_are_the_reference_functions(shape):
    from diffusion_e2e_ft_amd import noise
    assert shape in GOLD["shapes"] and len(GOLD["np_seeds"]) == 3
    for s in GOLD["np_seeds"]:
        rec = GOLD["sizes"][shape + (s,)]
        np.random.seed(s)
        sizes = noise.geowizard_pyramid_level_sizes(*shape)
        assert float(np.random.random()) == rec["next_random"]          # numpy's stream is where the reference leaves it
        assert sizes == [tuple(v) for v in rec["sizes"]]
        assert 1 <= len(sizes) <= 10 and (1 in sizes[-1] or len(sizes) == 10) and sizes[0] == shape
        # an explicit generator leaves the global stream alone
        np.random.seed(s)
        before = np.random.get_state()[1].copy()
        assert noise.geowizard_pyramid_level_sizes(*shape, rng=np.random.RandomState(s)) == sizes
        assert np.array_equal(np.random.get_state()[1], before)


def test_level_sizes_shrink_from_the_original_size_and_stop_at_ten():
    from diffusion_e2e_ft_amd import noise

    class Fixed:
        def __init__(self, v):
            self.v, self.calls = v, 0

        def random(self):
            self.calls += 1
            return self.v

    rng = Fixed(0.0)                                   # r = 1.5 at every level
    sizes = noise.geowizard_pyramid_level_sizes(100, 1000, rng=rng)
    assert sizes == [(max(1, int(100 / 1.5 ** i)), max(1, int(1000 / 1.5 ** i))) for i in range(10)] and rng.calls == 10      # never reaches 1 in ten levels
    rng = Fixed(0.0)
    assert noise.geowizard_pyramid_level_sizes(100, 100, rng=rng, scale=5.0) == [(100, 100), (20, 20), (4, 4), (1, 1)] and rng.calls == 4


def test_restatement_equals_the_reference_function_in_float64():
    case = GOLD["case"]
    shape, sizes, t = tuple(case["shape"]), [tuple(s) for s in case["sizes"]], list(case["timesteps"])
    assert shape == (4, 4, 12, 10) and t == [0, 999, 500, 1] and len(sizes) >= 3
    got = gref.weighted_pyramid(case["seed"], case["draw"], shape, sizes, t)
    err = (got - case["output"]).abs().max().item()
    print("float64 restatement against the reference's function: max abs err %.3e" % err)
    assert got.dtype == torch.float64 and err <= 1e-12
    # the t = 0 row is its base grid alone over the common std; the others are not
    base = gref.level_grids(case["seed"], case["draw"], shape, sizes)[0]
    ratio = case["output"] / base
    assert float((ratio[0] - ratio[0, 0, 0, 0]).abs().max()) <= 1e-12 and float((ratio[1] - ratio[0, 0, 0, 0]).abs().max()) > 1e-3
    # the sizes the reference drew for this case are the ones the product's function draws
    from diffusion_e2e_ft_amd import noise
    np.random.seed(case["np_seed"])
    assert noise.geowizard_pyramid_level_sizes(shape[2], shape[3]) == sizes


def test_fp32_evaluation_is_a_rounding_of_the_float64_one():
    """the independent fp32 evaluation from which the GPU test derives its bar: close to the float64 definition, and not equal to it"""
    case = GOLD["case"]
    shape, sizes, t = tuple(case["shape"]), [tuple(s) for s in case["sizes"]], list(case["timesteps"])
    lo = gref.weighted_pyramid_fp32(case["seed"], case["draw"], shape, sizes, t)
    assert lo.dtype == np.float32
    err = float(np.abs(lo.astype(np.float64) - case["output"].numpy()).max())
    print("fp32 evaluation against float64: max abs err %.3e" % err)
    assert 0.0 < err <= 1e-5
    assert [float(w) for w in gref.timestep_weights([0, 1000, 500])] == [0.0, 1.0, 0.5]


def test_signatures_message_and_host_refusals():
    from diffusion_e2e_ft_amd import noise, ops, training
    sig = inspect.signature(ops.pyramid_noise_weighted_)
    assert list(sig.parameters) == ["dst", "seed", "draw", "sizes", "timesteps", "discount", "timestep_div"]
    assert sig.parameters["discount"].default == 0.9 and sig.parameters["timestep_div"].default == 1000.0
    sig = inspect.signature(noise.geowizard_pyramid_level_sizes)
    assert list(sig.parameters) == ["rows", "cols", "rng", "scale"] and sig.parameters["rng"].default is np.random and sig.parameters["scale"].default == 1.5
    sig = inspect.signature(noise.geowizard_pyramid_noise_into)
    assert list(sig.parameters) == ["dst_nhwc_slice", "gen", "timesteps", "discount", "sizes"] and sig.parameters["discount"].default == 0.9
    msg = training.GEOWIZARD_PYRAMID_MESSAGE
    assert "geowizard_pyramid" in msg and "e2eft_pyramid_noise_weighted" in msg
    assert "t / 1000" in msg and "286-296" in msg and "not built" in msg                 # the pinned substrings stay
    assert "geowizard_pyramid" in training.GEOWIZARD_NOISE_TYPES and "pyramid" in training.GEOWIZARD_NOISE_TYPES
    dst = torch.zeros(2, 3, 5, 4)
    with pytest.raises(TypeError, match="int64"):
        ops.pyramid_noise_weighted_(dst, 1, 0, [(1, 1)], torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError, match="int64"):
        ops.pyramid_noise_weighted_(dst, 1, 0, [(1, 1)], [0, 999])
    with pytest.raises(ValueError, match="one entry per sample"):
        ops.pyramid_noise_weighted_(dst, 1, 0, [(1, 1)], torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        ops.pyramid_noise_weighted_(dst, 1, 0, [(1, 1)], torch.zeros(4, dtype=torch.int64)[::2])
    with pytest.raises(ValueError, match="at most 10 levels"):
        ops.pyramid_noise_weighted_(dst, 1, 0, [(1, 1)] * 11, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="timestep_div"):
        ops.pyramid_noise_weighted_(dst, 1, 0, [(1, 1)], torch.zeros(2, dtype=torch.int64), timestep_div=0.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                           # everything well-formed, but not on the device
        ops.pyramid_noise_weighted_(dst, 1, 0, [(1, 1)], torch.zeros(2, dtype=torch.int64))
    g = noise.DeviceNoise(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        noise.geowizard_pyramid_noise_into(dst, g, torch.zeros(2, dtype=torch.int64), sizes=[(1, 1)])


def test_weighted_entry_point_validates_before_launching():
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.e2eft_pyramid_noise_workspace_bytes(2, 4, 108)
    sizes = (ctypes.c_int32 * 22)(*([1] * 22))
    call = lambda *a: lib.e2eft_pyramid_noise_weighted(*a)      # noqa: E731
    assert call(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 1, sizes, None, 1000.0, p, p, need, None) == 1 and b"timesteps" in lib.e2eft_last_error()
    assert call(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 1, sizes, p, 0.0, p, p, need, None) == 1 and b"timestep_div" in lib.e2eft_last_error()
    assert call(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 1, sizes, p, -1000.0, p, p, need, None) == 1 and b"timestep_div" in lib.e2eft_last_error()
    assert call(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 1, sizes, p, float("nan"), p, p, need, None) == 1
    # the existing entry's checks
    assert call(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 11, sizes, p, 1000.0, p, p, need, None) == 1 and b"levels" in lib.e2eft_last_error()
    assert call(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 1, sizes, p, 1000.0, p, p, 16, None) == 2 and b"workspace" in lib.e2eft_last_error()
    assert call(0, 2, 4, 9, 12, 2, 1, 0, 0.9, 1, sizes, p, 1000.0, p, p, need, None) == 1 and b"shape" in lib.e2eft_last_error()          # ldy < c
    assert call(7, 2, 4, 9, 12, 4, 1, 0, 0.9, 1, sizes, p, 1000.0, p, p, need, None) == 1 and b"dtype" in lib.e2eft_last_error()
    assert call(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 1, sizes, p, 1000.0, None, p, need, None) == 1 and b"null" in lib.e2eft_last_error()
    assert call(0, 1, 1, 1, 1, 1, 1, 0, 0.9, 1, sizes, p, 1000.0, p, p, need, None) == 1                                                    # one element has no unbiased std
    sizes[0] = 0
    assert call(0, 2, 4, 9, 12, 4, 1, 0, 0.9, 1, sizes, p, 1000.0, p, p, need, None) == 1 and b"level 0" in lib.e2eft_last_error()
    assert lib.e2eft_version() == 119


def test_trainers_know_the_new_name_and_still_refuse_the_old_one():
    from diffusion_e2e_ft_amd import training
    fn = training._geowizard_noise
    with pytest.raises(ValueError, match="t / 1000"):
        fn("pyramid", None, None, 4, 4, 8, 8, torch.float32, "cpu")
    with pytest.raises(TypeError, match="DeviceNoise"):
        fn("geowizard_pyramid", None, None, 4, 4, 8, 8, torch.float32, "cpu", torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="Unknown noise type"):
        fn("perlin", None, None, 4, 4, 8, 8, torch.float32, "cpu")
