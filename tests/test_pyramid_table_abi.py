"""The capture-safe noise / EMA entry points without a GPU: e2eft_pyramid_table_set, e2eft_pyramid_noise_at / _weighted_at, e2eft_randint_fill /
_at and e2eft_ema_step_at refuse a bad argument BEFORE anything is launched (return code 1 and a message; every call here is a refused one: the pointers are
host memory, no well-formed call is made), the host
restatement of the integer draw on hand-computed words, and the host-side handles (noise.DrawAt's named draw words, the refusals of EMAModel's two halves)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import noise_ref
import randint_ref


def _lib_and_pointer():
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(22 * 8 + 64)
    base = ctypes.addressof(buf)
    return lib, buf, ctypes.c_void_p((base + 15) & ~15)          # (16-byte aligned inside the buffer, which the caller keeps alive)


def test_pyramid_table_set_validates_before_launching():
    lib, _keep, p = _lib_and_pointer()
    sizes = (ctypes.c_int32 * 22)(*([1] * 22))
    call = lib.e2eft_pyramid_table_set
    assert call(None, 0, 1, sizes, 8, 8, None) == 1 and b"pointer" in lib.e2eft_last_error()
    assert call(p, 0, 1, None, 8, 8, None) == 1 and b"pointer" in lib.e2eft_last_error()
    assert call(ctypes.c_void_p(p.value + 4), 0, 1, sizes, 8, 8, None) == 1 and b"misaligned" in lib.e2eft_last_error()
    assert call(p, 0, 11, sizes, 8, 8, None) == 1 and b"levels" in lib.e2eft_last_error()
    assert call(p, 0, -1, sizes, 8, 8, None) == 1 and b"levels" in lib.e2eft_last_error()
    assert call(p, 0, 1, sizes, 0, 8, None) == 1 and b"shape" in lib.e2eft_last_error()
    assert call(p, 0, 1, sizes, 8, -3, None) == 1 and b"shape" in lib.e2eft_last_error()
    sizes[2] = 0                                                   # level 1: rows 0
    assert call(p, 0, 2, sizes, 8, 8, None) == 1 and b"level 1 size" in lib.e2eft_last_error()
    sizes[2] = -4
    assert call(p, 0, 2, sizes, 8, 8, None) == 1 and b"level 1 size" in lib.e2eft_last_error()
    sizes[2] = 1
    sizes[0] = 9                                                   # level 0: 9 rows over an 8-row output
    assert call(p, 0, 1, sizes, 8, 8, None) == 1 and b"exceeds the output" in lib.e2eft_last_error()
    sizes[0], sizes[5] = 8, 9                                      # level 2: 9 cols
    assert call(p, 0, 3, sizes, 8, 8, None) == 1 and b"level 2" in lib.e2eft_last_error() and b"exceeds the output" in lib.e2eft_last_error()
    assert lib.e2eft_version() == 119


def test_pyramid_at_entry_points_validate_before_launching():
    lib, _keep, p = _lib_and_pointer()
    need = lib.e2eft_pyramid_noise_workspace_bytes(2, 4, 108)
    at, wat = lib.e2eft_pyramid_noise_at, lib.e2eft_pyramid_noise_weighted_at
    assert at(0, 2, 4, 9, 12, 4, 1, None, 0.9, p, p, need, None) == 1 and b"table" in lib.e2eft_last_error()
    assert at(0, 2, 4, 9, 12, 4, 1, ctypes.c_void_p(p.value + 4), 0.9, p, p, need, None) == 1 and b"table" in lib.e2eft_last_error()
    assert at(0, 2, 4, 9, 12, 4, 1, p, 0.9, None, p, need, None) == 1 and b"null" in lib.e2eft_last_error()
    assert at(0, 2, 4, 9, 12, 4, 1, p, 0.9, p, p, 16, None) == 2 and b"workspace" in lib.e2eft_last_error()
    assert at(7, 2, 4, 9, 12, 4, 1, p, 0.9, p, p, need, None) == 1 and b"dtype" in lib.e2eft_last_error()
    assert at(0, 2, 4, 9, 12, 2, 1, p, 0.9, p, p, need, None) == 1 and b"shape" in lib.e2eft_last_error()
    assert wat(0, 2, 4, 9, 12, 4, 1, None, 0.9, p, 1000.0, p, p, need, None) == 1 and b"table" in lib.e2eft_last_error()
    assert wat(0, 2, 4, 9, 12, 4, 1, p, 0.9, None, 1000.0, p, p, need, None) == 1 and b"timesteps" in lib.e2eft_last_error()
    assert wat(0, 2, 4, 9, 12, 4, 1, p, 0.9, p, 0.0, p, p, need, None) == 1 and b"timestep_div" in lib.e2eft_last_error()
    assert wat(0, 2, 4, 9, 12, 4, 1, p, 0.9, p, 1000.0, p, p, 16, None) == 2 and b"workspace" in lib.e2eft_last_error()


def test_randint_fill_validates_before_launching():
    lib, _keep, p = _lib_and_pointer()
    fill, fill_at = lib.e2eft_randint_fill, lib.e2eft_randint_fill_at
    assert fill(4, 1, 0, 1, 0, 0, p, None) == 1 and b"high" in lib.e2eft_last_error()
    assert fill(4, 1, -7, 1, 0, 0, p, None) == 1 and b"high" in lib.e2eft_last_error()
    assert fill(4, 1, 2 ** 31, 1, 0, 0, p, None) == 1 and b"high" in lib.e2eft_last_error()
    assert fill(0, 1, 1000, 1, 0, 0, p, None) == 1 and b"n must be" in lib.e2eft_last_error()
    assert fill(-2, 1, 1000, 1, 0, 0, p, None) == 1 and b"n must be" in lib.e2eft_last_error()
    assert fill(4, 0, 1000, 1, 0, 0, p, None) == 1 and b"repeat" in lib.e2eft_last_error()
    assert fill(4, 1, 1000, 1, 0, 0, None, None) == 1 and b"pointer" in lib.e2eft_last_error()
    assert fill_at(4, 1, 1000, 1, None, 0, p, None) == 1 and b"draw" in lib.e2eft_last_error()
    assert fill_at(4, 1, 0, 1, p, 0, p, None) == 1 and b"high" in lib.e2eft_last_error()
    assert fill_at(0, 1, 1000, 1, p, 0, p, None) == 1 and b"n must be" in lib.e2eft_last_error()


def test_ema_step_at_validates_before_launching():
    lib, _keep, p = _lib_and_pointer()
    assert lib.e2eft_ema_step_at(8, p, p, None, None) == 1 and b"one_minus_decay" in lib.e2eft_last_error()
    assert lib.e2eft_ema_step_at(8, p, p, ctypes.c_void_p(p.value + 2), None) == 1 and b"one_minus_decay" in lib.e2eft_last_error()
    assert lib.e2eft_ema_step_at(0, p, p, p, None) == 1 and b"bad args" in lib.e2eft_last_error()
    assert lib.e2eft_ema_step_at(8, None, p, p, None) == 1
    assert lib.e2eft_ema_step_at(8, ctypes.c_void_p(p.value + 4), p, p, None) == 1


def test_randint_restatement_on_hand_computed_words():
    f = randint_ref.from_word
    assert f(0, 1000) == 0 and f(0xFFFFFFFF, 1000) == 999 and f(0x80000000, 1000) == 500 and f(0x7FFFFFFF, 1000) == 499
    assert f(0x12345678, 1000) == 71                               # 305419896 * 1000 / 2^32 = 71.11...
    assert f(0xFFFFFFFF, 1) == 0 and f(0xFFFFFFFF, 2 ** 31 - 1) == 2 ** 31 - 2 and f(0x00000003, 2 ** 31 - 1) == 1
    seed, draw, slot, n = 0x5EED0123456789AB, 11, 3, 7
    words, _ = noise_ref.words(seed, draw, slot, n)
    for high in (1, 1000, 2 ** 31 - 1):
        got = randint_ref.randint(seed, draw, slot, n, high, repeat=2)
        assert got.dtype == np.int64 and got.shape == (2 * n,)
        want = [f(words[e, e & 3], high) for e in range(n)]      # element e: word e & 3 of the counter of quad e >> 2 (row e of `words`)
        assert got.tolist() == want + want
        assert 0 <= got.min() and got.max() < high
    assert not np.array_equal(randint_ref.randint(seed, draw, slot, n, 1000), randint_ref.randint(seed, draw + 1, slot, n, 1000))


def test_signatures_of_the_host_layer():
    from diffusion_e2e_ft_amd import noise, ops, training
    assert list(inspect.signature(noise.randint_into).parameters) == ["dst_int64", "high", "gen", "repeat"]
    assert inspect.signature(noise.randint_into).parameters["repeat"].default == 1
    assert list(inspect.signature(noise.set_pyramid_table).parameters) == ["table_dev", "gen", "sizes", "rows", "cols"]
    assert list(inspect.signature(noise.pyramid_noise_at).parameters)[:3] == ["dst_nhwc_slice", "seed", "table_dev"]
    assert list(inspect.signature(noise.geowizard_pyramid_noise_at).parameters)[:4] == ["dst_nhwc_slice", "seed", "table_dev", "timesteps"]
    assert list(inspect.signature(training.EMAModel.step_at).parameters) == ["self", "parameters", "word"]
    assert list(inspect.signature(training.EMAModel.set_decay_word).parameters) == ["self", "word"]
    assert issubclass(training.CapturedTrainStepAt, training.CapturedTrainStep)
    sig = inspect.signature(training.CapturedTrainStepAt.diffusion)
    assert list(sig.parameters)[:10] == ["unet", "vae", "optimizer", "domain", "noise_scheduler", "prediction_type", "noise_type", "generator", "accumulation", "ema"]
    assert sig.parameters["noise_type"].default == "gaussian"
    assert ops.PYRAMID_TABLE_WORDS == 22


def test_host_refusals_of_the_wrappers():
    from diffusion_e2e_ft_amd import ops
    table = torch.zeros(22, dtype=torch.int64)
    with pytest.raises(TypeError, match="22 elements"):
        ops.pyramid_table_set_(torch.zeros(21, dtype=torch.int64), 0, [(1, 1)], 8, 8)
    with pytest.raises(TypeError, match="int64"):
        ops.pyramid_table_set_(torch.zeros(22, dtype=torch.int32), 0, [(1, 1)], 8, 8)
    with pytest.raises(ValueError, match="at most 10 levels"):
        ops.pyramid_table_set_(table, 0, [(1, 1)] * 11, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pyramid_table_set_(table, 0, [(1, 1)], 8, 8)
    dst = torch.zeros(2, 3, 5, 4)
    with pytest.raises(TypeError, match="22 elements"):
        ops.pyramid_noise_at_(dst, 1, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="one entry per sample"):
        ops.pyramid_noise_weighted_at_(dst, 1, table, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pyramid_noise_weighted_at_(dst, 1, table, torch.zeros(2, dtype=torch.int64))
    out = torch.zeros(6, dtype=torch.int64)
    with pytest.raises(ValueError, match="high"):
        ops.randint_fill_(out, 0, 1, 0)
    with pytest.raises(ValueError, match="high"):
        ops.randint_fill_(out, 2 ** 31, 1, 0)
    with pytest.raises(ValueError, match="multiple of repeat"):
        ops.randint_fill_(out, 1000, 1, 0, repeat=4)
    with pytest.raises(TypeError, match="int64"):
        ops.randint_fill_(torch.zeros(6, dtype=torch.int32), 1000, 1, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.randint_fill_(out, 1000, 1, 0, repeat=2)
    with pytest.raises(TypeError, match="one-element fp32"):
        ops.ema_step_at_(torch.zeros(8), torch.zeros(8), torch.zeros(2))


def test_draw_at_names_one_word_per_draw_site_and_checks_its_table():
    from diffusion_e2e_ft_amd import noise
    one = noise.DrawAt(5, torch.arange(1, dtype=torch.int64))                     # the Gaussian word alone (CapturedTrainStep)
    assert one.randint_dev is None and one.table is None
    with pytest.raises(RuntimeError, match="no word for an integer draw"):
        one.randint_word()
    words = torch.tensor([10, 11], dtype=torch.int64)
    two = noise.DrawAt(5, words[1:2], torch.zeros(22, dtype=torch.int64), (8, 6), randint_dev=words[0:1])
    # no cursor: a draw site reads ITS word however often it is executed (a recomputed segment), in whatever order
    assert [int(two.randint_word()) for _ in range(3)] == [10, 10, 10] and int(two.draw_dev) == 11
    assert two.randint_word().data_ptr() == words.data_ptr() and two.draw_dev.data_ptr() == words.data_ptr() + 8      # views, not copies
    assert not hasattr(two, "take") and not hasattr(two, "rewind")
    assert two.table_for(8, 6) is two.table
    with pytest.raises(ValueError, match="filled for"):
        two.table_for(6, 8)
    with pytest.raises(RuntimeError, match="no pyramid table"):
        one.table_for(8, 6)
    with pytest.raises(RuntimeError, match="no host counter"):
        two.next_draw()
    with pytest.raises(ValueError, match="explicit `sizes`"):
        noise.pyramid_noise_into(torch.zeros(1, 8, 6, 4), two, sizes=[(1, 1)])


def test_ema_halves_refuse_outside_the_flat_one_launch_form():
    from diffusion_e2e_ft_amd import training
    params = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]
    ema = training.EMAModel(params)                                                # per-tensor shadow: no FlatAdamW buffer underneath
    word = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="flat one-launch form"):
        ema.set_decay_word(word)
    with pytest.raises(NotImplementedError, match="flat one-launch form"):
        ema.step_at(params, word)
    assert ema.optimization_step == 0 and ema.cur_decay_value is None            # a refusal moves nothing
