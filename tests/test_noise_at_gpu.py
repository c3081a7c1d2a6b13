"""The capture-safe forms of DESIGN.md §3.28 at kernel level: e2eft_pyramid_noise_at / _weighted_at (draw and level table read on the device) against the
by-value entry points, e2eft_pyramid_table_set, e2eft_randint_fill / _at against the host restatement tests/randint_ref.py, and e2eft_ema_step_at against
e2eft_ema_step.  The `_at` kernels are the by-value kernels' own bodies behind a loader, so every comparison is `torch.equal`: no tolerance anywhere."""
import pytest
import torch

import randint_ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
LAYOUTS = {"vec4": (2, 4, 8, 8), "scalar": (2, 3, 9, 13), "strided": (2, 4, 8, 8)}       # [B,C,H,W]; "strided": channels 4:8 of an 8-channel buffer


def _tables(H, W):
    """0 levels, 10 levels (explicit, non-increasing), one 1 x 1 level, one level of the output's own size"""
    ten = [(max(1, H - (H - 1) * i // 9), max(1, W - (W - 1) * i // 9)) for i in range(10)]
    assert ten[0] == (H, W) and ten[-1] == (1, 1) and all(a[0] >= b[0] and a[1] >= b[1] for a, b in zip(ten, ten[1:]))
    return {"none": [], "ten": ten, "one_by_one": [(1, 1)], "own_size": [(H, W)]}


def _dst(shape, dtype, dev, strided):
    B, C, H, W = shape
    if not strided:
        buf = torch.full((B, H, W, C), 7.0, dtype=dtype, device=dev)
        return buf, buf
    buf = torch.arange(B * H * W * 8, device=dev, dtype=torch.float32).reshape(B, H, W, 8).remainder(251.0).sub(125.0).to(dtype)
    return buf[..., 4:], buf


def _table(dev):
    return torch.full((22,), -1, dtype=torch.int64, device=dev)


def _t(values, dev):
    return torch.tensor(values, dtype=torch.int64, device=dev)


# ---- 1. pyramid `_at` against by-value --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_pyramid_at_equals_by_value(dev, dtype, layout):
    from diffusion_e2e_ft_amd import ops
    shape = LAYOUTS[layout]
    B, C, H, W = shape
    table = _table(dev)
    for k, (name, sizes) in enumerate(sorted(_tables(H, W).items())):
        draw = 9 + k
        want, _ = _dst(shape, dtype, dev, layout == "strided")
        ops.pyramid_noise_(want, SEED, draw, sizes)
        ops.pyramid_table_set_(table, draw, sizes, H, W)
        flat = [v for rc in sizes for v in rc]
        assert table.tolist() == [draw, len(sizes)] + flat + [1] * (20 - len(flat)), name
        got, buf = _dst(shape, dtype, dev, layout == "strided")
        before = buf.clone()
        assert ops.pyramid_noise_at_(got, SEED, table) is got
        assert torch.equal(got, want), (name, (got.float() - want.float()).abs().max().item())
        assert bool(torch.isfinite(got.float()).all()) and not torch.equal(got, before[..., 4:] if layout == "strided" else before)
        if layout == "strided":
            assert torch.equal(buf[..., :4], before[..., :4])                    # the other channels: bit-unchanged


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_weighted_pyramid_at_equals_by_value(dev, dtype, layout):
    """three samples, so that the timesteps {0, 999, 500} of the issue each weight a row of their own"""
    from diffusion_e2e_ft_amd import ops
    shape = (3,) + LAYOUTS[layout][1:]
    B, C, H, W = shape
    table, t = _table(dev), _t([0, 999, 500], dev)
    for k, (name, sizes) in enumerate(sorted(_tables(H, W).items())):
        draw = 0xFFFFFFF0 + k                                                     # (the high bit of the 32-bit draw travels through the int64 word)
        want, _ = _dst(shape, dtype, dev, layout == "strided")
        ops.pyramid_noise_weighted_(want, SEED, draw, sizes, t)
        ops.pyramid_table_set_(table, draw, sizes, H, W)
        got, buf = _dst(shape, dtype, dev, layout == "strided")
        before = buf.clone()
        ops.pyramid_noise_weighted_at_(got, SEED, table, t)
        assert torch.equal(got, want), (name, (got.float() - want.float()).abs().max().item())
        if layout == "strided":
            assert torch.equal(buf[..., :4], before[..., :4])
    # another divisor and discount travel as launch arguments, as in the by-value form
    sizes = _tables(H, W)["ten"]
    ops.pyramid_table_set_(table, 3, sizes, H, W)
    a = ops.pyramid_noise_weighted_at_(_dst(shape, dtype, dev, False)[0], SEED, table, t, discount=0.7, timestep_div=500.0)
    b = ops.pyramid_noise_weighted_(_dst(shape, dtype, dev, False)[0], SEED, 3, sizes, t, discount=0.7, timestep_div=500.0)
    assert torch.equal(a, b)


def test_a_table_outside_its_contract_is_clamped_on_the_device(dev):
    """the host cannot check device words: n_levels is clamped into [0, 10], level rows into [1, rows], level cols into [1, cols] — a foreign table changes the
    noise and nothing else.  The expected result is the by-value call with the clamped values."""
    from diffusion_e2e_ft_amd import ops
    B, C, H, W = 2, 4, 8, 8
    raw = [5, 99] + [10 ** 12, -3, 0, 2 ** 40, 7, 7, -(2 ** 62), 9, 3, 3, 2, 2 ** 31, 1, 1, 4, 4, 8, 8, 6, 5]
    clamped = [(8, 1), (1, 8), (7, 7), (1, 8), (3, 3), (2, 8), (1, 1), (4, 4), (8, 8), (6, 5)]
    table = _t(raw, dev)
    got = ops.pyramid_noise_at_(torch.empty((B, H, W, C), device=dev), SEED, table)
    want = ops.pyramid_noise_(torch.empty((B, H, W, C), device=dev), SEED, 5, clamped)
    assert torch.equal(got, want)
    table[1] = -4                                                                  # a negative count: no level at all
    got = ops.pyramid_noise_at_(torch.empty((B, H, W, C), device=dev), SEED, table)
    assert torch.equal(got, ops.pyramid_noise_(torch.empty((B, H, W, C), device=dev), SEED, 5, []))
    assert table.tolist()[2:] == raw[2:]                                           # the table is only read


# ---- 2. pyramid `_at` under capture: the test that catches a baked-in table -----------------------------------------------------------------------------------
def test_a_captured_pyramid_reads_its_table_at_replay(dev):
    from diffusion_e2e_ft_amd import ops
    B, C, H, W = 3, 4, 8, 8
    ten = _tables(H, W)["ten"]
    rounds = [(21, ten[:3], [0, 999, 500]), (22, [(2, 5)], [731, 0, 17]), (0xFFFFFFFF, ten[:6], [999, 999, 1]), (23, [], [5, 6, 7]), (24, ten, [250, 0, 999])]
    assert [len(r[1]) for r in rounds] == [3, 1, 6, 0, 10]
    table, t = _table(dev), _t([1, 2, 3], dev)
    xin = torch.zeros((B, H, W, 8), device=dev)
    plain = torch.zeros((B, H, W, C), device=dev)
    ops.pyramid_table_set_(table, 1, ten[:2], H, W)
    ops.pyramid_noise_at_(plain, SEED, table)                                     # code objects loaded before the capture
    ops.pyramid_noise_weighted_at_(xin[..., 4:], SEED, table, t)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                                  # one stream, no parallel branches
        ops.pyramid_noise_at_(plain, SEED, table)
        ops.pyramid_noise_weighted_at_(xin[..., 4:], SEED, table, t)
    seen = []
    for draw, sizes, steps in rounds:
        ops.pyramid_table_set_(table, draw, sizes, H, W)
        t.copy_(_t(steps, dev))
        graph.replay()
        torch.cuda.synchronize()
        want = ops.pyramid_noise_(torch.empty((B, H, W, C), device=dev), SEED, draw, sizes)
        assert torch.equal(plain, want), (draw, len(sizes))
        want = ops.pyramid_noise_weighted_(torch.empty((B, H, W, C), device=dev), SEED, draw, sizes, _t(steps, dev))
        assert torch.equal(xin[..., 4:], want), (draw, len(sizes))
        assert bool((xin[..., :4] == 0).all())
        seen.append(plain.clone())
    assert all(not torch.equal(a, b) for a, b in zip(seen, seen[1:]))             # five tables, five results


# ---- 3. randint ------------------------------------------------------------------------------------------------------------------------------------------
def test_randint_equals_the_host_restatement(dev):
    from diffusion_e2e_ft_amd import ops
    draw_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    for n in (1, 2, 5, 7):
        for high in (1, 1000, 2 ** 31 - 1):
            for repeat in (1, 2):
                for slot in (0, 3):
                    draw = 40 + n
                    want = randint_ref.randint(SEED, draw, slot, n, high, repeat)
                    out = torch.full((repeat * n,), -1, dtype=torch.int64, device=dev)
                    assert ops.randint_fill_(out, high, SEED, draw, slot=slot, repeat=repeat) is out
                    assert out.cpu().tolist() == want.tolist(), (n, high, repeat, slot)
                    assert int(out.min()) >= 0 and int(out.max()) < high
                    draw_dev.fill_(draw)
                    at = ops.randint_fill_at_(torch.full((repeat * n,), -1, dtype=torch.int64, device=dev), high, SEED, draw_dev, slot=slot, repeat=repeat)
                    assert torch.equal(at, out), (n, high, repeat, slot)
    a = ops.randint_fill_(torch.empty(7, dtype=torch.int64, device=dev), 1000, SEED, 1, slot=0)
    assert not torch.equal(a, ops.randint_fill_(torch.empty(7, dtype=torch.int64, device=dev), 1000, SEED, 1, slot=3))
    assert not torch.equal(a, ops.randint_fill_(torch.empty(7, dtype=torch.int64, device=dev), 1000, SEED, 2, slot=0))
    # more than one block and a ragged last quad
    n = 4 * 256 * 3 + 2
    big = ops.randint_fill_(torch.empty(2 * n, dtype=torch.int64, device=dev), 1000, SEED, 77, repeat=2)
    assert big.cpu().tolist() == randint_ref.randint(SEED, 77, 0, n, 1000, 2).tolist()
    assert len(set(big.cpu().tolist())) > 900                                      # all of [0, 1000) is reached, not a corner of it


def test_randint_into_advances_the_generator_once_and_dispatches_on_a_draw_at(dev):
    from diffusion_e2e_ft_amd import noise
    gen = noise.DeviceNoise(SEED, draw=5)
    out = noise.randint_into(torch.empty(4, dtype=torch.int64, device=dev), 1000, gen, repeat=2)
    assert gen.draw == 6 and out.cpu().tolist() == randint_ref.randint(SEED, 5, 0, 2, 1000, 2).tolist()
    words = torch.zeros(2, dtype=torch.int64, device=dev)
    at = noise.DrawAt(SEED, words[1:2], randint_dev=words[0:1])
    host = noise.DeviceNoise(SEED, draw=5)
    noise.set_draw(words[0:1], host)
    noise.set_draw(words[1:2], host)
    assert words.tolist() == [5, 6] and host.draw == 7
    first = noise.randint_into(torch.empty(4, dtype=torch.int64, device=dev), 1000, at, repeat=2)           # its own word
    second = noise.randn_into(torch.empty((1, 2, 2, 4), device=dev), at)                                   # the Gaussian word
    assert torch.equal(first, out)
    assert torch.equal(second, noise.randn_into(torch.empty((1, 2, 2, 4), device=dev), noise.DeviceNoise(SEED, draw=6)))


def test_a_captured_randint_redraws_when_its_word_changes(dev):
    from diffusion_e2e_ft_amd import ops
    draw_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.zeros(10, dtype=torch.int64, device=dev)
    ops.randint_fill_at_(out, 1000, SEED, draw_dev, repeat=2)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.randint_fill_at_(out, 1000, SEED, draw_dev, repeat=2)
    seen = []
    for draw in (3, 4, 0xFFFFFFFF, 3):
        draw_dev.fill_(draw)
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().tolist() == randint_ref.randint(SEED, draw, 0, 5, 1000, 2).tolist(), draw
        seen.append(out.clone())
    assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[3])


# ---- 4. ema_step_at ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 1027])
def test_ema_step_at_equals_ema_step(dev, n):
    import ctypes
    from diffusion_e2e_ft_amd import ops
    g = torch.Generator(device=dev).manual_seed(n)
    param = torch.randn(n, generator=g, device=dev)
    a = torch.randn(n, generator=g, device=dev)
    b = a.clone()
    word = torch.zeros(1, device=dev)
    for omd in (0.25, 1e-4, 1.0):                                                  # (1.0 last: it moves the shadow onto the parameters)
        assert not torch.equal(a, param)                                           # the comparison below is not one of two copies of `param`
        word.fill_(ctypes.c_float(omd).value)
        ops.ema_step_(a, param, omd)
        assert ops.ema_step_at_(b, param, word) is b
        assert torch.equal(a, b), (n, omd)


def test_a_captured_ema_step_reads_its_word_at_replay(dev):
    import ctypes
    from diffusion_e2e_ft_amd import ops
    n = 1027
    g = torch.Generator(device=dev).manual_seed(5)
    param = torch.randn(n, generator=g, device=dev)
    want = torch.randn(n, generator=g, device=dev)
    got = want.clone()
    word = torch.zeros(1, device=dev)
    ops.ema_step_at_(got.clone(), param, word)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ema_step_at_(got, param, word)
    for omd in (0.25, 1e-4, 1.0, 0.5):
        word.fill_(ctypes.c_float(omd).value)
        param.mul_(1.01)                                                           # the parameters move between steps, in place
        graph.replay()
        torch.cuda.synchronize()
        ops.ema_step_(want, param, omd)
        assert torch.equal(got, want), omd
