"""The bars and inputs of tests/test_gn_statistics_gpu.py, proven on the CPU with fp32 emulations of the producers' summation orders (tests/gn_stats_model.py) on
exactly the tensors the GPU tests use:
  * every order — one accumulator about the first row or about the column minimum, eight strided lanes added as a butterfly, Welford, 64-row blocks about their own
    first rows merged by Chan's formula, the stand-alone pass's per-lane pivots merged relative to lane 0's pivot — stays below 1.0 of the mean bar and of the M2
    bar on every (image, slab, channel) of every case, the two hostile cases included, and gives a constant channel EXACTLY (c, 0);
  * a column swap, a slab swap (an image swap where an image is one slab) and shifted sums about the NEXT column's pivot exceed a bar on every (image, slab, channel)
    they touch; so does a swap of two parity phases of the upsampler;
  * the cases are representable: building them asserts that the fp32 convolution equals the fp64 one bit for bit, that every operand is exact in fp16 and bf16, that
    rounding `pre` to fp16 / bf16 changes at least half of it; here also that the channels of an N tile are separated by 8 sigma."""
import pytest
import torch

import gn_stats_model as gm

CONV = list(gm.CONV_CASES)
STANDALONE = [(shape, dt) for shape in gm.STANDALONE_SHAPES for dt in gm.DTYPES] + [(gm.STANDALONE_HOSTILE, "hostile")]


def _standalone(shape, dt):
    return gm.standalone_case(*shape, "fp32" if dt == "hostile" else dt, hostile=dt == "hostile")


def _check_orders(cols, consts, pl=None):
    """cols [n, ...(image, slab)..., C] -> worst ratios over every order"""
    n, mu, m2, R = gm.triple(cols)
    flat = cols.reshape(cols.shape[0], -1)
    worst = (0.0, 0.0)
    for name, (gmu, gm2) in gm.emulations(flat, pl).items():
        gmu, gm2 = gmu.view(mu.shape), gm2.view(mu.shape)
        rm, r2 = gm.ratios(gmu, gm2, n, mu, m2, R)
        assert rm < 1.0 and r2 < 1.0, (name, rm, r2)
        assert torch.equal(gmu[..., consts].double(), mu[..., consts]) and bool((gm2[..., consts] == 0).all()), "%s: a constant channel is not exact" % name
        worst = (max(worst[0], rm), max(worst[1], r2))
    return worst


@pytest.mark.parametrize("name", CONV)
def test_every_order_stays_below_the_bars_on_the_conv_cases(name):
    c = gm.get_conv_case(name)
    worst = _check_orders(gm.slab_columns(c["pre"], c["slab_id"], c["nslabs"]), c["consts"])
    print("%s: worst %.3f of the mean bar, %.3f of the M2 bar" % (name, *worst))


@pytest.mark.parametrize("shape,dt", STANDALONE, ids=lambda v: str(v).replace(" ", ""))
def test_every_order_stays_below_the_bars_on_the_standalone_cases(shape, dt):
    c = _standalone(shape, dt)
    B, H, W, C = shape
    _, _, pl = gm.standalone_geometry(H * W, C, 2 if dt in ("fp16", "bf16") else 4)
    worst = (0.0, 0.0)
    for s in range(c["nslabs"]):
        w = _check_orders(c["t"][:, c["slab_id"] == s].transpose(0, 1).contiguous(), c["consts"], pl)
        worst = (max(worst[0], w[0]), max(worst[1], w[1]))
    print("%s %s: worst %.3f of the mean bar, %.3f of the M2 bar" % (shape, dt, *worst))


def _exceeds(got_mu, got_m2, n, mu, m2, R, keep):
    rm, r2 = gm.entry_ratios(got_mu, got_m2, n, mu, m2, R)
    return bool((torch.maximum(rm, r2)[..., keep] > 1.0).all()), torch.maximum(rm, r2)[..., keep].min().item()


def _mutants(cols, consts, what):
    """cols [n, B, S, C]"""
    n, mu, m2, R = gm.triple(cols)
    C = mu.shape[-1]
    everyone = torch.ones(C, dtype=torch.bool)
    varying = everyone.clone()
    varying[consts] = False
    ok, least = _exceeds(torch.roll(mu, 1, -1), torch.roll(m2, 1, -1), n, mu, m2, R, everyone)
    assert ok, "%s: a column swap stays inside the bars (%.2f)" % (what, least)
    axis = 1 if mu.shape[1] > 1 else 0
    assert mu.shape[axis] > 1
    ok, least2 = _exceeds(torch.roll(mu, 1, axis), torch.roll(m2, 1, axis), n, mu, m2, R, varying)
    assert ok, "%s: a slab swap stays inside the bars (%.2f)" % (what, least2)
    flat = cols.reshape(cols.shape[0], -1)
    gmu, gm2 = gm.emu_wrong_pivot(flat)
    rm, _ = gm.entry_ratios(gmu.view(mu.shape), gm2.view(mu.shape), n, mu, m2, R)
    rm = rm.reshape(-1)[:-1]          # (the roll wraps the last column of the last slab onto the first of the first)
    assert bool((rm > 1.0).all()), "%s: a pivot from the next column stays inside the mean bar (%.2f)" % (what, rm.min().item())
    return least, least2, rm.min().item()


@pytest.mark.parametrize("name", CONV)
def test_swaps_and_a_wrong_pivot_exceed_the_bars_on_the_conv_cases(name):
    c = gm.get_conv_case(name)
    cols = gm.slab_columns(c["pre"], c["slab_id"], c["nslabs"])
    print("%s: least excess column swap %.1f, slab swap %.1f, wrong pivot %.1f x the bar" % ((name,) + _mutants(cols, c["consts"], name)))
    if c["up"]:      # two phases of one run of low-resolution pixels: slabs ph * runs + r
        n, mu, m2, R = gm.triple(cols)
        runs = c["nslabs"] // 4
        varying = torch.ones(mu.shape[-1], dtype=torch.bool)
        varying[c["consts"]] = False
        ok, least = _exceeds(torch.roll(mu, runs, 1), torch.roll(m2, runs, 1), n, mu, m2, R, varying)
        assert ok, "%s: a phase swap stays inside the bars (%.2f)" % (name, least)


@pytest.mark.parametrize("shape,dt", STANDALONE, ids=lambda v: str(v).replace(" ", ""))
def test_swaps_and_a_wrong_pivot_exceed_the_bars_on_the_standalone_cases(shape, dt):
    c = _standalone(shape, dt)
    P = c["t"].shape[1]
    if P % c["nslabs"] == 0:
        cols = gm.slab_columns(c["t"], c["slab_id"], c["nslabs"])
    else:      # a shorter last slab: the whole slabs
        full = c["slab_id"] < c["nslabs"] - 1
        cols = gm.slab_columns(c["t"][:, full], c["slab_id"][full], c["nslabs"] - 1)
    _mutants(cols, c["consts"], "%s %s" % (shape, dt))


@pytest.mark.parametrize("name", CONV)
def test_conv_cases_are_representable_and_separated(name):
    c = gm.get_conv_case(name)          # (the construction asserts exactness, representability and the effect of rounding)
    assert len(c["consts"]) == (c["geom"][4] + 127) // 128
    gm.assert_separated(c["pre"], c["consts"])
    n, mu, m2, R = gm.slab_triples(c["pre"], c["slab_id"], c["nslabs"])
    assert bool((m2[..., c["consts"]] == 0).all()) and bool((R[..., c["consts"]] == 0).all())
    assert torch.equal(c["written"]["fp32"], c["pre"])
    if c["hostile"]:
        first = torch.stack([(c["slab_id"] == s).nonzero()[0, 0] for s in range(c["nslabs"])])
        varying = [ch for ch in range(mu.shape[-1]) if ch not in c["consts"]]
        sd = (m2 / n.view(1, -1, 1)).sqrt()[..., varying]
        assert bool((mu[..., varying].abs() >= 300.0 * sd).all())          # (sigma of a slab includes its outlier: 30 / 16 + 1; of the rest: 1)
        out = c["pre"][:, first][..., varying] - mu[..., varying]
        assert bool((out >= 25.0).all()), out.min()


@pytest.mark.parametrize("shape,dt", STANDALONE, ids=lambda v: str(v).replace(" ", ""))
def test_standalone_cases_are_separated(shape, dt):
    c = _standalone(shape, dt)
    gm.assert_separated(c["t"], c["consts"])
    if dt != "hostile":
        assert gm.representable(c["t"], gm.DTYPES[dt])


def test_welford_from_zero_misses_the_mean_bar_far_from_zero():
    """the row-by-row Welford update the generic branch of igemm_epilogue_rows used to hold (deleted: no launch reached it), started at zero on the values themselves: fine for M2, but its running mean is
    rounded at the size of the mean in every row — on the ladder (|mean| up to 2000, R ~ 5, n = 128) that is several times the mean bar; about a pivot it is not.
    Statistics for that branch would need another form: this one does not meet the bars."""
    c = gm.get_conv_case("rows_3x3")
    cols = gm.slab_columns(c["pre"], c["slab_id"], c["nslabs"])
    n, mu, m2, R = gm.triple(cols)
    gmu, gm2 = gm.emu_welford(cols.reshape(cols.shape[0], -1))
    rm, r2 = gm.ratios(gmu.view(mu.shape), gm2.view(mu.shape), n, mu, m2, R)
    print("welford from zero: %.2f of the mean bar, %.2f of the M2 bar" % (rm, r2))
    assert rm > 1.0 and r2 < 1.0, (rm, r2)
    near = mu.abs() <= R          # rungs next to zero
    rmn, _ = gm.entry_ratios(gmu.view(mu.shape), gm2.view(mu.shape), n, mu, m2, R)
    assert bool(near.any()) and bool((rmn[near] < 1.0).all())


@pytest.mark.parametrize("shape,dt,which", [((2, 5, 5, 320), "fp16", 0), ((2, 6, 6, 960), "bf16", 1)], ids=["5x5x320-fp16-mean", "6x6x960-bf16-M2"])
def test_merging_absolute_lane_means_exceeds_the_bars_on_short_slabs(shape, dt, which):
    """what gn_partial_kernel did before: the per-lane triples merged through their absolute means.  Every merge rounds at the size of the mean; on the 25-pixel slab
    of the fp16 case that is 1.09 x the mean bar, on the two 9-pixel lanes of the bf16 case (two levels of the bf16 grid, |mean| / R = 260) 3.5 x the M2 bar — the
    figures the kernel itself gave on the MI355X before it merged relative to lane 0's pivot."""
    c = _standalone(shape, dt)
    B, H, W, C = shape
    _, _, pl = gm.standalone_geometry(H * W, C, 2)
    worst = [0.0, 0.0]
    for s in range(c["nslabs"]):
        cols = c["t"][:, c["slab_id"] == s].transpose(0, 1).contiguous()
        n, mu, m2, R = gm.triple(cols)
        gmu, gm2 = gm.emu_standalone(cols.reshape(cols.shape[0], -1), pl, relative=False)
        r = gm.ratios(gmu.view(mu.shape), gm2.view(mu.shape), n, mu, m2, R)
        worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print("%s %s, absolute lane means: %.3f of the mean bar, %.3f of the M2 bar" % (shape, dt, *worst))
    assert worst[which] > 1.0, worst


def test_targets_cover_both_kinds():
    assert set(gm.TARGET.values()) == {"pre", "written"}
