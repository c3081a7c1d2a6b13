"""The radix select of csrc/select.h through its three callers, on the smallest inputs where a digit pass, the scan or the successor rule can go
wrong: ops.masked_quantiles (32-bit order keys, torch's rank rule), e2eft_normal_eval_finalize (raw fp32 bits, the median) and
ops.hypersim_preprocess (64-bit order keys, numpy's 90th percentile).  Expected values come from a CPU sort and are compared bit for bit; the one
interpolated masked_quantiles case keeps tests/test_data_gpu.py's bound of 1e-6 relative against torch.quantile."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hypersim_prep_ref as hpr  # noqa: E402

NEAR, FAR = 1e-5, 65.0
ONE, V = 0x3F800000, 0x3FC00000          # bits of 1.0f and of 1.5f (the value of the runs)
GAPS = {"next_bin": 1, "middle_digit": 1 << 10, "top_digit": 1 << 21}      # where the run's successor lies: the last histogram, or beyond it


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _shuffled(values, seed):
    return values[np.random.default_rng(seed).permutation(values.size)]


def run_then_gap(n, k, gap, seed=0):
    """n values whose sorted order has a run of equal values ending at index k and the next larger value, V + gap in bit patterns, at k + 1"""
    run = min(k + 1, 5)
    below = ONE + np.arange(k + 1 - run)
    above = V + gap + 3 * np.arange(n - k - 1)
    s = _f32(np.concatenate([below, np.full(run, V), above]))
    assert s.size == n and np.all(np.diff(s) >= 0) and s[k] == s[k - run + 1] and s[k + 1] > s[k]
    return _shuffled(s, seed)


def inputs32():
    """name -> fp32 valid values, all inside (NEAR, FAR) and below +inf"""
    two = np.float32(2.0)
    edge = _f32(np.concatenate([np.full(5, np.nextafter(two, np.float32(0))), np.full(3, two), np.full(9, np.nextafter(two, np.float32(3)))]).view(np.uint32))
    cases = {"a_last_digit_full": _shuffled(_f32(ONE + np.arange(1024)), 1), "b_top_digit_edge": _shuffled(edge, 2)}
    for name, gap in GAPS.items():
        cases["c_even_" + name] = run_then_gap(40, 19, gap, 3)           # the median's k = n / 2 - 1
        cases["c_odd_" + name] = run_then_gap(41, 20, gap, 4)
    cases.update(d_one=_f32([V]), d_two=_f32([V, ONE]), d_three=_f32([V + 1, ONE, V]), d_equal=_f32(np.full(37, V)), d_none=_f32([]))
    return cases


INPUTS32 = inputs32()


# ---- ops.masked_quantiles ------------------------------------------------------------------------------------------------------------------------
def _image(valid, length, seed):
    """the valid values among invalid ones (0.0 and values >= FAR), `length` elements"""
    assert length >= valid.size
    junk = np.resize(np.array([0.0, FAR, 100.0, 0.0], dtype=np.float32), length - valid.size)
    return _shuffled(np.concatenate([valid, junk]), seed)


def _pad_4m1(valid):
    """append copies of the largest value until the count is 4 m + 1: q (n - 1) is then an exact fp32 integer for q in {0, .25, .5, .75, 1}"""
    extra = (1 - valid.size) % 4
    return np.concatenate([valid, np.full(extra, valid.max(), dtype=np.float32)]) if valid.size else valid


def _exact_quantile_check(out_row, valid, q_lo, q_hi, what):
    s = np.sort(valid)
    n = s.size
    assert out_row[2] == n, what
    if n == 0:
        assert out_row[0] == 0 and out_row[1] == 0 and out_row[3] == 0, what
        return
    r_lo, r_hi = q_lo * (n - 1), q_hi * (n - 1)
    assert r_lo == int(r_lo) and r_hi == int(r_hi)
    lo, hi = s[int(r_lo)], s[int(r_hi)]
    assert out_row[:2].view(np.uint32).tolist() == [lo.view(np.uint32), hi.view(np.uint32)], (what, out_row, lo, hi)
    assert out_row[3] == (1.0 if lo != hi else 0.0), what


QS = (0.0, 0.25, 0.5, 0.75, 1.0)


@pytest.mark.parametrize("name", sorted(INPUTS32))
def test_masked_quantiles_exact_ranks(dev, name):
    from diffusion_e2e_ft_amd import ops
    valid = _pad_4m1(INPUTS32[name])
    img = torch.from_numpy(_image(valid, valid.size + 11, 5))[None].to(dev)
    for q_lo, q_hi in itertools.combinations_with_replacement(QS, 2):
        out = ops.masked_quantiles(img, NEAR, FAR, q_lo, q_hi).cpu().numpy()
        _exact_quantile_check(out[0], valid, q_lo, q_hi, (name, q_lo, q_hi))


def test_masked_quantiles_exact_ranks_mixed_batch(dev):
    """every input in one batch (per-selection state must not leak between images), twice: the second call reuses what the first left behind"""
    from diffusion_e2e_ft_amd import ops
    names = sorted(INPUTS32)
    valids = [_pad_4m1(INPUTS32[k]) for k in names]
    length = max(v.size for v in valids) + 7
    batch = torch.from_numpy(np.stack([_image(v, length, 10 + i) for i, v in enumerate(valids)])).to(dev)
    for q_lo, q_hi in ((0.25, 0.75), (0.0, 1.0), (0.5, 0.5)):
        out = ops.masked_quantiles(batch, NEAR, FAR, q_lo, q_hi).cpu().numpy()
        for i, name in enumerate(names):
            _exact_quantile_check(out[i], valids[i], q_lo, q_hi, (name, q_lo, q_hi))


@pytest.mark.parametrize("gap", sorted(GAPS))
def test_masked_quantiles_interpolated_across_a_run_end(dev, gap):
    """n = 102 (not 4 m + 1), q = (0.02, 0.98): ranks 2.02 and 98.98.  The run ends at the floor of each rank in turn, so the successor comes from
    the next bin, another middle digit or another top digit (the minimum pass).  Bound: 1e-6 relative against torch.quantile."""
    from diffusion_e2e_ft_amd import ops
    n = 102
    for k in (2, 98):
        valid = run_then_gap(n, k, GAPS[gap], 6)
        img = torch.from_numpy(_image(valid, n + 9, 7))[None].to(dev)
        out = ops.masked_quantiles(img, NEAR, FAR, 0.02, 0.98).cpu()[0]
        v = torch.from_numpy(valid)
        lo, hi = torch.quantile(v, 0.02), torch.quantile(v, 0.98)
        assert int(out[2]) == n and out[3] == 1.0
        assert abs(float(out[0]) - float(lo)) <= 1e-6 * max(1.0, abs(float(lo))), (k, float(out[0]), float(lo))
        assert abs(float(out[1]) - float(hi)) <= 1e-6 * max(1.0, abs(float(hi))), (k, float(out[1]), float(hi))


# ---- e2eft_normal_eval_finalize --------------------------------------------------------------------------------------------------------------
def _finalize(dev, ws, valid, n_nan=0, seed=0):
    """the record over an error buffer holding `valid` among +inf (masked) slots; the totals say n valid, n_nan NaNs (the sums do not enter the median)"""
    from diffusion_e2e_ft_amd import ops
    buf = _shuffled(np.concatenate([valid, np.full(valid.size // 3 + 5, np.inf, dtype=np.float32)]), seed)
    totals = torch.zeros(9, dtype=torch.int64)
    totals[0], totals[1] = valid.size, n_nan
    return ops.normal_eval_finalize(torch.from_numpy(buf).to(dev), buf.size, totals.to(dev), ws[0], ws[1]).cpu().numpy()


@pytest.fixture(scope="module")
def ne_ws(dev):
    from diffusion_e2e_ft_amd import ops
    return ops.normal_eval_workspace(dev)


@pytest.mark.parametrize("name", sorted(k for k in INPUTS32 if k != "d_none"))
def test_normal_eval_median_exact(dev, ne_ws, name):
    """one workspace for every case, as an accumulator reuses it: odd and even counts of each input"""
    valid = INPUTS32[name]
    for v in (valid, valid[:-1]):
        if v.size == 0:
            continue
        out = _finalize(dev, ne_ws, v, seed=v.size)
        want = np.median(v)
        assert want.dtype == np.float32 and out[8] == v.size
        assert np.float64(want) == out[1] and np.float32(out[1]).view(np.uint32) == want.view(np.uint32), (name, v.size, out[1], want)


def test_normal_eval_nan_records(dev, ne_ws):
    valid = INPUTS32["c_even_top_digit"]
    assert np.isnan(_finalize(dev, ne_ws, INPUTS32["d_none"])[:8]).all()                    # n = 0
    out = _finalize(dev, ne_ws, valid, n_nan=1)                                              # one NaN counted among the valid errors
    assert np.isnan(out[:3]).all() and out[8] == valid.size
    assert _finalize(dev, ne_ws, valid)[1] == np.float64(np.median(valid))                  # and the workspace serves the next call


# ---- ops.hypersim_preprocess: 64-bit keys --------------------------------------------------------------------------------------------------------
H = W = 16
NPIX = H * W


def _frame(colors, seed):
    """NPIX pixels: `colors` [n, 3] fp32 are the valid ones (id 1), the rest get id -1 and a bright colour that must not count"""
    colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
    n_invalid = NPIX - colors.shape[0]
    assert n_invalid >= 0
    c = np.concatenate([colors, np.full((n_invalid, 3), 7.0, dtype=np.float32)])
    ids = np.concatenate([np.ones(colors.shape[0], dtype=np.int32), np.full(n_invalid, -1, dtype=np.int32)])
    perm = np.random.default_rng(seed).permutation(NPIX)
    return c[perm].reshape(H, W, 3), ids[perm].reshape(H, W)


def _run_colors(n, successor):
    """n valid pixels whose brightness has a run of equal values ending at rank k = floor(0.9 (n - 1)), with `successor` the colour of rank k + 1"""
    k = int(np.floor(0.9 * (n - 1)))
    run = 6
    below = [(0.5, 0.5, j * 2.0 ** -20) for j in range(k + 1 - run)]
    above = [successor] + [(2.0, 2.0, float(j)) for j in range(n - k - 2)]
    return np.array(below + [(1.0, 1.0, 0.0)] * run + above, dtype=np.float32)


def hypersim_frames():
    rng = np.random.default_rng(11)
    frames = {
        # r = g = 1, b = j 2^-49: 256 distinct fp64 brightness values over 449 ulps; the first five digits are single-bin, the last one is not
        "last_digit": _frame([(1.0, 1.0, j * 2.0 ** -49) for j in range(256)], seed=1),
        "succ_last_digit": _frame(_run_colors(250, (1.0, 1.0, 2.0 ** -49)), seed=2),
        "succ_middle_digit": _frame(_run_colors(250, (1.0, 1.0, 2.0 ** -30)), seed=3),
        "succ_top_digit": _frame(_run_colors(250, (1.0, 1.5, 0.0)), seed=4),            # another exponent: nothing above a in any histogram of its prefix
        "one_valid": _frame([(0.25, 0.5, 0.75)], seed=5),
        "none_valid": _frame(np.zeros((0, 3)), seed=6),
        "both_signs": _frame(rng.uniform(-1.0, 1.0, size=(231, 3)), seed=7),
    }
    c, ids = frames["last_digit"]                                                        # what the construction claims, checked on the CPU
    c64 = c.astype(np.float64)
    keys = np.unique((0.3 * c64[..., 0] + 0.59 * c64[..., 1] + 0.11 * c64[..., 2]).view(np.uint64))
    assert keys.size == 256 and np.unique(keys >> 9).size == 2                           # two groups of the last 9-bit digit
    for name, (c, _) in frames.items():
        c64 = c.astype(np.float64)
        br = 0.3 * c64[..., 0] + 0.59 * c64[..., 1] + 0.11 * c64[..., 2]
        assert not np.any((br == 0) & np.signbit(br)), name                              # -0.0 stays out of the exact cases
    return frames


FRAMES = hypersim_frames()


def _hypersim_records(dev, names):
    from diffusion_e2e_ft_amd import ops
    color = torch.from_numpy(np.stack([FRAMES[k][0] for k in names])).to(dev)
    ids = torch.from_numpy(np.stack([FRAMES[k][1] for k in names])).to(dev)
    _, _, rec = ops.hypersim_preprocess(color, torch.ones(len(names), H, W, device=dev), ids)
    return rec.cpu().numpy()


def _check_percentile(rec_row, name):
    c, ids = FRAMES[name]
    want = hpr.preprocess(c, np.ones((H, W), dtype=np.float32), ids)["record"]
    for slot, key in ((11, "n_valid"), (12, "percentile"), (13, "scale")):
        got, w = rec_row[slot], np.float64(want[key])
        assert got.view(np.uint64) == w.view(np.uint64) or (np.isnan(got) and np.isnan(w)), (name, key, got, w)


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_hypersim_percentile_exact(dev, name):
    _check_percentile(_hypersim_records(dev, [name])[0], name)


def test_hypersim_percentile_exact_mixed_batch(dev):
    names = sorted(FRAMES) + sorted(FRAMES)[::-1]
    rec = _hypersim_records(dev, names)
    for i, name in enumerate(names):
        _check_percentile(rec[i], name)
