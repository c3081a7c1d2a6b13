"""The channel-aware error measures of tests/util.py (no GPU): what tests/test_f32split_range_gpu.py relies on them for."""
import torch

from util import chan_err_rows, chan_err_wgrad, rel_err


def _wgrad(dy, x):
    return dy.reshape(-1, dy.shape[-1]).t().double() @ x.reshape(-1, x.shape[-1]).double()      # 1x1: [cout, cin]


def test_chan_err_wgrad_is_invariant_to_channel_scales_and_sees_a_small_wrong_row():
    g = torch.Generator().manual_seed(3)
    dy, x = torch.randn(2, 4, 4, 8, generator=g).double(), torch.randn(2, 4, 4, 12, generator=g).double()
    ref = _wgrad(dy, x)
    got = ref + 1e-6 * torch.randn(ref.shape, generator=g).double()
    e0 = chan_err_wgrad(got, ref, dy, x, 1)
    sy, sx = 2.0 ** torch.randint(-30, 30, (8,), generator=g).double(), 2.0 ** torch.randint(-30, 30, (12,), generator=g).double()
    e1 = chan_err_wgrad(got * sy[:, None] * sx[None, :], ref * sy[:, None] * sx[None, :], dy * sy, x * sx, 1)
    assert abs(e1 - e0) <= 1e-12 * e0
    # a row 2^-20 below the rest that is wholly wrong: nothing in the global measure, everything in this one
    dy2 = dy.clone()
    dy2[..., 3] *= 2.0 ** -20
    ref2 = _wgrad(dy2, x)
    bad = ref2.clone()
    bad[3] = 0.0
    assert rel_err(bad, ref2) < 1e-5 and chan_err_wgrad(bad, ref2, dy2, x, 1) > 1e-2
    assert chan_err_rows(bad.t(), ref2.t()) == 1.0


def test_chan_err_leaves_all_zero_channels_out():
    g = torch.Generator().manual_seed(4)
    dy, x = torch.randn(1, 4, 4, 8, generator=g), torch.randn(1, 4, 4, 8, generator=g)
    dy[..., 2] = 0.0
    x[..., 5] = 0.0
    ref = _wgrad(dy, x)
    assert chan_err_wgrad(ref, ref, dy, x, 1) == 0.0
    got = ref.clone()
    got[2, 0] = 1.0          # in a dead row: the caller checks those for exact zeros itself
    assert chan_err_wgrad(got, ref, dy, x, 1) == 0.0
    assert chan_err_rows(ref.t(), ref.t()) == 0.0
