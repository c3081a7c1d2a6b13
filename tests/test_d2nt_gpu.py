"""Depth-to-normal translation on the GPU (csrc/d2nt.hip, e2eft_depth_to_normals): the kernel against the reference's recorded outputs
(tests/golden/d2nt_golden.pt) and the numpy restatement tests/d2nt_ref.py on full Virtual KITTI frames, ragged and minimal sizes, graph capture,
and the end-to-end claim: the reference's two-step workflow (generate vkitti_DAG_normals/, then train from the files) and the on-the-fly path
(VirtualKITTI2(normals="d2nt")) give identical training batches.

Tolerances: the kernel's powf is correctly rounded; numpy's float32 power (which made the fixture) is not, and differs by 1 ulp on
a share of inputs.  Where a snapping ratio lies within 1e-5 of e (margin < 1e-5: integer-centimetre depth makes exact ratios of e common), such a
difference may flip a snap; those pixels are counted, and FLIP_BUDGET bounds the count.  Everywhere else fp32 agrees within 2e-6 and the uint16 /
uint8 encodings are exact apart from +-1 LSB on at most 1e-4 of the components."""
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import d2nt_ref  # noqa: E402

GOLD = torch.load(os.path.join(HERE, "golden", "d2nt_golden.pt"), weights_only=False)
FLIP_BUDGET = 8           # pixels per image whose normal may differ beyond 2e-6 because a near-e snapping ratio flipped
F32_TOL = 2e-6
LSB_SHARE = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _run(depth_m, K, refine, fmt, dev, scale=100.0):
    from diffusion_e2e_ft_amd import ops
    d = torch.from_numpy(np.ascontiguousarray(depth_m)).to(dev)
    k = torch.tensor(np.asarray(K, dtype=np.float32), device=dev)
    out = ops.depth_to_normals(d, k, refine=refine, out_format=fmt, depth_scale=scale)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _source_margin(margin, choice, refine):
    if not refine:
        return margin
    src = d2nt_ref.refine(np.repeat(margin[..., None], 3, axis=2).astype(np.float64), choice)[..., 0]
    return np.minimum(margin, src)


def _compare(tag, got, ref_normal, ref_u16, margin):
    """got: {fmt: array [H,W,3]}; margin [H,W] (source margin).  Returns the number of near-threshold pixels that differ."""
    near = margin < 1e-5
    f32 = got["f32"].astype(np.float64)
    bad = np.abs(f32 - ref_normal).max(-1) > F32_TOL
    assert not (bad & ~near).any(), "%s: fp32 off by %.3g away from any snapping threshold" % (tag, np.abs(f32 - ref_normal).max(-1)[~near].max())
    flips = int((bad & near).sum())
    assert flips <= FLIP_BUDGET, "%s: %d near-threshold pixels flipped" % (tag, flips)
    keep = ~bad
    du = np.abs(got["u16"].astype(np.int64) - ref_u16.astype(np.int64))[keep]
    assert du.max(initial=0) <= 1 and (du > 0).mean() <= LSB_SHARE, "%s: u16 %d components differ" % (tag, int((du > 0).sum()))
    d8 = np.abs(got["u8"].astype(np.int64) - (ref_u16 >> 8).astype(np.int64))[keep]
    assert d8.max(initial=0) <= 1 and (d8 > 0).mean() <= LSB_SHARE, "%s: u8 %d components differ" % (tag, int((d8 > 0).sum()))
    return flips


@pytest.mark.parametrize("i", range(len(GOLD["cases"])))
def test_kernel_matches_reference_fixture(dev, i):
    c = GOLD["cases"][i]
    cm = c["depth_cm"].numpy()
    dm = d2nt_ref.cm_to_metres(cm)
    choice = c["choice"].numpy().astype(np.int64)
    margin = c["margin"].numpy()
    got = {r: {f: _run(dm, c["K"], r, f, dev) for f in ("f32", "u16", "u8")} for r in (False, True)}
    for r, v in ((False, "v2"), (True, "v3")):
        _compare("case %d %s" % (i, v), got[r], c["normal_" + v].numpy(), c["u16_" + v].numpy(), _source_margin(margin, choice, r))
    # the argmin map exactly: every v3 pixel carries, bit for bit, the v2 normal of the neighbour the reference chose (zeros beyond the image)
    for f in ("f32", "u16", "u8"):
        v2 = got[False][f]
        pad = np.pad(v2.astype(np.float64), ((1, 1), (1, 1), (0, 0)), constant_values=np.nan)
        H, W = choice.shape
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        dy, dx = np.array([0, 0, -1, 1, 0])[choice], np.array([-1, 1, 0, 0, 0])[choice]
        assert np.array_equal(pad[yy + 1 + dy, xx + 1 + dx], got[True][f].astype(np.float64)), f
    # u8 is u16's high byte from the same fp64 value
    for r in (False, True):
        assert np.array_equal(got[r]["u8"], (got[r]["u16"] >> 8).astype(np.uint8))


def test_full_frames_per_image_intrinsics_against_restatement(dev):
    from diffusion_e2e_ft_amd import ops
    rng = np.random.default_rng(2024)
    B, H, W = 8, 375, 1242
    cm = np.stack([d2nt_ref.vkitti_like_depth_cm(rng, H, W, sky=bool(b % 2 == 0)) for b in range(B)])
    dm = d2nt_ref.cm_to_metres(cm)
    K = np.array([[725.0087 + 13 * b, 725.0087 - 7 * b, 620.5 + b, 187.0 - 2 * b] for b in range(B)], dtype=np.float32)
    d = torch.from_numpy(dm).to(dev)
    k = torch.from_numpy(K).to(dev)
    got = {f: ops.depth_to_normals(d, k, refine=True, out_format=f, depth_scale=100.0).cpu().numpy() for f in ("f32", "u16", "u8")}
    v2 = ops.depth_to_normals(d, k, refine=False, out_format="f32", depth_scale=100.0).cpu().numpy()
    total = 0
    for b in (0, 3, 5, 7):
        ref = d2nt_ref.depth_to_normals(dm[b], tuple(float(x) for x in K[b]), True)
        total += _compare("image %d" % b, {f: got[f][b] for f in got}, ref["normal"], ref["u16"], _source_margin(ref["margin"], ref["choice"].astype(np.int64), True))
        # the restatement with the kernel's correctly rounded powf: the same values bit for bit (all but a rare fp64-exp rounding tie)
        cr = d2nt_ref.depth_to_normals(dm[b], tuple(float(x) for x in K[b]), True, power=d2nt_ref.correctly_rounded_power)
        assert (got["u16"][b] != cr["u16"]).any(-1).sum() <= 2
        assert (got["f32"][b] != cr["normal"].astype(np.float32)).any(-1).sum() <= 2
        crv2 = d2nt_ref.depth_to_normals(dm[b], tuple(float(x) for x in K[b]), False, power=d2nt_ref.correctly_rounded_power)
        assert (v2[b] != crv2["normal"].astype(np.float32)).any(-1).sum() <= 2
    print("near-threshold flips over 4 frames:", total)


@pytest.mark.parametrize("shape", [(2, 2), (3, 1241), (2, 65), (17, 2), (33, 130)])
def test_ragged_and_minimal_sizes(dev, shape):
    rng = np.random.default_rng(shape[0] * 10007 + shape[1])
    cm = d2nt_ref.vkitti_like_depth_cm(rng, *shape)
    dm = d2nt_ref.cm_to_metres(cm)
    for r in (False, True):
        ref = d2nt_ref.depth_to_normals(dm, d2nt_ref.VKITTI_K, r, power=d2nt_ref.correctly_rounded_power)
        got = {f: _run(dm, d2nt_ref.VKITTI_K, r, f, dev) for f in ("f32", "u16", "u8")}
        assert np.array_equal(got["f32"], ref["normal"].astype(np.float32)) and np.array_equal(got["u16"], ref["u16"]) and np.array_equal(got["u8"], ref["u8"])


def test_rejects_images_below_two_pixels(dev):
    from diffusion_e2e_ft_amd import ops
    k = torch.tensor(d2nt_ref.VKITTI_K, dtype=torch.float32, device=dev)
    for shape in ((1, 1, 5), (1, 5, 1), (2, 1, 1)):
        with pytest.raises(RuntimeError, match="height and width >= 2"):
            ops.depth_to_normals(torch.ones(shape, device=dev), k)
    with pytest.raises(ValueError):
        ops.depth_to_normals(torch.ones((1, 4, 4), device=dev), k, out_format="png")


def test_graph_capture_replays_bit_equal(dev):
    from diffusion_e2e_ft_amd import ops
    rng = np.random.default_rng(77)
    dm = torch.from_numpy(d2nt_ref.cm_to_metres(np.stack([d2nt_ref.vkitti_like_depth_cm(rng, 96, 200) for _ in range(3)]))).to(dev)
    k = torch.tensor([[700.0, 710.0, 99.5, 40.0], [725.0087, 725.0087, 620.5, 187.0], [500.0, 500.0, 100.0, 48.0]], dtype=torch.float32, device=dev)
    outs = {f: ops.depth_to_normals(dm, k, out_format=f, depth_scale=100.0) for f in ("f32", "u16", "u8")}
    eager = {f: v.cpu().clone() for f, v in outs.items()}
    static = {f: torch.empty_like(v) for f, v in outs.items()}
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for f in static:
            ops.depth_to_normals(dm, k, out_format=f, depth_scale=100.0, out=static[f])
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in static:
            ops.depth_to_normals(dm, k, out_format=f, depth_scale=100.0, out=static[f])
    for f in static:
        static[f].zero_() if f != "u16" else static[f].view(torch.int16).zero_()
    g.replay()
    torch.cuda.synchronize()
    for f in static:
        assert torch.equal(static[f].cpu().view(torch.uint8), eager[f].view(torch.uint8)), f
    # the replay reads the depth buffer as it is at replay time
    dm.mul_(1.5)
    g.replay()
    ref = ops.depth_to_normals(dm, k, out_format="f32", depth_scale=100.0)
    torch.cuda.synchronize()
    assert torch.equal(static["f32"], ref)


def _batches(loader, seed):
    torch.manual_seed(seed)
    random.seed(seed)
    return [{k: (v.cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()} for b in loader]


def test_generated_files_and_on_the_fly_normals_give_identical_batches(dev, tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts"))
    try:
        import gen_vkitti_normals as gen
    finally:
        sys.path.pop(0)
    import dataset_fixture as dfx
    from diffusion_e2e_ft_amd import data
    vroot = dfx.make_vkitti_tree(str(tmp_path), n=3)
    assert gen.main([vroot, "--batch", "2"]) == 3                       # the reference's step 1: the folder on disk (overwrites the fixture's maps)
    files = data.VirtualKITTI2(vroot, transform=True)
    syn = data.VirtualKITTI2(vroot, transform=True, normals="d2nt")
    # what the file holds is the kernel's u8 of the decoded depth
    smp = files[2]
    want = data.depth_to_normals_vkitti(torch.from_numpy(smp["depth"]).to(dev), out_format="u8").cpu().numpy()
    assert np.array_equal(smp["normal_u8"], want)
    for bs in (2, 1):
        a = _batches(data.DeviceLoader(files, batch_size=bs, device=dev, workers=2), 5)
        b = _batches(data.DeviceLoader(syn, batch_size=bs, device=dev, workers=2), 5)
        assert len(a) == len(b) == (3 + bs - 1) // bs
        for x, y in zip(a, b):
            for k in ("normals", "val_mask", "depth", "rgb", "metric"):
                assert torch.equal(x[k], y[k]), k
            assert x["domain"] == y["domain"] == ["outdoor"] * x["rgb"].shape[0]
    # the same through finish_samples directly, without a transform
    d = torch.from_numpy(np.stack([files[i]["depth"] for i in range(2)])).to(dev)
    rgb = torch.from_numpy(np.stack([files[i]["rgb_u8"] for i in range(2)])).to(dev)
    n = torch.from_numpy(np.stack([files[i]["normal_u8"] for i in range(2)])).to(dev)
    p = data.finish_samples(rgb, d, n, "vkitti", transform=False)
    q = data.finish_samples(rgb, d, None, "vkitti", transform=False)
    for k in ("normals", "val_mask", "depth", "rgb"):
        assert torch.equal(p[k], q[k]), k
    with pytest.raises(ValueError):
        data.finish_samples(rgb, d, None, "hypersim", transform=False)
