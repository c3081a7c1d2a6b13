"""Hypersim preprocessing on the GPU (csrc/hypersimprep.hip, e2eft_hypersim_preprocess): the kernels against the reference's recorded outputs
(tests/golden/hypersim_prep_golden.pt: every small case and the digests of the full 768 x 1024 frame the reference's whole script processed) —
uint8 image, uint16 depth and the float32 depth the loader would read back are BIT-EXACT, the record holds the CPU bounds (tests/hypersim_prep_ref.py
check_record) —, against the numpy restatement on ragged shapes and a mixed batch, under graph capture, and the end-to-end claim: the reference's
two-step workflow (write processed/, then train from the files) and Hypersim(source="raw") give identical training batches.

uint8 exactness: the device's fp64 pow may differ from the host's in the last place; that can change trunc(out * 255) only where out * 255 lies within
~1e-13 of an integer.  The fixture's generator asserts that none of its elements is within 1e-9; check_u8 prints the float64 value of any element
that differs and excuses it only inside that margin (none was seen)."""
import hashlib
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hypersim_prep_ref as hpr  # noqa: E402
import hypersim_raw_fixture as rawfx  # noqa: E402

GOLD = torch.load(os.path.join(HERE, "golden", "hypersim_prep_golden.pt"), weights_only=False)
NCASES = 14


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _run(color, distance, ids, dev):
    """-> (rgb_u8, u16, depth_f32, record) numpy, batch axis kept as given; both depth formats from the same inputs"""
    from diffusion_e2e_ft_amd import ops
    c, d, e = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (color, distance, ids))
    rgb, u16, rec = ops.hypersim_preprocess(c, d, e, depth_format="u16")
    rgb2, f32, rec2 = ops.hypersim_preprocess(c, d, e, depth_format="f32")
    torch.cuda.synchronize()
    assert torch.equal(rgb, rgb2) and torch.equal(rec.view(torch.int64), rec2.view(torch.int64))
    return rgb.cpu().numpy(), u16.cpu().numpy(), f32.cpu().numpy(), rec.cpu().numpy()


def _check_frame(got, b, ref, what):
    rgb, u16, f32, rec = got
    sel = (lambda a: a) if b is None else (lambda a: a[b])
    hpr.check_u8(sel(rgb), ref, what)
    assert np.array_equal(sel(u16), ref["u16"]), what
    assert np.array_equal(sel(f32).view(np.uint32), ref["depth_f32"].view(np.uint32)), what
    hpr.check_record(sel(rec), ref["record"], what)
    assert sel(rec)[14] == 0.0 and sel(rec)[15] == 0.0


@pytest.mark.parametrize("i", range(NCASES))
def test_kernel_matches_reference_fixture(dev, i):
    c = GOLD["cases"][i]
    color, distance, ids = c["color"].numpy(), c["distance"].numpy(), c["ids"].numpy()
    rgb, u16, f32, rec = _run(color, distance, ids, dev)
    ref = hpr.preprocess(color, distance, ids)           # (equal to the fixture: tests/test_hypersim_prep_cpu.py) for out * 255 and the two extra record fields
    want = c["rgb_u8"].numpy()
    if not np.array_equal(rgb, want):
        hpr.check_u8(rgb, ref, c["name"])                # prints the float64 value at each element that differs
    assert np.array_equal(rgb, want), c["name"]          # the fixture has no element within 1e-9 of an integer: nothing to excuse
    assert np.array_equal(u16, c["u16"].numpy().astype(np.uint16)), c["name"]
    assert np.array_equal(f32.view(np.uint32), c["depth_f32"].numpy().view(np.uint32)), c["name"]
    hpr.check_record(rec, dict(ref["record"], **c["record"]), c["name"])


def test_full_frame_matches_the_reference_script(dev):
    f = GOLD["full"]
    color, distance, ids = hpr.full_frame(f["color_palette"].numpy(), f["distance_palette"].numpy())
    rgb, u16, f32, rec = _run(color[None], distance[None], ids[None], dev)
    dig = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    if (dig(rgb[0]), dig(u16[0]), dig(f32[0])) != (f["rgb_sha256"], f["u16_sha256"], f["depth_f32_sha256"]):      # say where, before the digests fail
        ref = hpr.preprocess(color, distance, ids)
        hpr.check_u8(rgb[0], ref, "full frame")
        for name, got, want in (("u16", u16[0], ref["u16"]), ("f32", f32[0].view(np.uint32), ref["depth_f32"].view(np.uint32))):
            bad = np.argwhere(got != want)
            print("full frame %s: %d elements differ; first %s" % (name, len(bad), [(tuple(ix), got[tuple(ix)], want[tuple(ix)], ref["u16"][tuple(ix)]) for ix in bad[:8]]))
    assert dig(rgb[0]) == f["rgb_sha256"] and dig(u16[0]) == f["u16_sha256"]
    assert dig(f32[0]) == f["depth_f32_sha256"]
    hpr.check_record(rec[0], {k: float(f["csv_row"][k]) for k in hpr.RECORD_FIELDS[:9]}, "csv row")


def _random_frame(rng, H, W, cdt, ddt, invalid):
    color = (rng.random((H, W, 3)) ** 2 * 2.5 * (0.1 + rng.random())).astype(cdt)
    dist = (0.3 + rng.random((H, W)) * 20.0).astype(ddt)
    ids = rng.integers(1, 99, (H, W)).astype(np.int32)
    ids[rng.random((H, W)) < invalid] = -1
    return color, dist, ids


@pytest.mark.parametrize("shape", [(1, 1), (3, 1241), (17, 2), (33, 130), (260, 301)])
@pytest.mark.parametrize("cdt,ddt", [(np.float16, np.float32), (np.float32, np.float16)])
def test_ragged_shapes_against_restatement(dev, shape, cdt, ddt):
    rng = np.random.default_rng(shape[0] * 10007 + shape[1])
    color, dist, ids = _random_frame(rng, shape[0], shape[1], cdt, ddt, 0.2 if shape[0] > 1 else 0.0)
    _check_frame(_run(color, dist, ids, dev), None, hpr.preprocess(color, dist, ids), str(shape))


def test_batch_with_different_valid_counts_and_an_all_invalid_frame(dev):
    rng = np.random.default_rng(5)
    frames = [_random_frame(rng, 37, 53, np.float16, np.float16, inv) for inv in (0.05, 1.1, 0.6)]
    frames[0][2][3, 4] = 0                                # an id equal to 0: counted for the caller, the frame is still processed
    frames[2][0][7, 8, 1] = np.nan                        # a NaN colour on a valid pixel: flagged, the frame's scale is NaN, its image 0
    frames[2][2][7, 8] = 5
    frames[2][1][1, 1], frames[2][2][1, 1] = -0.75, 9     # a negative distance wraps like the x86 cast
    frames[0][1][2, 2], frames[0][2][2, 2] = np.inf, 9
    color, dist, ids = (np.stack([f[k] for f in frames]) for k in range(3))
    got = _run(color, dist, ids, dev)
    refs = [hpr.preprocess(*f) for f in frames]
    assert [r["record"]["n_valid"] for r in refs][1] == 0 and refs[1]["record"]["scale"] == 1.0 and len({r["record"]["n_valid"] for r in refs}) == 3
    assert refs[0]["record"]["zero_ids"] == 1 and refs[2]["record"]["nan_brightness"] == 1 and np.isnan(refs[2]["record"]["scale"])
    assert refs[2]["u16"][1, 1] > 60000 and refs[0]["u16"][2, 2] == 0
    for b, ref in enumerate(refs):
        _check_frame(got, b, ref, "frame %d" % b)
    # a frame's result does not depend on its neighbours in the batch
    for b, f in enumerate(frames):
        one = _run(*f, dev)
        for x, y in zip(one, got):
            assert np.array_equal(x.view(np.uint8), np.ascontiguousarray(y[b]).view(np.uint8))


def test_graph_capture_replays_bit_equal(dev):
    from diffusion_e2e_ft_amd import ops
    rng = np.random.default_rng(77)
    frames = [_random_frame(rng, 96, 200, np.float16, np.float16, inv) for inv in (0.1, 0.3, 1.1)]
    c, d, e = (torch.from_numpy(np.stack([f[k] for f in frames])).to(dev) for k in range(3))
    eager = {fmt: [t.cpu().clone() for t in ops.hypersim_preprocess(c, d, e, depth_format=fmt)] for fmt in ("u16", "f32")}
    static = {fmt: tuple(torch.empty_like(t, device=dev) for t in eager[fmt]) for fmt in eager}
    ops.hypersim_preprocess(c, d, e, depth_format="u16")           # (the workspace allocation is warm before capture)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for fmt in static:
            ops.hypersim_preprocess(c, d, e, depth_format=fmt, out=static[fmt])
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for fmt in static:
            ops.hypersim_preprocess(c, d, e, depth_format=fmt, out=static[fmt])
    for fmt in static:
        for t in static[fmt]:
            t.view(torch.uint8).zero_()
    g.replay()
    torch.cuda.synchronize()
    for fmt in static:
        for t, want in zip(static[fmt], eager[fmt]):
            assert torch.equal(t.cpu().view(torch.uint8), want.view(torch.uint8)), fmt
    # the replay reads the inputs as they are at replay time
    c.mul_(0.5)
    e[0, :48] = -1
    g.replay()
    ref = ops.hypersim_preprocess(c, d, e, depth_format="u16")
    torch.cuda.synchronize()
    for t, want in zip(static["u16"], ref):
        assert torch.equal(t.view(torch.uint8), want.view(torch.uint8))


def _batches(loader, seed):
    torch.manual_seed(seed)
    random.seed(seed)
    return [{k: (v.cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in b.items()} for b in loader]


def test_written_tree_and_raw_frames_give_identical_batches(dev, tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts"))
    try:
        import preprocess_hypersim as script
    finally:
        sys.path.pop(0)
    from diffusion_e2e_ft_amd import data
    raw, split, kept = rawfx.make_raw_tree(str(tmp_path), n=3, H=96, W=128)
    columns, by_split = script.read_split(split)

    def load(row):
        pr = data.Hypersim.raw_paths(raw, row["scene_name"], row["camera_name"], row["frame_id"])
        return tuple(rawfx.npy_decoder(pr[k], kind) for k, kind in (("color_path", "color"), ("distance_path", "distance"), ("entity_path", "entity_id")))

    # the reference's step 1 on the GPU: processed/train with its lists; frames 0 / 2 hold float32 distances, frame 1 float16 (separate launches)
    processed = os.path.join(str(tmp_path), "processed")
    assert script.write_split(os.path.join(processed, "train"), "train", by_split["train"], columns, load, batch=4) == 4
    rawfx.copy_normals(raw, processed, kept)
    files = data.Hypersim(processed, split_path=os.path.join(processed, "train", "filename_meta_train.csv"))
    live = data.Hypersim(raw, split_path=split, source="raw", decoder=rawfx.npy_decoder)
    assert len(files) == len(live) == 3
    # what the files hold is the restatement's output
    for k, (row, color, distance, ids, normal) in enumerate(kept):
        want = hpr.preprocess(color, distance, ids)
        smp = files[k]
        assert hpr.check_u8(smp["rgb_u8"], want, "file %d" % k) == 0 and np.array_equal(smp["depth"], want["depth_f32"])
    for bs in (2, 1):                                     # (a batch may mix float16 and float32 distances: staged as float32, which holds both exactly)
        a_ds, b_ds, keep = files, live, (0, 1, 2)
        a = _batches(data.DeviceLoader(a_ds, batch_size=bs, device=dev, workers=2), 5)
        b = _batches(data.DeviceLoader(b_ds, batch_size=bs, device=dev, workers=2), 5)
        assert len(a) == len(b) == (len(keep) + bs - 1) // bs
        for x, y in zip(a, b):
            assert sorted(x) == sorted(y)
            for k in ("rgb", "depth", "metric", "normals", "val_mask"):
                assert torch.equal(x[k], y[k]), k
            assert x["domain"] == y["domain"] == ["indoor"] * x["rgb"].shape[0]
    # the same through finish_samples directly, without a transform
    smp = [files[k] for k in (0, 2)]
    rw = [live[k] for k in (0, 2)]
    st = lambda items, key: torch.from_numpy(np.stack([s[key] for s in items])).to(dev)
    p = data.finish_samples(st(smp, "rgb_u8"), st(smp, "depth"), st(smp, "normal_u8"), "hypersim", transform=False)
    q = data.finish_samples(None, None, st(rw, "normal_u8"), "hypersim", transform=False, raw=(st(rw, "color"), st(rw, "distance"), st(rw, "entity_id")))
    for k in ("rgb", "depth", "metric", "normals", "val_mask"):
        assert torch.equal(p[k], q[k]), k
    # the reference's assertion on ids equal to 0: raised when the loader hands the batch out, and by finish_samples
    raw0, split0, _ = rawfx.make_raw_tree(os.path.join(str(tmp_path), "zero"), n=2, H=96, W=128, zero_id_frame=1)
    bad = data.Hypersim(raw0, split_path=split0, source="raw", decoder=rawfx.npy_decoder)
    with pytest.raises(ValueError, match="render_entity_id == 0"):
        list(data.DeviceLoader(bad, batch_size=1, device=dev, shuffle=False, workers=1))
    s1 = bad[1]
    with pytest.raises(ValueError, match="render_entity_id == 0"):
        data.finish_samples(None, None, st([s1], "normal_u8"), "hypersim", transform=False, raw=(st([s1], "color"), st([s1], "distance"), st([s1], "entity_id")))
