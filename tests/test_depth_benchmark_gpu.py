"""Depth benchmark datasets on the GPU (csrc/evalprep.hip, eval_data.py, evaluate.evaluate_depth_benchmark): every dataset class over its synthetic
tree against what the REFERENCE'S class returned (tests/golden/depth_benchmark_golden.pt) — depth by its bits, masks, rgb_int and valid counts by
equality, sha256 digests for the KITTI and 480 x 640 frames, directory and tar form alike; the kernel alone against the numpy restatement
(tests/benchmark_fixture.py restate; equal to the recordings: tests/test_depth_benchmark_cpu.py) on ragged shapes, at every load alignment, batched,
without a count and under graph capture; and the evaluation loop with a stand-in pipeline.  All comparisons are exact."""
import csv
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import benchmark_fixture as bfx  # noqa: E402
from test_depth_benchmark_cpu import GOLD, check_against_record  # noqa: E402

NP_DTYPES = {"u16": np.uint16, "i32": np.int32, "f32": np.float32}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("benchmarks"))
    return {name: bfx.make_tree(root, name) for name in bfx.NAMES}


@pytest.fixture(scope="module")
def eth3d_size():
    from diffusion_e2e_ft_amd import eval_data
    old = eval_data.ETH3DDataset.HEIGHT, eval_data.ETH3DDataset.WIDTH
    eval_data.ETH3DDataset.HEIGHT, eval_data.ETH3DDataset.WIDTH = bfx.ETH3D_HW
    yield
    eval_data.ETH3DDataset.HEIGHT, eval_data.ETH3DDataset.WIDTH = old


def _make(name, where, trees, dev, mode=None, **flags):
    from diffusion_e2e_ft_amd import eval_data
    return eval_data.dataset_name_class_dict[name](mode=mode or eval_data.DatasetMode.EVAL, filename_ls_path=trees[name]["filenames"], dataset_dir=where,
                                                   disp_name=name, device=dev, **dict(bfx.FLAGS[name], **flags))


def _check_item(item, rec, dev, what):
    assert sorted(k for k in item if not k.startswith("n_valid")) == rec["keys"], what
    assert item["index"] == rec["index"] and item["rgb_relative_path"] == rec["rgb_relative_path"], what
    rgb = item["rgb_int"]
    assert rgb.dtype == torch.int32 and rgb.device.type == "cuda" and tuple(rgb.shape) == (3,) + tuple(rec["shape"]), what
    if "rgb_int" in rec:
        assert torch.equal(rgb.cpu(), rec["rgb_int"].to(torch.int32)), what
    else:
        assert bfx.sha256(rgb.cpu().numpy()) == rec["rgb_int_sha256"], what
    if "n_valid_raw" not in rec:
        assert "depth_raw_linear" not in item
        return
    for which in ("raw", "filled"):
        d, m, n = item["depth_%s_linear" % which], item["valid_mask_%s" % which], item["n_valid_%s" % which]
        assert d.dtype == torch.float32 and m.dtype == torch.bool and d.device.type == m.device.type == "cuda", what
        assert tuple(d.shape) == tuple(m.shape) == (1,) + tuple(rec["shape"]), what
        check_against_record(rec, which, d[0].cpu().numpy(), m[0].cpu().numpy(), what + (which,))
        assert n.dtype == torch.int32 and int(n) == int(m.sum()) == rec["n_valid_%s" % which], what


@pytest.mark.parametrize("form", ["dir", "tar"])
@pytest.mark.parametrize("name,variant", [(n, "default") for n in bfx.NAMES if n != "kitti"] + [("kitti", v) for v in bfx.KITTI_VARIANTS])
def test_dataset_matches_the_reference_recordings(dev, trees, eth3d_size, name, variant, form):
    from diffusion_e2e_ft_amd import eval_data
    g = GOLD["benchmarks"][name]
    flags = bfx.KITTI_VARIANTS[variant] if name == "kitti" else {}
    ds = _make(name, trees[name][form], trees, dev, **flags)
    assert len(ds) == g["length"] and ds.is_tar == (form == "tar")
    for i, rec in enumerate(g["variants"][variant]):
        _check_item(ds[i], rec, dev, (name, variant, form, i))
    if variant in ("default", "eigen"):
        rgb_only = _make(name, trees[name][form], trees, dev, mode=eval_data.DatasetMode.RGB_ONLY)
        for i, rec in enumerate(g["rgb_only"]):
            _check_item(rgb_only[i], rec, dev, (name, "rgb_only", form, i))


@pytest.mark.parametrize("name", ["scannet", "nyu_v2", "kitti", "diode"])
def test_prepare_batch_equals_the_items(dev, trees, name):
    ds = _make(name, trees[name]["dir"], trees, dev)
    idx = list(range(len(ds)))
    if name in ("nyu_v2", "kitti"):                       # their two frames differ in shape: one launch cannot hold both
        with pytest.raises(ValueError, match="different"):
            ds.prepare_batch(idx)
        idx = [1, 1] if name == "nyu_v2" else [0, 0]
    batch = ds.prepare_batch(idx)
    assert batch["index"] == idx
    for b, i in enumerate(idx):
        item = ds[i]
        assert sorted(item) == sorted(batch)
        for k, v in item.items():
            if isinstance(v, torch.Tensor):
                assert batch[k][b].dtype == v.dtype and batch[k][b].shape == v.shape and batch[k][b].cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), (k, b)
            else:
                assert batch[k][b] == v


# ---- the kernel alone ----------------------------------------------------------------------------------------------------------------------------------
def _raster(rng, kind, shape):
    if kind == "f32":
        a = (rng.random(shape) * 30.0).astype(np.float32)
        flat = a.reshape(-1)
        for k, v in enumerate((np.inf, -np.inf, np.nan, 0.0, 1e-5, -3.5)):
            flat[(k * 7) % flat.size] = v
        return a
    hi = 24000 if kind == "u16" else 3000000
    a = rng.integers(0, hi, shape).astype(NP_DTYPES[kind])
    flat = a.reshape(-1)
    for k, v in enumerate((0, 1, 2, 9999, 10000, 65535 if kind == "u16" else -5)):
        flat[(k * 5) % flat.size] = v
    return a


def _run(raw, dev, ext_mask=None, **kw):
    from diffusion_e2e_ft_amd import ops
    e = None if ext_mask is None else torch.from_numpy(np.ascontiguousarray(ext_mask)).to(dev)
    d, m, n = ops.depth_gt_prepare(torch.from_numpy(np.ascontiguousarray(raw)).to(dev), ext_mask=e, **kw)
    torch.cuda.synchronize()
    return d.cpu().numpy(), m.cpu().numpy(), None if n is None else n.cpu().numpy()


def _check(raw, dev, what, ext_mask=None, **kw):
    d, m, n = _run(raw, dev, ext_mask=ext_mask, **kw)
    rkw = {k: v for k, v in kw.items() if k != "count"}
    if rkw.get("window") is not None:                      # slice semantics of the reference: the wrapper clamps
        rkw["window"] = tuple(rkw["window"])
    wd, wm = bfx.restate(raw, ext_mask=ext_mask, **rkw)
    assert d.shape == wd.shape and m.dtype == np.bool_, what
    assert np.array_equal(d.view(np.uint32), wd.view(np.uint32)), what
    assert np.array_equal(m, wm), what
    if n is not None:
        assert n.dtype == np.int32 and np.array_equal(n.reshape(-1), wm.reshape(n.size, -1).sum(1)), what
    return d, m, n


@pytest.mark.parametrize("kind", ["u16", "i32", "f32"])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (17, 33)])
def test_kernel_on_ragged_shapes(dev, kind, shape):
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    raw = _raster(rng, kind, shape)
    div = 1.0 if kind == "f32" else 1000.0
    _check(raw, dev, (kind, shape, "plain"), divisor=div, min_depth=1e-3, max_depth=10.0, inf_to_zero=kind == "f32")
    _check(raw, dev, (kind, shape, "window"), divisor=div, min_depth=1e-5, max_depth=float("inf"), window=(1, shape[0] - 1, 2, 471))
    _check(raw[None].repeat(2, 0), dev, (kind, shape, "ext"), divisor=div, min_depth=0.6, max_depth=350.0, ext_mask=rng.integers(0, 3, (2,) + shape).astype(np.uint8))
    if shape[0] > 2:
        _check(raw, dev, (kind, shape, "crop"), divisor=256.0, min_depth=1e-5, max_depth=80.0, crop=(1, 1, shape[0] - 2, shape[1] - 2), window=(0, 1, 1, 2))


@pytest.mark.parametrize("kind", ["u16", "i32", "f32"])
def test_kernel_at_every_load_alignment(dev, kind):
    """crop_left 0..7 moves the row's first element through every position of its 16-byte chunk (8 uint16, 4 x 32 bit); the odd raster width moves it
    again from row to row; widths of one chunk and less, and of several waves' worth (more than 64 chunks), with and without the external mask"""
    rng = np.random.default_rng(11)
    raw = _raster(rng, kind, (2, 9, 1241))
    ext = rng.integers(0, 2, raw.shape).astype(np.uint8)
    for left in range(8):
        for w in (1, 3, 8, 9, 530, 1216):
            kw = dict(divisor=256.0, min_depth=1e-5, max_depth=80.0, crop=(2, left, 6, w), window=(1, 5, 0, max(w - 1, 1)))
            _check(raw, dev, (kind, left, w), **kw)
        _check(raw, dev, (kind, left, "ext"), ext_mask=ext, divisor=1.0, crop=(0, left, 9, 1233))


def test_kernel_batch_without_count_and_frame_independence(dev):
    rng = np.random.default_rng(3)
    raw = _raster(rng, "u16", (3, 37, 53))
    raw[1] = 0                                            # a frame without a valid pixel
    kw = dict(divisor=1000.0, min_depth=1e-3, max_depth=10.0, window=(5, 30, 4, 50))
    d, m, n = _check(raw, dev, "batch 3", **kw)
    assert n.tolist()[1] == 0 and n.tolist()[0] > 0
    d2, m2, n2 = _check(raw, dev, "batch 3, no count", count=False, **kw)
    assert n2 is None and np.array_equal(d.view(np.uint32), d2.view(np.uint32)) and np.array_equal(m, m2)
    for b in range(3):
        d1, m1, n1 = _run(raw[b], dev, **kw)
        assert d1.shape == (37, 53) and np.array_equal(d1.view(np.uint32), d[b].view(np.uint32)) and np.array_equal(m1, m[b]) and n1.tolist() == [n[b]]


def test_kernel_rejects_bad_arguments(dev):
    from diffusion_e2e_ft_amd import ops
    raw = torch.zeros((4, 6), dtype=torch.int32, device=dev)
    with pytest.raises(TypeError, match="uint16, int32 or float32"):
        ops.depth_gt_prepare(raw.to(torch.int64))
    with pytest.raises(ValueError, match="outside"):
        ops.depth_gt_prepare(raw, crop=(0, 1, 4, 6))
    with pytest.raises(ValueError, match="does not match"):
        ops.depth_gt_prepare(raw, ext_mask=torch.zeros((4, 5), dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_gt_prepare(raw.cpu())


def test_kernel_under_graph_capture_on_a_side_stream(dev):
    from diffusion_e2e_ft_amd import ops
    rng = np.random.default_rng(77)
    raw_np = _raster(rng, "u16", (3, 40, 131))
    raw = torch.from_numpy(raw_np).to(dev)
    kw = dict(divisor=256.0, min_depth=1e-5, max_depth=80.0, crop=(3, 5, 30, 120), window=(2, 28, 3, 117))
    static = (torch.empty((3, 30, 120), dtype=torch.float32, device=dev), torch.empty((3, 30, 120), dtype=torch.uint8, device=dev),
              torch.empty((3,), dtype=torch.int32, device=dev))
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        ops.depth_gt_prepare(raw, out=static, **kw)        # warm, on the side stream
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ops.depth_gt_prepare(raw, out=static, **kw)
    for t in static:
        t.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    wd, wm = bfx.restate(raw_np, **kw)
    assert np.array_equal(static[0].cpu().numpy().view(np.uint32), wd.view(np.uint32)) and np.array_equal(static[1].cpu().numpy(), wm.astype(np.uint8))
    assert static[2].tolist() == wm.reshape(3, -1).sum(1).tolist()
    raw[1] = 0                                            # the replay reads the inputs as they are at replay time, and the count starts from zero again
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    raw_np[1] = 0
    wd, wm = bfx.restate(raw_np, **kw)
    assert np.array_equal(static[1].cpu().numpy(), wm.astype(np.uint8)) and static[2].tolist() == wm.reshape(3, -1).sum(1).tolist() and static[2].tolist()[1] == 0


# ---- the evaluation loop ---------------------------------------------------------------------------------------------------------------------------------
class StandInPipe:
    """depth_np is a fixed function of the image: no model needed"""

    def __init__(self):
        self.calls = []

    def __call__(self, image, **kw):
        self.calls.append(kw)
        a = np.asarray(image).astype(np.float32)
        H, W = a.shape[:2]
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        pred = (a[..., 0] * 0.5 + a[..., 1] * 0.3 + a[..., 2] * 0.2) / 255.0 * 0.6 + 0.3 * yy / H + 0.1 * xx / W
        return type("Out", (), {"depth_np": pred.astype(np.float32)})()


def _read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


@pytest.mark.parametrize("name,alignment,max_res", [("scannet", "least_square", None), ("scannet", "least_square_disparity", None), ("scannet", "least_square", 32),
                                                     ("diode", "least_square", None), ("eth3d", "least_square", None)])
def test_runner_matches_metrics_on_the_recorded_ground_truth(dev, trees, eth3d_size, tmp_path, name, alignment, max_res):
    from diffusion_e2e_ft_amd import eval_data, evaluate
    g = GOLD["benchmarks"][name]
    ds = _make(name, trees[name]["tar"], trees, dev)
    pipe = StandInPipe()
    out = str(tmp_path / "out")
    res = evaluate.evaluate_depth_benchmark(pipe, ds, alignment=alignment, alignment_max_res=max_res, output_dir=out, save_predictions=True, ensemble_size=1)
    assert pipe.calls == [{"ensemble_size": 1}] * len(ds)
    header, rows = _read_csv(os.path.join(out, "per_sample_metrics.csv"))
    assert header == ["filename"] + list(evaluate.METRIC_NAMES) and len(rows) == len(ds) == g["length"]
    tracker = evaluate.MetricTracker(*evaluate.METRIC_NAMES)
    for row, rec in zip(rows, g["variants"]["default"]):
        rgb_name = rec["rgb_relative_path"]
        pred_name = os.path.join(os.path.dirname(rgb_name), eval_data.get_pred_name(os.path.basename(rgb_name), ds.name_mode, suffix=".npy"))
        assert row[0] == pred_name
        rgb = rec["rgb_int"].permute(1, 2, 0).numpy()
        pred = StandInPipe()(rgb).depth_np
        saved = np.load(os.path.join(out, pred_name))
        assert saved.dtype == np.float32 and np.array_equal(saved, pred)
        m = evaluate.depth_metrics(torch.from_numpy(pred).to(dev), rec["depth_raw_linear"][0].to(dev), rec["valid_mask_raw"][0].to(dev).bool(), alignment=alignment,
                                   min_depth=g["min_depth"], max_depth=g["max_depth"], alignment_max_res=max_res)
        for k, cell in zip(evaluate.METRIC_NAMES, row[1:]):
            want = float(m[k][0])
            assert np.float64(cell).tobytes() == np.float64(want).tobytes(), (name, rgb_name, k, cell, want)
            tracker.update(k, want)
    assert res == tracker.result() and list(res) == list(evaluate.METRIC_NAMES)
    text = open(os.path.join(out, "eval_metrics-%s.txt" % alignment)).read()
    lines = text.split("\n")
    assert lines[0] == "Evaluation metrics:" and lines[1] == "    of predictions: " + out and lines[2] == "    on dataset: " + name
    assert lines[3] == "    with samples in: " + trees[name]["filenames"]
    assert lines[4] == "min_depth = %s" % ds.min_depth and lines[5] == "max_depth = %s" % ds.max_depth
    table = "\n".join(lines[6:])
    for k, v in res.items():
        assert k in table and (str(v) in table or ("%g" % v) in table or ("%.6g" % v) in table), (k, v, table)
    assert sorted(os.listdir(out)) == sorted(["per_sample_metrics.csv", "eval_metrics-%s.txt" % alignment] + sorted({r[0].split(os.sep)[0] for r in rows}))


def test_runner_skips_and_names_a_sample_without_valid_pixels(dev, tmp_path):
    from diffusion_e2e_ft_amd import eval_data, evaluate
    tree = bfx.make_tree(str(tmp_path), "scannet", all_invalid=1)
    ds = eval_data.ScanNetDataset(mode=eval_data.DatasetMode.EVAL, filename_ls_path=tree["filenames"], dataset_dir=tree["dir"], disp_name="scannet", device=dev)
    assert [int(ds[i]["n_valid_raw"]) > 0 for i in range(3)] == [True, False, True]
    out = str(tmp_path / "out")
    with pytest.warns(UserWarning, match="scene0012_00/color/000100.png has no valid"):
        res = evaluate.evaluate_depth_benchmark(StandInPipe(), ds, output_dir=out)
    header, rows = _read_csv(os.path.join(out, "per_sample_metrics.csv"))
    assert [r[0] for r in rows] == ["scene0011_00/color/pred_000000.npy", "scene0013_00/color/pred_000200.npy"]
    assert not os.path.exists(os.path.join(out, "scene0011_00"))          # predictions are written only on request
    assert "of predictions: (in memory)" in open(os.path.join(out, "eval_metrics-least_square.txt")).read()
    for j, k in enumerate(evaluate.METRIC_NAMES):
        vals = [float(r[1 + j]) for r in rows]
        assert np.isfinite(vals).all() and res[k] == (vals[0] + vals[1]) / 2
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)                    # nothing is skipped on the plain tree, and no files are written without an output_dir
        plain = bfx.make_tree(str(tmp_path / "plain"), "scannet")
        ds2 = eval_data.ScanNetDataset(mode=eval_data.DatasetMode.EVAL, filename_ls_path=plain["filenames"], dataset_dir=plain["dir"], disp_name="scannet", device=dev)
        res2 = evaluate.evaluate_depth_benchmark(StandInPipe(), ds2)
    assert list(res2) == list(evaluate.METRIC_NAMES)
    with pytest.raises(ValueError, match="EVAL"):
        evaluate.evaluate_depth_benchmark(StandInPipe(), eval_data.ScanNetDataset(mode=eval_data.DatasetMode.RGB_ONLY, filename_ls_path=plain["filenames"],
                                                                                  dataset_dir=plain["dir"], disp_name="scannet", device=dev))
