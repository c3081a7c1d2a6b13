"""Surface-normal benchmarks on the GPU (csrc/normalprep.hip, normal_eval_data.py, evaluate.evaluate_normal_benchmark) against what the REFERENCE'S
benchmark mode made of the same synthetic trees (tests/golden/normal_benchmark_golden.pt): normals by their bits (int32 views, so NaN payloads
count), masks, counts and the re-quantised image by equality — the allowed number of differing elements is 0 everywhere; a captured graph of both
kernels replayed on changed inputs; the evaluation loop with a stand-in pipeline (both normal_np layouts) within the bars
tests/test_normal_eval_gpu.py applies to the same eight quantities, and with the product MarigoldPipeline at 40 x 56 and 36 x 52 (36 = 4 mod 8,
Sintel's case at processing_res = 0)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import normal_benchmark_fixture as nfx  # noqa: E402
from test_normal_benchmark_cpu import GOLD, requantize_table  # noqa: E402
from test_normal_eval_gpu import _check_against_reference  # noqa: E402


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dsine_eval"))
    return {name: nfx.make_tree(root, name) for name in nfx.NAMES}


def _raw_normal(name, i):
    return nfx.normal_png(name, i) if nfx.SAMPLES[name][i][3] is None else nfx.normal_exr(name, i)


def _same_bits(t, want):
    """device tensor against a CPU tensor / array of the same dtype: 0 differing elements, compared as integers"""
    a = t.detach().cpu().contiguous().numpy()
    b = want.contiguous().numpy() if isinstance(want, torch.Tensor) else np.ascontiguousarray(want)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    view = {4: np.int32, 1: np.uint8}[a.dtype.itemsize]
    return int((a.view(view) != b.view(view)).sum()) == 0


@pytest.mark.parametrize("name", nfx.NAMES)
def test_normal_gt_prepare_matches_the_reference(dev, name):
    from diffusion_e2e_ft_amd import ops
    recs = GOLD["datasets"][name]["samples"]
    for i, rec in enumerate(recs):
        raw = torch.from_numpy(_raw_normal(name, i)).to(dev)
        normal, mask, nv = ops.normal_gt_prepare(raw)
        assert normal.dtype == torch.float32 and mask.dtype == torch.bool and nv.dtype == torch.int32
        assert _same_bits(normal, rec["normal"]), (name, i)
        assert _same_bits(mask.view(torch.uint8), rec["normal_mask"]), (name, i)
        assert int(nv) == int(rec["normal_mask"].sum()) == int(mask.sum()), (name, i)
    # the two frames of one shape in one launch, then again into the same tensors, and a frame at an odd byte offset (a view that starts mid-buffer)
    both = torch.from_numpy(np.stack([_raw_normal(name, 0), _raw_normal(name, 1)])).to(dev)
    out = ops.normal_gt_prepare(both)
    want_n, want_m = torch.stack([recs[0]["normal"], recs[1]["normal"]]), torch.stack([recs[0]["normal_mask"], recs[1]["normal_mask"]])
    assert _same_bits(out[0], want_n) and _same_bits(out[1].view(torch.uint8), want_m) and out[2].tolist() == [int(r["normal_mask"].sum()) for r in recs[:2]]
    static = (torch.full_like(out[0], 7.0), torch.full_like(out[1].view(torch.uint8), 7), torch.full_like(out[2], 7))
    again = ops.normal_gt_prepare(both, out=static)
    assert again[0].data_ptr() == static[0].data_ptr() and _same_bits(static[0], want_n) and _same_bits(static[1], want_m) and static[2].tolist() == out[2].tolist()
    flat = torch.zeros(both[1].numel() + 8, dtype=both.dtype, device=dev)
    shifted = flat[1:1 + both[1].numel()].view(both[1].shape)
    shifted.copy_(both[1])
    n1, m1, c1 = ops.normal_gt_prepare(shifted)
    assert _same_bits(n1, recs[1]["normal"]) and _same_bits(m1.view(torch.uint8), recs[1]["normal_mask"]) and int(c1) == int(recs[1]["normal_mask"].sum())


@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_dsine_rgb_requantize_matches_the_reference(dev, layout):
    from diffusion_e2e_ft_amd import ops
    for name in nfx.NAMES:
        recs = GOLD["datasets"][name]["samples"]
        for i, rec in enumerate(recs):
            got = ops.dsine_rgb_requantize(torch.from_numpy(nfx.image(name, i)).to(dev), layout=layout)
            want = rec["img_u8"] if layout == "chw" else rec["img_u8"].permute(1, 2, 0).contiguous()
            assert got.dtype == torch.uint8 and _same_bits(got, want), (name, i, layout)
        both = torch.from_numpy(np.stack([nfx.image(name, 0), nfx.image(name, 1)])).to(dev)          # frames 2 x 258 x 6 bytes: the second starts off 16
        want = torch.stack([recs[0]["img_u8"], recs[1]["img_u8"]])
        want = want if layout == "chw" else want.permute(0, 2, 3, 1).contiguous()
        got = ops.dsine_rgb_requantize(both, layout=layout)
        assert _same_bits(got, want), (name, layout)
        static = torch.full_like(got, 9)
        assert ops.dsine_rgb_requantize(both, layout=layout, out=static).data_ptr() == static.data_ptr() and _same_bits(static, want)
    # a frame large enough for several blocks and lanes with more than one group, against the numpy table (equal to the reference: the CPU tests)
    rng = np.random.default_rng(41)
    big = rng.integers(3, 250, (2, 97, 331, 3)).astype(np.uint8)
    big[1] = big[1] // 3 + 60
    got = ops.dsine_rgb_requantize(torch.from_numpy(big).to(dev), layout=layout)
    want = np.stack([requantize_table(big[0]), requantize_table(big[1])])
    assert _same_bits(got, want if layout == "hwc" else want.transpose(0, 3, 1, 2))
    # one single normalised value does not exist for three channels of one byte; zeros are written only when max == min, which no uint8 image reaches
    with pytest.raises(TypeError, match="uint8"):
        ops.dsine_rgb_requantize(torch.zeros((4, 4, 3), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="layout"):
        ops.dsine_rgb_requantize(torch.zeros((4, 4, 3), dtype=torch.uint8, device=dev), layout="nchw")
    with pytest.raises(ValueError, match=r"\[H,W,3\]"):
        ops.normal_gt_prepare(torch.zeros((4, 4), dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError, match="uint8 or float32"):
        ops.normal_gt_prepare(torch.zeros((4, 4, 3), dtype=torch.float16, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.normal_gt_prepare(torch.zeros((4, 4, 3), dtype=torch.uint8))


def _check_item(item, rec, name, i):
    assert sorted(item) == sorted(["img_u8", "normal", "normal_mask", "n_valid", "intrins", "dataset_name", "scene_name", "img_name", "index"])
    assert (item["dataset_name"], item["scene_name"], item["img_name"], item["index"]) == (name, rec["scene_name"], rec["img_name"], i)
    assert all(item[k].device.type == "cuda" for k in ("img_u8", "normal", "normal_mask", "n_valid", "intrins"))
    assert item["normal_mask"].dtype == torch.bool and item["intrins"].dtype == torch.float32 and tuple(item["intrins"].shape) == (3, 3)
    assert _same_bits(item["img_u8"], rec["img_u8"]), (name, i, "img_u8")
    assert _same_bits(item["normal"], rec["normal"]), (name, i, "normal")
    assert _same_bits(item["normal_mask"].view(torch.uint8), rec["normal_mask"]), (name, i, "normal_mask")
    assert _same_bits(item["intrins"], rec["intrins"]) and int(item["n_valid"]) == int(rec["normal_mask"].sum()), (name, i)


@pytest.mark.parametrize("name", nfx.NAMES)
def test_dataset_matches_the_reference_recordings(dev, trees, name):
    from diffusion_e2e_ft_amd import normal_eval_data as nd
    ds = nd.NormalBenchmarkDataset(name, trees[name]["dir"], trees[name]["split"], device=dev)
    recs = GOLD["datasets"][name]["samples"]
    assert len(ds) == len(recs)
    items = [ds[i] for i in range(len(ds))]
    for i, (item, rec) in enumerate(zip(items, recs)):
        _check_item(item, rec, name, i)
    batch = ds.prepare_batch([0, 1])
    assert batch["index"] == [0, 1] and sorted(batch) == sorted(items[0])
    for b in range(2):
        for k, v in items[b].items():
            if isinstance(v, torch.Tensor):
                assert batch[k][b].dtype == v.dtype and batch[k][b].shape == v.shape and batch[k][b].cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), (k, b)
            else:
                assert batch[k][b] == v, (k, b)
    keep = {k: batch[k].clone() for k in ("img_u8", "normal", "normal_mask", "n_valid")}
    for k in keep:
        batch[k].view(torch.uint8).fill_(5) if batch[k].dtype == torch.bool else batch[k].fill_(5)
    again = ds.prepare_batch([0, 1], out=batch)                      # a second call into the pre-allocated tensors: the same bytes, no new storage
    for k, v in keep.items():
        assert again[k].data_ptr() == batch[k].data_ptr() and again[k].cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), k
    with pytest.raises(ValueError, match="different image shapes"):
        ds.prepare_batch([0, 2])
    if name == "sintel":                                             # a user's decoder is called with the file's bytes
        seen = []

        def decoder(data):
            seen.append(len(data))
            return nd.read_exr(data)

        _check_item(nd.NormalBenchmarkDataset(name, trees[name]["dir"], trees[name]["split"], device=dev, exr_decoder=decoder)[3], recs[3], name, 3)
        assert len(seen) == 1 and seen[0] > 0


def test_both_kernels_replay_from_one_captured_graph(dev):
    """one capture of normal_gt_prepare followed by dsine_rgb_requantize, replayed twice with different contents in the same input buffers"""
    from diffusion_e2e_ft_amd import ops
    rng = np.random.default_rng(8)

    def contents(k):
        gt = rng.standard_normal((2, 6, 86, 3)).astype(np.float32) * np.float32(0.4 + 0.2 * k)
        gt[0, 0, 0] = (np.nan, 0, 0)
        img = rng.integers(20 * k, 200 + 20 * k, (2, 6, 86, 3)).astype(np.uint8)
        return gt, img

    def eager(gt, img):
        n, m, c = ops.normal_gt_prepare(torch.from_numpy(gt).to(dev))
        return n.clone(), m.clone(), c.clone(), ops.dsine_rgb_requantize(torch.from_numpy(img).to(dev), layout="chw").clone()

    gt0, img0 = contents(0)
    gt_buf, img_buf = torch.from_numpy(gt0).to(dev), torch.from_numpy(img0).to(dev)
    static = (torch.empty((2, 3, 6, 86), dtype=torch.float32, device=dev), torch.empty((2, 1, 6, 86), dtype=torch.uint8, device=dev),
              torch.empty((2,), dtype=torch.int32, device=dev))
    out_img = torch.empty((2, 3, 6, 86), dtype=torch.uint8, device=dev)
    ws = torch.empty((12,), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):                                       # warm, on the side stream
        ops.normal_gt_prepare(gt_buf, out=static)
        ops.dsine_rgb_requantize(img_buf, layout="chw", out=out_img, workspace=ws)
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ops.normal_gt_prepare(gt_buf, out=static)
        ops.dsine_rgb_requantize(img_buf, layout="chw", out=out_img, workspace=ws)
    for k in (1, 2):
        gt, img = contents(k)
        gt_buf.copy_(torch.from_numpy(gt))
        img_buf.copy_(torch.from_numpy(img))
        for t in static + (out_img,):
            t.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        n, m, c, q = eager(gt, img)
        assert _same_bits(static[0], n.cpu()) and _same_bits(static[1], m.view(torch.uint8).cpu()) and static[2].tolist() == c.tolist(), k
        assert _same_bits(out_img, q.cpu()), k
        assert _same_bits(q, np.stack([requantize_table(img[0]), requantize_table(img[1])]).transpose(0, 3, 1, 2)), k


# ---- the evaluation loop --------------------------------------------------------------------------------------------------------------------------------------
class StubPipe:
    """normal_np is nfx.stub_normals of the PIL image it is given: no model needed"""

    def __init__(self, hwc):
        self.hwc, self.images, self.calls = hwc, [], []

    def __call__(self, image, **kw):
        from PIL import Image
        assert isinstance(image, Image.Image)
        a = np.asarray(image)
        self.images.append(a)
        self.calls.append(kw)
        n = nfx.stub_normals(a)
        return type("Out", (), {"normal_np": np.ascontiguousarray(n.transpose(1, 2, 0)) if self.hwc else n})()


@pytest.mark.parametrize("hwc", [False, True])
@pytest.mark.parametrize("name", nfx.NAMES)
def test_runner_with_a_stand_in_pipeline(dev, trees, tmp_path, name, hwc):
    from diffusion_e2e_ft_amd import evaluate, normal_eval_data as nd
    g = GOLD["datasets"][name]
    ds = nd.NormalBenchmarkDataset(name, trees[name]["dir"], trees[name]["split"], device=dev)
    pipe = StubPipe(hwc)
    out = str(tmp_path / "out")
    res = evaluate.evaluate_normal_benchmark(pipe, ds, output_dir=out, domain="object", ensemble_size=1)
    assert pipe.calls == [{"ensemble_size": 1}] * len(ds)               # `domain` goes to a DepthNormalEstimationPipeline only
    for a, rec in zip(pipe.images, g["samples"]):
        assert a.dtype == np.uint8 and np.array_equal(a, rec["img_u8"].permute(1, 2, 0).numpy())
    for k, w in zip(evaluate.NORMAL_METRIC_NAMES, g["metrics"].tolist()):
        print(name, hwc, k, res[k], w)
    _check_against_reference(res, None, g["errors"], g["metrics"], g["n"], (name, hwc))
    text = open(os.path.join(out, "test", name, "metrics.txt")).read()
    assert text == evaluate.normal_metrics_text(res, len(ds))
    lines = text.split("\n")
    assert lines[0] == "Normal Estimation Metrics:" and lines[1] == "Metrics at iteration %d" % len(ds) and lines[2] == "mean median rmse 5 7.5 11.25 22.5 30"
    assert lines[3] == "%.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f" % tuple(res[k] for k in evaluate.NORMAL_METRIC_NAMES) and lines[4:] == [""]


def test_runner_refuses_a_wrong_shape_and_warns_without_valid_pixels(dev, trees, tmp_path):
    from diffusion_e2e_ft_amd import evaluate, normal_eval_data as nd
    ds = nd.NormalBenchmarkDataset("scannet", trees["scannet"]["dir"], trees["scannet"]["filenames"][:1], device=dev)
    with pytest.raises(ValueError, match=r"scannet/scene0001_00/000000: prediction \(3, 4, 7\)"):
        evaluate.evaluate_normal_benchmark(lambda image, **kw: type("Out", (), {"normal_np": np.zeros((3, 4, 7), np.float32)})(), ds)

    class Blank(nd.NormalBenchmarkDataset):
        def _read_normal(self, path):
            return np.zeros_like(super()._read_normal(path))

    with pytest.warns(UserWarning, match="no valid ground-truth pixel in scannet"):
        assert evaluate.evaluate_normal_benchmark(StubPipe(False), Blank("scannet", trees["scannet"]["dir"], trees["scannet"]["split"], device=dev),
                                                  output_dir=str(tmp_path)) is None
    assert not os.path.exists(str(tmp_path / "test"))


def _product_tree(root):
    """a two-image tree at 40 x 56 and one image at 36 x 52 (36 = 4 mod 8: Sintel's 436 rows), EXR ground truth"""
    from PIL import Image
    base = os.path.join(root, "dsine_eval", "sintel", "scene")
    os.makedirs(base)
    rng = np.random.default_rng(3)
    names = []
    for stem, (H, W) in (("a", (40, 56)), ("b", (40, 56)), ("c", (36, 52))):
        Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(os.path.join(base, stem + "_img.png"))
        n = rng.standard_normal((H, W, 3)).astype(np.float32)
        n /= np.linalg.norm(n, axis=2, keepdims=True)
        n[::5, ::3] = 0
        with open(os.path.join(base, stem + "_normal.exr"), "wb") as f:
            f.write(nfx.write_exr(n, compression="ZIP", pixel="FLOAT"))
        np.save(os.path.join(base, stem + "_intrins.npy"), np.eye(3, dtype=np.float32))
        names.append("scene/%s_img.png" % stem)
    return os.path.dirname(base), names


def test_runner_with_the_product_pipeline(dev, tmp_path):
    from diffusion_e2e_ft_amd import evaluate, normal_eval_data as nd
    from diffusion_e2e_ft_amd.pipeline import MarigoldPipeline
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    from oracle import config, synth, unet_ref, vae_ref
    unet = UNet2DConditionModel(**config.TINY_UNET)
    unet.load_state_dict(synth.synth_state_dict(unet_ref.unet_param_shapes(config.TINY_UNET), seed=1234))
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(synth.synth_state_dict(vae_ref.vae_param_shapes(config.TINY_VAE), seed=4321))
    pipe = MarigoldPipeline(unet.to(dev).eval(), vae.to(dev).eval(), DDIMScheduler())
    pipe.empty_text_embed = synth.synth_inputs(1, 64, 64, 2, 128, seed=11)[1].to(dev)
    d, names = _product_tree(str(tmp_path))
    ds = nd.NormalBenchmarkDataset("sintel", d, names, device=dev)
    preds = []

    def recording(image, **kw):
        out = pipe(image, **kw)
        preds.append(out.normal_np)
        return out

    kw = dict(denoising_steps=1, ensemble_size=1, processing_res=0, match_input_res=True, batch_size=1, color_map=None, show_progress_bar=False,
              noise="zeros", normals=True)
    res = evaluate.evaluate_normal_benchmark(recording, ds, output_dir=str(tmp_path / "out"), **kw)
    assert [p.shape for p in preds] == [(3, 40, 56), (3, 40, 56), (3, 36, 52)]
    assert all(np.isfinite(res[k]) for k in evaluate.NORMAL_METRIC_NAMES) and res["n"] == sum(int(ds[i]["n_valid"]) for i in range(3)) > 0
    acc = evaluate.NormalMetricAccumulator()
    for i, p in enumerate(preds):
        item = ds[i]
        acc.update(torch.from_numpy(p).to(dev), item["normal"], item["normal_mask"])
    assert acc.result() == res
    assert evaluate.evaluate_normal_benchmark(pipe, ds, **kw) == res                       # the pipeline itself, not the recording wrapper
    assert open(str(tmp_path / "out" / "test" / "sintel" / "metrics.txt")).read() == evaluate.normal_metrics_text(res, 3)
