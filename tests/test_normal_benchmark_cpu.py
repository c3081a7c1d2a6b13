"""Surface-normal benchmarks without a GPU (diffusion_e2e_ft_amd/normal_eval_data.py, evaluate.evaluate_normal_benchmark's text, scripts/eval_normals.py):
the OpenEXR reader against the fixture's own writer, bit for bit; split parsing and the error messages; NORMAL_BENCHMARKS against test.py's list; the
metrics.txt text; args-file parsing; and the 768-entry (channel, byte) table of the image round trip, stated in numpy, against what the REFERENCE'S
test.py:59-65 produced (tests/golden/normal_benchmark_golden.pt, tests/golden/make_normal_benchmark_golden.py) — byte for byte.  The kernel restates
the same table (tests/test_normal_benchmark_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import normal_benchmark_fixture as nfx  # noqa: E402

GOLD = torch.load(os.path.join(HERE, "golden", "normal_benchmark_golden.pt"))


def requantize_table(img):
    """uint8 [H,W,3] -> uint8 [H,W,3]: test.py:59-65 after Normalize as a function of (channel, byte).  f(c, v) = (float32(v) / 255 - mean_c) / std_c in
    fp32 is monotone in v, so the tensor's minimum / maximum are the least f(c, lo_c) / the greatest f(c, hi_c); the range is the float64 difference
    rounded to fp32 (the Python double that divides the fp32 tensor)."""
    mean = np.array([0.485, 0.456, 0.406], dtype=np.float32)
    std = np.array([0.229, 0.224, 0.225], dtype=np.float32)
    v = np.arange(256, dtype=np.float32)
    f = (v[None, :] / np.float32(255.0) - mean[:, None]) / std[:, None]                      # [3,256] fp32
    assert f.dtype == np.float32
    lo, hi = img.reshape(-1, 3).min(0), img.reshape(-1, 3).max(0)
    mn = min(f[c, lo[c]] for c in range(3))
    mx = max(f[c, hi[c]] for c in range(3))
    rng = np.float32(float(mx) - float(mn))
    if rng == 0:
        return np.zeros_like(img)
    table = (((f - mn) / rng) * np.float32(255.0))
    assert table.dtype == np.float32
    table = np.clip(table, 0, 255).astype(np.uint8)                                           # entries outside [lo_c, hi_c] are never read
    return np.stack([table[c][img[..., c]] for c in range(3)], axis=2)


def test_numpy_table_equals_the_reference_round_trip():
    kinds = set()
    for name in nfx.NAMES:
        for i, rec in enumerate(GOLD["datasets"][name]["samples"]):
            img = nfx.image(name, i)
            want = rec["img_u8"].permute(1, 2, 0).numpy()
            got = requantize_table(img)
            assert got.shape == want.shape and int((got != want).sum()) == 0, (name, i)
            assert int((want != img).sum()) > 0, "the round trip is not the identity"
            kinds.add((int(img.min()), int(img.max())))
    assert (37, 181) in kinds and (0, 255) in kinds and (10, 200) in kinds
    one = requantize_table(np.full((2, 3, 3), 91, dtype=np.uint8))                           # one byte value still spreads over three normalised ones
    assert len(set(one.reshape(-1).tolist())) == 3 and int(one.min()) == 0 and int(one.max()) == 255


def test_golden_holds_what_the_fixture_describes():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_normal_benchmark_golden as mk              # importable: the generator's shims are installed only when it runs
    finally:
        sys.path.pop(0)
    assert GOLD["sha256"] == mk.REF_SHA256 and tuple(GOLD["names"]) == mk.NAMES
    for name in nfx.NAMES:
        g = GOLD["datasets"][name]
        assert len(g["samples"]) == len(nfx.SAMPLES[name]) and g["n"] == int(g["errors"].numel()) == sum(int(s["normal_mask"].sum()) for s in g["samples"])
        for i, (rec, (scene, stem, (H, W), opt)) in enumerate(zip(g["samples"], nfx.SAMPLES[name])):
            assert tuple(rec["img_u8"].shape) == tuple(rec["normal"].shape) == (3, H, W) and tuple(rec["normal_mask"].shape) == (1, H, W)
            assert rec["scene_name"] == scene and rec["img_name"] == stem
            assert rec["keys"] == sorted(["img", "normal", "normal_mask", "intrins", "dataset_name", "scene_name", "img_name", "info", "flipped"])
            assert np.array_equal(rec["intrins"].numpy(), nfx.intrins(name, i))
            if opt is None:                                                                  # rule 2 in numpy
                raw = nfx.normal_png(name, i)
                want = (raw.astype(np.float32) / np.float32(255.0)) * np.float32(2.0) - np.float32(1.0)
                assert np.array_equal(rec["normal"].numpy().view(np.uint32), want.transpose(2, 0, 1).view(np.uint32))
                assert np.array_equal(rec["normal_mask"].numpy()[0], (raw.astype(np.int64).sum(2) > 0).astype(np.uint8))
                assert (raw.reshape(-1, 3).sum(1) == 0).any() and (raw.reshape(-1, 3).sum(1) == 1).any()
            else:                                                                            # rule 3: the values as stored, NaN payloads included
                raw = nfx.normal_exr(name, i)
                assert np.array_equal(rec["normal"].numpy().view(np.uint32), np.ascontiguousarray(raw.transpose(2, 0, 1)).view(np.uint32))
                with np.errstate(invalid="ignore"):
                    want = np.sqrt((raw[..., 0] * raw[..., 0] + raw[..., 1] * raw[..., 1]) + raw[..., 2] * raw[..., 2]) > np.float32(0.5)
                assert np.array_equal(rec["normal_mask"].numpy()[0], want.astype(np.uint8))
                assert np.isnan(raw).any() and not rec["normal_mask"].numpy()[0][np.isnan(raw).any(2)].any()


# ---- the OpenEXR reader -----------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("compression", ["NONE", "ZIPS", "ZIP"])
@pytest.mark.parametrize("pixel", ["HALF", "FLOAT"])
@pytest.mark.parametrize("origin,alpha", [((0, 0), False), ((-7, 5), False), ((0, 0), True), ((11, -3), True)])
def test_read_exr_returns_the_written_array_bit_for_bit(compression, pixel, origin, alpha):
    from diffusion_e2e_ft_amd.normal_eval_data import read_exr
    for name, i in (("sintel", 3), ("ibims", 2), ("sintel", 2)):                              # 20 x 33 (two ZIP blocks), 3 x 341, 9 x 1
        src = nfx.normal_exr(name, i)
        if pixel == "HALF":
            with np.errstate(over="ignore"):
                src = src.astype(np.float16).astype(np.float32)
        got = read_exr(nfx.write_exr(src, compression=compression, pixel=pixel, origin=origin, alpha=alpha))
        assert got.dtype == np.float32 and got.shape == src.shape and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(_bits(got), _bits(src)), (name, i)
        assert np.isnan(src).any()


def test_read_exr_reads_a_block_stored_raw_and_the_tree_files(tmp_path):
    from diffusion_e2e_ft_amd.normal_eval_data import read_exr
    noise = np.random.default_rng(5).integers(0, 2 ** 32, (4, 9, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)   # does not compress: stored raw
    data = nfx.write_exr(noise, compression="ZIP", pixel="FLOAT")
    assert len(data) > noise.nbytes
    assert np.array_equal(_bits(read_exr(data)), _bits(noise))
    for name in ("ibims", "sintel"):
        tree = nfx.make_tree(str(tmp_path), name)
        for i, (scene, stem, _, _) in enumerate(nfx.SAMPLES[name]):
            with open(os.path.join(tree["dir"], scene, stem + "_normal.exr"), "rb") as f:
                assert np.array_equal(_bits(read_exr(f.read())), _bits(nfx.normal_exr(name, i)))


def test_read_exr_refuses_what_it_does_not_read():
    from diffusion_e2e_ft_amd.normal_eval_data import read_exr
    ok = nfx.write_exr(nfx.normal_exr("sintel", 0))
    with pytest.raises(NotImplementedError, match="PIZ"):
        read_exr(nfx.declare_compression(ok, 4))
    with pytest.raises(NotImplementedError, match="DWAA"):
        read_exr(nfx.declare_compression(ok, 8))
    with pytest.raises(NotImplementedError, match="tiled"):
        read_exr(nfx.declare_tiled(ok))
    with pytest.raises(ValueError, match="not an OpenEXR"):
        read_exr(b"\x89PNG\r\n\x1a\n" + bytes(16))


# ---- the dataset class, host side ---------------------------------------------------------------------------------------------------------------------------
def test_split_parsing_names_and_paths(tmp_path):
    from diffusion_e2e_ft_amd import normal_eval_data as nd
    tree = nfx.make_tree(str(tmp_path), "ibims")
    ds = nd.NormalBenchmarkDataset("ibims", tree["dir"], tree["split"])
    assert len(ds) == 3 and ds.filenames == tree["filenames"] and ds.domain == "indoor" and ds.split == "ibims"
    from_list = nd.NormalBenchmarkDataset("ibims", tree["dir"], ["ibims/corridor_01_img.png\n", "", "  ibims/kitchen_01_img.png"])
    assert from_list.filenames == ["ibims/corridor_01_img.png", "ibims/kitchen_01_img.png"]
    scene, stem, img, normal, intr = ds.paths(2)
    assert (scene, stem) == ("ibims", "kitchen_01") and img == tree["dir"] + "/ibims/kitchen_01_img.png"
    assert normal == tree["dir"] + "/ibims/kitchen_01_normal.exr" and intr == tree["dir"] + "/ibims/kitchen_01_intrins.npy"
    assert nd.NormalBenchmarkDataset("nyuv2", "/x", ["test/000000_img.png"]).paths(0)[3] == "/x/test/000000_normal.png"
    with pytest.raises(ValueError, match="scene/name_img.ext"):
        nd.NormalBenchmarkDataset("ibims", tree["dir"], ["corridor_01_img.png"])
    with pytest.raises(FileNotFoundError, match="nowhere.txt"):
        nd.NormalBenchmarkDataset("ibims", tree["dir"], str(tmp_path / "nowhere.txt"))


def test_error_messages(tmp_path):
    from diffusion_e2e_ft_amd import normal_eval_data as nd
    for bad in ("oasis", "vkitti", "nyu_v2"):
        with pytest.raises(ValueError, match="nyuv2, scannet, ibims, sintel"):
            nd.NormalBenchmarkDataset(bad, str(tmp_path), [])
    tree = nfx.make_tree(str(tmp_path), "scannet")
    ds = nd.NormalBenchmarkDataset("scannet", tree["dir"], tree["filenames"] + ["scene0009_00/000000_img.png"])
    with pytest.raises(FileNotFoundError, match="scene0009_00/000000_img.png"):
        ds[3]
    os.remove(os.path.join(tree["dir"], "scene0001_00", "000100_normal.png"))
    with pytest.raises(FileNotFoundError, match="000100_normal.png"):
        ds[1]
    with pytest.raises(ValueError, match="different image shapes"):
        ds.prepare_batch([0, 2])
    with pytest.raises(ValueError, match="no index"):
        ds.prepare_batch([])
    with pytest.raises(IndexError):
        ds[7]


def test_benchmark_table_is_the_reference_list():
    from diffusion_e2e_ft_amd import normal_eval_data as nd
    assert [(k, v["split"]) for k, v in nd.NORMAL_BENCHMARKS.items()] == [("nyuv2", "test"), ("scannet", "test"), ("ibims", "ibims"), ("sintel", "sintel")]   # test.py:214-217
    assert {k: v["domain"] for k, v in nd.NORMAL_BENCHMARKS.items()} == {"nyuv2": "indoor", "scannet": "indoor", "ibims": "indoor", "sintel": "outdoor"}     # :47-51
    assert {k: v["normal_ext"] for k, v in nd.NORMAL_BENCHMARKS.items()} == {"nyuv2": ".png", "scannet": ".png", "ibims": ".exr", "sintel": ".exr"}
    assert tuple(nd.NORMAL_BENCHMARKS) == nfx.NAMES and {k: v["split"] for k, v in nd.NORMAL_BENCHMARKS.items()} == nfx.SPLITS


def test_metrics_text():
    from diffusion_e2e_ft_amd import evaluate
    m = {"mean": 16.123456, "median": 7.5, "rmse": 24.0004, "a1": 35.25, "a2": 50.0, "a3": 62.9996, "a4": 80.0, "a5": 85.1, "n": 12}
    assert evaluate.normal_metrics_text(m, 654) == ("Normal Estimation Metrics:\nMetrics at iteration 654\nmean median rmse 5 7.5 11.25 22.5 30\n"
                                                    "16.123 7.500 24.000 35.250 50.000 63.000 80.000 85.100\n")


# ---- the script's args file -----------------------------------------------------------------------------------------------------------------------------------
def _script():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "scripts"))
    try:
        import eval_normals
    finally:
        sys.path.pop(0)
    return eval_normals


def test_args_file_parsing(tmp_path):
    en = _script()
    p = tmp_path / "geowizard_e2e_ft.txt"
    p.write_text("--exp_name GeoWizard\n--exp_id GeoWizard-E2E-FT\n--ckpt_path ckpt/geowizard-e2e-ft\n--model_type geowizard\n--eval_data all\n--processing_res 0\n--seed 1234\n")
    cfg, ignored = en.parse_args_file(str(p))
    assert ignored == ["exp_name", "exp_id"]
    assert cfg == dict(en.DEFAULTS, ckpt_path="ckpt/geowizard-e2e-ft", model_type="geowizard", eval_data="all", processing_res=0, seed=1234)
    assert en.benchmarks_of(cfg["eval_data"]) == ["nyuv2", "scannet", "ibims", "sintel"] and en.benchmarks_of("sintel") == ["sintel"]
    kw = en.pipe_kwargs_of(cfg)
    assert kw == dict(denoising_steps=1, ensemble_size=1, processing_res=0, match_input_res=True, show_progress_bar=False, noise="zeros", color_map="Spectral")
    q = tmp_path / "m.txt"
    q.write_text("--model_type marigold --denoise_steps 2\n\n--ensemble_size 3\n--noise gaussian\n--domain outdoor\n--visualize\n--eval_data ibims\n")
    cfg, ignored = en.parse_args_file(str(q))
    assert ignored == ["visualize"] and (cfg["denoise_steps"], cfg["ensemble_size"], cfg["noise"], cfg["domain"], cfg["eval_data"], cfg["seed"]) == (2, 3, "gaussian", "outdoor", "ibims", None)
    assert en.pipe_kwargs_of(cfg) == dict(denoising_steps=2, ensemble_size=3, processing_res=0, match_input_res=True, show_progress_bar=False, noise="gaussian",
                                          color_map=None, resample_method="bilinear", batch_size=0, normals=True)
    q.write_text("--eval_data oasis\n")
    with pytest.raises(ValueError, match="eval_data oasis"):
        en.parse_args_file(str(q))
    q.write_text("--seed\n")
    with pytest.raises(ValueError, match="needs a value"):
        en.parse_args_file(str(q))
    a = en.parse([str(p), "--base_data_dir", "data", "--split_dir", "splits", "--output_dir", "out"])
    assert (a.args_file, a.base_data_dir, a.split_dir, a.output_dir, a.ckpt_path) == (str(p), "data", "splits", "out", None)
