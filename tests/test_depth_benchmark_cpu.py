"""Depth benchmark datasets without a GPU: the fixture generator reproduces the inputs the golden file was recorded from; the numpy restatement of the
decoding / crop / validity rules (tests/benchmark_fixture.py restate) equals what the REFERENCE'S dataset classes returned
(tests/golden/depth_benchmark_golden.pt) bit for bit; naming, filename filtering, tar / directory reading and configuration of eval_data; argument
validation of e2eft_depth_gt_prepare.  (That the new symbol is exported, bound and documented: tests/test_abi.py.)"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import benchmark_fixture as bfx  # noqa: E402

GOLD = torch.load(os.path.join(HERE, "golden", "depth_benchmark_golden.pt"), weights_only=False)
RULES = {"nyu_v2": dict(divisor=1000.0), "scannet": dict(divisor=1000.0), "kitti": dict(divisor=256.0), "eth3d": dict(inf_to_zero=True), "diode": {}}


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("benchmarks"))
    return {name: bfx.make_tree(root, name) for name in bfx.NAMES}


def expected(name, variant, frame, which="raw"):
    """the restatement for one fixture frame -> (depth, mask) as the reference's class with `variant`'s flags should return it"""
    g = GOLD["benchmarks"][name]
    a = frame["arrays"]
    raw = a["filled"] if which == "filled" else a["raw"]
    raw = raw.squeeze()
    kw = dict(RULES[name], min_depth=g["min_depth"], max_depth=g["max_depth"])
    if name == "nyu_v2":
        kw["window"] = bfx.NYU_WINDOW
    if name == "kitti":
        kw["crop"] = bfx.kitti_crop(*raw.shape)
        kw["window"] = bfx.kitti_window({"eigen": "eigen", "garg": "garg", "none": None}[variant], *bfx.KB_CROP)
    if name == "diode":
        kw["ext_mask"] = a["mask"].astype(bool)
    return bfx.restate(raw, **kw)


def check_against_record(rec, which, depth, mask, what):
    """depth float32 [h,w], mask bool [h,w] against one recorded sample (in full, or digests + probes + counts)"""
    dk, mk = "depth_%s_linear" % which, "valid_mask_%s" % which
    if dk in rec:
        assert np.array_equal(depth.view(np.uint32), rec[dk][0].numpy().view(np.uint32)), what
        assert np.array_equal(mask, rec[mk][0].numpy().astype(bool)), what
    else:
        for y, x, bits in rec[dk + "_probes"]:
            assert int(depth[y, x].view(np.uint32)) == bits, (what, y, x)
        for y, x, v in rec[mk + "_probes"]:
            assert int(mask[y, x]) == v, (what, y, x)
        assert bfx.sha256(depth[None]) == rec[dk + "_sha256"], what
        assert bfx.sha256(mask[None].view(np.uint8)) == rec[mk + "_sha256"], what
    assert int(mask.sum()) == rec["n_valid_%s" % which], what


def test_fixture_reproduces_the_recorded_inputs():
    for name in bfx.NAMES:
        assert bfx.input_digests(name) == GOLD["benchmarks"][name]["inputs"], name


def test_boundary_comparisons_of_the_issue():
    # float32(1 / 1000.0) > 1e-3 is False: a raw value of 1 mm is invalid for NYUv2 and ScanNet; raw 10000 (10 m) and KITTI's 20480 (80 m) are invalid
    d, m = bfx.restate(np.array([[0, 1, 2, 9999, 10000]], np.uint16), divisor=1000.0, min_depth=1e-3, max_depth=10)
    assert m.tolist() == [[False, False, True, True, False]]
    d, m = bfx.restate(np.array([[0, 1, 20479, 20480]], np.uint16), divisor=256.0, min_depth=1e-5, max_depth=80)
    assert m.tolist() == [[False, True, True, False]]
    assert bfx.kitti_crop(375, 1242)[:2] == (23, 13) and bfx.kitti_crop(370, 1241)[:2] == (18, 12)
    assert bfx.kitti_window("eigen", 352, 1216) == (117, 321, 43, 1172) and bfx.kitti_window("garg", 352, 1216) == (143, 349, 43, 1172)
    u = np.arange(65536, dtype=np.uint16)
    assert np.array_equal((u / 1000.0).astype(np.float32), u.astype(np.float32) / np.float32(1000.0))


@pytest.mark.parametrize("name", bfx.NAMES)
def test_restatement_equals_the_reference_recordings(name):
    g = GOLD["benchmarks"][name]
    frames = [f for f in bfx.frames(name) if f["arrays"] is not None]
    assert len(frames) == g["length"]
    for variant, recs in g["variants"].items():
        for f, rec in zip(frames, recs):
            assert rec["rgb_relative_path"] == f["line"][0]
            for which in ("raw", "filled"):
                depth, mask = expected(name, variant, f, which if g["has_filled_depth"] else "raw")
                check_against_record(rec, which, depth, mask, (name, variant, f["line"][0], which))
            rgb = f["arrays"]["rgb"]
            if name == "kitti":
                t, l, h, w = bfx.kitti_crop(*rgb.shape[:2])
                rgb = rgb[t:t + h, l:l + w]
            chw = np.ascontiguousarray(rgb.transpose(2, 0, 1))
            if "rgb_int" in rec:
                assert np.array_equal(chw, rec["rgb_int"].numpy())
            else:
                assert bfx.sha256(chw.astype(np.int32)) == rec["rgb_int_sha256"]
    # the planted boundary values decide as the issue states, in the recordings themselves
    if name in ("nyu_v2", "scannet"):
        rec, (y, x) = g["variants"]["default"][-1], ((50, 50) if name == "nyu_v2" else (20, 20))
        assert rec["valid_mask_raw"][0, y, x:x + 6].tolist() == [0, 0, 1, 1, 0, 0]        # raw 0, 1, 2, 9999, 10000, 10001


def test_get_pred_name_matches_the_reference():
    from diffusion_e2e_ft_amd import eval_data
    assert [m.name for m in eval_data.DepthFileNameMode] == list(GOLD["pred_names"])
    for mode in eval_data.DepthFileNameMode:
        for (rgb, suffix), want in GOLD["pred_names"][mode.name].items():
            if want == "IndexError":
                with pytest.raises(IndexError):
                    eval_data.get_pred_name(rgb, mode, suffix=suffix)
            else:
                assert eval_data.get_pred_name(rgb, mode, suffix=suffix) == want, (mode, rgb, suffix)
    assert [(m.name, m.value) for m in eval_data.DatasetMode] == [("RGB_ONLY", "rgb_only"), ("EVAL", "evaluate"), ("TRAIN", "train")]


def _make(name, where, trees, mode=None, **flags):
    from diffusion_e2e_ft_amd import eval_data
    cls = eval_data.dataset_name_class_dict[name]
    return cls(mode=mode or eval_data.DatasetMode.EVAL, filename_ls_path=trees[name]["filenames"], dataset_dir=where, disp_name=name,
               **dict(bfx.FLAGS[name], **flags))


@pytest.mark.parametrize("name", bfx.NAMES)
def test_host_side_reading_tar_and_directory_agree_and_decode_the_fixture(name, trees, monkeypatch):
    from diffusion_e2e_ft_amd import eval_data
    monkeypatch.setattr(eval_data.ETH3DDataset, "HEIGHT", bfx.ETH3D_HW[0])
    monkeypatch.setattr(eval_data.ETH3DDataset, "WIDTH", bfx.ETH3D_HW[1])
    g = GOLD["benchmarks"][name]
    a, b = _make(name, trees[name]["dir"], trees), _make(name, trees[name]["tar"], trees)
    assert not a.is_tar and b.is_tar and len(a) == len(b) == g["length"]
    assert (a.min_depth, float(a.max_depth), a.name_mode.name, a.has_filled_depth) == (g["min_depth"], g["max_depth"], g["name_mode"], g["has_filled_depth"])
    frames = [f for f in bfx.frames(name) if f["arrays"] is not None]
    for i, f in enumerate(frames):
        for ds in (a, b):
            rgb_path, depth_path, filled_path = ds._get_data_path(i)
            assert rgb_path == f["line"][0]
            assert np.array_equal(ds._read_rgb_file(rgb_path), f["arrays"]["rgb"])
            raw = ds._read_raw_depth(depth_path)
            assert raw.dtype == f["arrays"]["raw"].dtype and raw.tobytes() == f["arrays"]["raw"].squeeze().tobytes()
            if g["has_filled_depth"]:
                assert np.array_equal(ds._read_raw_depth(filled_path), f["arrays"]["filled"])
            ext = ds._read_ext_mask(ds.filenames[i])
            assert (ext is None) == (name != "diode")
            if ext is not None:
                assert ext.dtype == np.uint8 and np.array_equal(ext, f["arrays"]["mask"].astype(bool))


def test_kitti_drops_lines_without_ground_truth_and_rejects_small_frames(trees):
    from diffusion_e2e_ft_amd import eval_data
    with open(trees["kitti"]["filenames"]) as f:
        lines = [ln.split() for ln in f]
    assert len(lines) == 3 and lines[2][1] == "None"
    for mode in (eval_data.DatasetMode.EVAL, eval_data.DatasetMode.RGB_ONLY):
        ds = _make("kitti", trees["kitti"]["dir"], trees, mode=mode)
        assert len(ds) == 2 and all(f[1] != "None" for f in ds.filenames)
    assert ds._crop(375, 1242) == (23, 13, 352, 1216) and ds._crop(370, 1241) == (18, 12, 352, 1216)
    assert ds._window(352, 1216) == (117, 321, 43, 1172)
    assert _make("kitti", trees["kitti"]["dir"], trees, valid_mask_crop="garg")._window(352, 1216) == (143, 349, 43, 1172)
    assert _make("kitti", trees["kitti"]["dir"], trees, kitti_bm_crop=False)._crop(100, 100) is None
    with pytest.raises(ValueError, match="smaller than the benchmark crop"):
        ds._crop(351, 1242)
    with pytest.raises(ValueError, match="smaller than the benchmark crop"):
        ds._crop(375, 1215)
    with pytest.raises(ValueError, match="Unknown crop type"):
        _make("kitti", trees["kitti"]["dir"], trees, valid_mask_crop="uhrig")
    with pytest.raises(NotImplementedError):
        _make("kitti", trees["kitti"]["dir"], trees, mode=eval_data.DatasetMode.TRAIN)


def test_get_dataset_from_a_mapping_and_from_yaml(trees, tmp_path):
    from diffusion_e2e_ft_amd import eval_data
    assert sorted(eval_data.BENCHMARKS) == ["data_diode_all", "data_eth3d", "data_kitti_eigen_test", "data_nyu_test", "data_scannet_val"]
    assert {k: v["name"] for k, v in eval_data.BENCHMARKS.items()} == {"data_diode_all": "diode", "data_eth3d": "eth3d", "data_kitti_eigen_test": "kitti",
                                                                      "data_nyu_test": "nyu_v2", "data_scannet_val": "scannet"}
    for key, cfg in eval_data.BENCHMARKS.items():
        assert {k: v for k, v in cfg.items() if k not in ("name", "disp_name", "dir")} == bfx.FLAGS[cfg["name"]], key
        assert cfg["dir"].endswith(".tar") and cfg["disp_name"]
    base = os.path.dirname(trees["kitti"]["dir"])
    cfg = dict(eval_data.BENCHMARKS["data_kitti_eigen_test"], dir="kitti.tar")
    ds = eval_data.get_dataset(cfg, base, eval_data.DatasetMode.EVAL, filenames=trees["kitti"]["filenames"])
    assert isinstance(ds, eval_data.KITTIDataset) and ds.is_tar and len(ds) == 2 and ds.disp_name == "kitti_eigen_test_full"
    assert ds.kitti_bm_crop is True and ds.valid_mask_crop == "eigen" and ds.filename_ls_path == trees["kitti"]["filenames"]
    pytest.importorskip("yaml")
    y = tmp_path / "data_nyu_test.yaml"
    y.write_text("name: nyu_v2\ndisp_name: nyu_test_full\ndir: nyu_v2\nfilenames: %s # list\neigen_valid_mask: true" % trees["nyu_v2"]["filenames"])
    ds = eval_data.get_dataset(str(y), base, eval_data.DatasetMode.RGB_ONLY)
    assert isinstance(ds, eval_data.NYUDataset) and not ds.is_tar and ds.eigen_valid_mask is True and len(ds) == 2
    assert ds._window(480, 640) == bfx.NYU_WINDOW
    with pytest.raises(NotImplementedError):
        eval_data.get_dataset({"name": "sintel", "dir": "x"}, base, eval_data.DatasetMode.EVAL, filenames=trees["kitti"]["filenames"])
    with pytest.raises(ValueError, match="filename list"):
        eval_data.get_dataset(eval_data.BENCHMARKS["data_eth3d"], base, eval_data.DatasetMode.EVAL)


def test_argument_validation_without_gpu():
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    assert ctypes.sizeof(_lib.DepthGtDesc) == 72
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def desc(**kw):
        d = _lib.DepthGtDesc()
        d.batch, d.h0, d.w0, d.raw_dtype, d.divisor = 1, 8, 8, _lib.GT_U16, 1000.0
        d.crop_top, d.crop_left, d.crop_h, d.crop_w = 0, 0, 8, 8
        d.min_depth, d.max_depth = 1e-3, float("inf")
        d.win_y0, d.win_y1, d.win_x0, d.win_x1 = 0, 8, 0, 8
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def rc(d, raw=p, ext=None, depth=p, mask=p):
        return lib.e2eft_depth_gt_prepare(ctypes.byref(d) if d is not None else None, raw, ext, depth, mask, None, None)

    assert rc(None) == 1 and b"null descriptor" in lib.e2eft_last_error()
    for kw in (dict(crop_top=1), dict(crop_left=1), dict(crop_h=9), dict(crop_w=0), dict(crop_top=-1, crop_h=4), dict(crop_left=7, crop_w=2)):
        assert rc(desc(**kw)) == 1 and b"outside" in lib.e2eft_last_error(), kw
    assert rc(desc(raw_dtype=3)) == 1 and b"raw_dtype" in lib.e2eft_last_error()
    assert rc(desc(raw_dtype=-1)) == 1 and b"raw_dtype" in lib.e2eft_last_error()
    assert rc(desc(use_ext_mask=1)) == 1 and b"ext_mask is null" in lib.e2eft_last_error()
    assert rc(desc(divisor=0.0)) == 1 and b"divisor" in lib.e2eft_last_error()
    assert rc(desc(win_y1=9)) == 1 and b"window" in lib.e2eft_last_error()
    assert rc(desc(batch=0)) == 1 and b"shape" in lib.e2eft_last_error()
    assert rc(desc(), raw=None) == 1 and b"null pointer" in lib.e2eft_last_error()
    assert rc(desc(), raw=ctypes.c_void_p(p.value + 1)) == 1 and b"aligned" in lib.e2eft_last_error()


def test_eval_depth_script_help_runs_without_a_gpu():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_depth.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for opt in ("--checkpoint", "--dataset", "--dataset_config", "--base_data_dir", "--filenames", "--output_dir", "--denoise_steps", "--ensemble_size",
                "--processing_res", "--alignment", "--alignment_max_res", "--noise", "--seed", "--half_precision"):
        assert opt in r.stdout, opt
