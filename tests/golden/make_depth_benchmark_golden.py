"""Generate tests/golden/depth_benchmark_golden.pt : what the REFERENCE'S evaluation dataset classes (Marigold/src/dataset/*.py, imported and run
from source in the reference tree) return for the synthetic benchmark trees of tests/benchmark_fixture.py, in EVAL and RGB_ONLY mode, from the
directory and from the tar form (asserted equal here).  Run from the repo root: `python tests/golden/make_depth_benchmark_golden.py`.

Per benchmark and sample: rgb_int, depth_raw_linear, depth_filled_linear, valid_mask_raw, valid_mask_filled — small frames in full (rgb as uint8,
masks as uint8), the KITTI and 480 x 640 frames as sha256 digests plus valid counts and a few probed pixels (the arrangement of
hypersim_prep_golden.pt) —, the dataset's min / max depth, its length, get_pred_name for all four naming modes, and the digests of the decoded inputs.
KITTI is recorded for valid_mask_crop eigen / garg / None.  The file holds data only.

torchvision is not installed: tests/stubs stands in (appended to sys.path, so a real package wins); the stub lacks the Resize class that
base_depth_dataset.py imports for its training mode, which is never run here — a placeholder is set for the import.

Trust rule of tests/golden/reference_manifest.json: third-party source is executed only when its sha256 is the one that was reviewed (recorded
below); E2EFT_TRUST_REFERENCE=1 runs a changed file anyway, after you have looked at the diff."""
import hashlib
import importlib
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import benchmark_fixture as bfx  # noqa: E402

REF = os.environ.get("E2EFT_REFERENCE", "/root/reference")
REF_DIR = os.path.join(REF, "Marigold", "src", "dataset")
REF_SHA256 = {"__init__.py": "a64f1fe05f84ad893c04f36bcdb6253fc93e6ace2fb851b6b75c2f76bfaecb2b",
              "base_depth_dataset.py": "0340fee3b9a645397847a03d7d8fc15051b2af3b4c98b3ecbf074d69d97fa85b",
              "diode_dataset.py": "9f3d96cf2750561d648f02facb57c06b6f52e533cc32d2dc8f57fbbf4b5d9669",
              "eth3d_dataset.py": "25ea17e7010a29502436c7a09ca98d9563c45652e88da2e8132cb6af43c51e30",
              "kitti_dataset.py": "04933ef7375e1bf43bd3579f7cc5c81fd4337a58c3577ec5dc771579dadc5e1f",
              "nyu_dataset.py": "e5b2af0978c7574ce050ff1c87613acc5895d0ade9d0d96e9b6e6e42b226c8b5",
              "scannet_dataset.py": "012ef251808ad3d31337d9a72fc61222897936d75b63dc960a2d1d4fe9dffaee"}
FULL_LIMIT = 64 * 96          # frames up to this many pixels are stored in full
PROBES = 24
RASTERS = ("depth_raw_linear", "depth_filled_linear", "valid_mask_raw", "valid_mask_filled")
PRED_NAME_CASES = ("rgb_0001.png", "rgb_01_02.png", "0000000069.png", "00019_00183_indoors_000_010.png", "1_2_3_rgb.png", "DSC_0286.JPG")


def check_trust():
    for f, want in REF_SHA256.items():
        with open(os.path.join(REF_DIR, f), "rb") as fh:
            h = hashlib.sha256(fh.read()).hexdigest()
        if h != want and os.environ.get("E2EFT_TRUST_REFERENCE") != "1":
            raise RuntimeError("%s changed (sha256 %s, reviewed %s): look at the diff, then set E2EFT_TRUST_REFERENCE=1" % (f, h, want))


def load_reference():
    check_trust()
    saved = list(sys.path)
    sys.path.insert(0, os.path.join(REF, "Marigold"))
    sys.path.append(os.path.join(TESTS, "stubs"))
    try:
        tvt = importlib.import_module("torchvision.transforms")
        if not hasattr(tvt, "Resize"):
            tvt.Resize = type("Resize", (), {})
        return importlib.import_module("src.dataset")
    finally:
        sys.path[:] = saved


def ref_class(ref, name):
    return ref.dataset_name_class_dict[name]


def _record(item):
    """one sample of the reference -> what the golden file keeps of it"""
    rgb = item["rgb_int"]
    assert rgb.dtype == torch.int32 and int(rgb.min()) >= 0 and int(rgb.max()) <= 255
    rec = {"rgb_relative_path": item["rgb_relative_path"], "index": item["index"], "keys": sorted(item), "shape": tuple(rgb.shape[-2:])}
    small = rgb.shape[-2] * rgb.shape[-1] <= FULL_LIMIT
    if small:
        rec["rgb_int"] = rgb.to(torch.uint8)
    else:
        rec["rgb_int_sha256"] = bfx.sha256(rgb.numpy())
    if "depth_raw_linear" not in item:
        return rec
    H, W = item["depth_raw_linear"].shape[-2:]
    rng = np.random.default_rng(H * 10007 + W)
    probes = [(int(y), int(x)) for y, x in zip(rng.integers(0, H, PROBES), rng.integers(0, W, PROBES))] + [(0, 0), (H - 1, W - 1)]
    for k in RASTERS:
        t = item[k]
        assert tuple(t.shape) == (1, H, W) and t.dtype == (torch.bool if "mask" in k else torch.float32), (k, t.shape, t.dtype)
        if small:
            rec[k] = t.to(torch.uint8) if t.dtype == torch.bool else t.clone()
        else:
            a = t.numpy()
            rec[k + "_sha256"] = bfx.sha256(a.view(np.uint8) if a.dtype == np.bool_ else a)
            rec[k + "_probes"] = [(y, x, int(a[0, y, x]) if a.dtype == np.bool_ else int(a[0, y, x].view(np.uint32))) for y, x in probes]
    rec["n_valid_raw"], rec["n_valid_filled"] = int(item["valid_mask_raw"].sum()), int(item["valid_mask_filled"].sum())
    return rec


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].numpy().tobytes() == b[k].numpy().tobytes(), k
        else:
            assert a[k] == b[k], k


def run_reference(ref, name, tree, flags, mode):
    """the reference's class over the directory and over the tar file (must agree) -> [item]"""
    cls = ref_class(ref, name)
    out = []
    for where in (tree["dir"], tree["tar"]):
        ds = cls(mode=mode, filename_ls_path=tree["filenames"], dataset_dir=where, disp_name=name + "_synthetic", **flags)
        out.append((ds, [ds[i] for i in range(len(ds))]))
    for a, b in zip(out[0][1], out[1][1]):
        _same(a, b)
    return out[0]


def make():
    ref = load_reference()
    base = importlib.import_module("src.dataset.base_depth_dataset")
    out = {"sha256": dict(REF_SHA256), "benchmarks": {}, "pred_names": {}}
    for mode in base.DepthFileNameMode:
        out["pred_names"][mode.name] = {}
        for rgb in PRED_NAME_CASES:
            for suffix in (".png", ".npy"):
                try:
                    out["pred_names"][mode.name][(rgb, suffix)] = base.get_pred_name(rgb, mode, suffix=suffix)
                except IndexError:
                    out["pred_names"][mode.name][(rgb, suffix)] = "IndexError"
    eth = ref_class(ref, "eth3d")
    eth.HEIGHT, eth.WIDTH = bfx.ETH3D_HW
    with tempfile.TemporaryDirectory() as tmp:
        for name in bfx.NAMES:
            tree = bfx.make_tree(tmp, name)
            variants = bfx.KITTI_VARIANTS if name == "kitti" else {"default": bfx.FLAGS[name]}
            rec = {"inputs": bfx.input_digests(name), "variants": {}}
            for vname, flags in variants.items():
                ds, items = run_reference(ref, name, tree, flags, base.DatasetMode.EVAL)
                rec["variants"][vname] = [_record(it) for it in items]
                rec.update(min_depth=float(ds.min_depth), max_depth=float(ds.max_depth), length=len(ds), name_mode=ds.name_mode.name,
                           has_filled_depth=bool(ds.has_filled_depth))
            ds, items = run_reference(ref, name, tree, bfx.FLAGS[name], base.DatasetMode.RGB_ONLY)
            rec["rgb_only"] = [_record(it) for it in items]
            out["benchmarks"][name] = rec
    return out


if __name__ == "__main__":
    g = make()
    path = os.path.join(HERE, "depth_benchmark_golden.pt")
    torch.save(g, path)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: (v["length"], sorted(v["variants"])) for k, v in g["benchmarks"].items()})
