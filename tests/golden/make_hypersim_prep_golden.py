"""Generate tests/golden/hypersim_prep_golden.pt : the REFERENCE'S Hypersim preprocessing
(Marigold/script/dataset_preprocess/hypersim/preprocess_hypersim.py and hypersim_util.py, executed in place from the reference tree).
Run from the repo root: `python tests/golden/make_hypersim_prep_golden.py`.

  small cases   the reference's own tone_map and dist_2_depth (both take any H x W) on the frames of CASES; the script's glue between them
                (preprocess_hypersim.py:83-88,92,98-104,118-119,126-138) is restated in run_reference with the line numbers cited, the loader's
                read-back (training/dataloaders/load.py:220-222) likewise.
  full frame    the reference's WHOLE script through runpy on one 768 x 1024 frame, over stand-ins for h5py, cv2 and tqdm that exist only while it
                runs (neither is installed; pandas and pylab are real): h5py.File serves the frame's arrays, cv2.imwrite records what would be
                written.  Kept as sha256 digests of the two written arrays + the CSV row; the test rebuilds the inputs from the stored palettes by
                integer gathers (hypersim_prep_ref.full_frame).
The generator asserts that no float64 `out * 255` of the fixture lies within 1e-9 of an integer (apart from exact 0 and the clipped 255): the
condition under which a device pow that differs from this host's in the last place still truncates to the same uint8.

Trust rule of tests/golden/reference_manifest.json: third-party source is executed only when its sha256 is the one that was reviewed (recorded
below); E2EFT_TRUST_REFERENCE=1 runs a changed file anyway, after you have looked at the diff."""
import contextlib
import csv
import hashlib
import importlib.util
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import hypersim_prep_ref as hpr  # noqa: E402

REF_DIR = os.path.join(os.environ.get("E2EFT_REFERENCE", "/root/reference"), "Marigold", "script", "dataset_preprocess", "hypersim")
REF_SHA256 = {"preprocess_hypersim.py": "6431a2cf9c8f95e23ea0444c8fd86f5c6b5d1b80b4f930e79db1529c0813de61",
              "hypersim_util.py": "b3cb968e7a27c6a1f23ae9b36cd56f763f19699cb5549341bb9723fab6c96c08"}
MARGIN = 1e-9
NAN, F16, F32 = float("nan"), np.float16, np.float32


def sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def reference_available():
    return all(os.path.exists(os.path.join(REF_DIR, f)) for f in REF_SHA256)


def check_trust():
    shas = {f: sha256(os.path.join(REF_DIR, f)) for f in REF_SHA256}
    for f, h in shas.items():
        if h != REF_SHA256[f] and os.environ.get("E2EFT_TRUST_REFERENCE") != "1":
            raise RuntimeError("%s changed (sha256 %s, reviewed %s): look at the diff, then set E2EFT_TRUST_REFERENCE=1" % (f, h, REF_SHA256[f]))
    return shas


def load_util():
    check_trust()
    spec = importlib.util.spec_from_file_location("hypersim_util_reference", os.path.join(REF_DIR, "hypersim_util.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the small cases -------------------------------------------------------------------------------------------------------------------------------
def _frame(seed, H, W, cdt, ddt, invalid=0.1, gain=1.0, negative=False):
    rng = np.random.default_rng(seed)
    color = (rng.random((H, W, 3)) ** 2 * 3.0 * gain)
    if negative:
        color = rng.normal(0.2, 0.5, (H, W, 3))
    dist = 0.5 + rng.random((H, W)) * 12.0
    ids = rng.integers(1, 200, (H, W)).astype(np.int32)
    ids[rng.random((H, W)) < invalid] = -1
    return color.astype(cdt), dist.astype(ddt), ids


def build_cases():
    """-> [(name, color, distance, ids)]: the smallest frames at which each step can go wrong"""
    cases = []
    c, d, i = _frame(1, 1, 1, F32, F32, invalid=0.0)
    cases.append(("1x1", c, d, i))
    c, d, i = _frame(2, 2, 2, F16, F16, invalid=0.0)
    cases.append(("2x2 f16", c, d, i))
    c, d, i = _frame(3, 37, 53, F16, F16)
    i[5, 7], i[20, 30], i[20, 31], i[36, 52], i[0, 0] = 3, 4, 5, 6, 7
    d[5, 7] = NAN                                    # a NaN distance on a valid pixel
    d[20, 30], d[20, 31], d[36, 52] = 70.0, 1000.0, 65504.0      # beyond 65.535 m: the uint16 wraps
    cases.append(("ragged 37x53 f16, NaN and far distances", c, d, i))
    c, d, i = _frame(4, 37, 53, F32, F32)
    i[9, 9], i[10, 10] = 8, 9
    d[9, 9], d[10, 10] = NAN, 131.5
    cases.append(("ragged 37x53 f32", c, d, i))
    c, d, i = _frame(5, 5, 7, F32, F16)
    i[:] = -1
    cases.append(("every pixel invalid (scale 1)", c, d, i))
    c, d, i = _frame(6, 6, 5, F32, F32, gain=1e-5)
    cases.append(("percentile below 1e-4 (scale 0)", c, d, i))
    c, d, i = _frame(7, 4, 4, F16, F32)
    i[:] = -1
    i[2, 1] = 17
    cases.append(("exactly one valid pixel", c, d, i))
    c, d, i = _frame(8, 3, 7, F32, F32, invalid=0.0)
    cases.append(("n - 1 = 20: weight 0", c, d, i))
    c, d, i = _frame(9, 2, 3, F32, F32, invalid=0.0)
    cases.append(("n - 1 = 5: weight 0.5, second lerp branch", c, d, i))
    c, d, i = _frame(10, 4, 9, F16, F16, invalid=0.0)
    cases.append(("n - 1 = 35: weight 0.5 on f16", c, d, i))
    rng = np.random.default_rng(11)
    c = rng.integers(1, 5, (16, 24, 3)).astype(F16) * F16(0.25)
    _, d, i = _frame(11, 16, 24, F16, F16)
    cases.append(("heavy ties: 4 levels per channel, f16", c, d, i))
    c = np.zeros((8, 10, 3), F16)
    c[:, :9] = F16(0.5)
    c[:, 9:] = F16(2.0)                               # 72 dark, 8 bright, all valid: rank 71 ends the dark run, rank 72 starts the bright one
    _, d, i = _frame(12, 8, 10, F16, F16, invalid=0.0)
    cases.append(("two runs: the ranks straddle the boundary", c, d, i))
    c, d, i = _frame(13, 9, 11, F32, F32, negative=True)
    cases.append(("negative colour components", c, d, i))
    c, d, i = _frame(14, 4, 6, F32, F32, invalid=0.0)
    d[0, :] = [2.0e6, 3.0e6, 7.0e7, -2.0e6, -3.0e6, -0.75]      # millimetres on both sides of the int32 range (2.147e9), and a small negative distance
    d[1, :3] = [float("inf"), float("-inf"), 2147.0e3]
    cases.append(("distances around the int32 range of millimetres, negative and infinite", c, d, i))
    return cases


def run_reference(util, color, distance, ids):
    """one frame as preprocess_hypersim.py treats it, around the reference's two functions"""
    H, W = ids.shape
    rgb = np.array(color).astype(float)                                            # :84
    dist_from_center = np.array(distance).astype(float)                            # :86
    render_entity_id = np.array(ids).astype(int)                                   # :88
    with np.errstate(all="ignore"):
        rgb_color_tm = util.tone_map(rgb, render_entity_id)                        # :91
        rgb_int = (rgb_color_tm * 255).astype(np.uint8)                            # :92
        plane_depth = util.dist_2_depth(W, H, hpr.FOCAL, dist_from_center)         # :95-97 (IMG_WIDTH, IMG_HEIGHT = the frame's)
        valid_mask = render_entity_id != -1                                        # :98
        invalid_ratio = (np.prod(valid_mask.shape) - valid_mask.sum()) / np.prod(valid_mask.shape)      # :101-103
        plane_depth[~valid_mask] = 0                                               # :104
        plane_depth *= 1000.0                                                      # :118
        plane_depth = plane_depth.astype(np.uint16)                                # :119
    restored_depth = plane_depth / 1000.0                                          # :132
    rec = {"invalid_ratio": invalid_ratio, "rgb_mean": np.mean(rgb_int), "rgb_std": np.std(rgb_int), "rgb_min": np.min(rgb_int), "rgb_max": np.max(rgb_int),
           "depth_mean": np.mean(restored_depth), "depth_std": np.std(restored_depth), "depth_min": np.min(restored_depth),
           "depth_max": np.max(restored_depth)}                                    # :126-138
    depth_f32 = (plane_depth / 1000).astype(np.float32)                            # load.py:220-222 (np.array(Image.open(p)) / 1000 as a float32 image)
    return rgb_int, plane_depth, depth_f32, {k: float(v) for k, v in rec.items()}, rgb_color_tm * 255


def assert_margin(out255, what):
    x = out255[~np.isnan(out255)]
    x = x[(x != 0.0) & (x != 255.0)]
    gap = np.abs(x - np.rint(x))
    assert gap.size == 0 or gap.min() > MARGIN, "%s: out * 255 within %g of an integer (%g)" % (what, MARGIN, gap.min())
    return float(gap.min()) if gap.size else float("inf")


# ---- the full frame through the reference's whole script ------------------------------------------------------------------------------------------------
def full_frame_palettes():
    rng = np.random.default_rng(20)
    return (rng.random((4096, 3)) ** 2 * 4.0).astype(F16), (0.4 + rng.random(4096) * 30.0).astype(F16)


@contextlib.contextmanager
def _standins(arrays, written):
    class File:
        def __init__(self, path, mode="r"):
            kind = os.path.basename(path).split(".")[2]                             # frame.0000.<kind>.hdf5
            self.d = {"dataset": arrays[kind]}

        def __enter__(self):
            return self.d

        def __exit__(self, *a):
            return False

    h5py, cv2, tqdm = types.ModuleType("h5py"), types.ModuleType("cv2"), types.ModuleType("tqdm")
    h5py.File = File
    cv2.COLOR_RGB2BGR = 4
    cv2.cvtColor = lambda a, code: a[..., ::-1]
    cv2.imwrite = lambda path, a: written.__setitem__(os.path.basename(path), np.array(a)) or True
    tqdm.tqdm = lambda it, **k: it
    saved = {k: sys.modules.get(k) for k in ("h5py", "cv2", "tqdm", "hypersim_util")}
    argv, path = sys.argv, list(sys.path)
    sys.modules.update({"h5py": h5py, "cv2": cv2, "tqdm": tqdm})
    sys.modules.pop("hypersim_util", None)
    sys.path.insert(0, REF_DIR)
    try:
        yield
    finally:
        sys.argv, sys.path[:] = argv, path
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def run_script(color, distance, ids):
    """the reference's script end to end on one frame -> (rgb uint8 [H,W,3], depth uint16 [H,W], the CSV row as strings, filename_list line)"""
    check_trust()
    assert ids.shape == (768, 1024)                  # the script's IMG_HEIGHT, IMG_WIDTH
    scene, cam, frame = "ai_001_001", "cam_00", 7
    written = {}
    with tempfile.TemporaryDirectory() as tmp:
        raw, outdir, split = os.path.join(tmp, "raw"), os.path.join(tmp, "processed"), os.path.join(tmp, "split.csv")
        for sub, kind in (("final_hdf5", "color"), ("geometry_hdf5", "depth_meters"), ("geometry_hdf5", "render_entity_id")):
            d = os.path.join(raw, scene, "images", "scene_%s_%s" % (cam, sub))
            os.makedirs(d, exist_ok=True)
            open(os.path.join(d, "frame.%04d.%s.hdf5" % (frame, kind)), "wb").close()       # the script asserts the files exist; h5py.File is the stand-in
        with open(split, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["scene_name", "camera_name", "frame_id", "included_in_public_release", "exclude_reason", "split_partition_name"])
            for part in ("train", "val", "test"):      # (pandas' apply over an EMPTY split fails in the script's list writer: one row each, the same frame)
                w.writerow([scene, cam, frame, "True", "", part])
        with _standins({"color": color, "depth_meters": distance, "render_entity_id": ids}, written):
            sys.argv = ["preprocess_hypersim.py", "--split_csv", split, "--dataset_dir", raw, "--output_dir", outdir]
            with np.errstate(all="ignore"), contextlib.redirect_stdout(open(os.devnull, "w")):
                runpy.run_path(os.path.join(REF_DIR, "preprocess_hypersim.py"), run_name="__main__")
        with open(os.path.join(outdir, "train", "filename_meta_train.csv"), newline="") as f:
            rows = list(csv.DictReader(f))
        with open(os.path.join(outdir, "train", "filename_list_train.txt")) as f:
            listing = f.read()
    assert len(rows) == 1 and sorted(written) == ["depth_plane_cam_00_fr0007.png", "rgb_cam_00_fr0007.png"], (len(rows), sorted(written))
    return written["rgb_cam_00_fr0007.png"][..., ::-1], written["depth_plane_cam_00_fr0007.png"], rows[0], listing


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make(full=True):
    util = load_util()
    out = {"sha256": check_trust(), "cases": [], "margin": MARGIN}
    t = torch.from_numpy
    for name, color, distance, ids in build_cases():
        rgb_int, u16, depth_f32, rec, out255 = run_reference(util, color, distance, ids)
        gap = assert_margin(out255, name)
        mine = hpr.preprocess(color, distance, ids)
        assert np.array_equal(mine["rgb_u8"], rgb_int) and np.array_equal(mine["u16"], u16), "restatement != reference (%s)" % name
        out["cases"].append({"name": name, "color": t(color), "distance": t(distance), "ids": t(ids), "rgb_u8": t(rgb_int), "u16": t(u16.astype(np.int32)),
                             "depth_f32": t(depth_f32), "record": rec, "min_gap": gap})
    if full:
        cp, dp = full_frame_palettes()
        color, distance, ids = hpr.full_frame(cp, dp)
        rgb, u16, row, listing = run_script(color, distance, ids)
        mine = hpr.preprocess(color, distance, ids)
        gap = assert_margin(mine["out255"], "full frame")
        assert np.array_equal(mine["rgb_u8"], rgb) and np.array_equal(mine["u16"], u16), "restatement != reference (full frame)"
        out["full"] = {"color_palette": t(cp), "distance_palette": t(dp), "rgb_sha256": digest(rgb), "u16_sha256": digest(u16),
                       "depth_f32_sha256": digest((u16 / 1000).astype(np.float32)), "csv_row": dict(row), "filename_list": listing, "min_gap": gap}
    return out


if __name__ == "__main__":
    g = make()
    path = os.path.join(HERE, "hypersim_prep_golden.pt")
    torch.save(g, path)
    print("wrote", path, os.path.getsize(path), "bytes;", g["sha256"], "min gap", min(c["min_gap"] for c in g["cases"]), g["full"]["min_gap"])
