"""Synthetic stand-ins for the five depth benchmarks (NYUv2, KITTI, ETH3D, ScanNet, DIODE) in the reference's on-disk layout — a directory and a
tar file whose members are "./" + relative path — plus the numpy restatement of what the reference's dataset classes do to a decoded depth raster.
Deterministic (numpy.random.default_rng(seed)); files are written with Pillow and numpy only.  TEST INFRASTRUCTURE: used by
tests/golden/make_depth_benchmark_golden.py (which runs the REFERENCE'S classes over these trees) and by tests/test_depth_benchmark_{cpu,gpu}.py.

Every tree plants the values at which a rule can go wrong: raw 0 and 1 everywhere; raw 10000 and 9999 (NYUv2, ScanNet: 10 m is invalid); raw 20480 and
20479 (KITTI: 80 m is invalid); +inf, -inf and NaN (ETH3D); depth outside [0.6, 350] under a mask of 1 and inside it under a mask of 0 (DIODE); a
valid value on both sides of every edge of every evaluation window."""
import hashlib
import os
import tarfile

import numpy as np

NAMES = ("nyu_v2", "kitti", "eth3d", "scannet", "diode")
ETH3D_HW = (40, 56)           # set as HEIGHT, WIDTH on the ETH3D classes (reference and product) while they read this tree
KB_CROP = (352, 1216)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the rules, restated in numpy ---------------------------------------------------------------------------------------------------------------------
def kitti_crop(H0, W0):
    return int(H0 - KB_CROP[0]), int((W0 - KB_CROP[1]) / 2), KB_CROP[0], KB_CROP[1]


def kitti_window(kind, h, w):
    if kind == "garg":
        return int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w)
    if kind == "eigen":
        return int(0.3324324 * h), int(0.91351351 * h), int(0.0359477 * w), int(0.96405229 * w)
    return None


NYU_WINDOW = (45, 471, 41, 601)


def restate(raw, divisor=1.0, min_depth=0.0, max_depth=float("inf"), crop=None, window=None, inf_to_zero=False, ext_mask=None):
    """-> (depth float32 [h,w], mask bool [h,w]) of one raster [H0,W0] (or a batch [B,H0,W0]): float64 division rounded to float32, +inf -> 0,
    crop, range test in float32 against the float32-rounded bounds, evaluation window with slice semantics; or the external mask alone"""
    raw = np.asarray(raw)
    if raw.dtype == np.float32 and divisor == 1.0:
        d = raw.copy()
    else:
        d = (raw.astype(np.float64) / divisor).astype(np.float32)
    if inf_to_zero:
        d[d == np.inf] = 0.0
    if crop is not None:
        t, l, h, w = crop
        d = d[..., t:t + h, l:l + w]
        if ext_mask is not None:
            ext_mask = ext_mask[..., t:t + h, l:l + w]
    if ext_mask is not None:
        return np.ascontiguousarray(d), np.ascontiguousarray(np.asarray(ext_mask) != 0)
    with np.errstate(invalid="ignore"):
        m = (d > np.float32(min_depth)) & (d < np.float32(max_depth))
    if window is not None:
        y0, y1, x0, x1 = window
        win = np.zeros(d.shape[-2:], bool)
        win[y0:y1, x0:x1] = True
        m = m & win
    return np.ascontiguousarray(d), np.ascontiguousarray(m)


# ---- rasters ---------------------------------------------------------------------------------------------------------------------------------------------
def _plant_edges(a, window, value):
    """a valid value on both sides of each edge of the window (where the frame has them)"""
    H, W = a.shape
    y0, y1, x0, x1 = window
    ym, xm = min(max((y0 + min(y1, H)) // 2, 0), H - 1), min(max((x0 + min(x1, W)) // 2, 0), W - 1)
    for y in (y0 - 1, y0, y1 - 1, y1):
        if 0 <= y < H:
            a[y, xm] = value
    for x in (x0 - 1, x0, x1 - 1, x1):
        if 0 <= x < W:
            a[ym, x] = value
    for y in (y0 - 1, y0, y1 - 1, y1):
        for x in (x0 - 1, x0, x1 - 1, x1):
            if 0 <= y < H and 0 <= x < W:
                a[y, x] = value


def _rgb(rng, H, W):
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _u16(rng, H, W, hi, planted, windows=(), at=(50, 50)):
    a = rng.integers(0, hi, (H, W)).astype(np.uint16)
    for w in windows:
        _plant_edges(a, w, hi // 3)
    flat = a.reshape(-1)
    pos = rng.choice(flat.size, len(planted) * 3, replace=False)
    for k, p in enumerate(pos):
        flat[p] = planted[k % len(planted)]
    a[0, 0], a[-1, -1] = planted[0], planted[-1]
    a[at[0], at[1]:at[1] + len(planted)] = planted             # one copy of each at a known place (inside every window)
    return a


def frames(name, seed=0):
    """-> [dict(files={rel path: array or bytes}, line=[...], arrays={...})] for one benchmark; arrays are what the files decode to"""
    rng = np.random.default_rng([seed, NAMES.index(name)])
    out = []
    if name == "nyu_v2":
        for k, (H, W) in enumerate(((480, 640), (64, 96))):
            d = "test/room_%04d" % k
            rgb, raw, filled = _rgb(rng, H, W), _u16(rng, H, W, 12000, (0, 1, 2, 9999, 10000, 10001), [NYU_WINDOW]), None
            filled = _u16(rng, H, W, 11000, (0, 1, 2, 9999, 10000, 10001), [NYU_WINDOW])
            line = ["%s/rgb_%04d.png" % (d, k), "%s/depth_%04d.png" % (d, k), "%s/filled_%04d.png" % (d, k)]
            out.append({"line": line, "files": dict(zip(line, (rgb, raw, filled))), "arrays": {"rgb": rgb, "raw": raw, "filled": filled}})
    elif name == "scannet":
        for k in range(3):
            d = "scene%04d_00" % (11 + k)
            rgb, raw = _rgb(rng, 48, 64), _u16(rng, 48, 64, 12000, (0, 1, 2, 9999, 10000, 10001), at=(20, 20))
            line = ["%s/color/%06d.png" % (d, 100 * k), "%s/depth/%06d.png" % (d, 100 * k)]
            out.append({"line": line, "files": dict(zip(line, (rgb, raw))), "arrays": {"rgb": rgb, "raw": raw}})
    elif name == "kitti":
        for k, (H, W) in enumerate(((375, 1242), (370, 1241))):
            d = "2011_09_26/2011_09_26_drive_%04d_sync" % (2 + k)
            t, l, h, w = kitti_crop(H, W)
            wins = [tuple(np.add(kitti_window(kind, h, w), (t, t, l, l))) for kind in ("garg", "eigen")] + [(t, t + h, l, l + w)]
            rgb, raw = _rgb(rng, H, W), _u16(rng, H, W, 24000, (0, 1, 2, 20479, 20480, 20481), wins, at=(200, 100))
            raw[rng.random((H, W)) < 0.5] = 0                     # LiDAR ground truth is sparse
            for win in wins:
                _plant_edges(raw, win, 5000)
            raw[200, 100:106] = (0, 1, 2, 20479, 20480, 20481)
            line = ["%s/image_02/data/%010d.png" % (d, 69 + k), "%s/proj_depth/groundtruth/image_02/%010d.png" % (d, 69 + k), "721.5377"]
            out.append({"line": line, "files": dict(zip(line[:2], (rgb, raw))), "arrays": {"rgb": rgb, "raw": raw}})
        out.append({"line": ["2011_09_26/2011_09_26_drive_0009_sync/image_02/data/0000000001.png", "None", "721.5377"], "files": {}, "arrays": None})
    elif name == "eth3d":
        H, W = ETH3D_HW
        for k in range(2):
            rgb = _rgb(rng, H, W)
            raw = (rng.random((H, W)) * 40.0).astype(np.float32)
            raw[rng.random((H, W)) < 0.3] = np.inf                # ETH3D marks missing depth with +inf
            raw[1, 1:6] = [0.0, 1e-5, np.nan, -np.inf, np.float32(1.0000001e-5)]
            raw[0, 0], raw[-1, -1] = np.inf, 7.25
            line = ["rgb/courtyard/DSC_%04d.png" % (286 + k), "depth/courtyard/DSC_%04d.JPG" % (286 + k)]
            out.append({"line": line, "files": {line[0]: rgb, line[1]: raw.tobytes()}, "arrays": {"rgb": rgb, "raw": raw}})
    elif name == "diode":
        for k, part in enumerate(("indoors", "outdoor")):
            d = "%s/scene_%05d/scan_%05d" % (part, 19 + k, 183 + k)
            stem = "%s/%05d_%05d_%s_000_010" % (d, 19 + k, 183 + k, part)
            rgb = _rgb(rng, 48, 64)
            raw = (rng.random((48, 64, 1)) * 400.0).astype(np.float32)
            mask = (rng.random((48, 64)) < 0.7).astype(np.float32)
            raw[2, 2:6, 0], mask[2, 2:6] = [0.1, 351.0, 0.59, 350.0], 1.0      # outside the range, mask 1: valid all the same
            raw[3, 2:6, 0], mask[3, 2:6] = [5.0, 100.0, 0.6, 349.0], 0.0      # inside the range, mask 0: invalid
            line = [stem + ".png", stem + "_depth.npy", stem + "_depth_mask.npy"]
            out.append({"line": line, "files": dict(zip(line, (rgb, raw, mask))), "arrays": {"rgb": rgb, "raw": raw, "mask": mask}})
    else:
        raise KeyError(name)
    return out


# ---- trees -----------------------------------------------------------------------------------------------------------------------------------------------
def _write(path, content):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if isinstance(content, bytes):
        with open(path, "wb") as f:
            f.write(content)
    elif path.endswith(".npy"):
        np.save(path, content)
    else:
        Image.fromarray(content).save(path, format="PNG", compress_level=1)      # uint8 [H,W,3] -> RGB, uint16 [H,W] -> I;16


def make_tree(root, name, seed=0, all_invalid=None):
    """writes <root>/<name>/ (the directory form), <root>/<name>.tar (members "./" + relative path) and <root>/<name>_list.txt -> dict with dir, tar,
    filenames, frames (as frames() returns them).  all_invalid = k: frame k's depth file holds zeros only (scannet)."""
    fr = frames(name, seed)
    if all_invalid is not None:
        raw = np.zeros_like(fr[all_invalid]["arrays"]["raw"])
        fr[all_invalid]["arrays"]["raw"] = raw
        fr[all_invalid]["files"][fr[all_invalid]["line"][1]] = raw
    d = os.path.join(root, name)
    for f in fr:
        for rel, content in f["files"].items():
            _write(os.path.join(d, rel), content)
    tar = os.path.join(root, name + ".tar")
    with tarfile.open(tar, "w") as t:
        for f in fr:
            for rel in f["files"]:
                t.add(os.path.join(d, rel), arcname="./" + rel)
    listing = os.path.join(root, name + "_list.txt")
    with open(listing, "w") as fh:
        fh.write("".join(" ".join(f["line"]) + "\n" for f in fr))
    return {"dir": d, "tar": tar, "filenames": listing, "frames": fr}


def input_digests(name, seed=0):
    """{relative path: sha256 of the decoded array}: what the golden file recorded its inputs as"""
    return {rel: sha256(np.frombuffer(c, np.float32) if isinstance(c, bytes) else c) for f in frames(name, seed) for rel, c in f["files"].items()}


# the constructor flags of each benchmark as the reference's configuration files set them (eval_data.BENCHMARKS holds the same)
FLAGS = {"nyu_v2": {"eigen_valid_mask": True}, "kitti": {"kitti_bm_crop": True, "valid_mask_crop": "eigen"}, "eth3d": {}, "scannet": {}, "diode": {}}
# further flag sets recorded for KITTI: the other evaluation masks on the cropped frame
KITTI_VARIANTS = {"eigen": {"kitti_bm_crop": True, "valid_mask_crop": "eigen"}, "garg": {"kitti_bm_crop": True, "valid_mask_crop": "garg"},
                  "none": {"kitti_bm_crop": True, "valid_mask_crop": None}}
