"""Synthetic stand-ins for the four surface-normal benchmarks (NYUv2, ScanNet, iBims-1, Sintel) in the layout of DSINE's evaluation tree
(<root>/dsine_eval/<dataset>/<scene>/<name>_img.png, _normal.png | _normal.exr, _intrins.npy) with split files laid out as
<root>/splits/<dataset>/split/<split>.txt.  Deterministic (numpy.random.default_rng(seed)); files are written with Pillow, numpy and a minimal
OpenEXR WRITER of its own, which shares no code with the reader under test (diffusion_e2e_ft_amd.normal_eval_data.read_exr).  TEST INFRASTRUCTURE: used
by tests/golden/make_normal_benchmark_golden.py (which runs the REFERENCE'S loaders over these trees) and tests/test_normal_benchmark_{cpu,gpu}.py.

The shapes are the ones at which the kernels can go wrong: W = 1 and 5 x 7 (a row shorter than one 16-byte chunk), 6 x 86 (258 bytes per uint8 row:
the start alignment changes on every row, the last chunk is ragged), 3 x 341 (1023 bytes per row: more than one wave's 1008-byte run), 20 x 33 (more
than one 16-line ZIP block), and two frames of one shape first in every tree (the batch path).  Images: a narrow byte range (37-181), a full-range
one, and one whose channels span different ranges, so that the normalised tensor's minimum and maximum come from different channels.  PNG ground
truth plants (0,0,0), (0,0,1) and (1,0,0) pixels; EXR ground truth plants norms just below, at and just above 0.5, a NaN with a payload and an
all-zero pixel."""
import os
import struct
import zlib

import numpy as np

NAMES = ("nyuv2", "scannet", "ibims", "sintel")
SPLITS = {"nyuv2": "test", "scannet": "test", "ibims": "ibims", "sintel": "sintel"}
# per dataset: (scene, name, (H, W), EXR options)
SAMPLES = {
    "nyuv2": [("test", "000000", (6, 86), None), ("test", "000001", (6, 86), None), ("test", "000002", (3, 341), None)],
    "scannet": [("scene0001_00", "000000", (5, 7), None), ("scene0001_00", "000100", (5, 7), None), ("scene0002_00", "000000", (9, 1), None)],
    "ibims": [("ibims", "corridor_01", (6, 86), dict(compression="ZIP", pixel="FLOAT")), ("ibims", "corridor_02", (6, 86), dict(compression="NONE", pixel="HALF")),
              ("ibims", "kitchen_01", (3, 341), dict(compression="ZIP", pixel="HALF", origin=(3, -2)))],
    "sintel": [("alley_1", "frame_0001", (5, 7), dict(compression="NONE", pixel="FLOAT")), ("alley_1", "frame_0002", (5, 7), dict(compression="ZIPS", pixel="FLOAT", alpha=True)),
               ("bamboo_2", "frame_0001", (9, 1), dict(compression="ZIP", pixel="FLOAT", alpha=True)), ("bamboo_2", "frame_0002", (20, 33), dict(compression="ZIP", pixel="FLOAT"))],
}


def _seed(name, i):
    return 1000 * NAMES.index(name) + i + 17


def image(name, i):
    """the decoded image file: uint8 [H,W,3]"""
    H, W = SAMPLES[name][i][2]
    rng = np.random.default_rng(_seed(name, i))
    kind = (NAMES.index(name) + i) % 3
    if kind == 0:                                   # narrow range, the same for the three channels
        a = rng.integers(37, 182, (H, W, 3))
        a.reshape(-1, 3)[0] = 37
        a.reshape(-1, 3)[-1] = 181
    elif kind == 1:                                 # full range: the minimum comes from R (0), the maximum from B (255)
        a = rng.integers(0, 256, (H, W, 3))
        a.reshape(-1, 3)[0] = 0
        a.reshape(-1, 3)[-1] = 255
    else:                                           # the minimum comes from G, the maximum from R
        a = np.stack([rng.integers(100, 201, (H, W)), rng.integers(10, 121, (H, W)), rng.integers(60, 91, (H, W))], axis=2)
        a.reshape(-1, 3)[0] = (100, 10, 60)
        a.reshape(-1, 3)[-1] = (200, 120, 90)
    return a.astype(np.uint8)


def normal_png(name, i):
    """the decoded ground-truth PNG: uint8 [H,W,3]"""
    H, W = SAMPLES[name][i][2]
    rng = np.random.default_rng(_seed(name, i) + 500)
    a = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    flat = a.reshape(-1, 3)
    for k, v in enumerate(((0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 0, 0), (255, 255, 255), (0, 1, 0))):
        if 2 * k + 1 < flat.shape[0] - 1:
            flat[2 * k + 1] = v
    return a


def normal_exr(name, i):
    """what the ground-truth EXR file holds, as float32 [H,W,3] (R, G, B); a HALF file holds exactly these values as float16"""
    H, W = SAMPLES[name][i][2]
    opt = SAMPLES[name][i][3]
    rng = np.random.default_rng(_seed(name, i) + 900)
    v = rng.standard_normal((H, W, 3))
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    v *= rng.choice([1.0, 1.0, 1.0, 0.49, 0.51, 0.2], size=(H, W, 1))
    a = v.astype(np.float32)
    flat = a.reshape(-1, 3)
    up = np.nextafter(np.float32(0.5), np.float32(1.0))
    down = np.nextafter(np.float32(0.5), np.float32(0.0))
    nan = np.array([0x7FC12345], dtype=np.uint32).view(np.float32)[0]
    plants = ((0, 0, 0), (0.5, 0, 0), (up, 0, 0), (0, down, 0), (0.3, 0.4, 0.0), (nan, 1, 0), (0.5, 3e-4, 0), (0.2886751, 0.2886751, 0.2886752))
    for k, p in enumerate(plants):
        if k < flat.shape[0] - 1:
            flat[k] = p
    if opt["pixel"] == "HALF":
        with np.errstate(over="ignore"):
            a = a.astype(np.float16).astype(np.float32)
    return a


def intrins(name, i):
    H, W = SAMPLES[name][i][2]
    return np.array([[500.0 + i, 0, W / 2 - 0.5], [0, 510.0 + i, H / 2 - 0.5], [0, 0, 1]], dtype=np.float32)


def stub_normals(img_hwc_u8):
    """the stand-in pipeline's prediction: a fixed function of the image it is given -> float32 [3,H,W]"""
    a = np.asarray(img_hwc_u8).astype(np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)
    H, W = a.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    n = np.stack([a[..., 0] * np.float32(0.8) + np.float32(0.1) * xx / np.float32(W), a[..., 1] * np.float32(0.7) - np.float32(0.1) * yy / np.float32(H),
                  np.float32(0.3) + np.float32(0.5) * np.abs(a[..., 2])])
    return np.ascontiguousarray(n.astype(np.float32))


# ---- a minimal OpenEXR writer (scanline, single part) ---------------------------------------------------------------------------------------------------
def _attr(name, kind, value):
    return name.encode() + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(value)) + value


def write_exr(rgb, compression="NONE", pixel="FLOAT", origin=(0, 0), alpha=False):
    """rgb float32 [H,W,3] -> the bytes of an OpenEXR file whose channels are stored in the format's alphabetical order ([A,] B, G, R)"""
    H, W = rgb.shape[:2]
    ptype, dt = {"HALF": (1, "<f2"), "FLOAT": (2, "<f4")}[pixel]
    planes = {"B": rgb[..., 2], "G": rgb[..., 1], "R": rgb[..., 0]}
    if alpha:
        planes["A"] = np.full((H, W), 0.75, dtype=np.float32)
    names = sorted(planes)
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", ptype, 0, 1, 1) for n in names) + b"\0"
    x0, y0 = origin
    box = struct.pack("<4i", x0, y0, x0 + W - 1, y0 + H - 1)
    comp_id, lines = {"NONE": (0, 1), "ZIPS": (2, 1), "ZIP": (3, 16)}[compression]
    header = struct.pack("<ii", 20000630, 2)
    header += _attr("channels", "chlist", chlist) + _attr("compression", "compression", bytes([comp_id])) + _attr("dataWindow", "box2i", box)
    header += _attr("displayWindow", "box2i", box) + _attr("lineOrder", "lineOrder", b"\0") + _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    header += _attr("screenWindowCenter", "v2f", struct.pack("<ff", 0.0, 0.0)) + _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    with np.errstate(over="ignore"):
        rows = [b"".join(planes[n][y].astype(dt).tobytes() for n in names) for y in range(H)]
    chunks = []
    for r0 in range(0, H, lines):
        raw = b"".join(rows[r0:r0 + lines])
        body = raw
        if compression != "NONE":
            b = np.frombuffer(raw, dtype=np.uint8)
            t = np.concatenate([b[0::2], b[1::2]]).astype(np.int16)          # even bytes first, then the odd ones
            p = t.copy()
            p[1:] = t[1:] - t[:-1] + 128                                     # the predictor: differences, biased by 128
            z = zlib.compress((p & 0xFF).astype(np.uint8).tobytes(), 6)
            body = z if len(z) < len(raw) else raw                          # a block that does not shrink is stored raw
        chunks.append(struct.pack("<ii", y0 + r0, len(body)) + body)
    table, at = b"", len(header) + 8 * len(chunks)
    for c in chunks:
        table += struct.pack("<Q", at)
        at += len(c)
    return header + table + b"".join(chunks)


def declare_compression(exr_bytes, comp_id):
    """the same file with its header's compression byte changed (the body no longer matches: for the reader's refusals)"""
    key = b"compression\0compression\0" + struct.pack("<i", 1)
    k = exr_bytes.index(key) + len(key)
    return exr_bytes[:k] + bytes([comp_id]) + exr_bytes[k + 1:]


def declare_tiled(exr_bytes):
    """the same file with the version field's tiled bit set"""
    v = struct.unpack_from("<i", exr_bytes, 4)[0] | 0x200
    return exr_bytes[:4] + struct.pack("<i", v) + exr_bytes[8:]


# ---- trees ------------------------------------------------------------------------------------------------------------------------------------------------
def make_tree(root, name):
    """writes <root>/dsine_eval/<name>/... and <root>/splits/<name>/split/<split>.txt -> {"dir", "split", "filenames", "base", "split_dir"}"""
    from PIL import Image
    base = os.path.join(root, "dsine_eval", name)
    lines = []
    for i, (scene, stem, _, opt) in enumerate(SAMPLES[name]):
        d = os.path.join(base, scene)
        os.makedirs(d, exist_ok=True)
        Image.fromarray(image(name, i)).save(os.path.join(d, stem + "_img.png"))
        if opt is None:
            Image.fromarray(normal_png(name, i)).save(os.path.join(d, stem + "_normal.png"))
        else:
            with open(os.path.join(d, stem + "_normal.exr"), "wb") as f:
                f.write(write_exr(normal_exr(name, i), **opt))
        np.save(os.path.join(d, stem + "_intrins.npy"), intrins(name, i))
        lines.append("%s/%s_img.png" % (scene, stem))
    split = os.path.join(root, "splits", name, "split", SPLITS[name] + ".txt")
    os.makedirs(os.path.dirname(split), exist_ok=True)
    with open(split, "w") as f:
        f.write("\n".join(lines) + "\n")
    return {"dir": base, "split": split, "filenames": lines, "base": root, "split_dir": os.path.join(root, "splits")}
