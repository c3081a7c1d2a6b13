"""The surface-normal benchmarks of the zero-shot table (NYUv2, ScanNet, iBims-1, Sintel) as DSINE's benchmark mode reads them
(DSINE/projects/baseline_normal/dataloader.py:15-111, DSINE/data/datasets/{nyuv2,scannet,ibims,sintel}/__init__.py, the test-mode transform of
DSINE/data/augmentations/__init__.py:13-97 at input_height = input_width = 0: ToTensor, Normalize, ToDict) — and everything after file decoding on the
device (csrc/normalprep.hip): the image round trip of DSINE/projects/dsine/test.py:59-65 (ops.dsine_rgb_requantize) and the ground truth's decode,
mask, planar layout and valid count (ops.normal_gt_prepare).

  NormalBenchmarkDataset(dataset_name, dataset_dir, filenames, device=None, exr_decoder=None)
      dataset_dir is .../dsine_eval/<dataset_name>; a sample "scene/name_img.png" of the split list has its files at
      <dataset_dir>/scene/name_img.png, name_normal.png (nyuv2, scannet) or name_normal.exr (ibims, sintel), name_intrins.npy
  NORMAL_BENCHMARKS          per dataset: the reference's split name and the domain test.py:47-53 gives GeoWizard, in test.py:213-227's order
  read_exr(data)             a small OpenEXR reader (struct, zlib, numpy) for the two benchmarks whose ground truth is an .exr file

`ds[i]` returns device tensors: img_u8 [3,H,W] uint8 — the RE-QUANTISED image the reference feeds the pipeline, not the file's bytes —, normal [3,H,W]
fp32, normal_mask [1,H,W] bool, n_valid (int32 scalar, the mask's sum), intrins [3,3] fp32 (carried through as loaded; nothing consumes it here);
and dataset_name, scene_name, img_name, index.  `ds.prepare_batch(indices)` does several frames of one shape in ONE launch of each kernel
(tensors gain a leading batch axis, the names and index become lists).  Only file decoding (Pillow, numpy, read_exr) runs on the host; nothing is read
back.  The reference decodes images with OpenCV; an 8-bit RGB PNG decodes to the same bytes with Pillow (a JPEG may not: decoders differ)."""
import io
import os
import struct
import zlib

import numpy as np
import torch

from . import ops

# test.py:213-227 (the order `eval_data all` walks) and :47-53 (GeoWizard's domain when the args file gives none)
NORMAL_BENCHMARKS = {
    "nyuv2": {"split": "test", "domain": "indoor", "normal_ext": ".png"},
    "scannet": {"split": "test", "domain": "indoor", "normal_ext": ".png"},
    "ibims": {"split": "ibims", "domain": "indoor", "normal_ext": ".exr"},
    "sintel": {"split": "sintel", "domain": "outdoor", "normal_ext": ".exr"},
}

_EXR_MAGIC = 20000630
_EXR_COMPRESSION = ("NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB")
_EXR_LINES = {"NONE": 1, "ZIPS": 1, "ZIP": 16}
_EXR_PIXEL = {1: np.dtype("<f2"), 2: np.dtype("<f4")}          # HALF, FLOAT (0 is UINT)


def _cstr(data, pos, what):
    end = data.find(b"\0", pos)
    if end < 0:
        raise ValueError("read_exr: unterminated %s at byte %d" % (what, pos))
    return data[pos:end].decode("latin-1"), end + 1


def read_exr(data):
    """OpenEXR file bytes -> np.ndarray [H,W,3] float32 (R, G, B).  Reads single-part scanline files with compression NONE, ZIPS or ZIP (zlib, then
    the byte predictor, then the even / odd de-interleave), HALF or FLOAT channels found by the names R, G, B in whatever order the file stores them
    (other channels are skipped), any data-window origin.  Everything else — tiled, multi-part and deep files, RLE, PIZ, PXR24, B44 and DWA
    compression, UINT or subsampled channels — raises NotImplementedError naming what was met.
    Which compression the released dsine_eval .exr files use has not been checked against a real file: OpenCV's writer defaults suggest ZIP with
    FLOAT channels.  For anything this reader refuses, pass NormalBenchmarkDataset an exr_decoder (OpenCV's, for one)."""
    data = bytes(data)
    if len(data) < 8 or struct.unpack_from("<i", data, 0)[0] != _EXR_MAGIC:
        raise ValueError("read_exr: not an OpenEXR file (magic number)")
    version = struct.unpack_from("<i", data, 4)[0]
    if version & 0xFF != 2:
        raise NotImplementedError("read_exr: OpenEXR format version %d" % (version & 0xFF))
    for bit, name in ((0x200, "a tiled file"), (0x800, "a deep (non-image) file"), (0x1000, "a multi-part file")):
        if version & bit:
            raise NotImplementedError("read_exr: %s" % name)
    pos, attrs = 8, {}
    while True:
        name, pos = _cstr(data, pos, "attribute name")
        if name == "":
            break
        kind, pos = _cstr(data, pos, "attribute type")
        size = struct.unpack_from("<i", data, pos)[0]
        if size < 0 or pos + 4 + size > len(data):
            raise ValueError("read_exr: attribute %s runs past the file" % name)
        attrs[name] = (kind, data[pos + 4:pos + 4 + size])
        pos += 4 + size
    for need in ("channels", "compression", "dataWindow"):
        if need not in attrs:
            raise ValueError("read_exr: header without %s" % need)
    if "tiles" in attrs or attrs.get("type", ("", b"scanlineimage"))[1].rstrip(b"\0") not in (b"scanlineimage",):
        raise NotImplementedError("read_exr: a tiled or deep part (type %r)" % attrs.get("type", ("", b"tiledimage"))[1])
    comp_id = attrs["compression"][1][0]
    comp = _EXR_COMPRESSION[comp_id] if comp_id < len(_EXR_COMPRESSION) else "compression %d" % comp_id
    if comp not in _EXR_LINES:
        raise NotImplementedError("read_exr: %s compression (NONE, ZIPS and ZIP are read)" % comp)
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1][:16])
    W, H = x1 - x0 + 1, y1 - y0 + 1
    if W <= 0 or H <= 0:
        raise ValueError("read_exr: empty data window (%d, %d) - (%d, %d)" % (x0, y0, x1, y1))
    chans, cpos, cl = [], 0, attrs["channels"][1]
    while cpos < len(cl) and cl[cpos] != 0:
        cname, cpos = _cstr(cl, cpos, "channel name")
        ptype, _, xs, ys = struct.unpack_from("<iIii", cl, cpos)
        cpos += 16
        if xs != 1 or ys != 1:
            raise NotImplementedError("read_exr: channel %s is subsampled (%d, %d)" % (cname, xs, ys))
        if ptype not in _EXR_PIXEL:
            raise NotImplementedError("read_exr: channel %s has pixel type %d (HALF and FLOAT are read)" % (cname, ptype))
        chans.append((cname, _EXR_PIXEL[ptype]))
    start, where = 0, {}
    for cname, dt in chans:                     # one scanline holds each channel's W values in turn, in the file's (alphabetical) channel order
        where[cname] = (start, dt)
        start += W * dt.itemsize
    line_bytes = start
    missing = [c for c in "RGB" if c not in where]
    if missing:
        raise ValueError("read_exr: no channel %s (the file has %s)" % (", ".join(missing), ", ".join(c for c, _ in chans)))
    lines = _EXR_LINES[comp]
    nchunks = (H + lines - 1) // lines
    if pos + 8 * nchunks > len(data):
        raise ValueError("read_exr: the offset table runs past the file")
    offsets = struct.unpack_from("<%dQ" % nchunks, data, pos)
    out = np.empty((H, W, 3), dtype=np.float32)
    seen = np.zeros(H, dtype=bool)
    for off in offsets:
        if off + 8 > len(data):
            raise ValueError("read_exr: a chunk offset points past the file")
        y, size = struct.unpack_from("<ii", data, off)
        r0 = y - y0
        if r0 < 0 or r0 >= H or r0 % lines or size < 0 or off + 8 + size > len(data):
            raise ValueError("read_exr: bad chunk at byte %d (y %d, %d bytes)" % (off, y, size))
        n = min(lines, H - r0)
        want = n * line_bytes
        blob = data[off + 8:off + 8 + size]
        if comp != "NONE" and size < want:          # a block that did not shrink is stored as it is
            t = np.frombuffer(zlib.decompress(blob), dtype=np.uint8).copy()
            if t.size != want:
                raise ValueError("read_exr: chunk at y %d inflates to %d bytes, expected %d" % (y, t.size, want))
            t[1:] += 128                            # predictor: d[i] = d[i-1] + d[i] - 128 (mod 256)
            t = np.cumsum(t, dtype=np.uint8)
            raw = np.empty(want, dtype=np.uint8)
            raw[0::2] = t[:(want + 1) // 2]         # first half: the even bytes; second half: the odd ones
            raw[1::2] = t[(want + 1) // 2:]
        else:
            if size != want:
                raise ValueError("read_exr: chunk at y %d holds %d bytes, expected %d" % (y, size, want))
            raw = np.frombuffer(blob, dtype=np.uint8)
        block = raw.reshape(n, line_bytes)
        for k, c in enumerate("RGB"):
            s, dt = where[c]
            out[r0:r0 + n, :, k] = np.ascontiguousarray(block[:, s:s + W * dt.itemsize]).view(dt).astype(np.float32)
        seen[r0:r0 + n] = True
    if not seen.all():
        raise ValueError("read_exr: scanline %d is in no chunk" % (y0 + int(np.argmin(seen))))
    return out


def read_split(filenames):
    """a split file in the reference's format (one "scene/name_img.ext" per line; dataloader.py:24-27) or a list of such strings -> list"""
    if isinstance(filenames, (str, os.PathLike)):
        if not os.path.exists(filenames):
            raise FileNotFoundError("split file %s does not exist" % (filenames,))
        with open(filenames, "r") as f:
            lines = [s.strip() for s in f.readlines()]
    else:
        lines = [str(s).strip() for s in filenames]
    lines = [s for s in lines if s]
    for s in lines:
        parts = s.split("/")
        if len(parts) != 2 or "_img" not in parts[1]:
            raise ValueError("split entry %r is not of the form scene/name_img.ext" % s)
    return lines


class NormalBenchmarkDataset(torch.utils.data.Dataset):
    def __init__(self, dataset_name, dataset_dir, filenames, device=None, exr_decoder=None):
        super().__init__()
        if dataset_name not in NORMAL_BENCHMARKS:
            raise ValueError("unknown normals benchmark %r: %s are served (oasis and vkitti are not part of the reference's benchmark mode either)"
                             % (dataset_name, ", ".join(NORMAL_BENCHMARKS)))
        self.dataset_name = dataset_name
        self.dataset_dir = dataset_dir
        self.filenames = read_split(filenames)
        self.split = NORMAL_BENCHMARKS[dataset_name]["split"]
        self.domain = NORMAL_BENCHMARKS[dataset_name]["domain"]
        self.normal_ext = NORMAL_BENCHMARKS[dataset_name]["normal_ext"]
        self.device = torch.device(device) if device is not None else None      # None: the current HIP device at the time of the call
        self.exr_decoder = exr_decoder if exr_decoder is not None else read_exr  # bytes -> [H,W,3] float32, R, G, B

    def __len__(self):
        return len(self.filenames)

    # ---- host side: file decoding only ----
    def paths(self, index):
        """-> (scene_name, img_name, image path, normal path, intrinsics path) as the get_sample functions derive them"""
        sample_path = self.filenames[index]
        scene_name = sample_path.split("/")[0]
        img_name, img_ext = sample_path.split("/")[1].split("_img")
        img_path = "%s/%s" % (self.dataset_dir, sample_path)
        return (scene_name, img_name, img_path, img_path.replace("_img" + img_ext, "_normal" + self.normal_ext),
                img_path.replace("_img" + img_ext, "_intrins.npy"))

    @staticmethod
    def _read_bytes(path):
        if not os.path.exists(path):
            raise FileNotFoundError("benchmark file %s does not exist" % path)
        with open(path, "rb") as f:
            return f.read()

    def _read_png(self, path, what):
        from PIL import Image
        a = np.asarray(Image.open(io.BytesIO(self._read_bytes(path))))
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError("%s: expected an 8-bit RGB %s, got shape %s of %s" % (path, what, a.shape, a.dtype))
        return np.ascontiguousarray(a)

    def _read_normal(self, path):
        if self.normal_ext == ".png":
            return self._read_png(path, "normal map")
        a = np.asarray(self.exr_decoder(self._read_bytes(path)))
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.float32:
            raise ValueError("%s: the EXR decoder must return float32 [H,W,3], got shape %s of %s" % (path, a.shape, a.dtype))
        return np.ascontiguousarray(a)

    def _device(self):
        return self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())

    # ---- device side ----
    def prepare_batch(self, indices, out=None):
        """out: a dict this method returned before for frames of the same shape; its tensors are written in place (no allocation)"""
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("prepare_batch: no index given")
        paths = [self.paths(i) for i in indices]
        imgs = [self._read_png(p[2], "image") for p in paths]
        normals = [self._read_normal(p[3]) for p in paths]
        intrins = [np.asarray(np.load(io.BytesIO(self._read_bytes(p[4]))), dtype=np.float32) for p in paths]
        if len({a.shape for a in imgs}) != 1:
            raise ValueError("prepare_batch: frames of different image shapes %s (batch frames of one shape)" % sorted({a.shape for a in imgs}))
        for p, a, n in zip(paths, imgs, normals):
            if n.shape != a.shape:
                raise ValueError("%s: the normal map %s does not match the image %s" % (p[3], n.shape, a.shape))
        B = len(indices)
        o_img = o_gt = None
        if out is not None:
            o_img = out["img_u8"]
            o_gt = (out["normal"], out["normal_mask"].view(torch.uint8), out["n_valid"])
        dev = self._device()
        with ops.on_device_of(torch.empty(0, device=dev)):
            img = ops.dsine_rgb_requantize(torch.from_numpy(np.stack(imgs)).to(dev), layout="chw", out=o_img)
            normal, mask, nv = ops.normal_gt_prepare(torch.from_numpy(np.stack(normals)).to(dev), out=o_gt)
            k = torch.from_numpy(np.stack(intrins)).to(dev)
        return {"img_u8": img, "normal": normal, "normal_mask": mask, "n_valid": nv, "intrins": k, "dataset_name": [self.dataset_name] * B,
                "scene_name": [p[0] for p in paths], "img_name": [p[1] for p in paths], "index": indices}

    def __getitem__(self, index):
        if index < 0:
            index += len(self)
        if not 0 <= index < len(self):
            raise IndexError(index)
        return {k: v[0] for k, v in self.prepare_batch([index]).items()}
