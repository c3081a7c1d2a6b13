"""The depth benchmarks of the zero-shot table (NYUv2, KITTI, ETH3D, ScanNet, DIODE): the reference's evaluation dataset classes
(Marigold/src/dataset/*.py) with the same constructor arguments, file layout (a directory or a tar file whose members are "./" + relative path),
filename lists, naming modes and returned keys — and everything after file decoding on the device (csrc/evalprep.hip, ops.depth_gt_prepare):
the division that decodes the file, KITTI's benchmark crop, the range test, the eigen / garg evaluation windows, DIODE's mask, the valid counts.

  DatasetMode, DepthFileNameMode, get_pred_name      base_depth_dataset.py:17-20, :235-256
  BaseDepthDataset                                   base_depth_dataset.py:29-232 (RGB_ONLY and EVAL; TRAIN raises: training reads data.Hypersim / data.VirtualKITTI2)
  NYUDataset, KITTIDataset, ETH3DDataset, ScanNetDataset, DIODEDataset
  get_dataset(cfg, base_data_dir, mode)              dataset/__init__.py:23-36; cfg: a mapping, or the path of a YAML file in the reference's format
  BENCHMARKS                                         the five benchmark configurations, keyed by the reference's config names

`ds[i]` returns device tensors: rgb_int [3,H,W] int32 (cropped for KITTI); in EVAL mode depth_raw_linear / depth_filled_linear [1,H,W] fp32 and
valid_mask_raw / valid_mask_filled [1,H,W] bool, plus n_valid_raw / n_valid_filled (int32 scalars, the masks' sums); always index and
rgb_relative_path.  `ds.prepare_batch(indices)` does the same for several frames of one raw shape in ONE kernel launch (tensors gain a leading
batch axis, index / rgb_relative_path become lists).  Only file decoding (Pillow, numpy) runs on the host; nothing is read back."""
import io
import os
import tarfile
from enum import Enum

import numpy as np
import torch

from . import ops


class DatasetMode(Enum):
    RGB_ONLY = "rgb_only"
    EVAL = "evaluate"
    TRAIN = "train"


class DepthFileNameMode(Enum):
    """how a prediction file is named after its rgb file"""
    id = 1        # id.png
    rgb_id = 2    # rgb_id.png
    i_d_rgb = 3   # i_d_1_rgb.png
    rgb_i_d = 4


def get_pred_name(rgb_basename, name_mode, suffix=".png"):
    if name_mode == DepthFileNameMode.rgb_id:
        pred = "pred_" + rgb_basename.split("_")[1]
    elif name_mode == DepthFileNameMode.i_d_rgb:
        pred = rgb_basename.replace("_rgb.", "_pred.")
    elif name_mode == DepthFileNameMode.id:
        pred = "pred_" + rgb_basename
    elif name_mode == DepthFileNameMode.rgb_i_d:
        pred = "pred_" + "_".join(rgb_basename.split("_")[1:])
    else:
        raise NotImplementedError(name_mode)
    return os.path.splitext(pred)[0] + suffix


def _as_raw(a, what):
    """a decoded depth array -> a 2-D array of a dtype the kernel reads (uint16, int32, float32) holding the same values"""
    a = np.asarray(a).squeeze()
    if a.ndim != 2:
        raise ValueError("%s: expected one channel, got an array of shape %s" % (what, a.shape))
    if a.dtype in (np.uint16, np.int32, np.float32):
        return np.ascontiguousarray(a)
    if a.dtype in (np.uint8, np.bool_):
        return a.astype(np.uint16)
    if a.dtype in (np.int8, np.int16):
        return a.astype(np.int32)
    if a.dtype.kind in "iu":
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("%s: integer depth beyond int32 (%s)" % (what, a.dtype))
        return a.astype(np.int32)
    if a.dtype.kind == "f":
        return a.astype(np.float32)                 # torch's .float() of the reference, taken before the (identity) decode
    raise TypeError("%s: cannot read depth of dtype %s" % (what, a.dtype))


class BaseDepthDataset(torch.utils.data.Dataset):
    divisor = 1.0           # depth = raw / divisor (float64 division, rounded to float32)
    inf_to_zero = False

    def __init__(self, mode, filename_ls_path, dataset_dir, disp_name, min_depth, max_depth, has_filled_depth, name_mode, device=None, **kwargs):
        super().__init__()
        if mode == DatasetMode.TRAIN:
            raise NotImplementedError("the benchmark classes serve RGB_ONLY and EVAL; training reads data.Hypersim / data.VirtualKITTI2")
        if not isinstance(mode, DatasetMode):
            raise TypeError("mode must be a DatasetMode, got %r" % (mode,))
        self.mode = mode
        self.filename_ls_path = filename_ls_path
        self.dataset_dir = dataset_dir
        self.disp_name = disp_name
        self.has_filled_depth = has_filled_depth
        self.name_mode = name_mode
        self.min_depth = min_depth
        self.max_depth = max_depth
        self.device = torch.device(device) if device is not None else None      # None: the current HIP device at the time of the call
        with open(self.filename_ls_path, "r") as f:
            self.filenames = [s.split() for s in f.readlines()]
        self.tar_obj = None
        self.is_tar = os.path.isfile(dataset_dir) and tarfile.is_tarfile(dataset_dir)

    def __len__(self):
        return len(self.filenames)

    # ---- host side: file decoding only ----
    def _read_bytes(self, rel_path):
        if self.is_tar:
            if self.tar_obj is None:
                self.tar_obj = tarfile.open(self.dataset_dir)
            return self.tar_obj.extractfile("./" + rel_path).read()
        with open(os.path.join(self.dataset_dir, rel_path), "rb") as f:
            return f.read()

    def _read_image(self, rel_path):
        from PIL import Image
        return np.asarray(Image.open(io.BytesIO(self._read_bytes(rel_path))))

    def _read_rgb_file(self, rel_path):
        """-> [H,W,C] as decoded (the reference transposes and widens on the host; here both happen on the device)"""
        rgb = self._read_image(rel_path)
        if rgb.ndim != 3:
            raise ValueError("%s: expected a colour image, got shape %s" % (rel_path, rgb.shape))
        return np.ascontiguousarray(rgb)

    def _read_raw_depth(self, rel_path):
        """-> the file's raster before any arithmetic: 2-D uint16 / int32 / float32"""
        return _as_raw(self._read_image(rel_path), rel_path)

    def _read_ext_mask(self, line):
        return None

    def _get_data_path(self, index):
        line = self.filenames[index]
        rgb_rel_path, depth_rel_path, filled_rel_path = line[0], None, None
        if self.mode != DatasetMode.RGB_ONLY:
            depth_rel_path = line[1]
            if self.has_filled_depth:
                filled_rel_path = line[2]
        return rgb_rel_path, depth_rel_path, filled_rel_path

    # ---- what the kernel is told ----
    def _crop(self, H0, W0):
        """(top, left, h, w) of the raster that is returned; None: all of it"""
        return None

    def _window(self, h, w):
        """(y0, y1, x0, x1): the evaluation-mask window in output coordinates (slice semantics: clamped to the frame); None: no window"""
        return None

    def _device(self):
        return self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())

    # ---- device side ----
    def prepare_batch(self, indices):
        indices = [int(i) for i in indices]
        if not indices:
            raise ValueError("prepare_batch: no index given")
        dev = self._device()
        paths = [self._get_data_path(i) for i in indices]
        rgbs = [self._read_rgb_file(p[0]) for p in paths]
        if len({r.shape for r in rgbs}) != 1:
            raise ValueError("prepare_batch: frames of different image shapes %s (batch frames of one shape)" % sorted({r.shape for r in rgbs}))
        with ops.on_device_of(torch.empty(0, device=dev)):
            rgb = torch.from_numpy(np.stack(rgbs)).to(dev)                                  # [B,H,W,C] as decoded
            crop = self._crop(rgb.shape[1], rgb.shape[2])
            if crop is not None:
                rgb = rgb[:, crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3]]
            out = {"rgb_int": rgb.permute(0, 3, 1, 2).to(torch.int32).contiguous()}
            if self.mode != DatasetMode.RGB_ONLY:
                raws = [self._read_raw_depth(p[1]) for p in paths]
                if self.has_filled_depth:
                    raws += [self._read_raw_depth(p[2]) for p in paths]
                if len({(r.shape, r.dtype) for r in raws}) != 1:
                    kinds = {r.dtype for r in raws}
                    if len({r.shape for r in raws}) != 1 or not all(k.kind in "iu" for k in kinds):
                        raise ValueError("prepare_batch: depth rasters of different shapes / kinds %s" % sorted({(r.shape, str(r.dtype)) for r in raws}))
                    raws = [r.astype(np.int32) for r in raws]                               # uint16 and int32 files mixed: int32 holds both
                exts = [self._read_ext_mask(self.filenames[i]) for i in indices]
                ext = None
                if exts[0] is not None:
                    ext = torch.from_numpy(np.stack(exts * (2 if self.has_filled_depth else 1))).to(dev)
                raw = torch.from_numpy(np.stack(raws)).to(dev)
                H0, W0 = raw.shape[1:]
                crop = self._crop(H0, W0)
                h, w = (H0, W0) if crop is None else crop[2:]
                depth, mask, nv = ops.depth_gt_prepare(raw, divisor=self.divisor, min_depth=self.min_depth, max_depth=self.max_depth, crop=crop,
                                                       window=self._window(h, w), inf_to_zero=self.inf_to_zero, ext_mask=ext)
                B = len(indices)
                f = B if self.has_filled_depth else 0                                       # without a filled file the reference returns the raw one twice
                out["depth_raw_linear"], out["valid_mask_raw"], out["n_valid_raw"] = depth[:B, None], mask[:B, None], nv[:B]
                out["depth_filled_linear"], out["valid_mask_filled"], out["n_valid_filled"] = depth[f:f + B, None], mask[f:f + B, None], nv[f:f + B]
                if not self.has_filled_depth:
                    out["depth_filled_linear"], out["valid_mask_filled"] = out["depth_filled_linear"].clone(), out["valid_mask_filled"].clone()
        out["index"] = indices
        out["rgb_relative_path"] = [p[0] for p in paths]
        return out

    def __getitem__(self, index):
        if index < 0:
            index += len(self)
        if not 0 <= index < len(self):
            raise IndexError(index)
        return {k: v[0] for k, v in self.prepare_batch([index]).items()}

    def __del__(self):
        if getattr(self, "tar_obj", None) is not None:
            self.tar_obj.close()
            self.tar_obj = None


class NYUDataset(BaseDepthDataset):
    divisor = 1000.0

    def __init__(self, eigen_valid_mask, **kwargs):
        super().__init__(min_depth=1e-3, max_depth=10.0, has_filled_depth=True, name_mode=DepthFileNameMode.rgb_id, **kwargs)
        self.eigen_valid_mask = eigen_valid_mask

    def _window(self, h, w):
        return (45, 471, 41, 601) if self.eigen_valid_mask else None


class ScanNetDataset(BaseDepthDataset):
    divisor = 1000.0

    def __init__(self, **kwargs):
        super().__init__(min_depth=1e-3, max_depth=10, has_filled_depth=False, name_mode=DepthFileNameMode.id, **kwargs)


class KITTIDataset(BaseDepthDataset):
    divisor = 256.0
    KB_CROP_HEIGHT, KB_CROP_WIDTH = 352, 1216

    def __init__(self, kitti_bm_crop, valid_mask_crop, **kwargs):
        super().__init__(min_depth=1e-5, max_depth=80, has_filled_depth=False, name_mode=DepthFileNameMode.id, **kwargs)
        self.kitti_bm_crop = kitti_bm_crop
        self.valid_mask_crop = valid_mask_crop
        if valid_mask_crop not in (None, "garg", "eigen"):
            raise ValueError("Unknown crop type: %s" % (valid_mask_crop,))
        self.filenames = [f for f in self.filenames if f[1] != "None"]      # frames without ground truth

    def _crop(self, H0, W0):
        if not self.kitti_bm_crop:
            return None
        if H0 < self.KB_CROP_HEIGHT or W0 < self.KB_CROP_WIDTH:
            raise ValueError("KITTI frame %d x %d is smaller than the benchmark crop %d x %d" % (H0, W0, self.KB_CROP_HEIGHT, self.KB_CROP_WIDTH))
        return int(H0 - self.KB_CROP_HEIGHT), int((W0 - self.KB_CROP_WIDTH) / 2), self.KB_CROP_HEIGHT, self.KB_CROP_WIDTH

    def _window(self, h, w):
        """the bounds are fractions of the shape the mask is made for: the cropped frame when kitti_bm_crop is set"""
        if self.valid_mask_crop == "garg":
            return int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w)
        if self.valid_mask_crop == "eigen":
            return int(0.3324324 * h), int(0.91351351 * h), int(0.0359477 * w), int(0.96405229 * w)
        return None


class ETH3DDataset(BaseDepthDataset):
    HEIGHT, WIDTH = 4032, 6048
    inf_to_zero = True

    def __init__(self, **kwargs):
        super().__init__(min_depth=1e-5, max_depth=float("inf"), has_filled_depth=False, name_mode=DepthFileNameMode.id, **kwargs)

    def _read_raw_depth(self, rel_path):
        """the raw float32 raster of https://www.eth3d.net/documentation#format-of-multi-view-data-image-formats"""
        a = np.frombuffer(self._read_bytes(rel_path), dtype=np.float32)
        if a.size != self.HEIGHT * self.WIDTH:
            raise ValueError("%s: %d float32 values, expected %d x %d" % (rel_path, a.size, self.HEIGHT, self.WIDTH))
        return a.reshape(self.HEIGHT, self.WIDTH)


class DIODEDataset(BaseDepthDataset):
    def __init__(self, **kwargs):
        super().__init__(min_depth=0.6, max_depth=350, has_filled_depth=False, name_mode=DepthFileNameMode.id, **kwargs)

    def _read_npy(self, rel_path):
        return np.load(io.BytesIO(self._read_bytes(rel_path)))

    def _read_raw_depth(self, rel_path):
        return _as_raw(self._read_npy(rel_path), rel_path)

    def _get_data_path(self, index):
        return self.filenames[index]            # rgb, depth, mask on every line, in every mode

    def _read_ext_mask(self, line):
        """the validity mask comes from the file, not from the depth range"""
        m = self._read_npy(line[2]).squeeze().astype(bool)
        if m.ndim != 2:
            raise ValueError("%s: expected a 2-D mask, got shape %s" % (line[2], m.shape))
        return np.ascontiguousarray(m).view(np.uint8)


dataset_name_class_dict = {"nyu_v2": NYUDataset, "kitti": KITTIDataset, "eth3d": ETH3DDataset, "diode": DIODEDataset, "scannet": ScanNetDataset}

# the reference's five benchmark configurations, keyed by the names of its config files; `dir` is relative to base_data_dir, the filename list is the caller's
BENCHMARKS = {
    "data_nyu_test": {"name": "nyu_v2", "disp_name": "nyu_test_full", "dir": "nyuv2/nyu_labeled_extracted.tar", "eigen_valid_mask": True},
    "data_kitti_eigen_test": {"name": "kitti", "disp_name": "kitti_eigen_test_full", "dir": "kitti/kitti_eigen_split_test.tar", "kitti_bm_crop": True,
                              "valid_mask_crop": "eigen"},
    "data_eth3d": {"name": "eth3d", "disp_name": "eth3d_full", "dir": "eth3d/eth3d.tar"},
    "data_scannet_val": {"name": "scannet", "disp_name": "scannet_val_800_1", "dir": "scannet/scannet_val_sampled_800_1.tar"},
    "data_diode_all": {"name": "diode", "disp_name": "diode_val_all", "dir": "diode/diode_val.tar"},
}


def load_config(path):
    """a dataset YAML file in the reference's format (Marigold/config/dataset/*.yaml) -> dict; needs PyYAML"""
    try:
        import yaml
    except ImportError as e:
        raise RuntimeError("reading %s needs PyYAML; pass a mapping (eval_data.BENCHMARKS[...]) instead" % path) from e
    with open(path) as f:
        cfg = yaml.safe_load(f)
    if not isinstance(cfg, dict):
        raise ValueError("%s does not hold a mapping" % path)
    return cfg


def get_dataset(cfg_data_split, base_data_dir, mode, filenames=None, **kwargs):
    """cfg_data_split: a mapping with name, disp_name, dir [, filenames] and the dataset's flags, or the path of such a YAML file;
    filenames: the filename list (overrides the mapping's)"""
    cfg = load_config(cfg_data_split) if isinstance(cfg_data_split, (str, os.PathLike)) else dict(cfg_data_split)
    if cfg.get("name") not in dataset_name_class_dict:
        raise NotImplementedError("unknown dataset %r (one of %s)" % (cfg.get("name"), sorted(dataset_name_class_dict)))
    filenames = filenames if filenames is not None else cfg.get("filenames")
    if filenames is None:
        raise ValueError("no filename list: pass filenames=... or give the configuration a `filenames` entry")
    cfg.pop("filenames", None)
    return dataset_name_class_dict[cfg["name"]](mode=mode, filename_ls_path=filenames, dataset_dir=os.path.join(base_data_dir, cfg["dir"]), **cfg, **kwargs)
