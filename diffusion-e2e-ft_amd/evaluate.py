"""Depth evaluation on the device: the arithmetic of the reference's evaluation loop — least-squares alignment
(Marigold/src/util/alignment.py:8-56), range clipping (Marigold/eval.py:203-209) and the metric suite (Marigold/src/util/metric.py:34-158) —
for whole batches in one launch sequence (csrc/evalmetrics.hip), instead of numpy.linalg.lstsq on the host plus ten torch reductions per image.

  align_depth_least_square   same name and return convention as the reference's function, torch tensors on the device
  depth_metrics              per-image metric table (dict name -> tensor [B]) and its mean, named as eval.py's metric functions
  MetricTracker              running averages keyed by metric name (the reference's pandas-backed tracker, metric.py:9-31)
  evaluate_depth_benchmark   the reference's infer.py + eval.py pair over one benchmark dataset (eval_data.py) without the .npy round trip
  group_by_shape             the batches of both runners' predict_batch_size mode (pipe.predict_batch on device tensors): consecutive frames of one shape

Surface normals (DSINE's benchmark mode, csrc/normaleval.hip), named as DSINE/utils/utils.py names them:
  normal_error               compute_normal_error (utils.py:150-158): per-pixel angular error in degrees, [B,1,H,W] fp32
  normal_metrics             compute_normal_metrics(compute_normal_error(pred, gt)[mask]) (utils.py:161-178) in one call
  NormalMetricAccumulator    the accumulation loop of DSINE/projects/dsine/test.py:104-133 without the torch.cat per image or the host round trip
  format_normal_metrics      the two lines test.py prints and writes to metrics.txt
  evaluate_normal_benchmark  test.py:40-133 over one normal benchmark (normal_eval_data.py): re-quantised image in, pooled metrics and metrics.txt out
"""
import torch

from . import ops

METRIC_NAMES = ("abs_relative_difference", "squared_relative_difference", "rmse_linear", "rmse_log", "log10", "delta1_acc", "delta2_acc",
                "delta3_acc", "i_rmse", "silog_rmse")


def _b(t):
    """[H,W] / [B,H,W] / [B,1,H,W] -> [B,H,W]; anything else is an error (a [B,3,H,W] prediction must not spin here)"""
    t = torch.as_tensor(t)
    if t.dim() == 4:
        if t.shape[1] != 1:
            raise ValueError("expected a depth map [B,1,H,W], [B,H,W] or [H,W]; got shape %s" % (tuple(t.shape),))
        t = t[:, 0]
    if t.dim() == 2:
        return t[None]
    if t.dim() != 3:
        raise ValueError("expected a depth map [B,1,H,W], [B,H,W] or [H,W]; got shape %s" % (tuple(t.shape),))
    return t


@torch.no_grad()
@ops.tensor_scoped
def align_depth_least_square(gt_arr, pred_arr, valid_mask_arr, return_scale_shift=True, max_resolution=None):
    """alignment.py:8-56: returns pred * scale + shift (no clipping) [, scale, shift]; inputs [H,W] or [B,H,W] device tensors"""
    gt, pred, mask = _b(gt_arr).float(), _b(pred_arr).float(), _b(valid_mask_arr)
    m = ops.depth_eval(pred, gt, mask, align_max_res=max_resolution or 0, min_depth=1e-30, max_depth=3e38)
    scale, shift = m[:, 10], m[:, 11]
    aligned = (pred * scale[:, None, None] + shift[:, None, None]).reshape(torch.as_tensor(pred_arr).shape)
    if return_scale_shift:
        return (aligned, scale, shift) if scale.numel() > 1 else (aligned, scale[0], shift[0])
    return aligned


@torch.no_grad()
@ops.tensor_scoped
def depth_metrics(pred, gt, valid_mask, alignment="least_square", min_depth=1e-3, max_depth=80.0, alignment_max_res=None, return_aligned=False):
    """pred (affine-invariant prediction), gt (metric depth), valid_mask: [B,H,W] (or [H,W]) device tensors.  alignment: "least_square" |
    "least_square_disparity" (eval.py:172-201).  Returns {metric name: tensor [B]} plus "scale" / "shift" (and "aligned" when asked)."""
    if alignment not in ("least_square", "least_square_disparity"):
        raise ValueError("alignment must be least_square or least_square_disparity (the prediction is affine-invariant)")
    res = ops.depth_eval(_b(pred).float(), _b(gt).float(), _b(valid_mask), disparity=alignment == "least_square_disparity",
                         align_max_res=alignment_max_res or 0, min_depth=min_depth, max_depth=max_depth, return_aligned=return_aligned)
    table, aligned = res if return_aligned else (res, None)
    out = {n: table[:, i] for i, n in enumerate(METRIC_NAMES)}
    out["scale"], out["shift"] = table[:, 10], table[:, 11]
    if return_aligned:
        out["aligned"] = aligned
    return out


class MetricTracker:
    """metric.py:9-31 without pandas: update(key, value, n) / avg(key) / result()"""

    def __init__(self, *keys):
        self._tot = {k: 0.0 for k in keys}
        self._cnt = {k: 0 for k in keys}

    def reset(self):
        for k in self._tot:
            self._tot[k], self._cnt[k] = 0.0, 0

    def update(self, key, value, n=1):
        self._tot[key] = self._tot.get(key, 0.0) + float(value) * n
        self._cnt[key] = self._cnt.get(key, 0) + n

    def update_batch(self, metrics):
        for k in METRIC_NAMES:
            v = metrics[k]
            self.update(k, float(v.double().mean()), int(v.numel()))

    def avg(self, key):
        return self._tot[key] / self._cnt[key]

    def result(self):
        return {k: self.avg(k) for k in self._tot if self._cnt[k]}


def _metric_table(rows):
    """the name / value table of eval_metrics.txt: tabulate's when it imports (eval.py:237-239), two plain rows otherwise"""
    try:
        from tabulate import tabulate
    except ImportError:
        cells = [[str(c) for c in r] for r in rows]
        width = [max(len(r[i]) for r in cells) for i in range(len(cells[0]))]
        return "\n".join("  ".join(c.ljust(w) for c, w in zip(r, width)).rstrip() for r in cells)
    return tabulate(rows)


def _batches(pairs, batch_size):
    """(shape, payload) pairs in dataset order -> lists of payloads: consecutive pairs of one shape, at most batch_size per list; another shape starts a new list"""
    group, shape = [], None
    for s, payload in pairs:
        if group and (s != shape or len(group) == batch_size):
            yield group
            group = []
        shape = s
        group.append(payload)
    if group:
        yield group


def group_by_shape(shapes, batch_size):
    """the batches of the runners' predict_batch_size mode as index lists: [shape of frame i] -> [[i, ...], ...] — consecutive frames of one shape, at most batch_size
    per group, dataset order kept (a pure function: no tensors, no device)"""
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError("batch_size must be an integer >= 1, got %r" % (batch_size,))
    return list(_batches(((tuple(s), i) for i, s in enumerate(shapes)), batch_size))


def _batched_pipe(pipe, predict_batch_size, who):
    """predict_batch_size of a runner: None stays None (the per-frame loop); anything else must be an integer >= 1 and the pipe must have predict_batch"""
    if predict_batch_size is None:
        return None
    try:
        group_by_shape((), predict_batch_size)
    except ValueError:
        raise ValueError("%s: predict_batch_size must be None or an integer >= 1, got %r" % (who, predict_batch_size)) from None
    if not callable(getattr(pipe, "predict_batch", None)):
        raise TypeError("%s: predict_batch_size=%d needs a pipeline with a predict_batch method; %s has none" % (who, predict_batch_size, type(pipe).__name__))
    return predict_batch_size


def evaluate_depth_benchmark(pipe, dataset, alignment="least_square", alignment_max_res=None, output_dir=None, save_predictions=False, predict_batch_size=None,
                             **pipe_kwargs):
    """Marigold/infer.py:278-333 and Marigold/eval.py:146-249 in one loop over an eval_data dataset in EVAL mode: per sample, `pipe(PIL image,
    **pipe_kwargs).depth_np` is aligned to depth_raw_linear over valid_mask_raw, clipped to the dataset's range and measured (depth_metrics, on the
    device); the ten metrics are averaged over the samples (MetricTracker) and returned as a dict.  A sample without a valid pixel is named in a
    warning and left out of the average.  output_dir: per_sample_metrics.csv and eval_metrics[-<alignment>].txt as eval.py writes them;
    save_predictions: also the .npy predictions where infer.py puts them (<output_dir>/<scene dir>/<get_pred_name(...)>).
    predict_batch_size: None — the loop above; an integer >= 1 — consecutive frames of one shape go, up to predict_batch_size at a time, through
    `pipe.predict_batch(uint8 [B,3,H,W] device tensor, **pipe_kwargs)` (its keywords, not `__call__`'s) and its fp32 [B,H,W] device tensor is measured as
    it is, no PIL image and no numpy in between; rows, files and their text are those of the loop, in dataset order.  (A `batch_size` among the
    keywords is, as before, the pipeline's own: the ensemble members per pass of `__call__`.)"""
    import os
    import warnings

    import numpy as np
    from PIL import Image

    from .eval_data import DatasetMode, get_pred_name
    if alignment not in ("least_square", "least_square_disparity"):
        raise ValueError("alignment must be least_square or least_square_disparity (the prediction is affine-invariant)")
    if dataset.mode != DatasetMode.EVAL:
        raise ValueError("evaluate_depth_benchmark needs a dataset in DatasetMode.EVAL, got %s" % (dataset.mode,))
    if save_predictions and output_dir is None:
        raise ValueError("save_predictions needs an output_dir")
    tracker = MetricTracker(*METRIC_NAMES)
    per_sample = None
    if output_dir is not None:
        os.makedirs(output_dir, exist_ok=True)
        per_sample = os.path.join(output_dir, "per_sample_metrics.csv")
        with open(per_sample, "w") as f:
            f.write("filename," + ",".join(METRIC_NAMES) + "\n")
    predict_batch_size = _batched_pipe(pipe, predict_batch_size, "evaluate_depth_benchmark")

    def pred_name_of(rgb_name):
        return os.path.join(os.path.dirname(rgb_name), get_pred_name(os.path.basename(rgb_name), dataset.name_mode, suffix=".npy"))

    def save(pred_name, pred):
        os.makedirs(os.path.dirname(os.path.join(output_dir, pred_name)), exist_ok=True)
        np.save(os.path.join(output_dir, pred_name), pred)

    def has_valid_pixels(item, pred_shape):
        rgb_name, gt = item["rgb_relative_path"], item["depth_raw_linear"][0]
        if tuple(pred_shape) != tuple(gt.shape):
            raise ValueError("%s: prediction %s and ground truth %s differ in shape" % (rgb_name, tuple(pred_shape), tuple(gt.shape)))
        if int(item["n_valid_raw"]) == 0:
            warnings.warn("evaluate_depth_benchmark: %s has no valid ground-truth pixel; skipped" % rgb_name)
            return False
        return True

    def measure(items, pred):
        """the frames of `items` (one shape) against pred [len(items),H,W] on the device -> one row of the ten metrics per frame, recorded in order"""
        gt = torch.stack([item["depth_raw_linear"][0] for item in items])
        mask = torch.stack([item["valid_mask_raw"][0] for item in items])
        with ops.on_device_of(gt):
            m = depth_metrics(pred.to(gt.device), gt, mask, alignment=alignment, min_depth=dataset.min_depth, max_depth=dataset.max_depth,
                              alignment_max_res=alignment_max_res)
            table = torch.stack([m[k] for k in METRIC_NAMES], dim=1).cpu().tolist()
        for item, values in zip(items, table):
            for k, v in zip(METRIC_NAMES, values):
                tracker.update(k, v)
            if per_sample is not None:
                with open(per_sample, "a") as f:
                    f.write(pred_name_of(item["rgb_relative_path"]) + "," + ",".join(str(v) for v in values) + "\n")

    items = (dataset[i] for i in range(len(dataset)))
    if predict_batch_size is None:
        for item in items:
            image = Image.fromarray(item["rgb_int"].permute(1, 2, 0).to(torch.uint8).cpu().numpy())
            pred = np.asarray(pipe(image, **pipe_kwargs).depth_np)
            if save_predictions:
                save(pred_name_of(item["rgb_relative_path"]), pred)
            if has_valid_pixels(item, pred.shape):
                measure([item], torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32))[None])
    else:
        for group in _batches(((tuple(item["rgb_int"].shape), item) for item in items), predict_batch_size):
            preds = pipe.predict_batch(torch.stack([item["rgb_int"] for item in group]).to(torch.uint8), **pipe_kwargs)
            if not isinstance(preds, torch.Tensor) or preds.dim() != 3 or preds.shape[0] != len(group):
                raise ValueError("%s: predict_batch must return a depth tensor [%d,H,W], got %s"
                                 % (group[0]["rgb_relative_path"], len(group), tuple(preds.shape) if isinstance(preds, torch.Tensor) else type(preds).__name__))
            preds = preds.float()
            if save_predictions:
                for item, pred in zip(group, preds.cpu().numpy()):
                    save(pred_name_of(item["rgb_relative_path"]), pred)
            valid = [j for j, item in enumerate(group) if has_valid_pixels(item, preds.shape[1:])]
            if valid:                          # the group's frames in one call: depth_eval measures every image of a batch on its own
                measure([group[j] for j in valid], preds if len(valid) == len(group) else preds[valid])
    result = tracker.result()
    if output_dir is not None:
        text = ("Evaluation metrics:\n    of predictions: %s\n    on dataset: %s\n    with samples in: %s\n"
                % (output_dir if save_predictions else "(in memory)", dataset.disp_name, dataset.filename_ls_path))
        text += "min_depth = %s\nmax_depth = %s\n" % (dataset.min_depth, dataset.max_depth)
        text += _metric_table([list(result.keys()), list(result.values())])
        with open(os.path.join(output_dir, "eval_metrics-%s.txt" % alignment), "w") as f:
            f.write(text)
    return result


NORMAL_METRIC_NAMES = ("mean", "median", "rmse", "a1", "a2", "a3", "a4", "a5")
NORMAL_METRIC_HEADER = "mean median rmse 5 7.5 11.25 22.5 30"


def _normals4(t, name):
    """[B,3,H,W] or [3,H,W] device tensor -> fp32 [B,3,H,W] view (any strides: a permuted [H,W,3] array is read in place)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a device tensor" % name)
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError("%s: expected normals [B,3,H,W] or [3,H,W]; got shape %s" % (name, tuple(t.shape)))
    return t if t.dtype == torch.float32 else t.float()


def _normal_mask(mask, B, H, W):
    """[B,1,H,W] / [B,H,W] / [H,W] bool or uint8 -> uint8 [B,H,W] view (None stays None: every pixel counts)"""
    if mask is None:
        return None
    if mask.dtype not in (torch.bool, torch.uint8):
        raise TypeError("mask must be bool or uint8, got %s" % mask.dtype)
    if mask.dim() == 4:
        if mask.shape[1] != 1:
            raise ValueError("mask: expected [B,1,H,W]; got shape %s" % (tuple(mask.shape),))
        mask = mask[:, 0]
    if mask.dim() == 2:
        mask = mask.unsqueeze(0)
    if tuple(mask.shape) != (B, H, W):
        raise ValueError("mask shape %s does not match the normals' %s" % (tuple(mask.shape), (B, H, W)))
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _check_pair(pred, gt):
    pred, gt = _normals4(pred, "pred"), _normals4(gt, "gt")
    if pred.shape != gt.shape:
        raise ValueError("pred %s and gt %s differ in shape" % (tuple(pred.shape), tuple(gt.shape)))
    return pred, gt


@torch.no_grad()
@ops.tensor_scoped
def normal_error(pred, gt):
    """utils.py:150-158 compute_normal_error: acos(clamp(cosine_similarity(pred, gt, dim=1), -1, 1)) * 180 / pi -> [B,1,H,W] fp32 degrees"""
    pred, gt = _check_pair(pred, gt)
    B, _, H, W = pred.shape
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=pred.device)
    totals = torch.zeros((9,), dtype=torch.int64, device=pred.device)
    ws, nws = ops.normal_eval_workspace(pred.device)
    ops.normal_eval_update(pred, gt, None, out, 0, totals, ws, nws)
    return out


@torch.no_grad()
@ops.tensor_scoped
def normal_metrics(pred, gt, mask=None):
    """compute_normal_metrics(compute_normal_error(pred, gt)[mask]) (utils.py:150-178) -> dict (NORMAL_METRIC_NAMES + "n"); None when no pixel is valid"""
    acc = NormalMetricAccumulator()
    acc.update(pred, gt, mask)
    return acc.result()


class NormalMetricAccumulator:
    """DSINE/projects/dsine/test.py:104-133 on the device: update() per image (batch) appends the errors of its valid pixels — to a dense buffer that
    doubles when full, in the reference's order — and adds its totals on the device; result_tensor() finalizes (exact median) without a host read.
    The host knows how many errors each update writes (B * H * W), so nothing is read back to grow the buffer; H x W may change between updates."""

    def __init__(self, device=None, capacity=0):
        self._device = torch.device(device) if device is not None else None
        self._cap0 = int(capacity)
        self._err = None
        self._written = 0
        self._totals = None
        self._ws = None

    def _ensure(self, device, need):
        if self._totals is None:
            self._device = device
            self._totals = torch.zeros((9,), dtype=torch.int64, device=device)
            self._ws, self._nws = ops.normal_eval_workspace(device)
        elif device != self._totals.device:
            raise RuntimeError("NormalMetricAccumulator lives on %s, got a tensor on %s" % (self._totals.device, device))
        cap = 0 if self._err is None else self._err.numel()
        if self._written + need > cap:
            new = torch.empty((max(2 * cap, self._written + need, self._cap0),), dtype=torch.float32, device=device)
            if self._written:
                new[:self._written].copy_(self._err[:self._written])
            self._err = new

    def reset(self):
        """forget every update (buffer and workspace are kept); capturable"""
        self._written = 0
        if self._totals is not None:
            self._totals.zero_()

    @torch.no_grad()
    @ops.tensor_scoped
    def update(self, pred, gt, mask=None):
        """pred, gt: [B,3,H,W] or [3,H,W] device tensors (any strides); mask: [B,1,H,W] / [B,H,W] / [H,W] bool or uint8, None = all valid.
        No host synchronisation."""
        pred, gt = _check_pair(pred, gt)
        B, _, H, W = pred.shape
        mask = _normal_mask(mask, B, H, W)
        n = B * H * W
        self._ensure(pred.device, n)
        ops.normal_eval_update(pred, gt, mask, self._err, self._written, self._totals, self._ws, self._nws)
        self._written += n

    @property
    def pixels(self):
        """pixels seen so far (valid or not): the number of entries of the error buffer in use"""
        return self._written

    def result_tensor(self):
        """fp64 [9] device tensor: mean, median, rmse, a1..a5, n (NaN metrics when n == 0); no host read"""
        if self._totals is None:
            dev = self._device if self._device is not None else torch.device("cuda", torch.cuda.current_device())
            self._ensure(dev, 0)
        with ops.on_device_of(self._totals):
            return ops.normal_eval_finalize(self._err, self._written, self._totals, self._ws, self._nws)

    def result(self):
        """dict of python floats (NORMAL_METRIC_NAMES) plus "n"; None when no valid pixel was seen (test.py's "No normal errors" branch)"""
        r = self.result_tensor().cpu().tolist()
        if r[8] == 0:
            return None
        out = dict(zip(NORMAL_METRIC_NAMES, r[:8]))
        out["n"] = int(r[8])
        return out

    def errors(self):
        """1-D fp32 device tensor of the valid pixels' errors in update order: the reference's total_normal_errors"""
        if self._err is None:
            return torch.empty((0,), dtype=torch.float32, device=self._device)
        e = self._err[:self._written]
        return e[e != float("inf")]


def format_normal_metrics(m):
    """the header line and the "%.3f" x 8 line test.py:117-120 prints (and writes to metrics.txt, :126-129)"""
    return NORMAL_METRIC_HEADER + "\n" + "%.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f" % tuple(m[k] for k in NORMAL_METRIC_NAMES)


def normal_metrics_text(m, iterations):
    """the four lines test.py:126-132 writes to metrics.txt"""
    return "Normal Estimation Metrics:\nMetrics at iteration %d\n%s\n" % (iterations, format_normal_metrics(m))


def evaluate_normal_benchmark(pipe, dataset, output_dir=None, domain=None, predict_batch_size=None, **pipe_kwargs):
    """DSINE/projects/dsine/test.py:40-133 over one normal_eval_data.NormalBenchmarkDataset: per sample, `pipe(PIL image, **pipe_kwargs).normal_np` —
    the image is the RE-QUANTISED one of test.py:59-68 (the dataset's img_u8), so any callable with the reference's signature works — is measured
    against the ground truth over its valid pixels on the device (NormalMetricAccumulator: the errors of all images are pooled, then the metrics
    are taken, as the reference does).  normal_np may be [3,H,W] (Marigold) or [H,W,3] (GeoWizard).  A DepthNormalEstimationPipeline is also given
    `domain` (None: the dataset's, test.py:47-53).  Returns the metrics dict (evaluate.NORMAL_METRIC_NAMES and "n"), or None with a warning when no
    pixel is valid anywhere.  output_dir: <output_dir>/test/<dataset_name>/metrics.txt as test.py:123-132 writes it.
    predict_batch_size: None — the loop above; an integer >= 1 — consecutive frames of one shape go, up to predict_batch_size at a time, through
    `pipe.predict_batch(uint8 [B,3,H,W] device tensor of the re-quantised images, **pipe_kwargs)` (its keywords, not `__call__`'s; a MarigoldPipeline needs
    normals=True among them) and the planar fp32 [B,3,H,W] device tensor it returns — the second of a (depth, normals) pair — is pooled as it is.  (A `batch_size` among the keywords is, as before, the pipeline's own.)"""
    import os
    import warnings

    import numpy as np
    from PIL import Image

    from .pipeline import DepthNormalEstimationPipeline
    if isinstance(pipe, DepthNormalEstimationPipeline):
        pipe_kwargs = dict(pipe_kwargs, domain=domain if domain is not None else dataset.domain)
    predict_batch_size = _batched_pipe(pipe, predict_batch_size, "evaluate_normal_benchmark")
    acc = NormalMetricAccumulator()
    iterations = 0
    items = (dataset[i] for i in range(len(dataset)))

    def frame_by_frame():
        for item in items:
            name = "%s/%s/%s" % (item["dataset_name"], item["scene_name"], item["img_name"])
            gt, mask = item["normal"], item["normal_mask"]
            image = Image.fromarray(item["img_u8"].permute(1, 2, 0).contiguous().cpu().numpy())
            pred = np.asarray(pipe(image, **pipe_kwargs).normal_np)
            H, W = gt.shape[-2:]
            if pred.shape == (3, H, W):
                p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32))
            elif pred.shape == (H, W, 3):
                p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)).permute(2, 0, 1)          # test.py:84: a view, read in place
            else:
                raise ValueError("%s: prediction %s matches neither [3,%d,%d] nor [%d,%d,3], the ground truth's shape" % (name, tuple(pred.shape), H, W, H, W))
            yield p, gt, mask, 1

    def in_batches():
        for group in _batches(((tuple(item["img_u8"].shape), item) for item in items), predict_batch_size):
            preds = pipe.predict_batch(torch.stack([item["img_u8"] for item in group]), **pipe_kwargs)
            preds = preds[1] if isinstance(preds, tuple) else preds
            gt, mask = torch.stack([item["normal"] for item in group]), torch.stack([item["normal_mask"] for item in group])
            if not isinstance(preds, torch.Tensor) or tuple(preds.shape) != tuple(gt.shape):
                raise ValueError("%s/%s/%s: predict_batch returned %s, the ground truth of its %d frames is %s"
                                 % (group[0]["dataset_name"], group[0]["scene_name"], group[0]["img_name"],
                                    tuple(preds.shape) if isinstance(preds, torch.Tensor) else type(preds).__name__, len(group), tuple(gt.shape)))
            yield preds, gt, mask, len(group)          # the errors of a batch are pooled image after image: the order of the loop

    for p, gt, mask, frames in (frame_by_frame() if predict_batch_size is None else in_batches()):
        with ops.on_device_of(gt):
            acc.update(p.to(gt.device), gt, mask)
        iterations += frames
    result = acc.result() if iterations else None
    if result is None:
        warnings.warn("evaluate_normal_benchmark: no valid ground-truth pixel in %s (%d samples); no metrics" % (dataset.dataset_name, iterations))
        return None
    if output_dir is not None:
        path = os.path.join(output_dir, "test", dataset.dataset_name, "metrics.txt")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(normal_metrics_text(result, iterations))
    return result
