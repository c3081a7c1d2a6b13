"""Zero-shot surface-normal evaluation (NYUv2, ScanNet, iBims-1, Sintel): the reference's DSINE/projects/dsine/test.py in benchmark mode on the GPU — the
image round trip and the ground-truth preparation (normal_eval_data.py, csrc/normalprep.hip), the pipeline's __call__ and the metrics
(evaluate.NormalMetricAccumulator) all on the device.  Takes an args file in the reference's format (experiments/normals/eval_args/*.txt: one
`--key value` per line) and writes <output_dir>/test/<dataset>/metrics.txt as test.py does.

Keys used: ckpt_path, model_type (marigold | geowizard), eval_data (all | nyuv2 | scannet | ibims | sintel), processing_res, seed, denoise_steps,
ensemble_size, noise, domain.  Other keys are ignored, with a note.  ckpt_path is a local diffusers-format directory.

usage: python scripts/eval_normals.py experiments/normals/eval_args/marigold_e2e_ft.txt --base_data_dir data --split_dir DSINE/data/datasets
                                      --output_dir output/normals [--ckpt_path <dir>]
       --base_data_dir   the folder that holds dsine_eval/
       --split_dir       a folder laid out as <dataset>/split/<split>.txt (DSINE/data/datasets of a reference checkout)
       --batch_size N    up to N consecutive frames of one shape per pipe.predict_batch call (needs ensemble_size 1); the same metrics.txt"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDER = ("nyuv2", "scannet", "ibims", "sintel")           # test.py:213-218
DEFAULTS = {"ckpt_path": None, "model_type": "marigold", "eval_data": "all", "processing_res": 0, "seed": None, "denoise_steps": 1,
            "ensemble_size": 1, "noise": "zeros", "domain": None}            # DSINE/projects/__init__.py's parser
_INT = ("processing_res", "seed", "denoise_steps", "ensemble_size")
_CHOICES = {"model_type": ("marigold", "geowizard"), "eval_data": ("all",) + ORDER, "noise": ("gaussian", "pyramid", "zeros"),
            "domain": ("indoor", "outdoor", "object")}


def parse_args_file(path):
    """an args file in the reference's format -> (settings dict over DEFAULTS, [ignored keys]); a line is `--key value`, `--flag` or empty"""
    with open(path) as f:
        tokens = [t for line in f for t in line.split()]
    out, ignored, i = dict(DEFAULTS), [], 0
    while i < len(tokens):
        t = tokens[i]
        if not t.startswith("--"):
            raise ValueError("%s: expected --key, got %r" % (path, t))
        key = t[2:]
        value = None
        if i + 1 < len(tokens) and not tokens[i + 1].startswith("--"):
            value = tokens[i + 1]
            i += 1
        i += 1
        if key not in DEFAULTS:
            ignored.append(key)
            continue
        if value is None:
            raise ValueError("%s: --%s needs a value" % (path, key))
        if key in _INT:
            value = int(value)
        if key in _CHOICES and value not in _CHOICES[key]:
            raise ValueError("%s: --%s %s (one of %s)" % (path, key, value, ", ".join(_CHOICES[key])))
        out[key] = value
    return out, ignored


def benchmarks_of(eval_data):
    return list(ORDER) if eval_data == "all" else [eval_data]


def parse(argv=None):
    ap = argparse.ArgumentParser(description="Surface-normal benchmark evaluation (the reference's DSINE test.py, benchmark mode, on the device).")
    ap.add_argument("args_file", help="args file in the reference's format, one `--key value` per line")
    ap.add_argument("--base_data_dir", required=True, help="the folder that holds dsine_eval/")
    ap.add_argument("--split_dir", required=True, help="folder laid out as <dataset>/split/<split>.txt")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--ckpt_path", default=None, help="overrides the args file's ckpt_path (a local diffusers-format directory)")
    ap.add_argument("--half_precision", "--fp16", action="store_true")
    ap.add_argument("--batch_size", type=int, default=None, help="predict up to N consecutive frames of one shape per call (pipe.predict_batch, device tensors "
                                                                 "end to end); default: one pipe.__call__ per frame")
    args = ap.parse_args(argv)
    if args.batch_size is not None and args.batch_size < 1:
        ap.error("--batch_size needs an integer >= 1")
    return args


def load_pipeline(cfg, dtype, device="cuda"):
    """test.py:167-203 with this package's classes"""
    import torch  # noqa: F401

    from diffusion_e2e_ft_amd.pipeline import DepthNormalEstimationPipeline, MarigoldPipeline
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    ckpt = cfg["ckpt_path"]
    if cfg["model_type"] == "marigold":
        scheduler = DDIMScheduler.from_pretrained(ckpt, timestep_spacing="trailing", subfolder="scheduler")
        return MarigoldPipeline.from_pretrained(ckpt, scheduler=scheduler, torch_dtype=dtype).to(device, dtype)
    from diffusion_e2e_ft_amd.clip import CLIPVisionModelWithProjection
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    unet, vae, enc = (cls.from_pretrained(ckpt, subfolder=sub, torch_dtype=dtype).to(device, dtype).eval()
                      for cls, sub in ((UNet2DConditionModel, "unet"), (AutoencoderKL, "vae"), (CLIPVisionModelWithProjection, "image_encoder")))
    return DepthNormalEstimationPipeline(unet, vae, DDIMScheduler.from_pretrained(ckpt, timestep_spacing="trailing", subfolder="scheduler"), image_encoder=enc)


def pipe_kwargs_of(cfg):
    """the arguments test.py:72-97 calls the model with"""
    kw = dict(denoising_steps=cfg["denoise_steps"], ensemble_size=cfg["ensemble_size"], processing_res=cfg["processing_res"], match_input_res=True,
              show_progress_bar=False, noise=cfg["noise"])
    if cfg["model_type"] == "geowizard":
        kw.update(color_map="Spectral")
    else:
        kw.update(color_map=None, resample_method="bilinear", batch_size=0, normals=True)
    return kw


def batch_kwargs_of(cfg):
    """the same settings as predict_batch takes them (--batch_size): no ensembling, no colouring, no progress bar"""
    if cfg["ensemble_size"] != 1:
        raise ValueError("--batch_size predicts without ensembling: the args file sets ensemble_size %d" % cfg["ensemble_size"])
    kw = dict(denoising_steps=cfg["denoise_steps"], processing_res=cfg["processing_res"], match_input_res=True, noise=cfg["noise"])
    if cfg["model_type"] != "geowizard":
        kw.update(resample_method="bilinear", normals=True)
    return kw


def main(argv=None, pipe=None):
    """pipe: a ready pipeline (or any callable with the reference's signature) instead of loading ckpt_path"""
    args = parse(argv)
    cfg, ignored = parse_args_file(args.args_file)
    if ignored:
        print("note: keys of %s that this script does not use: %s" % (args.args_file, ", ".join(ignored)))
    if args.ckpt_path:
        cfg["ckpt_path"] = args.ckpt_path
    import random
    import time

    import numpy as np
    import torch

    from diffusion_e2e_ft_amd import evaluate, normal_eval_data
    seed = cfg["seed"] if cfg["seed"] is not None else int(time.time())            # test.py:156-160
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if not torch.cuda.is_available():
        raise RuntimeError("eval_normals needs a GPU: there is no CPU fallback")
    torch.cuda.manual_seed_all(seed)
    if pipe is None:
        if not cfg["ckpt_path"]:
            raise ValueError("no ckpt_path: give one in the args file or with --ckpt_path")
        dtype = torch.float16 if args.half_precision else torch.float32
        pipe = load_pipeline(cfg, dtype)
        pipe.unet.eval()
    results = {}
    for name in benchmarks_of(cfg["eval_data"]):
        split = os.path.join(args.split_dir, name, "split", normal_eval_data.NORMAL_BENCHMARKS[name]["split"] + ".txt")
        dataset = normal_eval_data.NormalBenchmarkDataset(name, os.path.join(args.base_data_dir, "dsine_eval", name), split)
        kw = pipe_kwargs_of(cfg) if args.batch_size is None else batch_kwargs_of(cfg)
        res = evaluate.evaluate_normal_benchmark(pipe, dataset, output_dir=args.output_dir, domain=cfg["domain"], predict_batch_size=args.batch_size, **kw)
        results[name] = res
        print("%s (%d samples)" % (name, len(dataset)))
        print(evaluate.format_normal_metrics(res) if res is not None else "No normal errors to compute metrics.")
    return results


if __name__ == "__main__":
    main()
