"""Zero-shot depth evaluation on one benchmark (NYUv2, KITTI, ETH3D, ScanNet, DIODE): the reference's Marigold/infer.py + Marigold/eval.py in one
run on the GPU — the pipeline's __call__, the ground-truth preparation (eval_data.py, csrc/evalprep.hip) and the metrics (evaluate.depth_metrics)
all on the device, without the .npy round trip between the two scripts (--save_predictions writes the files anyway, where infer.py would).
Defaults follow the reference's protocol for the E2E-FT models: native resolution, one step, no ensembling, zero noise, seed 1234.

usage: python scripts/eval_depth.py --checkpoint <diffusers-format dir> --dataset data_nyu_test --base_data_dir data/eval
                                    --filenames data_split/nyu/labeled/filename_list_test.txt --output_dir output/nyu_test
       (--dataset_config <yaml> instead of --dataset for a configuration file in the reference's format)
       --batch_size N: up to N consecutive frames of one shape per pipe.predict_batch call, device tensors from the dataset to the metrics; the same files"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DATASETS = ("data_nyu_test", "data_kitti_eigen_test", "data_eth3d", "data_scannet_val", "data_diode_all")      # eval_data.BENCHMARKS


def parse(argv=None):
    ap = argparse.ArgumentParser(description="Depth benchmark evaluation (infer + eval in one pass on the device).")
    ap.add_argument("--checkpoint", required=True, help="diffusers-format checkpoint directory (unet/, vae/, scheduler/, text_encoder/)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--dataset", choices=DATASETS, help="one of the five benchmark configurations")
    src.add_argument("--dataset_config", help="dataset YAML file in the reference's format (needs PyYAML)")
    ap.add_argument("--base_data_dir", required=True, help="directory the configuration's `dir` is relative to")
    ap.add_argument("--filenames", default=None, help="filename list (required with --dataset; overrides the YAML file's entry)")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--denoise_steps", type=int, default=1)
    ap.add_argument("--ensemble_size", type=int, default=1)
    ap.add_argument("--processing_res", type=int, default=0, help="0: the input's resolution")
    ap.add_argument("--alignment", choices=["least_square", "least_square_disparity"], default="least_square")
    ap.add_argument("--alignment_max_res", type=int, default=None)
    ap.add_argument("--noise", choices=["gaussian", "pyramid", "zeros"], default="zeros")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--half_precision", "--fp16", action="store_true")
    ap.add_argument("--save_predictions", action="store_true", help="also write the .npy predictions under --output_dir")
    ap.add_argument("--batch_size", type=int, default=None, help="predict up to N consecutive frames of one shape per call (pipe.predict_batch, device tensors "
                                                                 "end to end); default: one pipe.__call__ per frame")
    args = ap.parse_args(argv)
    if args.dataset and not args.filenames:
        ap.error("--dataset needs --filenames (the benchmark's filename list)")
    if args.batch_size is not None and args.batch_size < 1:
        ap.error("--batch_size needs an integer >= 1")
    if args.batch_size is not None and args.ensemble_size != 1:
        ap.error("--batch_size predicts without ensembling: leave --ensemble_size at 1")
    return args


def main(argv=None):
    args = parse(argv)
    import random

    import numpy as np
    import torch

    from diffusion_e2e_ft_amd import eval_data, evaluate
    from diffusion_e2e_ft_amd.pipeline import MarigoldPipeline
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if not torch.cuda.is_available():
        raise RuntimeError("eval_depth needs a GPU: there is no CPU fallback")
    torch.cuda.manual_seed_all(args.seed)
    cfg = eval_data.BENCHMARKS[args.dataset] if args.dataset else args.dataset_config
    dataset = eval_data.get_dataset(cfg, base_data_dir=args.base_data_dir, mode=eval_data.DatasetMode.EVAL, filenames=args.filenames)
    dtype = torch.float16 if args.half_precision else torch.float32
    pipe = MarigoldPipeline.from_pretrained(args.checkpoint, variant="fp16" if args.half_precision else None, torch_dtype=dtype).to("cuda", dtype)
    pipe.unet.eval()
    kw = dict(denoising_steps=args.denoise_steps, processing_res=args.processing_res, match_input_res=True, resample_method="bilinear", noise=args.noise)
    if args.batch_size is None:      # __call__'s further keywords (batch_size here is its own: the ensemble members per pass)
        kw.update(ensemble_size=args.ensemble_size, batch_size=0, color_map=None, show_progress_bar=False)
    result = evaluate.evaluate_depth_benchmark(pipe, dataset, alignment=args.alignment, alignment_max_res=args.alignment_max_res, output_dir=args.output_dir,
                                               save_predictions=args.save_predictions, predict_batch_size=args.batch_size, **kw)
    print("%s (%d samples, alignment %s)" % (dataset.disp_name, len(dataset), args.alignment))
    for k, v in result.items():
        print("  %-28s %.6f" % (k, v))
    return result


if __name__ == "__main__":
    main()
