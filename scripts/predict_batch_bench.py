"""images/s of the two public prediction routes on the full-size synthetic-weight models in fp16, at 480 x 640 (NYUv2, ScanNet) and 352 x 1216 (KITTI's
benchmark crop), native resolution (processing_res = 0) as the evaluation protocol runs them:

  call      the reference's surface: `pipe(PIL image, ensemble_size=1, denoising_steps=1, noise="zeros", color_map=None)` once per image, numpy out
            (two forced synchronisations per image: the host range assert and .cpu().numpy())
  batch<B>  `pipe.predict_batch(uint8 [B,3,H,W] device tensor)`, B = 1, 2, 4, 8: device tensors in and out, no synchronisation inside

Each timed window is a host clock around --images images that ends in one device synchronise; the routes alternate within a repeat, --repeats repeats;
median, min and max over the repeats are reported.  The `call` route is the baseline: this file's change does not touch `__call__`.

`--profile ROUTE --images N` only issues N images through one route (after one warm-up unit) and synchronises once at the end.  Run it under
  rocprofv3 --hip-trace --memory-copy-trace --stats --output-format csv -d DIR -- python scripts/predict_batch_bench.py --profile ROUTE --images N
twice with two values of N: set-up (building the models, the warm-up) costs the same in both, so the difference of the two runs' counts over the difference
of N is the count per image.  `--summarise ROUTE DIR_N1 N1 DIR_N2 N2` prints that: synchronising HIP calls and device <-> host copies per image.

usage: python scripts/predict_batch_bench.py [--model marigold|geowizard] [--images 16] [--repeats 5] [--out profiles/predict_batch.txt]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((480, 640), (352, 1216))
BATCHES = (1, 2, 4, 8)
ROUTES = ("call",) + tuple("batch%d" % b for b in BATCHES)
SYNC_CALLS = ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMemcpyWithStream", "hipMemcpyDtoH", "hipMemcpyHtoD",
              "hipStreamWaitEvent")          # the last one does not block the host; listed so that its absence is on record
COPY_KINDS = ("MEMORY_COPY_HOST_TO_DEVICE", "MEMORY_COPY_DEVICE_TO_HOST", "MEMORY_COPY_DEVICE_TO_DEVICE")


def build(model, dev, dtype):
    import torch

    from diffusion_e2e_ft_amd.pipeline import DepthNormalEstimationPipeline, MarigoldPipeline
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    from diffusion_e2e_ft_amd.synth import init_synthetic_
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    geo = model == "geowizard"
    ucfg = dict(in_channels=8, cross_attention_dim=768, class_embed_type="projection", projection_class_embeddings_input_dim=10, joint_attention=True) if geo \
        else dict(in_channels=8)
    with torch.device(dev):
        unet = UNet2DConditionModel(**ucfg).to(dtype)
        vae = AutoencoderKL().to(dtype)
    init_synthetic_(unet, seed=1234)
    init_synthetic_(vae, seed=4321)
    if geo:
        from diffusion_e2e_ft_amd.clip import CLIPVisionModelWithProjection
        with torch.device(dev):
            enc = CLIPVisionModelWithProjection().to(dtype)
        init_synthetic_(enc, seed=2468)
        return DepthNormalEstimationPipeline(unet.eval(), vae.eval(), DDIMScheduler(), image_encoder=enc.eval())
    pipe = MarigoldPipeline(unet.eval(), vae.eval(), DDIMScheduler())
    g = torch.Generator(device=dev).manual_seed(0)
    pipe.empty_text_embed = (0.5 * torch.randn((1, 2, unet.config.cross_attention_dim), generator=g, device=dev)).to(dtype)
    return pipe


def routes(pipe, shape, n_images, dev):
    """{route: fn()} — each fn sends the same n_images seeded images of `shape` through its route and returns the last output (nothing is synchronised here)"""
    import torch
    from PIL import Image
    H, W = shape
    u8 = torch.randint(0, 256, (n_images, 3, H, W), generator=torch.Generator().manual_seed(H * W), dtype=torch.uint8)
    pil = [Image.fromarray(im.permute(1, 2, 0).contiguous().numpy()) for im in u8]
    u8_dev = u8.to(dev)
    call_kw = dict(ensemble_size=1, denoising_steps=1, noise="zeros", color_map=None, processing_res=0, match_input_res=True, show_progress_bar=False)

    def call():
        out = None
        for im in pil:
            out = pipe(im, **call_kw)
        return out

    def batch(B):
        def run():
            out = None
            for s in range(0, n_images, B):
                out = pipe.predict_batch(u8_dev[s:s + B], processing_res=0)
            return out
        return run

    table = {"call": call}
    table.update({"batch%d" % B: batch(B) for B in BATCHES if n_images % B == 0})
    return table


def measure(args):
    import torch

    from diffusion_e2e_ft_amd import build as B
    if not torch.cuda.is_available():
        raise RuntimeError("predict_batch_bench needs a GPU: there is no CPU fallback")
    dev = torch.device("cuda:0")
    pipe = build(args.model, dev, torch.float16)
    lines = ["%s, fp16, full-size synthetic weights, processing_res = 0, %d images per window, %d repeats (routes alternate within a repeat), library build %s, %s"
             % (args.model, args.images, args.repeats, B.built_id(), torch.cuda.get_device_name(0)),
             "window = host clock around the images, one device synchronise at its end; images/s: median [min .. max] over the repeats"]
    record = {"model": args.model, "images": args.images, "repeats": args.repeats, "shapes": {}}
    for shape in SHAPES:
        table = routes(pipe, shape, args.images, dev)
        for fn in table.values():              # warm up every route at this shape: weight packing, resampler tables, code objects
            fn()
        torch.cuda.synchronize()
        times = {r: [] for r in table}
        for _ in range(args.repeats):
            for r, fn in table.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[r].append(time.perf_counter() - t0)
        lines.append("")
        lines.append("%d x %d" % shape)
        base = statistics.median(args.images / t for t in times["call"])
        rec = {}
        for r, ts in times.items():
            rates = sorted(args.images / t for t in ts)
            med = statistics.median(rates)
            rec[r] = {"median": med, "min": rates[0], "max": rates[-1]}
            lines.append("  %-7s %7.2f images/s  [%7.2f .. %7.2f]   x%.2f of the call loop" % (r, med, rates[0], rates[-1], med / base))
        record["shapes"]["%dx%d" % shape] = rec
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)
    print(json.dumps(record))


def profile(args):
    import torch
    dev = torch.device("cuda:0")
    pipe = build(args.model, dev, torch.float16)
    shape = tuple(int(v) for v in args.shape.split("x"))
    unit = 1 if args.profile == "call" else int(args.profile[len("batch"):])
    routes(pipe, shape, unit, dev)[args.profile]()               # one warm-up unit
    torch.cuda.synchronize()
    routes(pipe, shape, args.images, dev)[args.profile]()
    torch.cuda.synchronize()
    print(json.dumps({"profiled": args.profile, "model": args.model, "shape": list(shape), "images": args.images, "warm_up_images": unit}))


def _stats(directory, suffix):
    """{name: calls} summed over the rocprofv3 --stats files *<suffix> below `directory` (none: an empty dict — rocprofv3 writes no file for a domain without records)"""
    out = {}
    for path in glob.glob(os.path.join(directory, "**", "*" + suffix), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                out[row["Name"]] = out.get(row["Name"], 0) + int(row["Calls"])
    return out


def summarise(route, d1, n1, d2, n2, out=None):
    n1, n2 = int(n1), int(n2)
    assert n2 > n1
    api1, api2 = _stats(d1, "hip_api_stats.csv"), _stats(d2, "hip_api_stats.csv")
    cp1, cp2 = _stats(d1, "memory_copy_stats.csv"), _stats(d2, "memory_copy_stats.csv")
    assert api1 and api2, "no hip_api_stats.csv below %s / %s" % (d1, d2)
    lines = ["route %-7s per image = (count at %d images - count at %d images) / %d" % (route, n2, n1, n2 - n1)]
    for name in SYNC_CALLS + tuple(sorted(k for k in set(api1) | set(api2) if "Memcpy" in k and k not in SYNC_CALLS)):
        if name in api1 or name in api2:
            lines.append("  %-34s %8.3f   (%d, %d)" % (name, (api2.get(name, 0) - api1.get(name, 0)) / (n2 - n1), api1.get(name, 0), api2.get(name, 0)))
    for name in COPY_KINDS:
        lines.append("  %-34s %8.3f   (%d, %d)" % (name, (cp2.get(name, 0) - cp1.get(name, 0)) / (n2 - n1), cp1.get(name, 0), cp2.get(name, 0)))
    l1, l2 = (sum(v for k, v in api.items() if "Launch" in k) for api in (api1, api2))
    lines.append("  %-34s %8.3f   (%d, %d)" % ("kernel launches (hip*Launch*)", (l2 - l1) / (n2 - n1), l1, l2))
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text)


def main(argv=None):
    ap = argparse.ArgumentParser(description="images/s of pipe.__call__ per image against pipe.predict_batch at batch 1, 2, 4, 8")
    ap.add_argument("--model", choices=["marigold", "geowizard"], default="marigold")
    ap.add_argument("--images", type=int, default=16, help="images per timed window (a multiple of 8 times every batch size)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the table to this file")
    ap.add_argument("--profile", choices=ROUTES, help="issue --images images through one route and synchronise once (run under rocprofv3)")
    ap.add_argument("--shape", default="480x640", help="--profile: HxW")
    ap.add_argument("--summarise", nargs=5, metavar=("ROUTE", "DIR_N1", "N1", "DIR_N2", "N2"), help="per-image counts from two rocprofv3 --stats runs")
    args = ap.parse_args(argv)
    if args.summarise:
        return summarise(*args.summarise, out=args.out)
    if args.profile:
        return profile(args)
    return measure(args)


if __name__ == "__main__":
    main()
