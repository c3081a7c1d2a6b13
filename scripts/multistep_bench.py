"""Multi-step ensembled inference, the protocol of `MarigoldPipeline.__call__`'s defaults: 10 denoising steps x 10 ensemble members, Gaussian start, one 576 x 768
image (native resolution, processing_res = 0), fp16, full-size synthetic-weight models.  Two routes on ONE pipeline, alternating within a repeat:

  eager   `enable_hip_graphs(False)`: the host-driven loop — ten stacked copies through the VAE encoder, `scheduler.step` and the re-assembly of the UNet input per
          step, every library call launched from the host.  This is the baseline: the code path the fused loop leaves unchanged.
  graphs  `enable_hip_graphs(True)`: `_LatentPipeline._denoise` — one encode broadcast into ten rows, a head graph, ONE step graph replayed ten times with the DDIM
          update fused in (`ops.ddim_step_`), a tail graph.

Columns: wall time per image (host clock around one `__call__`, which ends in the device-to-host copy of the prediction; median [min .. max] over the repeats,
after one warm-up call per route — for `graphs` that call captures) and library launches per image (calls into libe2eft the host layer made during one call:
`_lib.CALLS`; a replayed graph makes none).  Both routes draw from `DeviceNoise(seed)` restarted per call, so they see the same noise; the largest difference of the
two predictions over the largest value is printed with the table.

usage: python scripts/multistep_bench.py [--steps 10] [--ensemble 10] [--shape 576x768] [--repeats 5] [--out profiles/multistep_inference.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description="10 steps x 10 members of MarigoldPipeline.__call__: the host-driven loop against the captured fused loop")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ensemble", type=int, default=10)
    ap.add_argument("--shape", default="576x768", help="HxW of the image")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=19)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multistep_inference.txt"))
    args = ap.parse_args(argv)
    import numpy as np
    import torch

    from diffusion_e2e_ft_amd import _lib
    from diffusion_e2e_ft_amd import build as B
    from diffusion_e2e_ft_amd.noise import DeviceNoise
    from predict_batch_bench import build
    if not torch.cuda.is_available():
        raise RuntimeError("multistep_bench needs a GPU: there is no CPU fallback")
    dev = torch.device("cuda:0")
    H, W = (int(v) for v in args.shape.split("x"))
    pipe = build("marigold", dev, torch.float16)
    img = torch.randint(0, 256, (3, H, W), generator=torch.Generator().manual_seed(H * W), dtype=torch.uint8).to(dev)
    kw = dict(denoising_steps=args.steps, ensemble_size=args.ensemble, processing_res=0, match_input_res=True, color_map=None, show_progress_bar=False,
              noise="gaussian")

    cache = pipe.enable_hip_graphs(True)._graphs      # ONE graph cache for the whole run: switching the route off and on again keeps what was captured

    def call(graphs):
        pipe._graphs = cache if graphs else None
        torch.cuda.synchronize()
        n0, t0 = _lib.CALLS[0], time.perf_counter()
        out = pipe(img, generator=DeviceNoise(args.seed), **kw).depth_np
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return out, dt, _lib.CALLS[0] - n0

    routes = (("eager", False), ("graphs", True))
    first = {name: call(g) for name, g in routes}          # warm-up: packed weights, code objects; `graphs` captures here
    times, launches, outs = {n: [] for n, _ in routes}, {}, {}
    for _ in range(args.repeats):
        for name, g in routes:
            outs[name], dt, launches[name] = call(g)
            times[name].append(dt)
    gap = float(np.abs(outs["graphs"].astype(np.float64) - outs["eager"]).max() / np.abs(outs["eager"]).max())
    lines = ["MarigoldPipeline.__call__, %d steps x %d members, gaussian (DeviceNoise), %d x %d, fp16, full-size synthetic weights, %d repeats (routes alternate), "
             "library build %s, %s" % (args.steps, args.ensemble, H, W, args.repeats, B.built_id(), torch.cuda.get_device_name(0)),
             "wall time: host clock around one call (ends in the copy of the prediction to the host); median [min .. max]",
             "",
             "  %-7s %-34s %s" % ("route", "wall time per image (s)", "library launches per image")]
    base = statistics.median(times["eager"])
    record = {"steps": args.steps, "ensemble": args.ensemble, "shape": [H, W], "repeats": args.repeats, "max_rel_diff": gap, "routes": {}}
    for name, _ in routes:
        ts = sorted(times[name])
        med = statistics.median(ts)
        lines.append("  %-7s %7.3f  [%7.3f .. %7.3f]  x%.2f     %d   (first call, warm-up / capture: %.3f s, %d)"
                     % (name, med, ts[0], ts[-1], base / med, launches[name], first[name][1], first[name][2]))
        record["routes"][name] = {"median_s": med, "min_s": ts[0], "max_s": ts[-1], "library_launches": launches[name], "first_call_s": first[name][1]}
    lines.append("")
    lines.append("max |graphs - eager| / max |eager| of the ensembled depth: %.3e" % gap)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps(record))


if __name__ == "__main__":
    main()
