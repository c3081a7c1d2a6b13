"""Time the initial-latent noise of the multi-step pipelines / the `--noise_type` training settings, host route against device route, at
(8,4,96,96) fp16 and (32,4,72,72) fp32; writes profiles/noise_bench.json and prints it.

  host route    what `single_infer(noise="pyramid")` does without a DeviceNoise generator: `pipeline.pyramid_noise_like(rgb_latent).to(device)` (host RNG per
                level, one host-to-device copy per level, torch's upsample / std on the device) + the layout copy into channels 4:8 of the UNet input;
                for "gaussian": `torch.randn(..., device=...)` + the same layout copy.  This code is unchanged from the parent commit.
  device route  `noise.pyramid_noise_into / randn_into(xin[..., 4:], DeviceNoise)`: csrc/noise.hip straight into the input buffer.
  device_ms     device events around one call (median of `--repeats`)
  wall_ms       host clock around one call that ends in a device synchronise (median)
  enqueue_ms    host clock around the call alone, no synchronise (what the host spends before it can go on)
Python's `random` is re-seeded before every call so that both routes draw the same level sizes every time.

`--profile ROUTE --calls N` only issues N calls of one route (after one warm-up call) and synchronises once at the end: run it under
`rocprofv3 --hip-trace --kernel-trace --memory-copy-trace --stats` to count kernels, copies and synchronising API calls per call.
usage: python scripts/noise_bench.py [--repeats 50] | --profile device|host [--calls 20] [--kind pyramid|gaussian]"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from diffusion_e2e_ft_amd import _lib, noise, ops, pipeline

CASES = [((8, 4, 96, 96), torch.float16), ((32, 4, 72, 72), torch.float32)]
dev = torch.device("cuda")


def routes(shape, dtype, kind):
    B, C, h, w = shape
    rgb_latent = torch.zeros(shape, dtype=dtype, device=dev)
    xin = torch.zeros((B, h, w, 2 * C), dtype=dtype, device=dev)
    gen = noise.DeviceNoise(1)

    def host():
        random.seed(0)
        latent = pipeline.pyramid_noise_like(rgb_latent).to(dev) if kind == "pyramid" else torch.randn(shape, device=dev, dtype=dtype)
        ops.copy_scale(latent.permute(0, 2, 3, 1).contiguous(), xin[..., C:])

    def device():
        random.seed(0)
        noise.noise_into(kind, xin[..., C:], gen)

    return {"host": host, "device": device}


def measure(fn, repeats):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    dev_ms, wall_ms, enq_ms = [], [], []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        dev_ms.append(e0.elapsed_time(e1))
        wall_ms.append((t2 - t0) * 1e3)
        enq_ms.append((t1 - t0) * 1e3)
    med = statistics.median
    return {"device_ms": round(med(dev_ms), 4), "wall_ms": round(med(wall_ms), 4), "enqueue_ms": round(med(enq_ms), 4),
            "device_ms_min_max": [round(min(dev_ms), 4), round(max(dev_ms), 4)]}


def clocks():
    """current clocks as rocm-smi reports them (read only), for the record next to the numbers"""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        return [l.strip() for l in out.splitlines() if "clk" in l.lower()][:8]
    except Exception as e:
        return ["unavailable: %s" % e]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--profile", choices=["device", "host"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kind", choices=["pyramid", "gaussian"], default="pyramid")
    a = ap.parse_args()
    if a.profile:
        for shape, dtype in CASES:
            fn = routes(shape, dtype, a.kind)[a.profile]
            fn()
            for _ in range(a.calls):
                fn()
        torch.cuda.synchronize()
        print(json.dumps({"profiled": a.profile, "kind": a.kind, "calls_per_case": a.calls + 1, "cases": len(CASES)}))
        return
    rows = []
    for shape, dtype in CASES:
        for kind in ("pyramid", "gaussian"):
            r = routes(shape, dtype, kind)
            random.seed(0)
            row = {"shape": list(shape), "dtype": str(dtype).replace("torch.", ""), "kind": kind,
                   "levels": noise.pyramid_level_sizes(shape[2], shape[3]) if kind == "pyramid" else None}
            # alternate the routes (two rounds each) so that a drift of the machine hits both
            parts = {"host": [], "device": []}
            for _ in range(2):
                for name in ("host", "device"):
                    parts[name].append(measure(r[name], a.repeats))
            for name in ("host", "device"):
                row[name] = min(parts[name], key=lambda m: m["device_ms"])
                row[name + "_rounds_device_ms"] = [m["device_ms"] for m in parts[name]]
            rows.append(row)
    res = {"bench": "noise", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(), "repeats": a.repeats, "clocks_after": clocks(), "rows": rows}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "noise_bench.json"), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
