"""Time the GeoWizard trainer's timestep-weighted multi-resolution noise (GeoWizard/geowizard/training/train_depth_normal.py:286-296, called at :658-659) at the
recipe's shape: 2 images of 480 x 640 per GPU, fp32, i.e. a [4,4,60,80] latent.  Writes profiles/geowizard_pyramid_noise.txt (stamped with the build id) and prints it.

  torch    the reference's formulation written with torch ops on device tensors: `torch.randn_like`, then per level one `np.random.random()` draw, a
           `torch.randn` of the level's size, `nn.Upsample(bilinear)`, the `timesteps / 1000 * discount ** i` weight, and `.std()` at the end
  kernel   noise.geowizard_pyramid_noise_into(xin[..., 4:], DeviceNoise, timesteps): e2eft_pyramid_noise_weighted straight into the noise channels of the UNet input
Both routes draw their level sizes from numpy's global stream per call, as the reference does; the stream is re-seeded before every measurement round so that both
see the same sequence of sizes.  Columns as scripts/diffusion_objective_bench.py: device_ms (events around one call, median of --repeats), wall_ms, enqueue_ms,
launches (torch.profiler), synchronises (torch.cuda.set_sync_debug_mode("error")).  A record, not a pass/fail bar.
usage: python scripts/geowizard_pyramid_bench.py [--repeats 50] [--out PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from torch import nn
from diffusion_e2e_ft_amd import _lib, noise
from diffusion_objective_bench import measure, synchronises, launches

dev = torch.device("cuda")
SHAPE = (4, 4, 60, 80)
NP_SEED = 5


def routes():
    B, C, h, w = SHAPE
    x = torch.zeros(SHAPE, device=dev)
    timesteps = torch.randint(0, 1000, (B // 2,), device=dev).repeat(2)
    xin = torch.zeros((B, h, w, 2 * C), device=dev)
    gen = noise.DeviceNoise(1)

    def torch_route(discount=0.9, scale=1.5):
        u = nn.Upsample(size=(h, w), mode="bilinear")
        nz = torch.randn_like(x)
        for i in range(10):
            r = np.random.random() * scale + scale
            lh, lw = max(1, int(h / (r ** i))), max(1, int(w / (r ** i)))
            nz += u(torch.randn(B, C, lh, lw, device=dev)) * (timesteps[..., None, None, None] / 1000) * discount ** i
            if lh == 1 or lw == 1:
                break
        return nz / nz.std()

    def kernel_route():
        return noise.geowizard_pyramid_noise_into(xin[..., C:], gen, timesteps)

    return {"torch": torch_route, "kernel": kernel_route}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geowizard_pyramid_noise.txt"))
    a = ap.parse_args()
    r = routes()
    res = {"bench": "geowizard_pyramid_noise", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(), "shape": list(SHAPE), "dtype": "float32",
           "repeats": a.repeats, "np_seed": NP_SEED, "routes": {}}
    np.random.seed(NP_SEED)
    res["levels_of_the_first_call"] = noise.geowizard_pyramid_level_sizes(SHAPE[2], SHAPE[3])
    parts = {"torch": [], "kernel": []}
    for _ in range(2):                                   # alternate the routes so that a drift of the machine hits both
        for name in ("torch", "kernel"):
            np.random.seed(NP_SEED)
            parts[name].append(measure(r[name], a.repeats))
    for name in ("torch", "kernel"):
        row = min(parts[name], key=lambda m: m["device_ms"])
        row["rounds_device_ms"] = [m["device_ms"] for m in parts[name]]
        np.random.seed(NP_SEED)
        row["launches"] = launches(r[name])              # (of the second call after the seed: the profiler's warm-up call takes the first sizes)
        row["synchronises"] = synchronises(r[name])
        res["routes"][name] = row
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# scripts/geowizard_pyramid_bench.py, build id %s, %s\n" % (res["build_id"], res["device"]))
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
