"""Time the depth-to-normal translator (csrc/d2nt.hip, e2eft_depth_to_normals) on B x H x W Virtual KITTI-like depth (default 64 x 375 x 1242) for each
output format with refinement on (d2nt_v3) and off (d2nt_v2), with device events; writes profiles/d2nt_bench.json and prints it.
  effective GB/s  over the bytes the pass must move: 4 B of depth in + 12 (fp32), 6 (uint16) or 3 (uint8) B out per pixel; share of the 8.0 TB/s
                  HBM3E peak (MI355X_MICROARCH: 6.29 TB/s measured for a float4 copy)
  host            the numpy restatement (tests/d2nt_ref.py: the reference's arithmetic, with its filter2D stand-in, NOT OpenCV) per image, on this host
usage: python scripts/d2nt_bench.py [B=64] [H=375] [W=1242] [host_images=2]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import d2nt_ref
from diffusion_e2e_ft_amd import _lib, ops

HBM_PEAK = 8.0e12
a = [int(float(v)) for v in sys.argv[1:]]
B, H, W, NH = (a + [64, 375, 1242, 2][len(a):])[:4]
dev = torch.device("cuda")
rng = np.random.default_rng(0)
cm = np.stack([d2nt_ref.vkitti_like_depth_cm(rng, H, W, sky=b % 2 == 0) for b in range(B)])
depth = torch.from_numpy(d2nt_ref.cm_to_metres(cm)).to(dev)
K = torch.tensor(d2nt_ref.VKITTI_K, dtype=torch.float32, device=dev)[None].expand(B, 4).contiguous()


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters   # ms


rows = []
px = B * H * W
for fmt, ob in (("f32", 12), ("u16", 6), ("u8", 3)):
    for refine in (True, False):
        out = ops.depth_to_normals(depth, K, refine=refine, out_format=fmt, depth_scale=100.0)
        ms = timeit(lambda: ops.depth_to_normals(depth, K, refine=refine, out_format=fmt, depth_scale=100.0, out=out), 50)
        gbs = px * (4 + ob) / (ms * 1e-3) / 1e9
        rows.append({"out_format": fmt, "refine": refine, "ms": round(ms, 4), "bytes_per_pixel": 4 + ob, "effective_GBps": round(gbs, 1),
                     "hbm_peak_share": round(gbs * 1e9 / HBM_PEAK, 3), "us_per_image": round(ms * 1e3 / B, 2)})

host = []
for b in range(min(NH, B)):
    t0 = time.perf_counter()
    d2nt_ref.depth_to_normals(d2nt_ref.cm_to_metres(cm[b]), d2nt_ref.VKITTI_K, True)
    host.append(time.perf_counter() - t0)
host_ms = 1e3 * float(np.median(host))
v3u16 = next(r for r in rows if r["out_format"] == "u16" and r["refine"])
res = {"bench": "d2nt", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(), "shape": [B, H, W], "kernel": rows,
       "host_numpy_ms_per_image": round(host_ms, 1), "host_what": "tests/d2nt_ref.py numpy restatement (filter2D stand-in, not OpenCV), d2nt_v3, one thread",
       "speedup_v3_u16_vs_host_per_image": round(host_ms / (v3u16["ms"] / B), 1)}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "d2nt_bench.json"), "w") as f:
    f.write(json.dumps(res) + "\n")
print(json.dumps(res))
