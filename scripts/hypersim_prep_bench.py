"""Time the Hypersim preprocessing entry point (csrc/hypersimprep.hip, e2eft_hypersim_preprocess) on B x H x W raw frames (default 64 x 768 x 1024, fp16
colour and distance, int32 ids) with device events after warm-up, for both depth formats; writes profiles/hypersim_prep_bench.json and prints it.
  bytes the passes must move   6 histogram passes + (where a frame needs it) the min pass read colour + id (6 + 4 B per pixel each; an invalid pixel's
                  colour is not read), the apply pass reads colour + distance + id (12 B) and writes 3 B of rgb + 2 (uint16) or 4 (float32) B of depth;
                  share of the 8.0 TB/s HBM3E peak (MI355X_MICROARCH: 6.29 TB/s measured for a float4 copy)
  host            the numpy restatement (tests/hypersim_prep_ref.py: the reference's arithmetic) per frame, on this host, one thread
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/hypersim_prep_bench.py` run (profiles/README.md).
usage: python scripts/hypersim_prep_bench.py [B=64] [H=768] [W=1024] [host_frames=2]      (loader throughput for source="raw": scripts/loader_bench.py)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import hypersim_prep_ref as hpr
from diffusion_e2e_ft_amd import _lib, ops

HBM_PEAK = 8.0e12
a = [int(float(v)) for v in sys.argv[1:]]
B, H, W, NH = (a + [64, 768, 1024, 2][len(a):])[:4]
dev = torch.device("cuda")
rng = np.random.default_rng(0)
palette = (rng.random((4096, 3)) ** 2 * 4.0).astype(np.float16)
dpal = (0.4 + rng.random(4096) * 30.0).astype(np.float16)
frames = []
for b in range(min(B, 4)):          # four distinct frames, repeated: the kernels' work does not depend on the values beyond the valid share
    c, d, i = hpr.full_frame(np.roll(palette, b * 17, axis=0) * np.float16(0.5 + 0.25 * b), dpal, H, W)
    frames.append((c, d, i))
color = torch.from_numpy(np.stack([frames[b % len(frames)][0] for b in range(B)])).to(dev)
dist = torch.from_numpy(np.stack([frames[b % len(frames)][1] for b in range(B)])).to(dev)
ids = torch.from_numpy(np.stack([frames[b % len(frames)][2] for b in range(B)])).to(dev)


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
valid = float((ids != -1).float().mean())
for fmt, ob in (("u16", 2), ("f32", 4)):
    out = ops.hypersim_preprocess(color, dist, ids, depth_format=fmt)
    ms = timeit(lambda: ops.hypersim_preprocess(color, dist, ids, depth_format=fmt, out=out), 20)
    select_bytes = px * 6 * (4 + 6 * valid)
    apply_bytes = px * (12 + 3 + ob)
    gbs = (select_bytes + apply_bytes) / (ms * 1e-3) / 1e9
    rows.append({"depth_format": fmt, "ms": round(ms, 4), "us_per_frame": round(ms * 1e3 / B, 2), "select_GB": round(select_bytes / 1e9, 3),
                 "apply_GB": round(apply_bytes / 1e9, 3), "effective_GBps": round(gbs, 1), "hbm_peak_share": round(gbs * 1e9 / HBM_PEAK, 3)})
rec = out[2].cpu().numpy()

host = []
for b in range(min(NH, len(frames))):
    t0 = time.perf_counter()
    r = hpr.preprocess(*frames[b])
    host.append(time.perf_counter() - t0)
    assert np.array_equal(r["depth_f32"], out[1][b].cpu().numpy()) and hpr.check_u8(out[0][b].cpu().numpy(), r, "frame %d" % b) == 0
    hpr.check_record(rec[b], r["record"], "frame %d" % b)
host_ms = 1e3 * float(np.median(host)) if host else None
res = {"bench": "hypersim_prep", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(), "shape": [B, H, W], "inputs": "fp16 colour, fp16 distance, int32 ids",
       "valid_share": round(valid, 4), "kernel": rows, "host_numpy_ms_per_frame": None if host_ms is None else round(host_ms, 1),
       "host_what": "tests/hypersim_prep_ref.py numpy restatement (the reference's float64 arithmetic), one thread; outputs equal the kernel's on the timed frames",
       "speedup_u16_vs_host_per_frame": None if host_ms is None else round(host_ms / (rows[0]["ms"] / B), 1)}

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "hypersim_prep_bench.json"), "w") as f:
    f.write(json.dumps(res) + "\n")
print(json.dumps(res))
