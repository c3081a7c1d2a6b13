"""Time the surface-normal evaluation (csrc/normaleval.hip) and DSINE's own path on the same data; prints one JSON line.
  update      e2eft_normal_eval_update on B x H x W fp32 normals + uint8 mask (default 64 x 480 x 640): effective GB/s over the bytes the pass must
              move (pred 12 + gt 12 + mask 1 + error 4 = 29 B / pixel)
  finalize    e2eft_normal_eval_finalize (exact median + record) over N errors (default 2e8, NYUv2's 654 x 480 x 640 before masking), 30 % masked
  dsine path  DSINE/projects/dsine/test.py:104-133 with utils.py:150-178 restated: per image compute_normal_error on the device, pred_error[mask]
              appended with torch.cat, then .cpu() and the numpy metrics — on the update's B images (what the host can take), against
              NormalMetricAccumulator on the same images
usage: python scripts/normal_eval_bench.py [B=64] [H=480] [W=640] [N=200000000]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from diffusion_e2e_ft_amd import _lib, evaluate, ops

THRESHOLDS = (5.0, 7.5, 11.25, 22.5, 30.0)
a = [int(float(v)) for v in sys.argv[1:]]
B, H, W, N = (a + [64, 480, 640, 200_000_000][len(a):])[:4]
dev = torch.device("cuda")
g = torch.Generator(device=dev).manual_seed(0)
gt = torch.nn.functional.normalize(torch.randn(B, 3, H, W, generator=g, device=dev), dim=1)
pred = torch.nn.functional.normalize(gt + 0.3 * torch.randn(B, 3, H, W, generator=g, device=dev), dim=1)
mask = torch.rand(B, H, W, generator=g, device=dev) > 0.3
mask_u8 = mask.view(torch.uint8)


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


ws, nws = ops.normal_eval_workspace(dev)
P = B * H * W
err = torch.empty(P, dtype=torch.float32, device=dev)
totals = torch.zeros(9, dtype=torch.int64, device=dev)
upd_ms = timeit(lambda: ops.normal_eval_update(pred, gt, mask_u8, err, 0, totals, ws, nws), 50)
upd_bytes = 29 * P
del err

# finalize at N: errors in [0, 60] deg, 30 % +inf (masked); the totals are computed from the same buffer with torch
big = torch.rand(N, generator=g, device=dev) * 60.0
big[torch.rand(N, generator=g, device=dev) < 0.3] = float("inf")
fin = big != float("inf")
n_valid = int(fin.sum())
host = np.zeros(9, dtype=np.int64)
host[0] = n_valid
for k, t in enumerate(THRESHOLDS):
    host[2 + k] = int((big < t).sum())
vals = big[fin].double()
host[7:9] = np.array([vals.sum().item(), (vals * vals).sum().item()], dtype=np.float64).view(np.int64)
kth = torch.kthvalue(big[fin], (n_valid + 1) // 2).values.item()        # lower middle element: checks the select at full size
del vals, fin
tot = torch.from_numpy(host).to(dev)
fin_ms = timeit(lambda: ops.normal_eval_finalize(big, N, tot, ws, nws), 20)
rec = ops.normal_eval_finalize(big, N, tot, ws, nws).cpu()
fin_median_ok = rec[1].item() == kth if n_valid % 2 else abs(rec[1].item() - kth) <= 1e-5 * kth
del big


def dsine_path():
    total = None
    for i in range(B):
        pe = torch.cosine_similarity(pred[i:i + 1], gt[i:i + 1], dim=1)
        pe = (torch.acos(torch.clamp(pe, min=-1.0, max=1.0)) * 180.0 / np.pi).unsqueeze(1)
        m = mask[i:i + 1].unsqueeze(1)
        total = pe[m] if total is None else torch.cat((total, pe[m]), dim=0)
    e = total.detach().cpu().numpy()
    n = e.shape[0]
    return {"mean": np.average(e), "median": np.median(e), "rmse": np.sqrt(np.sum(e * e) / n),
            **{"a%d" % (j + 1): 100.0 * (np.sum(e < t) / n) for j, t in enumerate(THRESHOLDS)}}


def ours():
    acc = evaluate.NormalMetricAccumulator(capacity=P)
    for i in range(B):
        acc.update(pred[i], gt[i], mask[i])
    return acc.result()


def wall(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3, r


ref_ms, ref = wall(dsine_path, 3)
our_ms, got = wall(ours, 5)
print(json.dumps({"bench": "normal_eval", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(),
                  "update_shape": [B, H, W], "update_ms": round(upd_ms, 4), "update_effective_gbps": round(upd_bytes / upd_ms / 1e6, 1),
                  "finalize_n": N, "finalize_valid": n_valid, "finalize_ms": round(fin_ms, 4), "finalize_median_checked": bool(fin_median_ok),
                  "dsine_path_images": B, "dsine_path_ms": round(ref_ms, 2), "accumulator_same_images_ms": round(our_ms, 2),
                  "median_equal_dsine_path": float(ref["median"]) == got["median"],
                  "max_abs_diff_shares_pct_dsine_path": max(abs(float(ref[k]) - got[k]) for k in ("a1", "a2", "a3", "a4", "a5")),
                  "max_rel_diff_mean_rmse": max(abs(float(ref[k]) - got[k]) / abs(got[k]) for k in ("mean", "rmse"))}))
