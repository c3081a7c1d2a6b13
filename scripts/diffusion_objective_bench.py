"""Time the diffusion objective of the GeoWizard trainer (GeoWizard/geowizard/training/train_depth_normal.py without --e2e_ft) at the recipe's shape: 2 images of
480 x 640 per GPU, fp32, i.e. 4 rows of 4 x 60 x 80 latents.  Writes profiles/diffusion_objective.txt (stamped with the build id) and prints it.

  objective part   lines 606-609 and 651-717 WITHOUT the UNet (a fixed random tensor stands in for its prediction), forward and the gradient w.r.t. the prediction:
      torch      the trainer's own composition on device tensors: max_pool2d mask, randint, randn, add_noise / get_velocity (diffusers' formulas, the table
                 already on the device), the cat into the UNet input, `if latent_mask.any()`, `F.mse_loss(pred[latent_mask], target[latent_mask])`, backward
      fused      ops.latent_valid_mask, randint, noise.randn_into, two copy_scale + e2eft_diffusion_mix into the [4,60,80,8] input, e2eft_masked_mse_fwd / _bwd
  micro-step       training.geowizard_diffusion_loss + backward on the full-size GeoWizard UNet (seeded synthetic weights), and training.geowizard_e2e_ft_loss +
                   backward on the same build, for scale  (skipped with --no-step)
  device_ms        device events around one call, median of --repeats;   wall_ms: host clock around a call that ends in a synchronise;   enqueue_ms: the call alone
  launches         kernels per call counted by torch.profiler (None when the profiler is unavailable);   synchronises: whether the route raises under
                   torch.cuda.set_sync_debug_mode("error")
usage: python scripts/diffusion_objective_bench.py [--repeats 50] [--steps 3] [--no-step]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as TF
from diffusion_e2e_ft_amd import _lib, noise, ops, training, autograd as F
from diffusion_e2e_ft_amd.scheduler import DDPMScheduler

dev = torch.device("cuda")
B, H, W, C = 2, 480, 640, 4
h, w = H // 8, W // 8


def routes():
    g = torch.Generator(device=dev).manual_seed(0)
    val_mask = torch.rand((B, 1, H, W), generator=g, device=dev) > 0.001
    rgb_latents = torch.randn((B, C, h, w), generator=g, device=dev)
    geo_latents = torch.randn((2 * B, C, h, w), generator=g, device=dev)
    pred0 = torch.randn((2 * B, C, h, w), generator=g, device=dev)
    sched = DDPMScheduler()
    abar = sched.alphas_cumprod_on(dev)
    gen = noise.DeviceNoise(1)
    geo_nhwc, rgb_nhwc, pred_nhwc = (t.permute(0, 2, 3, 1).contiguous() for t in (geo_latents, rgb_latents, pred0))

    def torch_route():
        invalid_mask = ~val_mask
        latent_mask = ~torch.max_pool2d(invalid_mask.float(), 8, 8).bool()
        latent_mask = latent_mask.repeat((2, 4, 1, 1)).detach()
        timesteps = torch.randint(0, 1000, (B,), device=dev).repeat(2).long()
        nz = torch.randn_like(geo_latents)
        sa = (abar[timesteps] ** 0.5).flatten()[:, None, None, None]
        sb = ((1 - abar[timesteps]) ** 0.5).flatten()[:, None, None, None]
        noisy = sa * geo_latents + sb * nz
        target = sa * nz - sb * geo_latents
        unet_input = torch.cat((rgb_latents.repeat(2, 1, 1, 1), noisy), dim=1)
        pred = pred0.detach().requires_grad_(True)
        loss = torch.tensor(0.0, device=dev, requires_grad=True)
        if latent_mask.any():
            loss = TF.mse_loss(pred[latent_mask].float(), target[latent_mask].float(), reduction="mean")
        loss.backward()
        return loss, pred.grad, unet_input

    def fused_route():
        lm = ops.latent_valid_mask(val_mask)
        timesteps = torch.randint(0, 1000, (B,), device=dev).repeat(2)
        nz = noise.randn_into(torch.empty((2 * B, h, w, C), device=dev), gen)
        xin = torch.empty((2 * B, h, w, 2 * C), device=dev)
        ops.copy_scale(rgb_nhwc, xin[:B, ..., :C])
        ops.copy_scale(rgb_nhwc, xin[B:, ..., :C])
        ops.diffusion_mix_(geo_nhwc, nz, timesteps, abar, xin[..., C:])
        pred = pred_nhwc.permute(0, 3, 1, 2).detach().requires_grad_(True)
        loss = F.masked_mse(pred, geo_nhwc, nz, timesteps, abar, lm, "v_prediction")[0]
        loss.backward()
        return loss, pred.grad, xin

    return {"torch": torch_route, "fused": fused_route}


def measure(fn, repeats, warm=5):
    for _ in range(warm):
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


def synchronises(fn):
    """does one call make torch wait for the device (an `.any()` in an `if`, a boolean-mask index)?"""
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:
        return "not measured (%s)" % e
    try:
        fn()
        return False
    except RuntimeError as e:
        return "yes: %s" % str(e).splitlines()[0][:120]
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()


def launches(fn):
    """kernels one call puts on the device, by torch.profiler"""
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return len(names) or None
    except Exception:
        return None


def micro_steps(steps):
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    from diffusion_e2e_ft_amd.synth import init_synthetic_
    with torch.device(dev):
        unet = UNet2DConditionModel(in_channels=8, cross_attention_dim=768, class_embed_type="projection", projection_class_embeddings_input_dim=10, joint_attention=True)
        vae = AutoencoderKL()
    init_synthetic_(unet, seed=1234)
    init_synthetic_(vae, seed=4321)
    unet.train()
    vae.eval().requires_grad_(False)
    batch = training.synthetic_batch(B, H, W, dev, seed=0)
    batch["depth"] = batch["metric"].repeat(1, 3, 1, 1)
    emb = 0.5 * torch.randn((B, 1, 768), device=dev)
    gen = noise.DeviceNoise(2)

    def diffusion():
        training.geowizard_diffusion_loss(unet, vae, batch, emb, "indoor", noise_type="gaussian", generator=gen).backward()
        unet.zero_grad(set_to_none=True)

    def e2e_ft():
        training.geowizard_e2e_ft_loss(unet, vae, batch, emb, "indoor").backward()
        unet.zero_grad(set_to_none=True)

    out = {}
    for name, fn in (("diffusion_micro_step", diffusion), ("e2e_ft_micro_step", e2e_ft), ("diffusion_micro_step_again", diffusion)):
        out[name] = measure(fn, steps, warm=1)
        out[name]["synchronises"] = synchronises(fn)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    r = routes()
    res = {"bench": "diffusion_objective", "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(), "shape": [2 * B, C, h, w], "dtype": "float32",
           "repeats": a.repeats, "objective_part": {}}
    parts = {"torch": [], "fused": []}
    for _ in range(2):                                   # alternate the routes so that a drift of the machine hits both
        for name in ("torch", "fused"):
            parts[name].append(measure(r[name], a.repeats))
    for name in ("torch", "fused"):
        row = min(parts[name], key=lambda m: m["device_ms"])
        row["rounds_device_ms"] = [m["device_ms"] for m in parts[name]]
        row["launches"] = launches(r[name])
        row["synchronises"] = synchronises(r[name])
        res["objective_part"][name] = row
    path = os.path.join(ROOT, "profiles", "diffusion_objective.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)

    def write():
        with open(path, "w") as f:
            f.write("# scripts/diffusion_objective_bench.py, build id %s, %s\n" % (res["build_id"], res["device"]))
            f.write(json.dumps(res, indent=1) + "\n")

    write()
    if not a.no_step:
        res["micro_step"] = micro_steps(a.steps)
        write()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
