"""GeoWizard's default optimizer step launched from the host against the same step replayed from hipGraphs (`training.CapturedTrainStepAt`), at the
benchmark's training resolution: the diffusion objective (v-prediction) with `geowizard_pyramid` noise, the two parameter groups of `geowizard_param_groups` on a
`GroupedFlatAdamW`, and the EMA — micro-batches of 2 images at 576 x 576, 4 accumulation micro-steps, full-size synthetic-weight GeoWizard UNet and VAE.  Four
configurations in ONE process on ONE build: strict fp32 and bf16 compute over fp32 master weights, each with activation recompute off and on.

The scheme is scripts/train_graph_bench.py's.  Per configuration, on ONE model, ONE optimizer, ONE EMA and ONE noise generator (both routes are real optimizer steps,
so they alternate on the same weights):
  eager     the loop the captured step reproduces: per micro-step `geowizard_diffusion_loss(..., timesteps=generator)` + backward, then `optimizer.step()`,
            `zero_grad()`, `ema.step()`;
  memory    eager: two warm-up steps, then the peak of one step; captured: the eager first call and the capturing second call, then the peak of one replayed step.
            allocated / reserved GiB of torch's caching allocator;
  time      `--repeats` (>= 5) rounds of [one eager step, one captured step], host clock around a step that ends in a device synchronise; median [min .. max];
  launches  calls into libe2eft the host layer made during one step (`_lib.CALLS`).  A replayed step still makes a few: the words it fills before the replays
            (`e2eft_pyramid_table_set` once per micro-step; the draw, rate and decay words are torch fills and are not counted here).
The losses of the two routes are printed as a plausibility check only: they step the same weights one after the other, so they are not the same step.

usage: python scripts/train_graph_at_bench.py [--micro-batch 2] [--accum 4] [--res 576] [--repeats 5] [--configs fp32,fp32+ckpt,bf16,bf16+ckpt] [--tiny]
                                              [--out profiles/train_step_graph_at.txt]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GIB = 2.0 ** 30


def run_config(name, args, dev):
    import numpy as np
    import torch

    from diffusion_e2e_ft_amd import _lib, noise, training
    from diffusion_e2e_ft_amd.scheduler import DDPMScheduler
    from diffusion_e2e_ft_amd.synth import init_synthetic_
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    cdt = torch.float32 if name.startswith("fp32") else torch.bfloat16
    ckpt = name.endswith("+ckpt")
    ucfg = dict(in_channels=8, cross_attention_dim=768, class_embed_type="projection", projection_class_embeddings_input_dim=10, joint_attention=True)
    vcfg = {}
    if args.tiny:
        ucfg.update(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=96)
        vcfg.update(block_out_channels=(32, 64, 128, 128))
    with torch.device(dev):
        unet = UNet2DConditionModel(**ucfg)                    # fp32 master weights
        vae = AutoencoderKL(**vcfg).to(cdt)
    init_synthetic_(unet, seed=1234)
    init_synthetic_(vae, seed=4321)
    unet.train().set_compute_dtype(cdt)
    vae.eval().requires_grad_(False)
    if ckpt:
        unet.enable_gradient_checkpointing()
        vae.enable_gradient_checkpointing()
    opt = training.GroupedFlatAdamW(training.geowizard_param_groups(unet, 3e-5), betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=1.0)
    ema = training.EMAModel(opt.params, decay=0.9999)
    gen = noise.DeviceNoise(2024)
    np.random.seed(0)
    sched = DDPMScheduler()
    batches = []
    for i in range(args.accum):
        b = training.synthetic_batch(args.micro_batch, args.res, args.res, dev, seed=i, dtype=cdt)
        b["depth"] = b["metric"].repeat(1, 3, 1, 1)
        b["val_mask"] = torch.ones_like(b["val_mask"])         # (a 5 % random mask leaves no 8 x 8 cell whole: every latent cell selected instead)
        batches.append({k: b[k] for k in ("rgb", "depth", "normals", "val_mask")})
    embeds = [0.5 * torch.randn((args.micro_batch, 1, ucfg["cross_attention_dim"]), generator=torch.Generator(device=dev).manual_seed(i), device=dev)
              for i in range(args.accum)]
    lr_of = training.lr_lambda_for_world(20000, 100, num_processes=1)
    captured = training.CapturedTrainStepAt.diffusion(unet, vae, opt, "indoor", sched, "v_prediction", "geowizard_pyramid", generator=gen, accumulation=args.accum,
                                                      ema=ema)
    it = [0]

    def eager_step(lr_scale):
        n, total = len(batches), None
        for i, batch in enumerate(batches):
            opt.sync_grads = i == n - 1
            loss = training.geowizard_diffusion_loss(unet, vae, batch, embeds[i], "indoor", sched, "geowizard_pyramid", gen, timesteps=gen,
                                                     prediction_type="v_prediction")
            (loss / n).backward()
            total = loss.detach() if total is None else total + loss.detach()
        opt.step(lr_scale=lr_scale)
        opt.zero_grad()
        ema.step(opt.params)
        return total / n

    def step(route):
        """one optimizer step -> (seconds, library calls, loss tensor)"""
        torch.cuda.synchronize()
        n0, t0 = _lib.CALLS[0], time.perf_counter()
        if route == "eager":
            loss = eager_step(lr_of(it[0]))
        else:
            loss = captured(batches, lr_scale=lr_of(it[0]), imgs_embed=embeds)
        torch.cuda.synchronize()
        it[0] += 1
        return time.perf_counter() - t0, _lib.CALLS[0] - n0, loss

    def peak_of(route):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step(route)
        return torch.cuda.max_memory_allocated() / GIB, torch.cuda.max_memory_reserved() / GIB

    mem, first = {}, {}
    step("eager")
    step("eager")
    mem["eager"] = peak_of("eager")
    first["captured_eager_call"] = step("captured")[0]
    first["captured_capture_call"] = step("captured")[0]
    mem["captured"] = peak_of("captured")
    times, calls, loss = {"eager": [], "captured": []}, {}, {}
    for _ in range(args.repeats):
        for route in ("eager", "captured"):
            dt, calls[route], loss[route] = step(route)
            times[route].append(dt)
    for route in loss:
        if not torch.isfinite(loss[route]).all():
            raise RuntimeError("%s %s: non-finite loss" % (name, route))
    if opt.skipped_steps() or ema.optimization_step != it[0] or gen.draw != 2 * args.accum * it[0]:
        raise RuntimeError("%s: %d skipped steps, %d EMA steps and %d draws after %d optimizer steps" % (name, opt.skipped_steps(), ema.optimization_step, gen.draw, it[0]))
    rec = {"config": name, "entries": len(captured._entries), "first_calls_s": first, "routes": {}}
    for route in ("eager", "captured"):
        ts = sorted(times[route])
        rec["routes"][route] = {"median_s": statistics.median(ts), "min_s": ts[0], "max_s": ts[-1], "library_calls": calls[route],
                                "peak_allocated_gib": mem[route][0], "peak_reserved_gib": mem[route][1], "last_loss": float(loss[route])}
    del captured, opt, ema, unet, vae, batches, embeds
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser(description="GeoWizard's default step, eager against CapturedTrainStepAt: time, peak memory and library launches per optimizer step")
    ap.add_argument("--micro-batch", type=int, default=2)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--res", type=int, default=576)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--configs", default="fp32,fp32+ckpt,bf16,bf16+ckpt")
    ap.add_argument("--tiny", action="store_true", help="small models (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_graph_at.txt"))
    args = ap.parse_args(argv)
    if args.repeats < 5:
        raise SystemExit("--repeats: the median is taken over at least 5 steps")
    import torch

    from diffusion_e2e_ft_amd import build as B
    if not torch.cuda.is_available():
        raise RuntimeError("train_graph_at_bench needs a GPU: there is no CPU fallback")
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    names = [c for c in args.configs.split(",") if c]
    for c in names:
        if c not in ("fp32", "fp32+ckpt", "bf16", "bf16+ckpt"):
            raise SystemExit("unknown configuration %r" % c)
    recs = [run_config(c, args, dev) for c in names]
    lines = ["GeoWizard default optimizer step (diffusion objective, v-prediction, geowizard_pyramid noise, two parameter groups, EMA), %d micro-steps x %d images at "
             "%d x %d, %s synthetic-weight models, GroupedFlatAdamW (direct_grads), %d rounds of [eager, captured] on one model, library build %s, %s"
             % (args.accum, args.micro_batch, args.res, args.res, "TINY (rehearsal)" if args.tiny else "full-size", args.repeats, B.built_id(), torch.cuda.get_device_name(0)),
             "time: host clock around one step ending in a device synchronise, median [min .. max]; memory: peak of one step, allocated / reserved GiB; "
             "library launches: calls into libe2eft from the host per step (captured: the pyramid table of every micro-step)",
             "",
             "  %-10s %-9s %-36s %-22s %s" % ("config", "route", "step time (s)", "peak GiB alloc / resv", "library launches per step")]
    for r in recs:
        base = r["routes"]["eager"]["median_s"]
        for route in ("eager", "captured"):
            q = r["routes"][route]
            lines.append("  %-10s %-9s %7.4f  [%7.4f .. %7.4f]  x%.3f   %7.2f / %7.2f      %d"
                         % (r["config"], route, q["median_s"], q["min_s"], q["max_s"], base / q["median_s"], q["peak_allocated_gib"], q["peak_reserved_gib"],
                            q["library_calls"]))
        lines.append("  %-10s captured route's first call (eager) %.3f s, second call (capture + replay) %.3f s; last losses eager %.6f captured %.6f"
                     % ("", r["first_calls_s"]["captured_eager_call"], r["first_calls_s"]["captured_capture_call"], r["routes"]["eager"]["last_loss"],
                        r["routes"]["captured"]["last_loss"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps(recs))


if __name__ == "__main__":
    main()
