"""The flat AdamW update at the size of the full SD-v2 UNet: the existing single-group entry point (`e2eft_adamw_step_guarded`) against the grouped one
(`e2eft_adamw_step_groups`) with (a) one group over the whole buffer and (b) GeoWizard's two groups (everything | class embedding, laid out as
`training.GroupedFlatAdamW` lays them out).  All three move the same 28 bytes per element, so the expectation is "equal"; this script measures it.

One process, one build, one set of buffers.  `--rounds` rounds; in each round the three variants take turns (their order rotates from round to round) and each is
timed `--samples` times between two events on the stream (one entry-point call = the one-thread prepare launch + the update launch; the sum of squares is computed
once, outside).  Per variant: the median of every round, then the median over the rounds.  The yardstick is the existing kernel in the same run: the spread
(max - min) of ITS per-round medians is the margin the grouped forms get, and no more.

usage: python scripts/adamw_groups_bench.py [--rounds 7] [--samples 9] [--tiny] [--out profiles/adamw_groups.txt]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LR, MULT, B1, B2, EPS, WD = 3e-5, 10.0, 0.9, 0.999, 1e-8, 1e-2


def geowizard_layout(tiny=False):
    """(flat length, [range of group 0, range of group 1]) of GroupedFlatAdamW(geowizard_param_groups(unet, ...)) for the GeoWizard UNet, from the parameter shapes
    alone (the model is built on the meta device: no storage)"""
    import torch

    from diffusion_e2e_ft_amd.training import geowizard_param_groups
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    cfg = dict(in_channels=8, class_embed_type="projection", projection_class_embeddings_input_dim=10)
    if tiny:
        cfg.update(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4), cross_attention_dim=128)
    with torch.device("meta"):
        unet = UNet2DConditionModel(**cfg)
    sizes = [sum((p.numel() + 7) // 8 * 8 for p in g["params"]) for g in geowizard_param_groups(unet, LR, MULT)]
    return sum(sizes), [(0, sizes[0]), (sizes[0], sizes[0] + sizes[1])]


def main(argv=None):
    ap = argparse.ArgumentParser(description="e2eft_adamw_step_guarded against e2eft_adamw_step_groups at the flat size of the SD-v2 UNet")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--tiny", action="store_true", help="a small UNet's flat size (a rehearsal of the script, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_groups.txt"))
    args = ap.parse_args(argv)
    if args.rounds < 5 or args.samples < 5:
        raise SystemExit("--rounds / --samples: medians are taken over at least 5")
    import torch

    from diffusion_e2e_ft_amd import build as B
    from diffusion_e2e_ft_amd import ops
    if not torch.cuda.is_available():
        raise RuntimeError("adamw_groups_bench needs a GPU: there is no CPU fallback")
    dev = torch.device("cuda:0")
    n, (g0, g1) = geowizard_layout(args.tiny)
    gen = torch.Generator(device=dev).manual_seed(0)
    p = 0.05 * torch.randn(n, device=dev, generator=gen)
    g = 1e-3 * torch.randn(n, device=dev, generator=gen)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    state = torch.zeros(2, dtype=torch.int64, device=dev)
    coef4, coef_g = torch.zeros(4, device=dev), torch.zeros(2 + 2 * 2, device=dev)
    ss = ops.sumsq(g)
    one = ops.adamw_groups([(0, n, LR, B1, B2, EPS, WD)])
    two = ops.adamw_groups([(g0[0], g0[1], LR, B1, B2, EPS, WD), (g1[0], g1[1], LR * MULT, B1, B2, EPS, WD)])
    variants = {
        "guarded": lambda: ops.adamw_step_guarded_(p, g, m, v, LR, B1, B2, EPS, WD, state, coef4, ss, grad_scale=1.0, max_norm=1.0),
        "groups_1": lambda: ops.adamw_step_groups_(p, g, m, v, one, state, coef_g, ss, grad_scale=1.0, max_norm=1.0),
        "groups_2": lambda: ops.adamw_step_groups_(p, g, m, v, two, state, coef_g, ss, grad_scale=1.0, max_norm=1.0),
    }
    names = list(variants)
    for name in names:          # warm-up: code objects loaded, clocks up
        for _ in range(3):
            variants[name]()
    torch.cuda.synchronize()
    per_round = {name: [] for name in names}
    for r in range(args.rounds):
        for name in names[r % 3:] + names[:r % 3]:
            ts = []
            for _ in range(args.samples):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                variants[name]()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            per_round[name].append(statistics.median(ts))
    if not torch.isfinite(p).all() or int(state[1].item()) != 0:
        raise RuntimeError("the update went non-finite or skipped a step: not a measurement")
    med = {name: statistics.median(per_round[name]) for name in names}
    spread = max(per_round["guarded"]) - min(per_round["guarded"])
    gb = 28.0 * n / 1e9          # read p, g, m, v; write p, m, v
    lines = ["flat AdamW update, %d elements (%s GeoWizard UNet: group 0 = [%d, %d), class embedding = [%d, %d)), %.2f GB moved per update, %d rounds x %d samples,"
             % (n, "TINY (rehearsal)" if args.tiny else "full-size SD-v2", g0[0], g0[1], g1[0], g1[1], gb, args.rounds, args.samples),
             "library build %s, %s; one call = prepare launch + update launch, timed between two stream events" % (B.built_id(), torch.cuda.get_device_name(0)),
             "",
             "  %-44s %-12s %-10s %s" % ("entry point", "median (ms)", "GB/s", "per-round medians (ms)")]
    label = {"guarded": "e2eft_adamw_step_guarded (the yardstick)", "groups_1": "e2eft_adamw_step_groups, 1 group", "groups_2": "e2eft_adamw_step_groups, 2 groups (GeoWizard)"}
    for name in names:
        lines.append("  %-44s %-12.4f %-10.0f %s" % (label[name], med[name], gb / (med[name] * 1e-3), " ".join("%.4f" % t for t in per_round[name])))
    lines.append("")
    lines.append("  spread of the yardstick's own per-round medians (max - min): %.4f ms = the margin of the grouped forms" % spread)
    for name in names[1:]:
        d = med[name] - med["guarded"]
        lines.append("  %-44s %+.4f ms against the yardstick: %s" % (label[name], d, "within the margin" if d <= spread else "BEYOND the margin"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"n": n, "ranges": [g0, g1], "median_ms": med, "per_round_ms": per_round, "yardstick_spread_ms": spread}))


if __name__ == "__main__":
    main()
