"""Generate tests/golden/diffusion_objective_golden.pt (run on the CPU from the repo root: `python tests/golden/make_diffusion_objective_golden.py`).

One diffusion-objective micro-step of the GeoWizard trainer (train_depth_normal.py:598-717 without --e2e_ft) through torch autograd over the CPU restatement
tests/diffusion_objective_ref.py, with the tiny GeoWizard UNet and VAE of golden_cases, per prediction type: the loss, n_selected, the target at a stride, every
parameter's gradient norm and the gradients sampled as train_golden.pt samples them.  Also: the E2E-FT step with x_t = noise (the restatement's
`geowizard_e2e_ft_noise_forward_ref`), and `bf16_loss_error` — the relative error of the restatement run in bfloat16 on the CPU against its own fp32 loss on the
same inputs, from which tests/test_diffusion_objective_gpu.py derives the bar of the 16-bit micro-step.
The inputs are regenerated from seeds by the tests (diffusion_objective_ref.objective_inputs); only results are stored."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import config  # noqa: E402
import golden_cases as gc  # noqa: E402
import diffusion_objective_ref as ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def check_mask(val_mask):
    """the conditions the fixture's mask has to meet (it must hide neither the selected nor the excluded cells)"""
    lm = ref.latent_mask_ref(val_mask)[:, 0]
    per_image = [int(m.sum()) for m in lm]
    cells = lm[0].numel()
    assert tuple(per_image) == ref.SELECTED_CELLS, per_image
    assert all(n >= cells // 4 for n in per_image), per_image                      # at least a quarter of the cells of each image selected
    assert all(n < cells for n in per_image), per_image                            # at least one cell of each image excluded
    valid_per_cell = val_mask[:, 0].float().unfold(1, 8, 8).unfold(2, 8, 8).sum(dim=(-1, -2))
    assert bool((valid_per_cell == 63).any()), "no cell is excluded by a single invalid pixel"
    return per_image


def grads_of(loss, usd):
    loss.backward()
    keys = [k for k in gc.TRAIN_FULL_GRADS if k in usd] + ["class_embedding.linear_1.weight"]
    out = {"grad_norms": {k: float(v.grad.norm()) for k, v in usd.items()}, "grads": {k: gc.sample_grad(usd[k].grad) for k in keys}}
    return out


def main():
    torch.set_num_threads(8)
    batch, emb, timesteps, noise = ref.objective_inputs()
    per_image = check_mask(batch["val_mask"])
    out = {"selected_cells": per_image, "timesteps": timesteps.clone()}
    cfg, vsd = config.TINY_GEOWIZARD_UNET, gc.tiny_vae_sd()
    for pt in ("epsilon", "v_prediction"):
        usd = {k: v.clone().requires_grad_(True) for k, v in gc.tiny_geo_sd().items()}
        loss, n_sel, target, x_t = ref.geowizard_diffusion_forward_ref(usd, cfg, vsd, config.TINY_VAE, batch, emb, timesteps, noise, pt)
        assert n_sel == 2 * 4 * sum(per_image), (n_sel, per_image)
        rec = {"loss": loss.detach().clone(), "n_selected": n_sel, "target": target.detach().reshape(-1)[::ref.TARGET_STRIDE].clone(),
               "x_t": x_t.detach().reshape(-1)[::ref.TARGET_STRIDE].clone()}
        rec.update(grads_of(loss, usd))
        with torch.no_grad():
            lo, n16, _, _ = ref.geowizard_diffusion_forward_ref(gc.tiny_geo_sd(), cfg, vsd, config.TINY_VAE, batch, emb, timesteps, noise, pt, dtype=torch.bfloat16)
        assert n16 == n_sel
        loss = loss.detach()
        rec["bf16_loss_error"] = abs(float(lo) - float(loss)) / abs(float(loss))
        out[pt] = rec
        print(pt, "loss", float(loss), "n_selected", n_sel, "bf16 restatement", float(lo), "relative error", rec["bf16_loss_error"])
    usd = {k: v.clone().requires_grad_(True) for k, v in gc.tiny_geo_sd().items()}
    e2e_batch, _ = gc.geo_train_inputs()
    loss, ssi, ang = ref.geowizard_e2e_ft_noise_forward_ref(usd, cfg, vsd, config.TINY_VAE, e2e_batch, emb, noise)
    rec = {"loss": loss.detach().clone(), "ssi": ssi.detach().clone(), "angular": ang.detach().clone()}
    rec.update(grads_of(loss, usd))
    out["e2e_ft_noise"] = rec
    print("e2e_ft_noise loss", float(loss.detach()))
    path = os.path.join(HERE, "diffusion_objective_golden.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
