"""`training.GroupedFlatAdamW` on the tiny GeoWizard UNet with the reference trainer's parameter groups (GeoWizard/geowizard/training/train_depth_normal.py:428-444:
the class embedding at ten times the rate): every element against the float64 reference of tests/optimizer_ref.py with its group's learning rate, checkpoints
exchanged with a two-group `torch.optim.AdamW` in both directions, and `CapturedTrainStep` replaying a grouped update.  The models are built the way
tests/test_train_graph_gpu.py builds them."""
import pytest
import torch

import golden_cases as gc
import optimizer_ref as R
from oracle import config

pytestmark = pytest.mark.gpu

LR, MULT = 3e-5, 10.0


def _models(dev):
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    unet = UNet2DConditionModel(**config.TINY_GEOWIZARD_UNET)
    unet.load_state_dict(gc.tiny_geo_sd())
    unet = unet.to(dev).train()
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(gc.tiny_vae_sd())
    vae = vae.to(dev).eval()
    vae.requires_grad_(False)
    return unet, vae


def _grouped(unet, lr=LR, mult=MULT):
    from diffusion_e2e_ft_amd import training
    return training.GroupedFlatAdamW(training.geowizard_param_groups(unet, lr, mult), betas=(0.9, 0.999), weight_decay=1e-2, eps=1e-8, max_grad_norm=1.0)


def _scheduler(opt):
    from diffusion_e2e_ft_amd import training
    return torch.optim.lr_scheduler.LambdaLR(opt, training.IterExponential(total_iter_length=6, final_ratio=0.01))


def _batch(seed, dev):
    return {k: v.to(dev) for k, v in gc.train_batch(seed, B=2, H=64, W=64)[0].items()}


def _embed(seed):
    return 0.5 * torch.randn(2, 1, config.TINY_GEOWIZARD_UNET["cross_attention_dim"], generator=torch.Generator().manual_seed(seed))


def _loss(unet, vae, seed, dev):
    from diffusion_e2e_ft_amd import training
    return training.geowizard_e2e_ft_loss(unet, vae, _batch(100 + seed, dev), _embed(200 + seed), "indoor", 0.5, 1.0)


def _step(unet, vae, opt, sched, seed, dev, clip=False):
    loss = _loss(unet, vae, seed, dev)
    loss.backward()
    if clip:
        torch.nn.utils.clip_grad_norm_(unet.parameters(), 1.0)
    opt.step()
    sched.step()
    opt.zero_grad()
    return loss.detach()


# ---- 7. per element against float64, each group at its own rate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("checked", (1, 2, 3))
def test_geowizard_groups_step_every_element_at_its_group_rate(dev, checked):
    """three steps of the GeoWizard loss under LambdaLR(IterExponential); one case per step: the case runs the steps before its own unchecked (the float64
    reference over the 3e7 elements of the tiny UNet is what takes the time) and holds step `checked` to the bounds, element by element"""
    unet, vae = _models(dev)
    names = [n for n, _ in unet.named_parameters()]
    opt = _grouped(unet)
    sched = _scheduler(opt)
    assert len(opt.param_groups) == 2 and len(opt.param_groups[1]["params"]) == sum("class_embedding" in n for n in names) > 0
    (b0, e0), (b1, e1) = opt.group_ranges
    assert b0 == 0 and e0 == b1 and e1 == opt.numel and e1 - b1 >= sum(p.numel() for p in opt.param_groups[1]["params"]) > 0
    rates = []
    for s in range(checked):
        lrs = [g["lr"] for g in opt.param_groups]
        assert abs(lrs[1] - MULT * lrs[0]) <= 1e-12 * lrs[1]
        rates.append(tuple(lrs))
        if s + 1 < checked:
            _step(unet, vae, opt, sched, s, dev)
            continue
        p0, m0, v0 = opt.flat_param.cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu()
        loss = _loss(unet, vae, s, dev)
        loss.backward()
        opt.step()
        g, ss = opt.flat_grad.cpu(), opt._sumsq.item()          # the SAME flat gradient the kernel read, and its sum of squares
        got = (opt.flat_param.cpu(), opt.exp_avg.cpu(), opt.exp_avg_sq.cpu())
        assert torch.isfinite(loss).all() and ss > 0 and opt.step_count == s + 1
        for k, (b, e) in enumerate(opt.group_ranges):
            sl = slice(b, e)
            inputs = {"p": p0[sl], "g": g[sl], "m": m0[sl], "v": v0[sl]}
            ref = R.adamw_ref(p0[sl], g[sl], m0[sl], v0[sl], lrs[k], 0.9, 0.999, 1e-8, 1e-2, s + 1, ss, 1.0, 1.0, "fp32")
            r = R.check_step("step %d, group %d" % (s + 1, k), tuple(x[sl] for x in got), ref, inputs)
            print("step %d group %d: ratio to the bound p %.3f m %.3f v %.3f" % (s + 1, k, r["p"], r["m"], r["v"]))
        # the class embedding moved at ten times the rate: held against group 0's rate it leaves the bound
        sl = slice(b1, e1)
        wrong = R.adamw_ref(p0[sl], g[sl], m0[sl], v0[sl], lrs[0], 0.9, 0.999, 1e-8, 1e-2, s + 1, ss, 1.0, 1.0, "fp32")
        with pytest.raises(AssertionError, match="outside the bound"):
            R.check_step("group 1 at group 0's rate", tuple(x[sl] for x in got), wrong, {"p": p0[sl]})
        assert (got[0][sl] != p0[sl]).any()
        opt.zero_grad()
    assert len(set(rates)) == checked
    # the parameters are still the model's: the class embedding's own tensors are views of the second range
    for p in opt.param_groups[1]["params"]:
        off = (p.data_ptr() - opt.flat_param.data_ptr()) // 4
        assert b1 <= off and off + p.numel() <= e1


# ---- 8. checkpoints, both directions -------------------------------------------------------------------------------------------------------------------
def _same_state(a, b, what):
    assert a.keys() == b.keys() and len(a) > 0, what
    for k in a:
        for name in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a[k][name].cpu(), b[k][name].cpu()), (what, k, name)
        assert float(a[k]["step"]) == float(b[k]["step"]), (what, k)


def test_checkpoints_travel_between_grouped_flat_adamw_and_torch_adamw(dev):
    from diffusion_e2e_ft_amd import training
    unet, vae = _models(dev)
    opt = _grouped(unet)
    sched = _scheduler(opt)
    for s in range(2):
        _step(unet, vae, opt, sched, s, dev)
    ckpt = {"model": {k: v.detach().clone() for k, v in unet.state_dict().items()}, "opt": opt.state_dict(), "sched": sched.state_dict()}
    saved_lrs = [g["lr"] for g in ckpt["opt"]["param_groups"]]
    assert abs(saved_lrs[1] - MULT * saved_lrs[0]) <= 1e-12 * saved_lrs[1] and saved_lrs[0] != LR
    _step(unet, vae, opt, sched, 2, dev)              # the uninterrupted run's step 3

    def fresh():
        u = _models(dev)[0]
        u.load_state_dict(ckpt["model"])
        return u

    # ---- ours -> ours: other rates at construction, the checkpoint's come back per group
    u2 = fresh()
    opt2 = _grouped(u2, lr=123.0, mult=2.0)
    sched2 = _scheduler(opt2)
    opt2.load_state_dict(ckpt["opt"])
    sched2.load_state_dict(ckpt["sched"])
    assert [g["lr"] for g in opt2.param_groups] == saved_lrs and opt2.step_count == 2
    _same_state(opt2.state_dict()["state"], ckpt["opt"]["state"], "ours -> ours")
    _step(u2, vae, opt2, sched2, 2, dev)
    for name in ("flat_param", "exp_avg", "exp_avg_sq", "_steps"):
        assert torch.equal(getattr(opt2, name), getattr(opt, name)), name
    # ---- ours -> torch.optim.AdamW with the same two groups (torch's own state format, same parameter indices)
    u3 = fresh()
    topt = torch.optim.AdamW(training.geowizard_param_groups(u3, 1.0, 1.0), betas=(0.5, 0.5), weight_decay=0.0, eps=1.0)
    assert [g["params"] for g in topt.state_dict()["param_groups"]] == [g["params"] for g in ckpt["opt"]["param_groups"]]
    tsched = _scheduler(topt)
    topt.load_state_dict({k: v for k, v in ckpt["opt"].items() if k != "flat_adamw"})
    tsched.load_state_dict(ckpt["sched"])
    assert [g["lr"] for g in topt.param_groups] == saved_lrs
    assert all(g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and g["weight_decay"] == 1e-2 for g in topt.param_groups)
    tsd = topt.state_dict()
    _same_state(tsd["state"], ckpt["opt"]["state"], "ours -> torch")
    # ---- torch -> ours: torch's checkpoint of that state, loaded into a fresh grouped optimizer, takes the uninterrupted run's step 3
    u4 = fresh()
    opt4 = _grouped(u4, lr=55.0, mult=3.0)
    sched4 = _scheduler(opt4)
    opt4.load_state_dict(tsd)
    sched4.load_state_dict(tsched.state_dict())
    assert [g["lr"] for g in opt4.param_groups] == saved_lrs and opt4.step_count == 2 and opt4.skipped_steps() == 0
    _step(u4, vae, opt4, sched4, 2, dev)
    for name in ("flat_param", "exp_avg", "exp_avg_sq", "_steps"):
        assert torch.equal(getattr(opt4, name), getattr(opt, name)), name
    # and torch itself steps from our checkpoint to the same parameters, as closely as its double-precision scalars allow
    _step(u3, vae, topt, tsched, 2, dev, clip=True)
    for (n, p), (_, q) in zip(unet.named_parameters(), u3.named_parameters()):
        err = (p - q).abs().max().item()
        assert err <= 2e-5 * max(q.abs().max().item(), 1e-3), (n, err)


# ---- 9. the captured step --------------------------------------------------------------------------------------------------------------------------------
def test_captured_grouped_steps_equal_eager_steps(dev):
    """eager warm-up, capture, two replays; the scheduler changes both groups' rates after every step and nothing is captured again"""
    from diffusion_e2e_ft_amd import training
    eu, ev = _models(dev)
    cu, cv = _models(dev)
    eo, co = _grouped(eu), _grouped(cu)
    scheds = [_scheduler(o) for o in (eo, co)]
    step = training.CapturedTrainStep.geowizard(cu, cv, co, "indoor", 0.5, 1.0, accumulation=1)
    assert step._hyper.numel() == 3
    rates = []
    for s in range(4):
        batch, embed = _batch(100 + s, dev), _embed(200 + s)
        lr_scale = 1.0 if s != 2 else 0.5
        loss = training.geowizard_e2e_ft_loss(eu, ev, batch, embed, "indoor", 0.5, 1.0)
        loss.backward()
        eo.step(lr_scale=lr_scale)
        eo.zero_grad()
        got = step([batch], lr_scale, imgs_embed=[embed])
        assert torch.isfinite(loss).all() and torch.equal(got, loss.detach()), (s, got.item(), loss.item())
        for name in ("flat_param", "exp_avg", "exp_avg_sq", "_steps", "_coef"):
            assert torch.equal(getattr(co, name), getattr(eo, name)), (s, name)
        rates.append(tuple(g["lr"] for g in co.param_groups))
        assert rates[-1] == tuple(g["lr"] for g in eo.param_groups)
        for sc in scheds:
            sc.step()
    assert len(step._entries) == 1 and next(iter(step._entries.values()))["graphs"] is not None
    assert len(set(r[0] for r in rates)) == 4 and len(set(r[1] for r in rates)) == 4 and co.step_count == eo.step_count == 4 and co.skipped_steps() == 0
    a, b = co.state_dict(), eo.state_dict()
    assert a["param_groups"] == b["param_groups"] and a["flat_adamw"] == b["flat_adamw"]
    _same_state(a["state"], b["state"], "captured vs eager")
