"""`training.GroupedFlatAdamW` and `training.geowizard_param_groups` without a GPU: the layout of the flat buffer, the `torch.optim.Optimizer` surface (live
`param_groups`, schedulers, state in torch's format), the refusals — and the argument validation of e2eft_adamw_step_groups / e2eft_adamw_step_groups_at
through ctypes, which returns before anything is launched.  The update itself is a HIP kernel: tests/test_adamw_groups_gpu.py, tests/test_grouped_optimizer_gpu.py."""
import ctypes as C

import pytest
import torch


class _Net(torch.nn.Module):
    """parameters in definition order: conv, lin, (class_embedding.0, class_embedding.1,) norm"""

    def __init__(self, class_embedding=True):
        super().__init__()
        torch.manual_seed(0)
        self.conv = torch.nn.Conv2d(3, 5, 3)
        self.lin = torch.nn.Linear(7, 3)
        if class_embedding:
            self.class_embedding = torch.nn.Sequential(torch.nn.Linear(10, 6), torch.nn.Linear(6, 6))
        self.norm = torch.nn.LayerNorm(5)


def _offset(opt, p):
    return (p.data_ptr() - opt.flat_param.data_ptr()) // 4


def test_geowizard_param_groups_split_by_name():
    from diffusion_e2e_ft_amd.training import geowizard_param_groups
    net = _Net()
    groups = geowizard_param_groups(net, 3e-5)
    named = dict(net.named_parameters())
    assert [g["lr"] for g in groups] == [3e-5, 3e-5 * 10.0] and set(groups[0]) == set(groups[1]) == {"params", "lr"}
    assert [id(p) for p in groups[1]["params"]] == [id(p) for n, p in named.items() if "class_embedding" in n] and len(groups[1]["params"]) == 4
    assert [id(p) for p in groups[0]["params"]] == [id(p) for n, p in named.items() if "class_embedding" not in n] and len(groups[0]["params"]) == 6
    groups = geowizard_param_groups(_Net(False), 1e-4, class_embedding_lr_mult=3.0)
    assert len(groups) == 2 and groups[1]["params"] == [] and groups[1]["lr"] == 1e-4 * 3.0 and len(groups[0]["params"]) == 6
    assert "learning_rate * gradient_accumulation_steps * train_batch_size * num_processes" in geowizard_param_groups.__doc__


def test_layout_is_group_after_group_and_agrees_with_torch():
    from diffusion_e2e_ft_amd.training import GroupedFlatAdamW, geowizard_param_groups
    net, ref = _Net(), _Net()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    opt = GroupedFlatAdamW(geowizard_param_groups(net, 3e-5), betas=(0.9, 0.99), weight_decay=0.1, eps=1e-6)
    topt = torch.optim.AdamW(geowizard_param_groups(ref, 3e-5), betas=(0.9, 0.99), weight_decay=0.1, eps=1e-6)
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 2
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())              # flattening keeps the values
    a, b = opt.state_dict()["param_groups"], topt.state_dict()["param_groups"]
    assert [g["params"] for g in a] == [g["params"] for g in b] == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9]]
    for ga, gb in zip(a, b):
        assert all(ga[k] == gb[k] for k in ("lr", "betas", "eps", "weight_decay"))
    assert (a[1]["lr"], a[1]["betas"], a[1]["eps"], a[1]["weight_decay"]) == (3e-5 * 10.0, (0.9, 0.99), 1e-6, 0.1)
    # each group one contiguous, 8-element aligned range; the ranges tile the buffer in order; every parameter lies inside its group's range
    (b0, e0), (b1, e1) = opt.group_ranges
    assert b0 == 0 and e0 == b1 and e1 == opt.numel and all(x % 8 == 0 for x in (b0, e0, b1, e1))
    for (lo, hi), g in zip(opt.group_ranges, opt.param_groups):
        at = lo
        for p in g["params"]:
            assert _offset(opt, p) == at and at % 8 == 0
            at += (p.numel() + 7) // 8 * 8
        assert at == hi
    assert [id(p) for p in opt.params] == [id(p) for g in opt.param_groups for p in g["params"]]
    assert opt.hyper_words == 3 and opt._coef.numel() == 6
    # per-group hyper-parameters of the caller win over the keyword defaults, as in torch
    net2 = _Net()
    opt2 = GroupedFlatAdamW([{"params": [net2.conv.weight, net2.lin.weight], "weight_decay": 1e-2},
                             {"params": [net2.conv.bias, net2.lin.bias, net2.norm.weight, net2.norm.bias], "weight_decay": 0.0, "betas": [0.8, 0.99], "eps": 1e-6}],
                            lr=1e-4)
    g0, g1 = opt2.param_groups
    assert (g0["lr"], g0["betas"], g0["eps"], g0["weight_decay"]) == (1e-4, (0.9, 0.999), 1e-8, 1e-2)
    assert (g1["lr"], g1["betas"], g1["eps"], g1["weight_decay"]) == (1e-4, (0.8, 0.99), 1e-6, 0.0)
    assert opt2._table(0.5)[1] == (opt2.group_ranges[1][0], opt2.numel, 0.5e-4, 0.8, 0.99, 1e-6, 0.0)
    # a plain parameter list is one group
    net3 = _Net()
    opt3 = GroupedFlatAdamW(net3.parameters(), lr=1e-3)
    assert len(opt3.param_groups) == 1 and opt3.group_ranges == [(0, opt3.numel)] and opt3.hyper_words == 2


def test_empty_and_frozen_groups_are_kept_and_own_nothing():
    from diffusion_e2e_ft_amd.training import GroupedFlatAdamW, geowizard_param_groups
    net = _Net(False)
    opt = GroupedFlatAdamW(geowizard_param_groups(net, 3e-5))
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["params"] == [] and opt.param_groups[1]["lr"] == 3e-5 * 10.0
    assert opt.group_ranges == [(0, opt.numel), (opt.numel, opt.numel)]
    sd = opt.state_dict()
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2, 3, 4, 5], []]
    # frozen parameters are dropped, as FlatAdamW drops them; a group of frozen parameters only stays, empty, between its neighbours
    net = _Net()
    net.lin.requires_grad_(False)
    net.conv.bias.requires_grad_(False)
    opt = GroupedFlatAdamW([{"params": net.conv.parameters()}, {"params": net.lin.parameters(), "lr": 1.0}, {"params": net.norm.parameters(), "lr": 2.0}], lr=0.5)
    assert [len(g["params"]) for g in opt.param_groups] == [1, 0, 2] and [g["lr"] for g in opt.param_groups] == [0.5, 1.0, 2.0]
    n0 = (net.conv.weight.numel() + 7) // 8 * 8
    assert opt.group_ranges == [(0, n0), (n0, n0), (n0, opt.numel)] and opt.numel == n0 + 16
    with pytest.raises(ValueError, match="no trainable parameters"):
        GroupedFlatAdamW([{"params": net.lin.parameters()}, {"params": []}])


def test_refusals():
    from diffusion_e2e_ft_amd.training import FlatAdamW, GroupedFlatAdamW, geowizard_param_groups
    ps = [torch.nn.Parameter(torch.zeros(3)) for _ in range(9)]
    with pytest.raises(ValueError, match="at most 8"):
        GroupedFlatAdamW([{"params": [p]} for p in ps])
    assert len(GroupedFlatAdamW([{"params": [p]} for p in ps[:8]]).param_groups) == 8
    net = _Net()
    with pytest.raises(ValueError, match="more than one parameter group"):          # torch's own check
        GroupedFlatAdamW([{"params": [net.conv.weight, net.conv.bias]}, {"params": [net.lin.weight, net.conv.bias]}])
    assert not hasattr(net.conv.weight, "_e2eft_flat")                                  # refused before any parameter was moved
    with pytest.raises(ValueError, match="single parameter group"):                     # the single-group class keeps refusing
        FlatAdamW(geowizard_param_groups(net, 3e-5))
    with pytest.raises(TypeError, match="fp32 master"):
        GroupedFlatAdamW([{"params": [torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))]}])


def test_schedulers_scale_every_group_from_its_own_base_rate():
    from torch.optim.lr_scheduler import LambdaLR
    from diffusion_e2e_ft_amd.training import GroupedFlatAdamW, IterExponential, geowizard_param_groups
    opt = GroupedFlatAdamW(geowizard_param_groups(_Net(), 3e-5, 10.0))
    lam = IterExponential(total_iter_length=20000, final_ratio=0.01, warmup_steps=100)
    sched = LambdaLR(opt, lr_lambda=lam)
    assert [g["lr"] for g in opt.param_groups] == [0.0, 0.0] and opt.lr == 0.0            # warm-up starts at 0
    opt._opt_called = True      # (silences LambdaLR's "step order" warning: no optimizer.step() on a CPU box)
    for _ in range(50):
        sched.step()
    assert abs(opt.param_groups[0]["lr"] - 3e-5 * 0.5) < 1e-15 and abs(opt.param_groups[1]["lr"] - 3e-4 * 0.5) < 1e-15
    assert [row[2] for row in opt._table(lr_scale=0.5)] == [g["lr"] * 0.5 for g in opt.param_groups]      # step(lr_scale=) multiplies all of them
    opt.lr = 7.0                                                                                    # the property is group 0's
    assert opt.param_groups[0]["lr"] == 7.0 and opt.lr == 7.0 and abs(opt.param_groups[1]["lr"] - 1.5e-4) < 1e-15
    # diffusers' get_scheduler("constant", ...) and ("constant_with_warmup", ...) are LambdaLR over these lambdas
    opt = GroupedFlatAdamW(geowizard_param_groups(_Net(), 1e-4, 10.0))
    sched = LambdaLR(opt, lambda _: 1.0)
    opt._opt_called = True
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 1e-4 * 10.0]
    sched = LambdaLR(opt, lambda step: min(1.0, step / 4.0))
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == [1e-4 * 0.25, 1e-4 * 10.0 * 0.25]


def test_state_dict_round_trip_restores_state_and_group_hyper_parameters():
    from diffusion_e2e_ft_amd.training import GroupedFlatAdamW, geowizard_param_groups
    net, ref = _Net(), _Net()
    topt = torch.optim.AdamW(geowizard_param_groups(ref, 2e-3, 5.0), betas=(0.8, 0.99), weight_decay=0.0, eps=1e-6)
    topt.param_groups[1]["weight_decay"] = 0.25
    sum(((p + 1.0) ** 2).sum() for p in ref.parameters()).backward()
    topt.step()
    opt = GroupedFlatAdamW(geowizard_param_groups(net, 123.0, 2.0))
    opt.load_state_dict(topt.state_dict())                                            # a two-group torch.optim.AdamW checkpoint
    assert [(g["lr"], g["betas"], g["eps"], g["weight_decay"]) for g in opt.param_groups] == [(2e-3, (0.8, 0.99), 1e-6, 0.0), (2e-3 * 5.0, (0.8, 0.99), 1e-6, 0.25)]
    assert opt.step_count == 1 and opt.skipped_steps() == 0
    for p, rp in zip(opt.params, [q for g in topt.param_groups for q in g["params"]]):
        o = _offset(opt, p)
        assert torch.equal(opt.exp_avg[o:o + p.numel()].view(p.shape) if p.dim() < 4 else opt.state[p]["exp_avg"], topt.state[rp]["exp_avg"])
        assert torch.equal(opt.state[p]["exp_avg_sq"], topt.state[rp]["exp_avg_sq"]) and opt.state[p]["exp_avg_sq"].abs().sum() > 0
        assert opt.state[p]["exp_avg"].data_ptr() == opt.exp_avg.data_ptr() + 4 * o             # state stays a VIEW of the flat moments
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "flat_adamw"} and sorted(sd["state"]) == list(range(10)) and set(sd["state"][7]) == {"step", "exp_avg", "exp_avg_sq"}
    # ours -> a fresh grouped optimizer, and -> torch
    net2 = _Net()
    opt2 = GroupedFlatAdamW(geowizard_param_groups(net2, 9.0, 9.0))
    opt2.load_state_dict(sd)
    assert opt2.state_dict()["param_groups"] == sd["param_groups"] and opt2.step_count == 1
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
    topt2 = torch.optim.AdamW(geowizard_param_groups(_Net(), 1.0, 1.0))
    topt2.load_state_dict({k: v for k, v in sd.items() if k != "flat_adamw"})
    assert [g["lr"] for g in topt2.param_groups] == [2e-3, 2e-3 * 5.0] and topt2.param_groups[1]["weight_decay"] == 0.25
    for k, st in topt2.state_dict()["state"].items():
        assert torch.equal(st["exp_avg"], sd["state"][k]["exp_avg"]) and float(st["step"]) == 1.0
    # one flat buffer has one step count
    bad = topt.state_dict()
    bad["state"][7]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError, match="different step counts"):
        opt2.load_state_dict(bad)


# ---- 11. the C ABI refuses bad tables before it launches anything --------------------------------------------------------------------------------------------
def test_argument_validation_of_both_entry_points_without_gpu():
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    assert _lib.ADAMW_MAX_GROUPS == 8 and C.sizeof(_lib.AdamwGroup) == 40
    buf = C.create_string_buffer(256)
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)
    G = _lib.AdamwGroup

    def table(*ranges):
        return (G * len(ranges))(*[G(b, e, 1e-3, 0.9, 0.999, 1e-8, 1e-2) for b, e in ranges])

    def by_value(n=100, t=table((0, 8), (8, 100)), ng=2, ptrs=(p,) * 7):
        pa, g, m, v, st, co, ss = ptrs
        return lib.e2eft_adamw_step_groups(n, pa, g, m, v, t, ng, st, co, ss, 1.0, 1.0, None)

    def at(n=100, t=table((0, 8), (8, 100)), ng=2, ptrs=(p,) * 7, hyper=p):
        pa, g, m, v, st, co, ss = ptrs
        return lib.e2eft_adamw_step_groups_at(n, pa, g, m, v, t, ng, hyper, st, co, ss, 1.0, None)

    for call, name in ((by_value, b"adamw_groups:"), (at, b"adamw_groups_at:")):
        def refused(text, **kw):
            rc = call(**kw)
            err = lib.e2eft_last_error()
            assert rc == 1 and name in err and text in err, (rc, err, kw)
        for i in range(7):                                                   # every pointer
            refused(b"null", ptrs=tuple(None if j == i else p for j in range(7)))
        refused(b"null groups", t=None)
        refused(b"n <= 0", n=0)
        refused(b"n_groups 0 outside 1..8", ng=0)
        refused(b"n_groups 9 outside 1..8", t=table(*[(8 * k, 8 * k + 8) for k in range(9)]), ng=9)
        refused(b"n_groups -1 outside 1..8", ng=-1)
        refused(b"begin 16 > end 8", t=table((0, 8), (16, 8)))
        refused(b"begin -8", t=table((-8, 8), (8, 100)))
        refused(b"ascend", t=table((8, 100), (0, 8)))                        # not ascending
        refused(b"overlap", t=table((0, 16), (8, 100)))                      # overlapping
        refused(b"overlap", t=table((0, 16), (8, 8)))                        # an empty group inside another one
        refused(b"end 101 > n 100", t=table((0, 8), (8, 101)))
    assert at(hyper=None) == 1 and b"null" in lib.e2eft_last_error()
    assert at(hyper=odd) == 1 and b"4-byte aligned" in lib.e2eft_last_error()
    assert buf.raw == b"\0" * 256                                            # nothing was written through any of the pointers


def test_ops_wrappers_build_the_table_the_library_reads():
    from diffusion_e2e_ft_amd import _lib, ops
    rows = [(0, 8, 1e-3, 0.9, 0.999, 1e-8, 1e-2), (8, 8, 2e-3, 0.8, 0.99, 1e-6, 0.0)]
    t = ops.adamw_groups(rows)
    assert len(t) == 2 and isinstance(t[0], _lib.AdamwGroup) and ops.adamw_groups(t) is t
    assert (t[1].begin, t[1].end) == (8, 8) and t[1].beta1 == C.c_float(0.8).value and t[1].weight_decay == 0.0 and t[0].lr == C.c_float(1e-3).value
    x = torch.zeros(16)
    with pytest.raises(RuntimeError, match="no CPU fallback|device"):
        ops.adamw_step_groups_(x, x, x, x, rows, torch.zeros(2, dtype=torch.int64), torch.zeros(6), torch.zeros(1, dtype=torch.float64))
