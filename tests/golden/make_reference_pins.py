"""Generate tests/golden/reference_pins.pt — the results of the reference's own functions that the CPU pins compare the oracle and the
product against (run from the repo root where the reference tree is present: `python tests/golden/make_reference_pins.py`).

Each entry of LIVE computes one result by importing / executing the reference's source in place (tests/refimport.py for the model
wiring, plain file imports for the leaf utilities) on seeded inputs that the tests rebuild themselves; the fixture holds only the
results.  `pinned(name)` is what the tests call: the live result (checked against the recorded one) where the reference tree is present,
the recorded result everywhere else, so the pins also hold on a checkout that has no reference tree next to it.
"""
import importlib.util
import os
import random
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
import golden_cases as gc  # noqa: E402
import refimport  # noqa: E402
from oracle import config  # noqa: E402

REF = refimport.REF
PATH = os.path.join(HERE, "reference_pins.pt")
MIXED_CASES = [(90, 10, 9, 1), (50, 50, 9, 1), (300, 7, 9, 1), (13, 200, 3, 2)]
UNET_CASES = [((16, 16), 2, 2, False), ((20, 12), 2, 2, False), ((8, 8), 3, 77, True), ((9, 7), 1, 2, False)]
NOISE_SHAPES = ((2, 4, 12, 16), (1, 4, 9, 7), (3, 4, 32, 32))
LR_POINTS = (0, 5, 10, 500, 999, 1000, 2000)


def _import(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def import_reference_load():
    """training/dataloaders/load.py with its four unavailable third-party imports stubbed (only names used at import time)"""
    stubs = {}
    for name in ("torchvision", "torchvision.transforms", "PIL", "PIL.Image", "pandas", "cv2"):
        if name not in sys.modules:
            stubs[name] = types.ModuleType(name)
    if "torchvision" in stubs:
        stubs["torchvision"].transforms = stubs["torchvision.transforms"]
    if "PIL" in stubs:
        stubs["PIL"].Image = stubs["PIL.Image"]
    sys.modules.update(stubs)
    try:
        return _import("training/dataloaders/load.py", "ref_load")
    finally:
        for k in stubs:
            sys.modules.pop(k, None)


def mixed_dataloader(n1, n2, s1, s2):
    ref = import_reference_load()
    a, b = [("a", i) for i in range(n1)], [("b", i) for i in range(n2)]
    np.random.seed(123)
    loader = ref.MixedDataLoader(a, b, s1, s2)
    return {"order": list(loader), "len": len(loader), "frac1": loader.frac1, "frac2": loader.frac2}


def ensemble_depths():
    m = _import("Marigold/marigold/util/ensemble.py", "ref_ensemble_live")
    stack = gc.ensemble_depth_stack(n=6, H=21, W=30, seed=77)
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kw in ({}, dict(reduction="mean"), dict(max_res=16)):
            out.append(m.ensemble_depths(stack.clone(), **kw))
    return out


def pyramid_noise():
    ref = _import("training/util/noise.py", "ref_noise")
    out = []
    for shape in NOISE_SHAPES:
        torch.manual_seed(5)
        random.seed(5)
        out.append(ref.pyramid_noise_like(torch.zeros(shape)))
    return out


def hook_draws():
    """the seeded (pred, target, mask) / (normal, normal, mask) draws of test_hooks_against_live_reference"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(3):
        tgt = torch.rand(2, 1, 24, 32, generator=g)
        pred = torch.randn(2, 1, 24, 32, generator=g)
        mask = torch.rand(2, 1, 24, 32, generator=g) > 0.3
        n = F.normalize(torch.randn(2, 3, 24, 32, generator=g), dim=1)
        t = F.normalize(torch.randn(2, 3, 24, 32, generator=g), dim=1)
        out.append((pred, tgt, mask, n, t))
    return out


def hooks():
    loss, lr = _import("training/util/loss.py", "ref_loss"), _import("training/util/lr_scheduler.py", "ref_lr_scheduler")
    ssi, ang = [], []
    for pred, tgt, mask, n, t in hook_draws():
        ssi.append(loss.ScaleAndShiftInvariantLoss()(pred, tgt, mask))
        ang.append(loss.AngularLoss()(n, t, mask))
    s = lr.IterExponential(1000, 0.05, 10)
    return {"ssi": ssi, "angular": ang, "iter_exponential": [s(i) for i in LR_POINTS]}


def absrel_inputs():
    g = torch.Generator().manual_seed(5)
    gt = torch.rand(48, 64, generator=g) * 9 + 1
    pred = (gt - 2.0) / 7.0 + 0.03 * torch.randn(48, 64, generator=g)
    mask = torch.rand(48, 64, generator=g) > 0.1
    return gt, pred, mask


def absrel():
    al, me = _import("Marigold/src/util/alignment.py", "ref_alignment"), _import("Marigold/src/util/metric.py", "ref_metric")
    gt, pred, mask = absrel_inputs()
    a_ref, s_ref, t_ref = al.align_depth_least_square(gt.numpy(), pred.numpy(), mask.numpy())
    x = torch.from_numpy(a_ref).float()
    return {"aligned": a_ref, "scale": float(s_ref), "shift": float(t_ref),
            "absrel_masked": me.abs_relative_difference(x.clone(), gt, mask), "absrel": me.abs_relative_difference(x.clone(), gt)}


def _shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def unet_keys():
    out = {}
    with refimport.reference_modules() as ref:
        for name in ("TINY_UNET", "TINY_GEOWIZARD_UNET"):
            out[name] = _shapes(ref.UNet2DConditionModel(**refimport.ref_unet_kwargs(getattr(config, name))))
        with torch.device("meta"):
            full = ref.UNet2DConditionModel(**refimport.ref_unet_kwargs(config.SD2_UNET))
        out["SD2_UNET"] = _shapes(full)
        out["SD2_UNET_numel"] = sum(p.numel() for p in full.parameters())
    return out


def vae_keys():
    out = {}
    with refimport.reference_modules() as ref:
        for name in ("TINY_VAE", "SD_VAE"):
            with torch.device("meta"):
                vae = ref.AutoencoderKL(**refimport.ref_vae_kwargs(getattr(config, name)))
            out[name] = _shapes(vae)
            out[name + "_numel"] = sum(p.numel() for p in vae.parameters())
    return out


def unet_wiring():
    import make_refwiring_golden as gen
    out = []
    with refimport.reference_modules() as ref, torch.no_grad():
        unet, _ = gen.build_models(ref)
        for hw, batch, ctx_len, per_sample_t in UNET_CASES:
            x, ctx = gc.unet_inputs(hw, batch=batch, ctx_len=ctx_len, seed=8)
            t = torch.tensor([999, 500, 1][:batch]) if per_sample_t else 999
            out.append(unet(x, t, encoder_hidden_states=ctx).sample)
    return out


def joint_attention():
    import make_refwiring_golden as gen
    with refimport.reference_modules() as ref, torch.no_grad():
        unet, _ = gen.build_models(ref, geo=True)
        procs = sorted({type(m.processor).__name__ for m in unet.modules() if hasattr(m, "processor")})
        x, ctx, cls = gc.geo_unet_inputs()
        return {"processors": procs, "out": unet(x, 999, encoder_hidden_states=ctx, class_labels=cls).sample}


def vae_blocks():
    import make_refwiring_golden as gen
    with refimport.reference_modules() as ref, torch.no_grad():
        _, vae = gen.build_models(ref)
        rgb, z = gc.vae_inputs()
        return {"moments": vae.quant_conv(vae.encoder(rgb)), "dec": vae.decoder(vae.post_quant_conv(z))}


LIVE = {"mixed_dataloader": lambda: [mixed_dataloader(*c) for c in MIXED_CASES], "ensemble_depths": ensemble_depths, "pyramid_noise": pyramid_noise,
        "hooks": hooks, "absrel": absrel, "unet_keys": unet_keys, "vae_keys": vae_keys, "unet_wiring": unet_wiring,
        "joint_attention": joint_attention, "vae_blocks": vae_blocks}
# what each entry needs of the reference tree: where it is absent (or not readable), the recorded result stands in
NEEDS = {"mixed_dataloader": "training/dataloaders/load.py", "ensemble_depths": "Marigold/marigold/util/ensemble.py", "pyramid_noise": "training/util/noise.py",
         "hooks": "training/util/loss.py", "absrel": "Marigold/src/util/alignment.py"}


def live_available(name):
    if name in NEEDS:
        return os.access(os.path.join(REF, NEEDS[name]), os.R_OK)
    return refimport.reference_available()


def same(a, b, rtol=1e-6):
    """recorded against live: structure and exact values for everything but floating-point data, which may differ in the last bits"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k], rtol) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y, rtol) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    if isinstance(b, np.ndarray):
        b = torch.from_numpy(b)
    if torch.is_tensor(a):
        if not torch.is_tensor(b) or a.shape != b.shape or a.dtype != b.dtype:
            return False
        if not a.is_floating_point():
            return torch.equal(a, b)
        return bool(((a.double() - b.double()).abs() <= rtol * b.double().abs().max().clamp_min(1e-30)).all())
    if isinstance(a, float):
        return abs(a - b) <= rtol * max(abs(b), 1e-30)
    return a == b


_RECORDED = None
_LIVE_RESULTS = {}


def recorded():
    global _RECORDED
    if _RECORDED is None:
        _RECORDED = torch.load(PATH, weights_only=False)
    return _RECORDED


def pinned(name):
    """the reference's result `name`: computed live from the reference's source where it is present (and then the recorded copy must agree
    with it), else the recorded copy"""
    want = recorded()[name]
    if live_available(name):
        if name not in _LIVE_RESULTS:
            _LIVE_RESULTS[name] = LIVE[name]()
        now = _LIVE_RESULTS[name]
        assert same(want, now), "tests/golden/reference_pins.pt[%r] differs from what the reference computes now: re-run %s" % (name, os.path.basename(__file__))
        return now
    return want


def main():
    missing = [n for n in LIVE if not live_available(n)]
    assert not missing, "reference tree not present at %s (needed for %s)" % (REF, missing)
    out = {name: fn() for name, fn in LIVE.items()}
    torch.save(out, PATH)
    print("wrote %s (%d bytes): %s" % (PATH, os.path.getsize(PATH), sorted(out)))


if __name__ == "__main__":
    main()
