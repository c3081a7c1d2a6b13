"""Generate tests/golden/normal_eval_golden.pt: outputs of the REFERENCE'S surface-normal evaluation functions (DSINE/utils/utils.py:150-178,
compute_normal_error and compute_normal_metrics, executed in place from /root/reference) on seeded synthetic (prediction, ground truth, mask)
cases, chained as DSINE/projects/dsine/test.py:104-118 chains them.
Run from the repo root: `python tests/golden/make_normal_eval_golden.py`.

Trust rule of tests/golden/reference_manifest.json: third-party source is executed only when its sha256 is the one that was reviewed (recorded
below); E2EFT_TRUST_REFERENCE=1 runs a changed file anyway, after you have looked at the diff."""
import hashlib
import importlib.util
import math
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.environ.get("E2EFT_REFERENCE", "/root/reference"), "DSINE", "utils", "utils.py")
REF_SHA256 = "0f9787bb53b60e1a20362277f1a35f806ddb57ec2d8d8b5d36089eaae560dbf5"
THRESHOLDS = (5.0, 7.5, 11.25, 22.5, 30.0)
NAMES = ("mean", "median", "rmse", "a1", "a2", "a3", "a4", "a5")


def smooth_gt(g, B, H, W):
    """ground-truth normals as a dataset stores them: a smooth unit field quantised to uint8 and decoded x / 255 * 2 - 1 (many tied errors)"""
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H, dtype=torch.float64), torch.linspace(-1, 1, W, dtype=torch.float64), indexing="ij")
    out = []
    for _ in range(B):
        a, b, c = (torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1).tolist()
        nx = a * torch.sin(2.0 * xx + b) + 0.3 * yy
        ny = b * torch.cos(1.5 * yy - c) - 0.2 * xx
        n = torch.stack([nx, ny, torch.ones_like(nx) * (1.0 + abs(c))])
        n = n / n.norm(dim=0, keepdim=True)
        q = ((n + 1.0) * 0.5 * 255.0).round().clamp(0, 255).to(torch.uint8)
        out.append(q.float() / 255.0 * 2.0 - 1.0)
    return torch.stack(out)


def perturb(g, gt, max_deg=60.0):
    """rotate each unit(gt) by a random angle in [0, max_deg] about a random axis orthogonal to it; then exact copies (0 deg), antiparallel
    vectors (180 deg) and zero vectors (90 deg) on a few pixels each"""
    B, _, H, W = gt.shape
    u = gt.double() / gt.double().norm(dim=1, keepdim=True)
    r = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)
    v = r - (r * u).sum(1, keepdim=True) * u
    v = v / v.norm(dim=1, keepdim=True)
    ang = torch.rand(B, 1, H, W, generator=g, dtype=torch.float64) * math.radians(max_deg)
    pred = (u * torch.cos(ang) + v * torch.sin(ang)) * (0.5 + torch.rand(B, 1, H, W, generator=g, dtype=torch.float64))
    pred = pred.float()
    kind = torch.rand(B, 1, H, W, generator=g)
    pred = torch.where(kind < 0.03, gt, pred)
    pred = torch.where((kind >= 0.03) & (kind < 0.05), -gt, pred)
    pred = torch.where((kind >= 0.05) & (kind < 0.06), torch.zeros_like(pred), pred)
    return pred.contiguous()


def make_case(seed, B, H, W, invalid=0.3, parity=None):
    g = torch.Generator().manual_seed(seed)
    gt = smooth_gt(g, B, H, W)
    pred = perturb(g, gt)
    mask = torch.rand(B, 1, H, W, generator=g) > invalid
    if parity is not None and int(mask.sum()) % 2 != parity:
        mask[0, 0, 0, 0] = ~mask[0, 0, 0, 0]
    return pred, gt, mask


CASES = [dict(seed=1, B=1, H=37, W=53, parity=1), dict(seed=2, B=1, H=37, W=53, parity=0), dict(seed=3, B=4, H=24, W=40, parity=0),
         dict(seed=4, B=2, H=31, W=29, invalid=0.5, parity=1)]


def _load_reference():
    with open(REF, "rb") as f:
        have = hashlib.sha256(f.read()).hexdigest()
    if have != REF_SHA256 and os.environ.get("E2EFT_TRUST_REFERENCE") != "1":
        raise SystemExit("%s differs from the reviewed file (sha256 %s, reviewed %s): review it, then E2EFT_TRUST_REFERENCE=1" % (REF, have, REF_SHA256))
    spec = importlib.util.spec_from_file_location("ref_dsine_utils", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    ref = _load_reference()
    out = {"names": NAMES, "thresholds": THRESHOLDS, "cases": []}
    for c in CASES:
        pred, gt, mask = make_case(**c)
        err = ref.compute_normal_error(pred, gt)
        errors = err[mask]
        met = ref.compute_normal_metrics(errors)
        out["cases"].append({"pred": pred, "gt": gt, "mask": mask, "errors": errors.clone(),
                             "metrics": torch.tensor([float(met[k]) for k in NAMES], dtype=torch.float64), "n": int(errors.numel())})
        print(c, "n", errors.numel(), " ".join("%s %.4f" % (k, float(met[k])) for k in NAMES))
    torch.save(out, os.path.join(HERE, "normal_eval_golden.pt"))


if __name__ == "__main__":
    main()
