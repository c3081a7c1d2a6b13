"""Generate tests/golden/geowizard_pyramid_golden.pt (run on the CPU from the repo root: `python tests/golden/make_geowizard_pyramid_golden.py`).

The GeoWizard trainer's `pyramid_noise_like(x, timesteps)` (GeoWizard/geowizard/training/train_depth_normal.py:286-296) is executed IN PLACE from the reference tree
(tests/refimport.py `run_source`; the trainer itself is not importable here) with `torch.randn` / `torch.randn_like` replaced by recorders — nothing of its text is
copied.  Recorded, as data:
  sizes    per (rows, cols) and `np.random.seed` value: the level sizes the function asked `torch.randn` for, and the next `np.random.random()` after it returned
           (the state it leaves numpy's global stream in)
  case     the function's float64 output for a [4,4,12,10] input with timesteps [0, 999, 500, 1], when the replaced randn_like / randn hand it the grids of the
           generator restatement (tests/noise_ref.normal_grid: slot 0 the base, slot 1 + i level i) — with the level sizes it drew under the recorded numpy seed
tests/test_geowizard_pyramid_cpu.py compares noise.geowizard_pyramid_level_sizes and tests/geowizard_pyramid_ref.weighted_pyramid against these."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import noise_ref  # noqa: E402
import refimport  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(96, 96), (60, 80), (8, 8), (3, 200), (1, 7)]
NP_SEEDS = [0, 7, 2024]
CASE = dict(shape=(4, 4, 12, 10), timesteps=(0, 999, 500, 1), seed=0x5EED0123456789AB, draw=9, np_seed=3)


def reference_function(randn, randn_like):
    """the reference's function object, its `torch` narrowed to the two replaced draws (everything else it uses: nn.Upsample, np.random, tensor methods)"""
    ns = {"torch": types.SimpleNamespace(randn=randn, randn_like=randn_like), "nn": torch.nn, "np": np}
    refimport._Ref().run_source("GeoWizard/geowizard/training/train_depth_normal.py", 286, 296, ns)
    return ns["pyramid_noise_like"]


def main():
    out = {"sizes": {}, "shapes": SHAPES, "np_seeds": NP_SEEDS}
    asked = []

    def spy_randn(*size):
        asked.append(tuple(int(s) for s in size))
        return torch.zeros(*size)

    fn = reference_function(spy_randn, torch.zeros_like)
    for rows, cols in SHAPES:
        for s in NP_SEEDS:
            del asked[:]
            np.random.seed(s)
            fn(torch.ones(2, 4, rows, cols), torch.tensor([999, 999]))
            nxt = float(np.random.random())
            assert all(a[:2] == (2, 4) for a in asked)
            out["sizes"][(rows, cols, s)] = {"sizes": [a[2:] for a in asked], "next_random": nxt}
            print((rows, cols), "np seed", s, [a[2:] for a in asked], nxt)

    shape, seed, draw = CASE["shape"], CASE["seed"], CASE["draw"]
    levels = []

    def grid_randn(*size):
        levels.append(tuple(int(s) for s in size[2:]))
        return noise_ref.normal_grid(seed, draw, len(levels), tuple(int(s) for s in size))

    fn = reference_function(grid_randn, lambda x: noise_ref.normal_grid(seed, draw, 0, tuple(x.shape)))
    np.random.seed(CASE["np_seed"])
    y = fn(torch.zeros(shape, dtype=torch.float64), torch.tensor(CASE["timesteps"], dtype=torch.long))
    assert y.dtype == torch.float64 and tuple(y.shape) == shape
    out["case"] = dict(CASE, sizes=levels, output=y.clone())
    print("case", shape, "levels", levels, "std", float(y.std()))
    path = os.path.join(HERE, "geowizard_pyramid_golden.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
