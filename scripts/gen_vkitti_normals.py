"""Write Virtual KITTI 2's vkitti_DAG_normals/ on the GPU: the folder the fine-tuning authors' depth-to-normal-translator/python/gen_vkitti_normals.py
makes (VERSION = 'd2nt_v3') and the training loader reads (training/dataloaders/load.py:332), without OpenCV.

    python scripts/gen_vkitti_normals.py data/virtual_kitti_2 [--batch 16] [--workers 8] [--v2]

Same walk as the generator's VirtualKITTI2._find_pairs (gen_vkitti_normals.py:27-51: five scenes, ten conditions including the 15-deg / 30-deg
ones, both cameras; every rgb_*.jpg with a depth directory), with each listdir sorted.  Host threads decode the uint16 depth PNGs; the kernel
(e2eft_depth_to_normals) turns batches into the file's uint16 values ((n + 1) * 32767.5 truncated); host threads write 16-bit RGB PNGs
(data.write_png16).  Existing files are overwritten."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCENES = ["Scene01", "Scene02", "Scene06", "Scene18", "Scene20"]
CONDITIONS = ["15-deg-left", "15-deg-right", "30-deg-left", "30-deg-right", "clone", "morning", "fog", "rain", "sunset", "overcast"]
CAMERAS = ["Camera_0", "Camera_1"]


def find_pairs(root_dir):
    """gen_vkitti_normals.py:27-51 -> [(depth_path, normal_path)] in the generator's order (listdir sorted)"""
    pairs = []
    for scene in SCENES:
        for cond in CONDITIONS:
            for cam in CAMERAS:
                rgb_dir = os.path.join(root_dir, "vkitti_2.0.3_rgb", scene, cond, "frames", "rgb", cam)
                depth_dir = os.path.join(root_dir, "vkitti_2.0.3_depth", scene, cond, "frames", "depth", cam)
                normal_dir = os.path.join(root_dir, "vkitti_DAG_normals", scene, cond, "frames", "normal", cam)
                if os.path.exists(rgb_dir) and os.path.exists(depth_dir):
                    for f in sorted(os.listdir(rgb_dir)):
                        if f.endswith(".jpg"):
                            stem = f[3:].replace(".jpg", ".png")
                            pairs.append((os.path.join(depth_dir, "depth" + stem), os.path.join(normal_dir, "normal" + stem)))
    return pairs


def _read_depth_m(path):
    from diffusion_e2e_ft_amd import data
    return data.pil_decoder(path, "depth").astype(np.float32) / 100.0       # gen_vkitti_normals.py:61-62 (cm -> m in float32)


def _write(path, u16):
    from diffusion_e2e_ft_amd import data
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data.write_png16(path, u16)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("root_dir")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--v2", action="store_true", help="d2nt_v2: no MRF refinement")
    a = ap.parse_args(argv)
    import torch
    from diffusion_e2e_ft_amd import data
    pairs = find_pairs(a.root_dir)
    print("samples:", len(pairs))
    dev = torch.device("cuda")
    t0 = time.time()
    with ThreadPoolExecutor(max_workers=max(1, a.workers)) as pool:
        writes = []
        for s in range(0, len(pairs), a.batch):
            chunk = pairs[s:s + a.batch]
            depths = list(pool.map(lambda p: _read_depth_m(p[0]), chunk))
            groups = {}
            for i, d in enumerate(depths):          # one launch per image size in the batch
                groups.setdefault(d.shape, []).append(i)
            for shape, idx in groups.items():
                x = torch.from_numpy(np.stack([depths[i] for i in idx])).to(dev)
                u16 = data.depth_to_normals_vkitti(x, refine=not a.v2, out_format="u16").cpu().numpy()
                writes += [pool.submit(_write, chunk[i][1], u16[j]) for j, i in enumerate(idx)]
            for w in writes:
                w.result()
            writes = []
    print("wrote %d files in %.1f s" % (len(pairs), time.time() - t0))
    return len(pairs)


if __name__ == "__main__":
    main()
