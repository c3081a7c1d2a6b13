"""Generate tests/golden/d2nt_golden.pt : the REFERENCE'S depth-to-normal translator
(depth-to-normal-translator/python/utils/myApis.py and utils/apis.py, executed in place from /root/reference) on seeded Virtual KITTI-like depth maps, driven as gen_vkitti_normals.py:100-133 drives it
with VERSION = 'd2nt_v3' (and 'd2nt_v2': the same without MRF_optim).
Run from the repo root: `python tests/golden/make_d2nt_golden.py`.

OpenCV is not installed; the two calls the translator makes are served by the stand-in below (defined here, put in sys.modules only while the
reference's files are loaded): filter2D = correlation with BORDER_REFLECT_101, the result in the input dtype, fp32 accumulation over the non-zero
taps in row-major order; merge = np.dstack.  The MRF argmin map is recorded by wrapping np.argmin inside the loaded myApis module only.

Trust rule of tests/golden/reference_manifest.json: third-party source is executed only when its sha256 is the one that was reviewed (recorded
below); E2EFT_TRUST_REFERENCE=1 runs a changed file anyway, after you have looked at the diff."""
import hashlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import d2nt_ref  # noqa: E402

REF_DIR = os.path.join(os.environ.get("E2EFT_REFERENCE", "/root/reference"), "depth-to-normal-translator", "python", "utils")
REF_SHA256 = {"myApis.py": "885812e2f5f2d247a802c362dd90b240292c882a084f33f09f7794995b7e76bc",
              "apis.py": "30d9e08c6e004a832d1148dc0581ebd312ee720eb0d0401bf35162d8e76fee76"}
K2 = (512.3, 498.75, 30.25, 14.5)
# (seed, H, W, intrinsics, sky)
CASES = [(1, 2, 2, d2nt_ref.VKITTI_K, True), (2, 37, 53, d2nt_ref.VKITTI_K, True), (3, 40, 150, d2nt_ref.VKITTI_K, True), (4, 29, 67, K2, False)]
POWER_PROBE_SEED = 5


def sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def reference_available():
    return all(os.path.exists(os.path.join(REF_DIR, f)) for f in REF_SHA256)


def cv2_standin():
    def filter2D(src, ddepth, kernel):
        assert ddepth == -1
        k = np.asarray(kernel)
        kh, kw = k.shape
        ay, ax = kh // 2, kw // 2
        H, W = src.shape
        P = np.pad(src, ((ay, kh - 1 - ay), (ax, kw - 1 - ax)), mode="reflect")      # BORDER_REFLECT_101
        acc = None
        for i in range(kh):
            for j in range(kw):
                if k[i, j] != 0:
                    t = src.dtype.type(k[i, j]) * P[i:i + H, j:j + W]
                    acc = t if acc is None else acc + t
        return acc.astype(src.dtype)

    m = types.ModuleType("cv2")
    m.filter2D = filter2D
    m.merge = lambda planes: np.dstack(planes)
    return m


def load_reference():
    """-> (myApis module, apis module, sha256 dict, argmin log)"""
    shas = {f: sha256(os.path.join(REF_DIR, f)) for f in REF_SHA256}
    for f, h in shas.items():
        if REF_SHA256[f] and h != REF_SHA256[f] and os.environ.get("E2EFT_TRUST_REFERENCE") != "1":
            raise RuntimeError("%s changed (sha256 %s, reviewed %s): look at the diff, then set E2EFT_TRUST_REFERENCE=1" % (f, h, REF_SHA256[f]))
    saved = sys.modules.get("cv2")
    sys.modules["cv2"] = cv2_standin()
    mods = {}
    try:
        for f in ("myApis.py", "apis.py"):
            spec = importlib.util.spec_from_file_location("d2nt_ref_" + f[:-3], os.path.join(REF_DIR, f))
            mods[f] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[f])
    finally:
        if saved is None:
            sys.modules.pop("cv2", None)
        else:
            sys.modules["cv2"] = saved
    log = []

    class _np:                                   # numpy for myApis.py, with argmin recorded
        def __getattr__(self, name):
            return getattr(np, name)

        @staticmethod
        def argmin(*a, **k):
            r = np.argmin(*a, **k)
            log.append(r)
            return r

    mods["myApis.py"].np = _np()
    return mods["myApis.py"], mods["apis.py"], shas, log


def run_reference(myapis, apis, log, depth_cm, K, version):
    """gen_vkitti_normals.py:61-77 (the dataset's depth and intrinsics) and :100-133 (the translation), restated around the reference's calls"""
    depth_m = depth_cm.astype(np.float32) / 100.0                                  # :62
    depth = torch.from_numpy(depth_m.copy())[None].numpy()[0] * 100                 # ToTensor of the float32 PIL image, [:,0].squeeze().numpy() * 100
    intrinsics = torch.tensor([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]).numpy()
    cam_fx, cam_fy, u0, v0 = intrinsics[0, 0], intrinsics[1, 1], intrinsics[0, 2], intrinsics[1, 2]
    h, w = depth.shape
    u_map = np.ones((h, 1)) * np.arange(1, w + 1) - u0
    v_map = np.arange(1, h + 1).reshape(h, 1) * np.ones((1, w)) - v0
    Gu, Gv = myapis.get_DAG_filter(depth)
    est_nx = Gu * cam_fx
    est_ny = Gv * cam_fy
    est_nz = -(depth + v_map * Gv + u_map * Gu)
    est_normal = np.dstack((est_nx, est_ny, est_nz))                                # cv2.merge
    est_normal = apis.vector_normalization(est_normal)
    choice = None
    if version == "d2nt_v3":
        del log[:]
        est_normal = myapis.MRF_optim(depth, est_normal)
        choice = log[0]
    est_normal = est_normal * -1
    u16 = ((est_normal + 1) * 32767.5).astype(np.uint16)                           # RGB2BGR + imwrite cancel: channel 0 of the file's RGB is n_x
    return est_normal, u16, choice


def power_probe():
    x = np.random.default_rng(POWER_PROBE_SEED).random(4096).astype(np.float32) * np.float32(40)
    return x, np.power(np.e, -x)


def make():
    myapis, apis, shas, log = load_reference()
    out = {"sha256": shas, "cases": []}
    for seed, H, W, K, sky in CASES:
        cm = d2nt_ref.vkitti_like_depth_cm(np.random.default_rng(seed), H, W, sky=sky)
        n2, u2, _ = run_reference(myapis, apis, log, cm, K, "d2nt_v2")
        n3, u3, ch = run_reference(myapis, apis, log, cm, K, "d2nt_v3")
        r3 = d2nt_ref.depth_to_normals(d2nt_ref.cm_to_metres(cm), K, True)
        r2 = d2nt_ref.depth_to_normals(d2nt_ref.cm_to_metres(cm), K, False)
        assert np.array_equal(r2["normal"], n2) and np.array_equal(r2["u16"], u2), "restatement != reference (v2)"
        assert np.array_equal(r3["normal"], n3) and np.array_equal(r3["choice"], ch) and np.array_equal(r3["u16"], u3), "restatement != reference"
        arrays = {"depth_cm": cm, "normal_v2": n2, "normal_v3": n3, "choice": ch.astype(np.uint8), "u16_v2": u2, "u16_v3": u3,
                  "u8_v2": (u2 >> 8).astype(np.uint8), "u8_v3": (u3 >> 8).astype(np.uint8), "margin": r3["margin"].astype(np.float32)}
        out["cases"].append(dict({"seed": seed, "K": K}, **{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in arrays.items()}))
    x, p = power_probe()
    out["power_probe"] = {"x": torch.from_numpy(x), "p": torch.from_numpy(p)}
    return out


if __name__ == "__main__":
    g = make()
    path = os.path.join(HERE, "d2nt_golden.pt")
    torch.save(g, path)
    print("wrote", path, os.path.getsize(path), "bytes;", g["sha256"])
