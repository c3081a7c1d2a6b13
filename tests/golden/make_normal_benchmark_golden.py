"""Generate tests/golden/normal_benchmark_golden.pt : what the REFERENCE'S benchmark mode makes of the synthetic dsine_eval trees of
tests/normal_benchmark_fixture.py.  Run from the repo root: `python tests/golden/make_normal_benchmark_golden.py`.

Executed from source in the reference tree: the four get_sample functions (DSINE/data/datasets/{nyuv2,scannet,ibims,sintel}/__init__.py), get_transform
in test mode at input_height = input_width = 0 (DSINE/data/augmentations/__init__.py: ToTensor, Normalize, ToDict), the image round trip of
DSINE/projects/dsine/test.py:59-65 (those seven lines are cut out of the file and executed on the CPU, with the batch axis the DataLoader adds), and
compute_normal_error / compute_normal_metrics (DSINE/utils/utils.py:150-178) chained as test.py:102-115 chains them, over predictions that are a
fixed function of the re-quantised image (normal_benchmark_fixture.stub_normals, the function the tests' stand-in pipeline uses).

cv2 and torchvision are not installed.  This file installs STAND-INS for them in sys.modules before importing the reference — they are shims, not
the real packages:
  cv2.imread            a PNG: Pillow's decode with the channels reversed to BGR; an .exr: the FIXTURE'S OWN source array reversed to BGR (so the
                        reader under test, normal_eval_data.read_exr, is not its own oracle); contiguous arrays, as OpenCV returns them
  cv2.cvtColor          BGR to RGB by channel reversal (contiguous)
  torchvision.transforms.Compose, .Normalize    as torchvision defines them: Normalize is tensor.clone().sub_(mean).div_(std) with mean and std as
                        tensors of the input's dtype, shaped [C,1,1]
  torchvision.transforms.functional             an empty module (imported by the augmentation files, not used in test mode)

Per dataset and sample the file keeps img_u8 [3,H,W] (the re-quantised image), normal [3,H,W] fp32, normal_mask [1,H,W] uint8, intrins, the names;
per dataset the valid pixels' errors, the eight metrics and n.  Data only.

Trust rule of tests/golden/reference_manifest.json: third-party source is executed only when its sha256 is the one that was reviewed (recorded
below); E2EFT_TRUST_REFERENCE=1 runs a changed file anyway, after you have looked at the diff."""
import hashlib
import importlib
import os
import sys
import tempfile
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
import normal_benchmark_fixture as nfx  # noqa: E402

REF = os.environ.get("E2EFT_REFERENCE", "/root/reference")
REF_SHA256 = {
    "DSINE/projects/dsine/test.py": "adbe9bd1152f51ae7d7687fdf04b91008cce030e383e68327ea8f7e2c3be4450",
    "DSINE/projects/__init__.py": "17a16c0913f097eedddfa6f26a5a028431141551d4d903bd295d88dce7e15c56",
    "DSINE/data/__init__.py": "1f25dc1a5a16c15d9419ee12b25a2d95799d6b4e48f7acd9152c38b9cdfe8381",
    "DSINE/data/datasets/nyuv2/__init__.py": "89d9095ea6ffd5bdb7bc53b352c1139478b0a299178efc1692b71db4edb8fc2b",
    "DSINE/data/datasets/scannet/__init__.py": "10e20e84d9c2d461986c714c4834b12b63511fcd38d006259fa972d4549fc8ac",
    "DSINE/data/datasets/ibims/__init__.py": "7e3089b6fbb291a86f63d1922bfbf73049ae5446652f86855b26232020382db5",
    "DSINE/data/datasets/sintel/__init__.py": "d7759905f2900f96e8b3f7023eb70443bd8aacc3dcf95bfe30a7862abad43aac",
    "DSINE/data/augmentations/__init__.py": "00626f6d07ac3687e8b48ccba34a6a59b758fb93506fe20d75019cbaa2c94158",
    "DSINE/data/augmentations/basic.py": "97fccfcd5620693629ca28416385f01e1b48a7c92c81105f59a815a12f7f51e0",
    "DSINE/data/augmentations/appearance.py": "1d935293cb1455d8df306c219191975694e8d8b00e81fedd6a4ac0afa6e8d6e3",
    "DSINE/data/augmentations/perspective.py": "34b15dbdf8f5ea9ed85ef2eca32acab7aa849e09a976692fb71d6b6b0ea78917",
    "DSINE/utils/utils.py": "0f9787bb53b60e1a20362277f1a35f806ddb57ec2d8d8b5d36089eaae560dbf5",
    "DSINE/utils/rotation.py": "c2b012204fd1f1efa04d2a9b04a55634fa53a35a8e811df2dc680df7799d3c94",
    "DSINE/utils/projection.py": "7581218060317ca52b13a045984d6c4b4c60d9933e8dbcc4bba27543d6f0f488",
}
TEST_PY_LINES = (59, 65)
NAMES = ("mean", "median", "rmse", "a1", "a2", "a3", "a4", "a5")


def check_trust(loaded=None):
    """every listed file has the reviewed sha256; `loaded`: also, no OTHER file of the reference tree was imported"""
    for f, want in REF_SHA256.items():
        with open(os.path.join(REF, f), "rb") as fh:
            h = hashlib.sha256(fh.read()).hexdigest()
        if h != want and os.environ.get("E2EFT_TRUST_REFERENCE") != "1":
            raise RuntimeError("%s changed (sha256 %s, reviewed %s): look at the diff, then set E2EFT_TRUST_REFERENCE=1" % (f, h, want))
    for path in loaded or ():
        rel = os.path.relpath(path, REF)
        if rel not in REF_SHA256 and os.path.getsize(path) > 0:
            raise RuntimeError("the reference imported %s, which is not among the reviewed files" % rel)


class _Args:
    """what config.get_args(test=True) and test.py:208-211 leave of the arguments the loaders read"""
    load_img = load_normal = load_intrins = True
    input_height = input_width = 0
    data_augmentation_same_fov = 0
    data_augmentation_intrins = False


def install_shims(exr_sources):
    from PIL import Image
    cv2 = types.ModuleType("cv2")
    cv2.IMREAD_UNCHANGED, cv2.COLOR_BGR2RGB = -1, 4

    def imread(path, flags=None):
        if path.endswith(".exr"):
            return np.ascontiguousarray(exr_sources[os.path.normpath(path)][..., ::-1])
        return np.ascontiguousarray(np.asarray(Image.open(path))[..., ::-1])

    def cvtColor(a, code):
        assert code == cv2.COLOR_BGR2RGB
        return np.ascontiguousarray(a[..., ::-1])

    cv2.imread, cv2.cvtColor = imread, cvtColor
    tv = types.ModuleType("torchvision")
    tvt = types.ModuleType("torchvision.transforms")
    tvf = types.ModuleType("torchvision.transforms.functional")

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
            return x

    class Normalize:
        def __init__(self, mean, std, inplace=False):
            self.mean, self.std = mean, std

        def __call__(self, tensor):
            tensor = tensor.clone()
            mean = torch.as_tensor(self.mean, dtype=tensor.dtype, device=tensor.device).view(-1, 1, 1)
            std = torch.as_tensor(self.std, dtype=tensor.dtype, device=tensor.device).view(-1, 1, 1)
            return tensor.sub_(mean).div_(std)

    tvt.Compose, tvt.Normalize, tvt.functional = Compose, Normalize, tvf
    tv.transforms = tvt
    sys.modules.update({"cv2": cv2, "torchvision": tv, "torchvision.transforms": tvt, "torchvision.transforms.functional": tvf})


def requantize_from_source(img):
    """test.py:59-65 executed from the file: img is data_dict['img'] as the DataLoader hands it over ([1,3,H,W]) -> uint8 [H,W,3]"""
    with open(os.path.join(REF, "DSINE/projects/dsine/test.py")) as f:
        lines = f.readlines()
    src = textwrap.dedent("".join(lines[TEST_PY_LINES[0] - 1:TEST_PY_LINES[1]]))
    assert src.startswith("img = data_dict['img'].to(device)") and src.rstrip().endswith(".astype(np.uint8)"), src
    ns = {"data_dict": {"img": img}, "device": torch.device("cpu"), "np": np, "torch": torch}
    exec(compile(src, "test.py:%d-%d" % TEST_PY_LINES, "exec"), ns)
    return ns["img"]


def make():
    check_trust()
    out = {"sha256": dict(REF_SHA256), "names": NAMES, "datasets": {}}
    saved = list(sys.path)
    with tempfile.TemporaryDirectory() as tmp:
        trees = {name: nfx.make_tree(tmp, name) for name in nfx.NAMES}
        exr_sources = {}
        for name in nfx.NAMES:
            for i, (scene, stem, _, opt) in enumerate(nfx.SAMPLES[name]):
                if opt is not None:
                    exr_sources[os.path.normpath(os.path.join(trees[name]["dir"], scene, stem + "_normal.exr"))] = nfx.normal_exr(name, i)
        install_shims(exr_sources)
        sys.path.insert(0, REF)
        try:
            before = set(sys.modules)
            pkg = types.ModuleType("DSINE.utils")          # DSINE/utils/__init__.py pulls in the visualisation module: its submodules are imported without it
            pkg.__path__ = [os.path.join(REF, "DSINE", "utils")]
            sys.modules["DSINE.utils"] = pkg
            aug = importlib.import_module("DSINE.data.augmentations")
            utils = importlib.import_module("DSINE.utils.utils")
            mods = {name: importlib.import_module("DSINE.data.datasets.%s" % name) for name in nfx.NAMES}
            loaded = [m.__file__ for k, m in sys.modules.items() if k not in before and getattr(m, "__file__", None) and m.__file__.startswith(REF)]
            check_trust(loaded)
            for name in nfx.NAMES:
                mods[name].DATASET_PATH = trees[name]["dir"]
                transform = aug.get_transform(_Args, dataset_name=name, mode="test")
                samples, errors = [], []
                for sample_path in trees[name]["filenames"]:
                    d = transform(mods[name].get_sample(args=_Args, sample_path=sample_path, info={}))
                    img_u8 = requantize_from_source(d["img"].unsqueeze(0))
                    assert img_u8.dtype == np.uint8 and img_u8.shape == tuple(d["img"].shape[1:]) + (3,)
                    assert d["normal"].dtype == torch.float32 and d["normal_mask"].dtype == torch.bool and d["dataset_name"] == name
                    pred = torch.from_numpy(nfx.stub_normals(img_u8)).unsqueeze(0)                                 # test.py:99
                    err = utils.compute_normal_error(pred, d["normal"].unsqueeze(0))                               # :106
                    errors.append(err[d["normal_mask"].unsqueeze(0)])                                              # :108-110
                    samples.append({"img_u8": torch.from_numpy(np.ascontiguousarray(img_u8.transpose(2, 0, 1))), "normal": d["normal"].contiguous().clone(),
                                    "normal_mask": d["normal_mask"].contiguous().to(torch.uint8), "intrins": d["intrins"].clone(),
                                    "scene_name": d["scene_name"], "img_name": d["img_name"], "keys": sorted(d)})
                total = torch.cat(errors, dim=0)
                met = utils.compute_normal_metrics(total)                                                          # :115
                out["datasets"][name] = {"samples": samples, "errors": total.clone(), "n": int(total.numel()),
                                         "metrics": torch.tensor([float(met[k]) for k in NAMES], dtype=torch.float64)}
        finally:
            sys.path[:] = saved
    return out


if __name__ == "__main__":
    g = make()
    path = os.path.join(HERE, "normal_benchmark_golden.pt")
    torch.save(g, path)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: (len(v["samples"]), v["n"], [round(x, 3) for x in v["metrics"].tolist()]) for k, v in g["datasets"].items()})
