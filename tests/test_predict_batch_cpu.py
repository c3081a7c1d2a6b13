"""Batched prediction without a GPU: the two new C entry points are declared and bound, argument validation that never launches, the signatures of
`predict_batch` on both pipelines and of the runners' `predict_batch_size`, the scripts' `--batch_size`, and the grouping rule of the runners (a pure function)."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("e2eft_minmax_unit_batched_workspace_bytes", "e2eft_minmax_unit_batched")


def test_header_declares_and_binding_lists_the_batched_minmax():
    from diffusion_e2e_ft_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "e2eft.h")).read(), flags=re.S)
    assert re.search(r"size_t\s+e2eft_minmax_unit_batched_workspace_bytes\s*\(\s*int32_t\s+batch\s*\)\s*;", src)
    assert re.search(r"int\s+e2eft_minmax_unit_batched\s*\(\s*int32_t\s+batch\s*,\s*int64_t\s+n_per_image\s*,\s*const\s+float\s*\*\s*x\s*,\s*float\s*\*\s*out\s*,"
                     r"\s*float\s*\*\s*minmax\s*,\s*void\s*\*\s*workspace\s*,\s*size_t\s+ws_bytes\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    C = ctypes
    assert _lib.SIGNATURES[NEW[0]] == (C.c_size_t, [C.c_int32])
    assert _lib.SIGNATURES[NEW[1]] == (C.c_int32, [C.c_int32, C.c_int64] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p])
    lib = _lib.load()
    for n in NEW:
        assert hasattr(lib, n)
    assert lib.e2eft_version() == 119


def test_batched_minmax_argument_validation_launches_nothing():
    """the workspace is sized by the batch alone; an empty batch or an empty image is success without a look at the pointers; a null pointer and a short
    workspace are the library's usual codes with a text (no kernel is launched on any of these paths, so this needs no GPU)"""
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    size = lib.e2eft_minmax_unit_batched_workspace_bytes
    assert size(0) == 0 and size(-3) == 0
    sizes = [size(b) for b in (1, 2, 3, 8, 65535)]
    assert sizes[0] > 0 and sizes == [sizes[0] * b for b in (1, 2, 3, 8, 65535)]
    p = ctypes.c_void_p(4096)                      # never dereferenced: every call below returns before a launch
    f = lib.e2eft_minmax_unit_batched
    assert f(0, 10, None, None, None, None, 0, None) == 0 and f(-1, 10, p, p, p, p, 0, None) == 0
    assert f(2, 0, None, None, None, None, 0, None) == 0 and f(2, -5, p, p, p, p, 0, None) == 0
    for args in ((2, 10, None, p, p, p, size(2), None), (2, 10, p, None, p, p, size(2), None), (2, 10, p, p, p, None, size(2), None)):
        assert f(*args) == 1 and b"minmax_unit_batched" in lib.e2eft_last_error() and b"null" in lib.e2eft_last_error()
    assert f(2, 10, p, p, None, p, size(2) - 1, None) == 2 and b"minmax_unit_batched: workspace" in lib.e2eft_last_error()
    assert f(65536, 10, p, p, None, p, 1 << 40, None) == 1 and b"65535" in lib.e2eft_last_error()


def _params(fn):
    return [(p.name, p.default, p.kind) for p in inspect.signature(fn).parameters.values()]


def test_predict_batch_signatures():
    from diffusion_e2e_ft_amd.pipeline import DepthNormalEstimationPipeline, MarigoldPipeline
    E, K = inspect.Parameter.empty, inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert _params(MarigoldPipeline.predict_batch) == [("self", E, K), ("images", E, K), ("processing_res", 768, K), ("match_input_res", True, K),
                                                       ("resample_method", "bilinear", K), ("normals", False, K), ("denoising_steps", 1, K),
                                                       ("noise", "zeros", K), ("generator", None, K)]
    assert _params(DepthNormalEstimationPipeline.predict_batch) == [("self", E, K), ("images", E, K), ("processing_res", 768, K), ("match_input_res", True, K),
                                                                    ("domain", "indoor", K), ("denoising_steps", 1, K), ("noise", "zeros", K)]
    for cls in (MarigoldPipeline, DepthNormalEstimationPipeline):
        doc = cls.predict_batch.__doc__
        assert "ensemble_size" in doc and "`__call__`" in doc
    assert "HWC" in DepthNormalEstimationPipeline.predict_batch.__doc__


def test_runner_predict_batch_size_is_the_last_keyword_and_defaults_to_none():
    """the keyword is `predict_batch_size`, not `batch_size`: the runners have always handed a `batch_size` among their keywords on to the pipeline's `__call__`
    (its ensemble members per pass; tests/test_normal_benchmark_gpu.py does so), and they still do"""
    from diffusion_e2e_ft_amd import evaluate
    for fn in (evaluate.evaluate_depth_benchmark, evaluate.evaluate_normal_benchmark):
        params = _params(fn)
        assert params[-1][0] == "pipe_kwargs" and params[-1][2] == inspect.Parameter.VAR_KEYWORD
        assert params[-2] == ("predict_batch_size", None, inspect.Parameter.POSITIONAL_OR_KEYWORD), params
        assert "batch_size" not in [p[0] for p in params]


@pytest.mark.parametrize("script,args", [("eval_depth.py", []), ("eval_normals.py", [])])
def test_scripts_list_batch_size(script, args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--batch_size" in r.stdout


def test_grouping_rule():
    from diffusion_e2e_ft_amd.evaluate import group_by_shape
    a, b = (3, 40, 56), (3, 36, 52)
    assert group_by_shape([], 4) == []
    assert group_by_shape([a], 1) == [[0]] and group_by_shape([a], 9) == [[0]]
    assert group_by_shape([a] * 5, 1) == [[0], [1], [2], [3], [4]]
    assert group_by_shape([a] * 5, 2) == [[0, 1], [2, 3], [4]]
    assert group_by_shape([a] * 5, 5) == [[0, 1, 2, 3, 4]] == group_by_shape([a] * 5, 6)
    assert group_by_shape([a, b, a, b], 8) == [[0], [1], [2], [3]]                        # only CONSECUTIVE frames of one shape share a batch
    assert group_by_shape([a, a, a, b, b, a], 2) == [[0, 1], [2], [3, 4], [5]]
    assert group_by_shape([list(a), a], 2) == [[0, 1]]                                   # a shape is compared as a tuple
    import torch
    assert group_by_shape([torch.Size(a), a, torch.Size(b)], 3) == [[0, 1], [2]]
    for groups, n in ((group_by_shape([a, a, b, a, a, a, a], 3), 7),):
        assert [i for g in groups for i in g] == list(range(n))                          # dataset order, every frame once
    for bad in (0, -1, None, 2.0, True, "2"):
        with pytest.raises(ValueError, match="batch_size"):
            group_by_shape([a], bad)
