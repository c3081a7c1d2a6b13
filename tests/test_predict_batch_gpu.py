"""Batched, device-resident prediction on the GPU: the per-image min-max kernel (csrc/prepost.hip, ops.minmax_unit_batched) against the single-image op
bit for bit, `predict_batch` of both pipelines against the same steps composed from the existing public pieces, no host synchronisation, and the two
benchmark runners with `predict_batch_size` against their per-frame loop.  Every comparison is exact (tensors as int32 views, CSV cells as float64 bytes)."""
import csv
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import benchmark_fixture as bfx  # noqa: E402
import containment as ct  # noqa: E402
import golden_cases as gc  # noqa: E402
import normal_benchmark_fixture as nfx  # noqa: E402

BATCHES = (1, 2, 3, 8)
SIZES = (1, 2, 63, 64, 65, 255, 1000, 4097, 48 * 64)
KINDS = ("gauss", "const", "ends", "wide", "negzero", "nan", "inf")
FINITE = ("gauss", "const", "ends", "wide", "negzero")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((_bits(a) == _bits(b)).all())


def _image(kind, n, g):
    """one image of n floats (host); every kind is valid at n = 1, where it is a constant image"""
    x = torch.randn(n, generator=g) * 3 + 5
    if kind == "const":
        x = torch.full((n,), 2.5)
    elif kind == "ends":                       # max at the first element, min at the last
        x = torch.rand(n, generator=g) * 0.8 + 0.1
        x[0], x[-1] = 2.0, -1.0
    elif kind == "wide":                       # 1e-30 .. 1e30
        x = (10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 60 - 30)).float()
        x[0], x[-1] = 1e-30, 1e30
    elif kind == "negzero":                    # the minimum is a zero, and zeros of both signs are present
        x = x.abs()
        x[n // 2], x[0], x[-1] = 0.0, 0.0, -0.0
    elif kind == "nan":
        x[n // 2] = float("nan")
    elif kind == "inf":
        x[n // 3] = float("inf")
    return x


def _batch(B, n, shift, seed):
    g = torch.Generator().manual_seed(seed)
    kinds = [KINDS[(shift + b) % len(KINDS)] for b in range(B)]
    return kinds, torch.stack([_image(k, n, g) for k in kinds])


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
def test_kernel_equals_the_single_image_op_bit_for_bit(dev, B):
    """every image kind at every batch position, at every size (odd n: images 1.. start off 16-byte alignment); the yardstick is ops.minmax_unit of the image
    alone in its own allocation — NaN and +inf images included, whatever it gives.  Independent of it: a non-constant finite image has min exactly 0.0, max
    exactly 1.0 and nothing outside [0,1] ((x - mn) <= (mx - mn) survives rounding, and d / d == 1); a constant one is all zeros; minmax is x[b].min(), .max()."""
    from diffusion_e2e_ft_amd import ops
    for n in SIZES:
        for shift in range(len(KINDS)):
            kinds, x = _batch(B, n, shift, seed=1000 * n + shift)
            xd = x.to(dev)
            out, mm = ops.minmax_unit_batched(xd, return_minmax=True)
            assert out.shape == xd.shape and out.dtype == torch.float32 and tuple(mm.shape) == (B, 2)
            assert _same_bits(ops.minmax_unit_batched(xd), out)
            want = torch.stack([ops.minmax_unit(xd[b].clone()) for b in range(B)])
            diff = (_bits(out) != _bits(want)).sum(dim=1).tolist()
            assert diff == [0] * B, (B, n, kinds, diff)
            o, mmh = out.cpu(), mm.cpu()
            for b, kind in enumerate(kinds):
                if kind not in FINITE:
                    continue
                assert mmh[b, 0] == x[b].min() and mmh[b, 1] == x[b].max(), (B, n, kind, mmh[b].tolist())
                if x[b].min() == x[b].max():                      # "const", every kind at n = 1, the two zeros of "negzero" at n = 2
                    assert kind == "const" or n <= 2
                    assert (_bits(o[b]) == 0).all(), (B, n, kind)
                else:
                    assert o[b].min().item() == 0.0 and o[b].max().item() == 1.0, (B, n, kind, o[b].min().item(), o[b].max().item())


def test_kernel_on_a_bigger_shape(dev):
    """480 x 640 x 8: more than 256 row blocks per image, so the first stage strides (the benchmark's shape)"""
    from diffusion_e2e_ft_amd import ops
    x = torch.randn(8, 480, 640, generator=torch.Generator().manual_seed(5)).to(dev)
    x[3] = 7.0
    out = ops.minmax_unit_batched(x)
    for b in range(8):
        assert _same_bits(out[b], ops.minmax_unit(x[b].clone())), b
    assert (_bits(out[3]) == 0).all()


@pytest.mark.parametrize("n", [65, 1000])
def test_images_are_independent(dev, n):
    """rewriting image 1 (with a NaN and an inf in it) changes no bit of images 0 and 2"""
    from diffusion_e2e_ft_amd import ops
    _, x = _batch(3, n, 0, seed=7)
    a = ops.minmax_unit_batched(x.to(dev))
    y = x.clone()
    y[1] = torch.randn(n, generator=torch.Generator().manual_seed(8)) * 1e6
    y[1, 0], y[1, n - 1] = float("nan"), float("inf")
    b = ops.minmax_unit_batched(y.to(dev))
    assert _same_bits(a[0], b[0]) and _same_bits(a[2], b[2]) and not _same_bits(a[1], b[1])


@pytest.mark.parametrize("B,n", [(3, 65), (2, 4097), (8, 64)])
def test_input_one_float_into_an_allocation(dev, B, n):
    from diffusion_e2e_ft_amd import ops
    _, x = _batch(B, n, 2, seed=9)
    want = ops.minmax_unit_batched(x.to(dev))
    buf = torch.zeros(B * n + 8, device=dev)
    view = buf[1:1 + B * n].view(B, n)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert _same_bits(ops.minmax_unit_batched(view), want)


@pytest.mark.parametrize("B,n,col0", [(3, 65, None), (3, 65, 5), (2, 4097, None), (3, 1, 5)])
def test_kernel_writes_only_out_minmax_and_workspace(dev, B, n, col0):
    """containment: x, out, minmax and the workspace are interior views of filled allocations; after the call the bands of all four are intact (x is not
    written at all), and the result does not depend on the fill — the workspace needs no clearing and no image reads past its end"""
    from diffusion_e2e_ft_amd import _lib, ops
    lib = _lib.load()
    _, x = _batch(B, n, 0, seed=11)
    x = x.reshape(-1)
    want = torch.stack([ops.minmax_unit(x.view(B, n)[b].to(dev)) for b in range(B)]).reshape(-1)
    nbytes = lib.e2eft_minmax_unit_batched_workspace_bytes(B)

    def run(fill):
        xb, xv = ct.guarded((B * n,), torch.float32, dev, fill, data=x.to(dev), col0=col0)
        ob, ov = ct.guarded((B * n,), torch.float32, dev, fill, col0=col0)
        mb, mv = ct.guarded((B * 2,), torch.float32, dev, fill, col0=col0)
        wb, wv = ct.guarded((nbytes // 4,), torch.float32, dev, fill)
        rc = lib.e2eft_minmax_unit_batched(B, n, ops._ptr(xv), ops._ptr(ov), ops._ptr(mv), ops._ptr(wv), nbytes, ops._stream())
        assert rc == 0, lib.e2eft_last_error()
        assert _same_bits(xv, x.to(dev)), "the input was written"
        return dict(out=ov, minmax=mv), [(xb, xv), (ob, ov), (mb, mv), (wb, wv)]

    def check(name, t):
        if name == "out":
            assert _same_bits(t, want)
        else:
            assert torch.equal(t.cpu().view(B, 2), torch.stack([x.view(B, n).min(dim=1).values, x.view(B, n).max(dim=1).values], dim=1))

    ct.check_two_fills(run, check, what="minmax_unit_batched B=%d n=%d" % (B, n))


def test_kernel_bad_arguments(dev):
    from diffusion_e2e_ft_amd import _lib, ops
    lib = _lib.load()
    x = torch.randn(2, 10, device=dev)
    out = torch.full_like(x, 7.0)
    nbytes = lib.e2eft_minmax_unit_batched_workspace_bytes(2)
    ws = torch.empty(nbytes // 4, device=dev)
    f = lib.e2eft_minmax_unit_batched
    args = (ops._ptr(x), ops._ptr(out), ops._ptr(None), ops._ptr(ws), nbytes, ops._stream())
    assert f(0, 10, *args) == 0 and f(-2, 10, *args) == 0 and f(2, 0, *args) == 0 and f(2, -1, *args) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                               # nothing was done
    assert f(2, 10, ops._ptr(None), *args[1:]) == 1 and b"null" in lib.e2eft_last_error()
    assert f(2, 10, args[0], ops._ptr(None), *args[2:]) == 1 and f(2, 10, args[0], args[1], args[2], ops._ptr(None), nbytes, args[5]) == 1
    assert f(2, 10, *args[:4], nbytes - 1, args[5]) == 2 and b"workspace" in lib.e2eft_last_error()
    assert (out == 7.0).all()
    assert f(2, 10, *args) == 0 and _same_bits(out, torch.stack([ops.minmax_unit(x[b].clone()) for b in range(2)]))
    with pytest.raises(RuntimeError):
        ops.minmax_unit_batched(x.cpu())
    with pytest.raises(AssertionError):
        ops.minmax_unit_batched(x.t())
    assert tuple(ops.minmax_unit_batched(x[:0]).shape) == (0, 10)


# ---- predict_batch against the composition of the existing pieces ----------------------------------------------------------------------------------------
H0, W0 = 40, 56
PROCESSED_HW = (16, 32)      # processing_res = 32 resizes 40 x 56 to 22 x 32; the VAE's three stride-2 stages keep 22 // 8 = 2 latent rows, so single_infer returns 16 x 32


def _images(B, seed=21):
    return torch.randint(0, 256, (B, 3, H0, W0), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.fixture(scope="module")
def pipe(dev):
    from diffusion_e2e_ft_amd.pipeline import MarigoldPipeline
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    from oracle import config, synth
    unet = UNet2DConditionModel(**config.TINY_UNET)
    unet.load_state_dict(gc.tiny_unet_sd())
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(gc.tiny_vae_sd())
    p = MarigoldPipeline(unet.to(dev).eval(), vae.to(dev).eval(), DDIMScheduler())
    p.empty_text_embed = synth.synth_inputs(2, 64, 96, 2, 128, seed=3)[1][:1].to(dev)
    return p


@pytest.fixture(scope="module")
def geo_pipe(dev):
    from diffusion_e2e_ft_amd.pipeline import DepthNormalEstimationPipeline
    from diffusion_e2e_ft_amd.scheduler import DDIMScheduler
    from diffusion_e2e_ft_amd.unet import UNet2DConditionModel
    from diffusion_e2e_ft_amd.vae import AutoencoderKL
    from oracle import config
    unet = UNet2DConditionModel(**config.TINY_GEOWIZARD_UNET)
    unet.load_state_dict(gc.tiny_geo_sd())
    vae = AutoencoderKL(**config.TINY_VAE)
    vae.load_state_dict(gc.tiny_vae_sd())
    return DepthNormalEstimationPipeline(unet.to(dev).eval(), vae.to(dev).eval(), DDIMScheduler())


def _geo_embed(B, dev):
    from oracle import config
    return (0.5 * torch.randn(B, 1, config.TINY_GEOWIZARD_UNET["cross_attention_dim"], generator=torch.Generator().manual_seed(6))).to(dev)


def _resized_inputs(imgs, processing_res, method):
    """resize_max_res per image (bilinear: the function itself; the other kinds: the same table-driven resampler, rounded to uint8 as resize_max_res does)"""
    from diffusion_e2e_ft_amd.pipeline import resize_device, resize_max_res
    if processing_res == 0:
        return imgs
    if method == "bilinear":
        return torch.stack([resize_max_res(im, processing_res) for im in imgs])
    f = min(processing_res / W0, processing_res / H0)
    return torch.stack([resize_device(im, (int(H0 * f), int(W0 * f)), round_u8=True, kind=method).to(torch.uint8) for im in imgs])


def _compose_marigold(pipe, imgs, processing_res, match, method, normals):
    from diffusion_e2e_ft_amd import ops
    from diffusion_e2e_ft_amd.pipeline import resize_device
    rgb_norm = (_resized_inputs(imgs, processing_res, method) / 255.0 * 2.0 - 1.0).to(pipe.dtype)
    pred = pipe.single_infer(rgb_norm, 1, False, noise="zeros", normals=normals).float()
    out = []
    for p in pred:
        if normals:
            p = p / (torch.norm(p, p=2, dim=0, keepdim=True) + 1e-5)
        else:
            p = ops.minmax_unit(p[0].contiguous())[None]
        if match and tuple(p.shape[-2:]) != (H0, W0):
            p = resize_device(p, (H0, W0), kind=method)
        out.append(p.clamp(-1.0, 1.0) if normals else p[0].clamp(0.0, 1.0))
    return torch.stack(out)


CASES = [(32, m, match) for m in ("bilinear", "bicubic", "nearest") for match in (True, False)] + [(0, "bilinear", True), (0, "nearest", False)]


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("processing_res,method,match", CASES)
def test_marigold_predict_batch_equals_the_composed_steps(dev, pipe, processing_res, method, match, normals):
    imgs = _images(3).to(dev)
    got = pipe.predict_batch(imgs, processing_res=processing_res, match_input_res=match, resample_method=method, normals=normals)
    want = _compose_marigold(pipe, imgs, processing_res, match, method, normals)
    hw = (H0, W0) if match or processing_res == 0 else PROCESSED_HW
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == ((3, 3) if normals else (3,)) + hw
    assert _same_bits(got, want)
    lo = -1.0 if normals else 0.0
    assert got.min().item() >= lo and got.max().item() <= 1.0
    if not normals and (processing_res == 0 or not match):
        assert got.flatten(1).min(dim=1).values.tolist() == [0.0] * 3 and got.flatten(1).max(dim=1).values.tolist() == [1.0] * 3     # per image, not per batch


@pytest.mark.parametrize("processing_res,match", [(32, True), (32, False), (0, True)])
def test_geowizard_predict_batch_equals_the_composed_steps(dev, geo_pipe, processing_res, match):
    from diffusion_e2e_ft_amd import ops
    from diffusion_e2e_ft_amd.pipeline import resize_device
    imgs = _images(3, seed=22).to(dev)
    geo_pipe.img_embed = _geo_embed(3, dev)
    try:
        depth, normal = geo_pipe.predict_batch(imgs, processing_res=processing_res, match_input_res=match, domain="outdoor")
        rgb_norm = (_resized_inputs(imgs, processing_res, "bilinear").float() / 255.0 * 2.0 - 1.0).clamp(-1.0, 1.0).to(geo_pipe.dtype)
        d, n = geo_pipe.single_infer(rgb_norm, domain="outdoor", num_inference_steps=1, noise="zeros")
    finally:
        geo_pipe.img_embed = None
    want_d, want_n = [], []
    for b in range(3):
        db, nb = ops.minmax_unit(d[b, 0].float().contiguous()), n[b].float()
        if match and tuple(db.shape) != (H0, W0):
            db = resize_device(db[None], (H0, W0), kind="bicubic")[0]
            nb = resize_device(nb, (H0, W0), kind="nearest")
        want_d.append(db.clamp(0, 1))
        want_n.append(nb.clamp(-1, 1))
    hw = (H0, W0) if match or processing_res == 0 else PROCESSED_HW
    assert tuple(depth.shape) == (3,) + hw and tuple(normal.shape) == (3, 3) + hw and normal.is_contiguous() and depth.is_contiguous()
    assert _same_bits(depth, torch.stack(want_d)) and _same_bits(normal, torch.stack(want_n))


@pytest.mark.parametrize("processing_res", [32, 0])
def test_batch_of_one_equals_call(dev, pipe, geo_pipe, processing_res):
    """B = 1 against `__call__(..., ensemble_size=1, denoising_steps=1, noise="zeros", color_map=None)`: depth_np and normal_np bit for bit (GeoWizard's
    normal_np is HWC after its resize, so it is compared after permute); a list of PIL images gives what the tensor gives.

    B = 3 against three single calls is printed, not asserted (small layers may pick split-K by tile count, which depends on the batch).  Measured on an MI355X
    with these tiny fp32 models at 40 x 56, processing_res 32 and 0: equal bit for bit in all six cases (Marigold depth, Marigold normals, GeoWizard depth and
    normals).  That is a property of these shapes, not a promise of the kernels."""
    from PIL import Image
    imgs = _images(3, seed=23)
    kw = dict(processing_res=processing_res, match_input_res=True)
    call_kw = dict(kw, ensemble_size=1, denoising_steps=1, noise="zeros", color_map=None, show_progress_bar=False)
    for normals in (False, True):
        batch = pipe.predict_batch(imgs, normals=normals, **kw)
        singles = []
        for b in range(3):
            one = pipe.predict_batch(imgs[b:b + 1], normals=normals, **kw)
            out = pipe(imgs[b], normals=normals, **call_kw)
            ref = out.normal_np if normals else out.depth_np
            assert ref.dtype == np.float32 and _same_bits(one[0], torch.from_numpy(ref)), (normals, b)
            singles.append(one[0])
        print("marigold normals=%s processing_res=%d: B=3 equals three single calls bit for bit: %s"
              % (normals, processing_res, _same_bits(batch, torch.stack(singles))))
        pil = [Image.fromarray(im.permute(1, 2, 0).numpy()) for im in imgs]
        assert _same_bits(pipe.predict_batch(pil, normals=normals, **kw), batch)
    emb = _geo_embed(3, dev)
    try:
        geo_pipe.img_embed = emb
        bd, bn = geo_pipe.predict_batch(imgs, **kw)
        sd, sn = [], []
        for b in range(3):
            geo_pipe.img_embed = emb[b:b + 1]
            d1, n1 = geo_pipe.predict_batch(imgs[b:b + 1], **kw)
            out = geo_pipe(imgs[b], ensemble_size=1, denoising_steps=1, noise="zeros", color_map=None, **kw)
            assert _same_bits(d1[0], torch.from_numpy(out.depth_np)), b
            assert _same_bits(n1[0], torch.from_numpy(out.normal_np).permute(2, 0, 1).contiguous()), b
            sd.append(d1[0])
            sn.append(n1[0])
        print("geowizard processing_res=%d: B=3 equals three single calls bit for bit: depth %s, normals %s"
              % (processing_res, _same_bits(bd, torch.stack(sd)), _same_bits(bn, torch.stack(sn))))
    finally:
        geo_pipe.img_embed = None


def test_predict_batch_refuses_mixed_sizes_and_wrong_tensors(dev, pipe, geo_pipe):
    from PIL import Image
    a = Image.fromarray(np.zeros((40, 56, 3), np.uint8))
    b = Image.fromarray(np.zeros((36, 52, 3), np.uint8))
    for p in (pipe, geo_pipe):
        with pytest.raises(ValueError, match=r"\(36, 52\), \(40, 56\)"):
            p.predict_batch([a, b, a])
        with pytest.raises(ValueError, match="uint8"):
            p.predict_batch(torch.zeros(2, 3, 40, 56))
        with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
            p.predict_batch(torch.zeros(3, 40, 56, dtype=torch.uint8))
        with pytest.raises(ValueError, match="no images"):
            p.predict_batch([])
    with pytest.raises(ValueError, match="resampling"):
        pipe.predict_batch([a], resample_method="lanczos")
    with pytest.raises(TypeError):
        pipe.predict_batch([a], ensemble_size=2)


def test_predict_batch_does_not_synchronise(dev, pipe, geo_pipe):
    """after one warm-up call per configuration (weight packing, resampler tables, the timestep tensor), the calls run under torch's sync debug mode "error",
    which raises on every synchronising torch call: .item(), .cpu(), a host assert on a tensor, a blocking copy"""
    imgs = _images(3, seed=24).to(dev)
    geo_pipe.img_embed = _geo_embed(3, dev)
    calls = [lambda: pipe.predict_batch(imgs, processing_res=32), lambda: pipe.predict_batch(imgs, processing_res=32, normals=True, resample_method="bicubic"),
             lambda: pipe.predict_batch(imgs, processing_res=0, match_input_res=False), lambda: geo_pipe.predict_batch(imgs, processing_res=32)]
    try:
        warm = [c() for c in calls]
        torch.cuda.synchronize()
        old = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = [c() for c in calls]
        finally:
            torch.cuda.set_sync_debug_mode(old)
    finally:
        geo_pipe.img_embed = None
    for w, a in zip(warm, again):
        for tw, ta in zip(w if isinstance(w, tuple) else (w,), a if isinstance(a, tuple) else (a,)):
            assert _same_bits(tw, ta)
    with pytest.raises(RuntimeError):                       # the mode does catch a synchronising call here
        torch.cuda.set_sync_debug_mode("error")
        try:
            warm[0].sum().item()
        finally:
            torch.cuda.set_sync_debug_mode(old)


# ---- the runners -----------------------------------------------------------------------------------------------------------------------------------------
class _Out:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class DepthStandIn:
    """depth is one fixed function of the image, computed on the device in fp32 in one operation order by `__call__` (one frame) and `predict_batch`"""

    def __init__(self, dev):
        self.dev, self.calls, self.batches = dev, [], []

    def _depth(self, rgb):
        a = rgb.to(torch.float32)
        H, W = a.shape[-2:]
        yy = torch.arange(H, device=a.device, dtype=torch.float32)[:, None]
        xx = torch.arange(W, device=a.device, dtype=torch.float32)[None, :]
        return (a[:, 0] * 0.5 + a[:, 1] * 0.3 + a[:, 2] * 0.2) / 255.0 * 0.6 + 0.3 * yy / H + 0.1 * xx / W

    def __call__(self, image, **kw):
        self.calls.append(kw)
        rgb = torch.from_numpy(np.ascontiguousarray(np.asarray(image).transpose(2, 0, 1)))[None].to(self.dev)
        return _Out(depth_np=self._depth(rgb)[0].cpu().numpy())

    def predict_batch(self, images, **kw):
        assert images.dtype == torch.uint8 and images.is_cuda and images.dim() == 4 and images.shape[1] == 3
        self.batches.append((images.shape[0], tuple(images.shape[2:]), kw))
        return self._depth(images)


class NormalStandIn(DepthStandIn):
    def _normals(self, rgb):
        a = rgb.to(torch.float32) / 255.0 * 2.0 - 1.0
        H, W = a.shape[-2:]
        yy = torch.arange(H, device=a.device, dtype=torch.float32)[:, None]
        xx = torch.arange(W, device=a.device, dtype=torch.float32)[None, :]
        return torch.stack([a[:, 0] * 0.8 + 0.1 * xx / W, a[:, 1] * 0.7 - 0.1 * yy / H, 0.3 + 0.5 * a[:, 2].abs()], dim=1)

    def __call__(self, image, **kw):
        self.calls.append(kw)
        rgb = torch.from_numpy(np.ascontiguousarray(np.asarray(image).transpose(2, 0, 1)))[None].to(self.dev)
        return _Out(normal_np=self._normals(rgb)[0].cpu().numpy())

    def predict_batch(self, images, **kw):
        assert images.dtype == torch.uint8 and images.is_cuda and images.dim() == 4 and images.shape[1] == 3
        self.batches.append((images.shape[0], tuple(images.shape[2:]), kw))
        return self._normals(images)


class GeoStyleStandIn(NormalStandIn):
    """returns the (depth, normals) pair of DepthNormalEstimationPipeline.predict_batch"""

    def predict_batch(self, images, **kw):
        return self._depth(images), super().predict_batch(images, **kw)


def _read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def _npy_files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs if f.endswith(".npy"))


def _expected_batches(shapes, bs):
    from diffusion_e2e_ft_amd.evaluate import group_by_shape
    return [(len(g), tuple(shapes[g[0]])) for g in group_by_shape(shapes, bs)]


@pytest.fixture(scope="module")
def depth_trees(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("depth_batched"))
    return {"scannet": bfx.make_tree(root, "scannet"), "nyu_v2": bfx.make_tree(root, "nyu_v2")}


def _depth_ds(name, tree, dev):
    from diffusion_e2e_ft_amd import eval_data
    return eval_data.dataset_name_class_dict[name](mode=eval_data.DatasetMode.EVAL, filename_ls_path=tree["filenames"], dataset_dir=tree["tar"], disp_name=name,
                                                   device=dev, **bfx.FLAGS[name])


@pytest.mark.parametrize("name,alignment", [("scannet", "least_square"), ("scannet", "least_square_disparity"), ("nyu_v2", "least_square")])
def test_depth_runner_in_batches_equals_the_loop(dev, depth_trees, tmp_path, name, alignment):
    """scannet: three frames of one shape; nyu_v2: 480 x 640 then 64 x 96, so a group ends at the shape change.  The same result dict, CSV (text, and cells as
    float64 bytes), metrics text and .npy files for predict_batch_size None, 1, 2 and len + 1: ops.depth_eval gives a frame the same bits whatever its batch neighbours."""
    from diffusion_e2e_ft_amd import evaluate
    ds = _depth_ds(name, depth_trees[name], dev)
    shapes = [tuple(ds[i]["rgb_int"].shape[1:]) for i in range(len(ds))]
    base_pipe, base_out = DepthStandIn(dev), str(tmp_path / "loop")
    base = evaluate.evaluate_depth_benchmark(base_pipe, ds, alignment=alignment, output_dir=base_out, save_predictions=True)
    assert len(base_pipe.calls) == len(ds) and base_pipe.batches == []
    header, base_rows = _read_csv(os.path.join(base_out, "per_sample_metrics.csv"))
    base_text = open(os.path.join(base_out, "eval_metrics-%s.txt" % alignment)).read()
    assert len(base_rows) == len(ds) and len(_npy_files(base_out)) == len(ds)
    for bs in (1, 2, len(ds) + 1):
        pipe, out = DepthStandIn(dev), str(tmp_path / ("bs%d" % bs))
        res = evaluate.evaluate_depth_benchmark(pipe, ds, alignment=alignment, output_dir=out, save_predictions=True, predict_batch_size=bs, processing_res=0)
        assert pipe.calls == [] and len(pipe.batches) == sum(math.ceil(n / bs) for n in ([len(ds)] if len(set(shapes)) == 1 else [1] * len(ds)))
        assert [(b, hw) for b, hw, _ in pipe.batches] == _expected_batches(shapes, bs) and all(kw == {"processing_res": 0} for _, _, kw in pipe.batches)
        assert res == base and list(res) == list(evaluate.METRIC_NAMES)
        h, rows = _read_csv(os.path.join(out, "per_sample_metrics.csv"))
        assert h == header and [r[0] for r in rows] == [r[0] for r in base_rows]
        for r, b in zip(rows, base_rows):
            assert [np.float64(c).tobytes() for c in r[1:]] == [np.float64(c).tobytes() for c in b[1:]], (bs, r[0])
        assert open(os.path.join(out, "per_sample_metrics.csv")).read() == open(os.path.join(base_out, "per_sample_metrics.csv")).read()
        assert open(os.path.join(out, "eval_metrics-%s.txt" % alignment)).read() == base_text.replace(base_out, out)
        assert _npy_files(out) == _npy_files(base_out)
        for rel in _npy_files(out):
            a, b = np.load(os.path.join(out, rel)), np.load(os.path.join(base_out, rel))
            assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes(), (bs, rel)
        assert sorted(os.listdir(out)) == sorted(os.listdir(base_out))


def test_depth_runner_in_batches_skips_a_frame_without_valid_pixels(dev, tmp_path):
    from diffusion_e2e_ft_amd import eval_data, evaluate
    tree = bfx.make_tree(str(tmp_path), "scannet", all_invalid=1)
    ds = eval_data.ScanNetDataset(mode=eval_data.DatasetMode.EVAL, filename_ls_path=tree["filenames"], dataset_dir=tree["dir"], disp_name="scannet", device=dev)
    with pytest.warns(UserWarning, match="scene0012_00/color/000100.png has no valid"):
        base = evaluate.evaluate_depth_benchmark(DepthStandIn(dev), ds, output_dir=str(tmp_path / "loop"))
    for bs in (1, 2, 3):
        pipe = DepthStandIn(dev)
        with pytest.warns(UserWarning, match="scene0012_00/color/000100.png has no valid"):
            res = evaluate.evaluate_depth_benchmark(pipe, ds, output_dir=str(tmp_path / ("bs%d" % bs)), predict_batch_size=bs)
        assert res == base and pipe.calls == [] and [b for b, _, _ in pipe.batches] == {1: [1, 1, 1], 2: [2, 1], 3: [3]}[bs]
        assert open(str(tmp_path / ("bs%d" % bs) / "per_sample_metrics.csv")).read() == open(str(tmp_path / "loop" / "per_sample_metrics.csv")).read()
        assert not os.path.exists(str(tmp_path / ("bs%d" % bs) / "scene0011_00"))


def test_depth_runner_with_the_product_pipeline(dev, pipe, depth_trees):
    """the runner over MarigoldPipeline.predict_batch itself: the metrics are those of the batches' predictions measured by hand"""
    from diffusion_e2e_ft_amd import evaluate
    ds = _depth_ds("scannet", depth_trees["scannet"], dev)
    res = evaluate.evaluate_depth_benchmark(pipe, ds, predict_batch_size=2, processing_res=0)
    tracker = evaluate.MetricTracker(*evaluate.METRIC_NAMES)
    for idx in ([0, 1], [2]):
        items = [ds[i] for i in idx]
        pred = pipe.predict_batch(torch.stack([it["rgb_int"] for it in items]).to(torch.uint8), processing_res=0)
        m = evaluate.depth_metrics(pred, torch.stack([it["depth_raw_linear"][0] for it in items]), torch.stack([it["valid_mask_raw"][0] for it in items]),
                                   min_depth=ds.min_depth, max_depth=ds.max_depth)
        for j in range(len(idx)):
            for k in evaluate.METRIC_NAMES:
                tracker.update(k, float(m[k][j]))
    assert res == tracker.result() and all(np.isfinite(v) for v in res.values())


@pytest.fixture(scope="module")
def normal_trees(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("normals_batched"))
    return {name: nfx.make_tree(root, name) for name in nfx.NAMES}


@pytest.mark.parametrize("cls", [NormalStandIn, GeoStyleStandIn])
@pytest.mark.parametrize("name", nfx.NAMES)
def test_normal_runner_in_batches_equals_the_loop(dev, normal_trees, tmp_path, name, cls):
    """every tree has two image shapes (sintel: 5 x 7, 5 x 7, 9 x 1, 20 x 33): groups end at a shape change"""
    from diffusion_e2e_ft_amd import evaluate, normal_eval_data as nd
    ds = nd.NormalBenchmarkDataset(name, normal_trees[name]["dir"], normal_trees[name]["split"], device=dev)
    shapes = [tuple(s[2]) for s in nfx.SAMPLES[name]]
    assert len(set(shapes)) > 1
    base_pipe = cls(dev)
    base = evaluate.evaluate_normal_benchmark(base_pipe, ds, output_dir=str(tmp_path / "loop"))
    assert len(base_pipe.calls) == len(ds) and base_pipe.batches == [] and base["n"] > 0
    base_text = open(str(tmp_path / "loop" / "test" / name / "metrics.txt")).read()
    for bs in (1, 2, len(ds) + 1):
        pipe = cls(dev)
        res = evaluate.evaluate_normal_benchmark(pipe, ds, output_dir=str(tmp_path / ("bs%d" % bs)), predict_batch_size=bs, processing_res=0)
        assert pipe.calls == [] and [(b, hw) for b, hw, _ in pipe.batches] == _expected_batches(shapes, bs)
        assert all(kw == {"processing_res": 0} for _, _, kw in pipe.batches)
        assert res == base, (bs, res, base)
        assert open(str(tmp_path / ("bs%d" % bs) / "test" / name / "metrics.txt")).read() == base_text


def test_runners_need_predict_batch(dev, depth_trees, normal_trees):
    from diffusion_e2e_ft_amd import evaluate, normal_eval_data as nd

    class CallOnly:
        def __call__(self, image, **kw):
            raise AssertionError("not reached")

    ds = _depth_ds("scannet", depth_trees["scannet"], dev)
    nds = nd.NormalBenchmarkDataset("scannet", normal_trees["scannet"]["dir"], normal_trees["scannet"]["split"], device=dev)
    with pytest.raises(TypeError, match="predict_batch"):
        evaluate.evaluate_depth_benchmark(CallOnly(), ds, predict_batch_size=2)
    with pytest.raises(TypeError, match="predict_batch"):
        evaluate.evaluate_normal_benchmark(CallOnly(), nds, predict_batch_size=1)
    with pytest.raises(TypeError, match="predict_batch"):
        evaluate.evaluate_normal_benchmark(lambda image, **kw: None, nds, predict_batch_size=3)
    both = DepthStandIn(dev)              # a `batch_size` among the keywords is still the pipeline's own, in the loop and in batches
    evaluate.evaluate_depth_benchmark(both, ds, batch_size=1)
    evaluate.evaluate_depth_benchmark(both, ds, predict_batch_size=2, batch_size=1)
    assert both.calls == [{"batch_size": 1}] * len(ds) and [kw for _, _, kw in both.batches] == [{"batch_size": 1}] * 2
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError, match="predict_batch_size must be"):
            evaluate.evaluate_depth_benchmark(DepthStandIn(dev), ds, predict_batch_size=bad)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match=r"predict_batch returned \(1, 5, 7\)"):
            evaluate.evaluate_normal_benchmark(DepthStandIn(dev), nds, predict_batch_size=1)             # a depth tensor where normals are due
