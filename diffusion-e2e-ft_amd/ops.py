"""Thin Python wrappers over the libe2eft C ABI (include/e2eft.h).

Tensors are torch CUDA(HIP) tensors used purely as device memory: NHWC activations are `[B, H, W, C]` tensors whose
last dim is contiguous and whose pixel stride `ld = t.stride(-2)` may exceed C (channel slice of a wider buffer).
Every function enqueues on torch's current stream and raises RuntimeError on any library error; there is no
fallback path."""
import ctypes as C
from types import SimpleNamespace

import torch

from . import _lib
from ._lib import ConvDesc, GemmDesc, GroupNormDesc, AttnDesc, check, dtype_id


class KernelTimer:
    """Optional per-launch timing with HIP events on the launch stream (torch's current stream): bench.py uses it to
    compute achieved TFLOP/s / GB/s per kernel family over the timed region.  Inactive (zero overhead) by default."""

    def __init__(self, only=None):
        self.rec = {}
        self.only = only      # None: every instrumented launch; else a set of family names ("igemm", ...): the others run un-instrumented

    def add(self, name, start, end, flops, nbytes, label=None, launches=1, flops_nominal=None):
        # flops: what the kernels multiply; flops_nominal: the layer's work in the reference's formulation when that is more (e2eft_upconv2x_fwd multiplies 4/9 of it)
        self.rec.setdefault(name, []).append((start, end, flops, nbytes, label, launches, flops if flops_nominal is None else flops_nominal))      # launches: kernels of the family behind ONE library call (e2eft_upconv2x_fwd: four)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, lst in self.rec.items():
            ms = sum(r[0].elapsed_time(r[1]) for r in lst)
            out[name] = dict(launches=sum(r[5] for r in lst), ms=ms, flops=float(sum(r[2] for r in lst)), bytes=float(sum(r[3] for r in lst)),
                             flops_nominal=float(sum(r[6] for r in lst)))
        return out

    def by_label(self):
        """{(name, label): dict(launches, ms, flops, bytes)} for shape-level analysis"""
        torch.cuda.synchronize()
        out = {}
        for name, lst in self.rec.items():
            for r in lst:
                d = out.setdefault((name, r[4]), dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
                d["launches"] += r[5]
                d["ms"] += r[0].elapsed_time(r[1])
                d["flops"] += r[2]
                d["bytes"] += r[3]
        return out


TIMER = None  # set to a KernelTimer to record


class _timed:
    def __init__(self, name, flops=0.0, nbytes=0.0, label=None, launches=1, flops_nominal=None):
        self.name, self.flops, self.nbytes, self.label, self.launches, self.flops_nominal = name, flops, nbytes, label, launches, flops_nominal

    def __enter__(self):
        self.on = TIMER is not None and (TIMER.only is None or self.name in TIMER.only)
        if self.on:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *a):
        if self.on:
            self.e.record()
            label = self.label
            if self.name == "igemm":     # which kernel symbol the library's dispatch picked for this launch (debug entry, not in e2eft.h)
                label = (label, _last_kernel())
            TIMER.add(self.name, self.s, self.e, self.flops, self.nbytes, label, self.launches, self.flops_nominal)
        return False


def _last_kernel():
    lib = _lib.load()
    fn = lib.e2eft_debug_last_kernel
    fn.restype = C.c_char_p
    return fn().decode()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def dtype_size(dtype):
    return 4 if dtype == torch.float32 else 2


def epc(dtype):
    """elements per 16-byte chunk"""
    return 4 if dtype == torch.float32 else 8


def round_up(v, m):
    return (v + m - 1) // m * m


def _check_cuda(*ts):
    """Every wrapper passes its tensors through here before it launches: they must be HIP tensors of ONE device, and that device must
    be the calling thread's current device — the library launches on `torch.cuda.current_stream()`, i.e. on a stream of the CURRENT
    device, so device-1 pointers under a current device 0 would be launched on the wrong GPU.  The caller's current device is never
    changed behind their back: run a model that lives on another device inside `with torch.cuda.device(model.device):` (the pipelines'
    entry points do that themselves, `pipeline._on_device`)."""
    idx = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("libe2eft ops need device (HIP) tensors; got a %s tensor. There is no CPU fallback." % t.device)
        if idx is None:
            idx = t.device.index
        elif t.device.index != idx:
            raise RuntimeError("libe2eft ops need all tensors of a call on one device; got cuda:%d and cuda:%d" % (idx, t.device.index))
    if idx is not None and idx != torch.cuda.current_device():
        raise RuntimeError("libe2eft ops launch on the current device's stream: tensors live on cuda:%d but the current device is cuda:%d; "
                           "wrap the call in `with torch.cuda.device(%d):`" % (idx, torch.cuda.current_device(), idx))


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NULL = _NullCtx()


def on_device_of(t):
    """context manager: the device of tensor / module-parameter `t` is the current device inside (a no-op object when it already is)"""
    dev = t.device
    if dev.type != "cuda" or dev.index is None or dev.index == torch.cuda.current_device():
        return _NULL
    return torch.cuda.device(dev)


def device_scoped(fn):
    """decorator for the entry points of the host layer (module forwards, pipeline calls): runs the call with the device of the first
    tensor argument (or of `self`'s first parameter) as the current device and restores the caller's current device afterwards"""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        t = next((a for a in args if isinstance(a, torch.Tensor) and a.is_cuda), None)
        if t is None and isinstance(self, torch.nn.Module):
            t = next(self.parameters(), None)
        if t is None and isinstance(getattr(type(self), "device", None), property):   # pipelines: .device of their UNet
            dev = self.device
            if dev.type == "cuda" and dev.index is not None and dev.index != torch.cuda.current_device():
                with torch.cuda.device(dev):
                    return fn(self, *args, **kwargs)
            return fn(self, *args, **kwargs)
        if t is None or not t.is_cuda:
            return fn(self, *args, **kwargs)
        with on_device_of(t):
            return fn(self, *args, **kwargs)

    return wrapper


def tensor_scoped(fn):
    """the free-function twin of device_scoped (evaluate / data / ensemble entry points): the call runs with the device of its first HIP tensor argument as
    the current device — a model on cuda:1 can be evaluated from a thread whose current device is cuda:0 (these raised since _check_cuda stopped switching)"""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        t = next((a for a in list(args) + list(kwargs.values()) if isinstance(a, torch.Tensor) and a.is_cuda), None)
        if t is None:
            return fn(*args, **kwargs)
        with on_device_of(t):
            return fn(*args, **kwargs)

    return wrapper


def _nhwc_ld(t):
    """pixel stride of an NHWC view [B,H,W,C]; validates that pixels are densely strided"""
    assert t.dim() == 4, t.shape
    B, H, W, Cc = t.shape
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if B > 1 else max(Cc, 1)))
    if Cc > 1 and t.stride(3) != 1:
        raise ValueError("NHWC view must have unit channel stride, got strides %s" % (t.stride(),))
    if (W > 1 and t.stride(2) != ld) or (H > 1 and t.stride(1) != W * ld) or (B > 1 and t.stride(0) != H * W * ld):
        raise ValueError("NHWC view must be pixel-dense: shape %s strides %s" % (tuple(t.shape), t.stride()))
    return ld


def _rows_ld(t):
    """row stride of a 2-D row-major view [rows, C]"""
    assert t.dim() == 2, t.shape
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError("row view must have unit column stride")
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))


def new_nhwc(B, H, W, Cc, dtype, device):
    """Output buffer; channel count padded to a 16-byte multiple with zeros in the pad (returned view has C channels)."""
    cp = round_up(Cc, epc(dtype))
    if cp == Cc:
        return torch.empty((B, H, W, Cc), dtype=dtype, device=device)
    return torch.zeros((B, H, W, cp), dtype=dtype, device=device)[..., :Cc]


def pad_channels(x):
    """Copy an NHWC view whose C is not a 16-byte multiple into a zero-padded buffer (rgb / 4-channel latents only)."""
    B, H, W, Cc = x.shape
    e = epc(x.dtype)
    if Cc % e == 0:
        return x
    out = torch.zeros((B, H, W, round_up(Cc, e)), dtype=x.dtype, device=x.device)
    copy_scale(x, out[..., :Cc])
    return out  # full padded view: consumers index weights packed with the same padding


class GnStats:
    """GroupNorm partial statistics emitted by the producer of a tensor (e2eft_*_gnstats): [images, nslabs, C, 3] fp32."""
    __slots__ = ("partial", "nslabs")

    def __init__(self, partial, nslabs):
        self.partial, self.nslabs = partial, nslabs


GN_STATS_ENABLED = True   # tests flip this to cross-check the fused statistics against the stand-alone pass
SPLITK_ENABLED = True     # tests flip this to cross-check split-K convolutions against the single-pass kernel


UPCONV_PHASES_ENABLED = True     # tests / A-B: False keeps 2x-upsample convolutions on the fused-upsample 3x3 form


def _launch_with_stats(launch, out, want, images, rows_per_image, cout):
    """One library call that can emit the GroupNorm partial statistics of `out` from its epilogue.  launch(buf_ptr, nbytes, slab_ref) makes the call and returns its
    status; with `want` it is handed the statistics buffer, and the statistics are attached to `out` when the kernel reports a slab height (0: it emitted none)."""
    buf, nbytes = None, 0
    if want:
        nbytes = images * ((rows_per_image + 127) // 128) * cout * 12
        buf = torch.empty(nbytes // 4, dtype=torch.float32, device=out.device)
    slab = C.c_int32(0)
    check(launch(_ptr(buf), nbytes, C.byref(slab)))
    if want and slab.value > 0:
        nslabs = rows_per_image // slab.value
        out._e2eft_gn = GnStats(buf[: images * nslabs * cout * 3], nslabs)
    return out


def f32_split2(x, keep=False, x2=None):
    """fp32 NHWC [B,H,W,C] or row view [M,C] (C % 8 == 0) -> (planes f16 [..., 2C] = [x0 | x1] with x * s = x0 + x1 to 2^-22, scale workspace fp32 [4]: [1] = s, [2] = 1 / s).
    s is the power of two that brings the tensor's maximum into [2^14, 2^15), found on the device (csrc/f32split.hip).
    keep: park the result on the tensor object; a second call returns it only while x has the same `_version` AND no library call has been made since — the
    library's kernels write through raw pointers (ops.add(out=), ops.copy_scale, ops.cast_, ...) and bump no version, so any launch in between may have refilled x.
    For a caller that splits one tensor for several consumers before it launches any of them; nothing in the package does at present (a weight gradient takes
    per-channel planes of dY, f32_split2_cols, and the data gradient of the same dY launches its convolution right behind its split).  The planes live as long as x
    does.  x2 (NHWC only): a second source — the planes are then those of cat(x, x2) along the channels, under one scale."""
    _check_cuda(x, x2)
    Cc = x.shape[-1]
    assert x.dtype == torch.float32 and Cc % 8 == 0
    if x.dim() == 2:
        pixels, ld, label = x.shape[0], _rows_ld(x), "split2 rows M%d K%d" % (x.shape[0], Cc)
    else:
        B, H, W, _ = x.shape
        pixels, ld, label = B * H * W, _nhwc_ld(x), "split2 B%d %dx%d C%d" % (B, H, W, Cc)
    ent = getattr(x, "_e2eft_planes", None) if keep else None
    if ent is not None and ent[0] == (x._version, _lib.CALLS[0]):
        return ent[1], ent[2]
    c2 = 0 if x2 is None else x2.shape[3]
    planes = torch.empty(tuple(x.shape[:-1]) + (2 * (Cc + c2),), dtype=torch.float16, device=x.device)
    scale = torch.empty(4, dtype=torch.float32, device=x.device)
    if x2 is not None:
        assert tuple(x2.shape[:3]) == tuple(x.shape[:3]) and x2.dtype == torch.float32 and c2 % 8 == 0 and not keep
        with _timed("f32split", 0.0, 12.0 * pixels * (Cc + c2), label="%s+%d" % (label, c2), launches=4):
            check(_lib.load().e2eft_f32_split2_cat(_ptr(x), Cc, ld, _ptr(x2), c2, _nhwc_ld(x2), pixels, _ptr(planes), 2 * (Cc + c2), _ptr(scale), _stream()))
    else:
        with _timed("f32split", 0.0, 12.0 * pixels * Cc, label=label, launches=2):
            check(_lib.load().e2eft_f32_split2(_ptr(x), pixels, Cc, ld, _ptr(planes), 2 * Cc, _ptr(scale), _stream()))
    if keep:
        x._e2eft_planes = ((x._version, _lib.CALLS[0]), planes, scale)
    return planes, scale


def f32_split2_cols(x, x2=None):
    """fp32 NHWC x (x2: cat(x, x2) along the channels) -> (planes f16 [..., 2C] = [x0 | x1], inverse scales fp32 [C]): f32_split2 under one power-of-two scale per
    CHANNEL, found on the device (e2eft_f32_split2_cols) — the operands of a weight gradient, whose algebra separates per channel (conv2d_wgrad)."""
    _check_cuda(x, x2)
    B, H, W, Cc = x.shape
    c2 = 0 if x2 is None else x2.shape[3]
    assert x.dtype == torch.float32 and Cc % 8 == 0 and c2 % 8 == 0 and (x2 is None or (tuple(x2.shape[:3]) == (B, H, W) and x2.dtype == torch.float32))
    ctot, pixels = Cc + c2, B * H * W
    planes = torch.empty((B, H, W, 2 * ctot), dtype=torch.float16, device=x.device)
    cs = torch.empty(2 * ctot, dtype=torch.float32, device=x.device)
    with _timed("f32split", 0.0, 12.0 * pixels * ctot, label="split2 cols B%d %dx%d C%d" % (B, H, W, ctot), launches=2 if x2 is None else 4):
        check(_lib.load().e2eft_f32_split2_cols(_ptr(x), Cc, _nhwc_ld(x), _ptr(x2), c2, _nhwc_ld(x2) if x2 is not None else 0, pixels, _ptr(planes), 2 * ctot, _ptr(cs),
                                                _stream()))
    return planes, cs[ctot:]


def f32_split_weight(w_packed, taps, c):
    """fp32 packed weight [cout, taps*c] (rows (tap, c)) -> (f16 [cout, taps*3c] rows (tap, [w0 | w1 | w0]) with w * s_w = w0 + w1, device scalar 1 / s_w).  s_w is the
    power of two that brings the weight's maximum into [2^14, 2^15), computed on the device (trainable weights change every optimizer step: no host read).  Cached on
    the packed tensor object per version (autograd.packed_conv_weight hands out one object per parameter version)."""
    ent = getattr(w_packed, "_e2eft_split", None)
    if ent is not None and ent[0] == w_packed._version:
        return ent[1], ent[2]
    rows = w_packed.numel() // c                   # cout * taps (a [4, cout, taps * c] stack of phase weights splits as one tensor: one scale)
    assert w_packed.dtype == torch.float32 and w_packed.shape[-1] == taps * c and w_packed.is_contiguous() and c % 8 == 0
    src = w_packed.detach() if w_packed.data_ptr() % 16 == 0 else w_packed.detach().clone()      # (a slice of a flat buffer may start off a 16-byte boundary)
    wsp = torch.empty((rows // taps, taps * 3 * c), dtype=torch.float16, device=w_packed.device)
    scale = torch.empty(4, dtype=torch.float32, device=w_packed.device)
    check(_lib.load().e2eft_f32_split_weight(_ptr(src), rows, c, _ptr(wsp), _ptr(scale), _stream()))      # (two launches; as tensor-library calls this was a dozen per weight)
    inv = scale[2:3]
    w_packed._e2eft_split = (w_packed._version, wsp, inv)
    return wsp, inv


# ---------------------------------------------------------------------------------------------------------
# the descriptors of the C ABI (include/e2eft.h): each struct is created in one place
def _conv_out_hw(hl, wl, kh, kw, stride, pad):
    """output grid of a convolution over the logical (upsampled) hl x wl input, pad = (top, bottom, left, right)"""
    pt, pb, pl, pr = pad
    return (hl + pt + pb - kh) // stride + 1, (wl + pl + pr - kw) // stride + 1


def _conv_desc(x, x2, cout, kh, kw, stride, pad, up_to, alpha, ldo=0, ldr=0, ldw=0, dtype=None):
    """x: the NHWC tensor [B,H,W,c1] the launch reads, or — for operands that are no such tensor (split planes, the shape a gradient will have) — the geometry
    (B, H, W, c1, ldx1) with `dtype` the library's id; x2: the second source likewise, a tensor, (c2, ldx2) or None.  pad = (top, bottom, left, right), up_to = (hl, wl)
    of a fused nearest upsample; hout / wout follow from them.  ldo / ldr / ldw stay 0 for the entries that take those strides as arguments of their own."""
    if isinstance(x, torch.Tensor):
        (B, H, W, c1), ldx1, dtype = x.shape, _nhwc_ld(x), dtype_id(x.dtype)
    else:
        B, H, W, c1, ldx1 = x
    if isinstance(x2, torch.Tensor):
        x2 = (x2.shape[3], _nhwc_ld(x2))
    hl, wl = (H, W) if up_to is None else up_to
    d = ConvDesc()
    d.dtype = dtype
    d.batch, d.hin, d.win, d.hl, d.wl = B, H, W, hl, wl
    d.c1, d.ldx1 = c1, ldx1
    d.c2, d.ldx2 = (0, 0) if x2 is None else x2
    d.kh, d.kw, d.stride, d.pad_t, d.pad_l = kh, kw, stride, pad[0], pad[2]
    d.hout, d.wout = _conv_out_hw(hl, wl, kh, kw, stride, pad)
    d.cout, d.ldo, d.ldr, d.ldw = cout, ldo, ldr, ldw
    d.alpha = alpha
    return d


def _gemm_desc(dtype, m, n, k, lda, ldw, ldo, ldr=0, nz=(1, 1), sa=(0, 0), sw=(0, 0), so=(0, 0), bias_along_m=False, alpha=1.0):
    """dtype: the library's id; nz = (outer, inner) batch counts, sa / sw / so = (outer, inner) batch strides in elements (the residual is not batched)"""
    d = GemmDesc()
    d.dtype = dtype
    d.m, d.n, d.k = m, n, k
    d.lda, d.ldw, d.ldo, d.ldr = lda, ldw, ldo, ldr
    d.nzo, d.nzi = nz
    d.sa_o, d.sa_i = sa
    d.sw_o, d.sw_i = sw
    d.so_o, d.so_i = so
    d.sr_o = d.sr_i = 0
    d.bias_along_m = 1 if bias_along_m else 0
    d.alpha = alpha
    return d


def _gn_desc(x, x2, groups, eps, silu, ldy):
    B, H, W, c1 = x.shape
    d = GroupNormDesc()
    d.dtype = dtype_id(x.dtype)
    d.batch, d.hw = B, H * W
    d.c1, d.ldx1 = c1, _nhwc_ld(x)
    d.c2, d.ldx2 = (x2.shape[3], _nhwc_ld(x2)) if x2 is not None else (0, 0)
    d.groups, d.ldy, d.silu, d.eps = groups, ldy, 1 if silu else 0, eps
    return d


def _gn_workspace(d, device, who="groupnorm", bwd=False):
    """-> (fp32 workspace tensor of the norm `d` describes, its size in bytes as the library counts it); bwd: the backward's.  0 bytes is the library's refusal."""
    lib = _lib.load()
    nbytes = (lib.e2eft_groupnorm_bwd_workspace_bytes if bwd else lib.e2eft_groupnorm_workspace_bytes)(C.byref(d))
    if nbytes == 0:
        raise RuntimeError("%s: %s" % (who, lib.e2eft_last_error().decode()))
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device), nbytes


def _gn_stats_args(s):
    """optional GnStats of a norm's source -> the (partial, nslabs) argument pair; (null, 0): the norm makes its own statistics pass"""
    return (_ptr(s.partial), s.nslabs) if s else (C.c_void_p(0), 0)


def _f32split_desc(B, H, W, c1, cout, kh, kw, stride, pad, ldo, ldr, up_to=None, alpha=1.0):
    """descriptor of a launch that reads split planes of c1 fp32 channels (pixel stride 2 c1); up_to = (hl, wl): the fused 2x upsample of e2eft_upconv2x_fwd_f32split"""
    return _conv_desc((B, H, W, c1, 2 * c1), None, cout, kh, kw, stride, pad, up_to, alpha, ldo, ldr, kh * kw * 3 * c1, dtype=_lib.F32)


def _f32split_takes(dtype, cin, ldw, taps, alpha, bias, up_to=None, rowadd=None, sk=0):
    """What every fp32 convolution must meet to go through split planes, whichever wrapper asks (conv2d, conv2d_norm_split, conv2d_dgrad), before the library judges its
    descriptor: no fused upsample, row vector or split-K; an alpha other than 1 only without a bias; weight rows of exactly taps * cin columns (f32_split_weight splits
    the packed tensor as it lies).  What a site asks beyond these — channel multiples: conv2d_norm_split leaves the input's to the library's query — stays at the site."""
    return dtype == torch.float32 and not sk and up_to is None and rowadd is None and (alpha == 1.0 or bias is None) and ldw == taps * cin


def f32split_shape_ok(B, H, W, c1, cout, kh=3, kw=3, stride=1, pad=(1, 1, 1, 1)):
    """pure host arithmetic: would the library run this fp32 convolution [B,H,W,c1] -> cout from f16 split planes (e2eft_conv2d_fwd_f32split_supported: 0 for every
    shape while E2EFT_OPT_F32_SPLIT is off)?"""
    if c1 % 64 != 0 or cout % 8 != 0:
        return False
    d = _f32split_desc(B, H, W, c1, cout, kh, kw, stride, pad, cout, cout)
    return _lib.load().e2eft_conv2d_fwd_f32split_supported(C.byref(d)) == 1


def f32split_operands_ok(sources, others=()):
    """What every launch of the split route asks of its operands, beyond the shape its `*_supported` query judges.  sources: the fp32 tensors the split pass reads
    (NHWC or row views, None skipped) — 16-byte aligned base, channels % 8, pixel stride % 4 (e2eft_f32_split2's requirements; a view that is not pixel-dense is not
    eligible either).  others: bias / residual / output (None skipped) — 16-byte aligned base."""
    try:
        for t in sources:
            if t is not None and (t.data_ptr() % 16 or t.shape[-1] % 8 or (_rows_ld(t) if t.dim() == 2 else _nhwc_ld(t)) % 4):
                return False
    except ValueError:
        return False
    return all(t is None or t.data_ptr() % 16 == 0 for t in others)


def groupnorm_fwd_split_ws(x, gamma, beta, groups, eps, silu=False, s1=None):
    """fp32 GroupNorm(+SiLU) of x [B,H,W,C] whose output leaves as f16 split planes (e2eft_groupnorm_fwd_split) -> (planes [B,H,W,2C], scale workspace [4] for the
    consuming convolution, workspace for groupnorm_bwd).  The scale comes from a bound of the output, |y| <= max|gamma| * sqrt(H W C / groups) + max|beta|, computed
    on the device: no host read of the parameters, no pass over the data."""
    _check_cuda(x, gamma, beta)
    B, H, W, c1 = x.shape
    assert x.dtype == torch.float32
    planes = torch.empty((B, H, W, 2 * c1), dtype=torch.float16, device=x.device)
    scale = torch.empty(4, dtype=torch.float32, device=x.device)
    d = _gn_desc(x, None, groups, eps, silu, c1)
    ws, nbytes = _gn_workspace(d, x.device)
    if not GN_STATS_ENABLED:
        s1 = None
    with _timed("groupnorm", 0.0, 2.0 * B * H * W * c1 * 4, label="gn->split B%d %dx%d C%d" % (B, H, W, c1)):
        check(_lib.load().e2eft_groupnorm_fwd_split(C.byref(d), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(planes), 2 * c1, _ptr(scale), *_gn_stats_args(s1), _ptr(ws), nbytes,
                                                    _stream()))
    return planes, scale, ws


def _f32split_conv_desc(B, H, W, c1, w_packed, bias, cout, residual, alpha, out, geom, sources):
    """The descriptor of e2eft_conv2d_fwd_f32split for an fp32 convolution (geom = kh, kw, stride, pads; no fused upsample) of [B,H,W,c1], or None when the route does
    not take it.  Host arithmetic only: nothing is launched.  sources: the fp32 tensors that will be split (none when the planes come from a producer)."""
    d = _f32split_desc(B, H, W, c1, cout, *geom, _nhwc_ld(out), _nhwc_ld(residual) if residual is not None else 0, alpha=alpha)
    assert (d.hout, d.wout) == (out.shape[1], out.shape[2])
    if (_lib.load().e2eft_conv2d_fwd_f32split_supported(C.byref(d)) != 1 or not w_packed.is_contiguous()
            or not f32split_operands_ok(sources, (out, residual, bias))):
        return None
    return d


def _f32split_conv_launch(d, planes, scale, wsplit, bias, residual, out, want, label):
    B, H, W, cout, kk = d.batch, d.hout, d.wout, d.cout, d.kh * d.kw * d.c1          # (H, W: the OUTPUT grid)
    wsp, inv_sw = wsplit
    lib = _lib.load()
    nb = (planes.numel() * 2 + B * H * W * cout * 4 * (2 if residual is not None else 1) + cout * 3 * kk * 2)
    # (flops: what the f16 pipe multiplies — three products per fp32 product; flops_nominal: the fp32 convolution)
    with _timed("igemm", 6.0 * B * H * W * cout * kk, nb, label=label + " f32split", flops_nominal=2.0 * B * H * W * cout * kk):
        _launch_with_stats(lambda buf, nbytes, slab: lib.e2eft_conv2d_fwd_f32split(
            C.byref(d), _ptr(planes), _ptr(scale), _ptr(wsp), _ptr(inv_sw), _ptr(bias), _ptr(residual), _ptr(out), buf, nbytes, slab, _stream()), out, want, B, H * W, cout)
    return out


def _conv2d_f32split(x, w_packed, bias, cout, residual, alpha, out, want, label, geom=(3, 3, 1, (1, 1, 1, 1)), x2=None):
    """An fp32 convolution of x (x2: of cat(x, x2) — one pair of planes, one scale) through e2eft_conv2d_fwd_f32split, or None when the route does not take it."""
    c1 = x.shape[3] + (x2.shape[3] if x2 is not None else 0)
    d = _f32split_conv_desc(*x.shape[:3], c1, w_packed, bias, cout, residual, alpha, out, geom, (x, x2))
    if d is None:
        return None
    wsplit = f32_split_weight(w_packed, geom[0] * geom[1], c1)
    planes, scale = f32_split2(x, x2=x2)
    return _f32split_conv_launch(d, planes, scale, wsplit, bias, residual, out, want, label)


def conv2d_norm_split(x, norm, w_packed, bias, cout, residual=None, alpha=1.0, out=None, gn_stats=False, s1=None):
    """The fp32 3x3 / stride-1 / pad-1 convolution of GroupNorm(+SiLU)(x), norm = (gamma, beta, groups, eps, silu): the norm's apply pass writes the f16 split planes the
    convolution reads (csrc/f32split.hip) — no fp32 intermediate, no maximum pass.  s1: GnStats of x from its producer.  -> (out, the workspace groupnorm_bwd wants), or
    None when the route does not take the convolution: that is known before anything is launched."""
    B, H, W, c1 = x.shape
    if not _f32split_takes(x.dtype, c1, w_packed.shape[1], 9, alpha, bias) or cout % 8 != 0:
        return None
    _check_cuda(x, w_packed, bias, residual, out)
    if out is None:
        out = new_nhwc(B, H, W, cout, x.dtype, x.device)
    d = _f32split_conv_desc(B, H, W, c1, w_packed, bias, cout, residual, alpha, out, (3, 3, 1, (1, 1, 1, 1)), ())
    if d is None:
        return None
    gamma, beta, groups, eps, silu = norm
    planes, scale, ws = groupnorm_fwd_split_ws(x, gamma, beta, groups, eps, silu=silu, s1=s1)
    _f32split_conv_launch(d, planes, scale, f32_split_weight(w_packed, 9, c1), bias, residual, out, gn_stats and GN_STATS_ENABLED, "conv3x3s1n B%d %dx%d %d->%d" % (B, H, W, c1, cout))
    return out, ws


# ---------------------------------------------------------------------------------------------------------
# ops.conv2d: the validated call (a namespace `c`: operands, arguments, descriptor `d`, and `geom` = (B, H, W, cin, cout, kh, kw, stride, hout, wout) as plain
# integers — reading them back from the ctypes struct costs more than everything else a route does on the host) is offered to the routes below in order.  A route
# either takes the call and returns `out`, or returns None having launched nothing.
def _conv_label(c, normed=False):
    B, H, W, cin, cout, kh, kw, stride, hout, wout = c.geom
    return c.label or "conv%dx%ds%d%s%s B%d %dx%d %d->%d" % (kh, kw, stride, "u" if c.up_to else "", "n" if normed else "", B, hout, wout, cin, cout)


def _conv_timed(c, normed=False):
    """the timer entry of a launch of the implicit-GEMM kernels on the operands as they lie"""
    B, H, W, cin, cout, kh, kw, stride, hout, wout = c.geom
    nb = (B * H * W * cin + B * hout * wout * cout * (2 if c.residual is not None else 1) + cout * kh * kw * cin) * c.x.element_size()
    return _timed("igemm", 2.0 * B * hout * wout * cout * kh * kw * cin, nb, label=_conv_label(c, normed))


def _upconv_phases_apply(c):
    """nearest-2x upsample + 3x3 / stride 1 / pad 1: four 2x2 phase convolutions of the low-resolution input (4/9 of the multiply-adds)"""
    B, H, W, cin, cout, kh, kw, stride, hout, wout = c.geom
    return (c.w_phase is not None and UPCONV_PHASES_ENABLED and c.up_to is not None and c.x2 is None and c.rowadd is None and c.residual is None and c.norm is None
            and c.alpha == 1.0 and (kh, kw, stride) == (3, 3, 1) and c.pad == (1, 1, 1, 1) and tuple(c.up_to) == (2 * H, 2 * W))


def _conv_upconv_f32split(c):
    """fp32: the four 2x2 phases on the f16 matrix pipe from split planes (csrc/f32split.hip)"""
    x, d, out = c.x, c.d, c.out
    B, H, W, c1, cout, kh, kw, stride, hout, wout = c.geom      # (one source: cin is c1)
    if not (_upconv_phases_apply(c) and x.dtype == torch.float32 and c1 % 64 == 0 and f32split_operands_ok((x,), (out, c.bias))):
        return None
    lib = _lib.load()
    ds = _f32split_desc(B, H, W, c1, cout, kh, kw, stride, c.pad, d.ldo, 0, up_to=c.up_to)
    if lib.e2eft_upconv2x_fwd_f32split_supported(C.byref(ds)) != 1:
        return None
    wp = c.w_phase()
    assert tuple(wp.shape) == (4, cout, 4 * c1) and wp.dtype == torch.float32
    wsp, inv_sw = f32_split_weight(wp, 4, c1)
    planes, scale = f32_split2(x)
    nbp = planes.numel() * 2 + B * hout * wout * cout * 4 + wsp.numel() * 2
    with _timed("igemm", 6.0 * B * H * W * 4 * cout * 4 * c1, nbp, label="upconv2x(4 phases) B%d %dx%d %d->%d f32split" % (B, hout, wout, c1, cout), launches=4,
                flops_nominal=2.0 * B * hout * wout * cout * 9 * c1):
        _launch_with_stats(lambda buf, nbytes, slab: lib.e2eft_upconv2x_fwd_f32split(
            C.byref(ds), _ptr(planes), _ptr(scale), _ptr(wsp), _ptr(inv_sw), _ptr(c.bias), _ptr(out), buf, nbytes, slab, _stream()), out, c.want, B, hout * wout, cout)
    return out


def _conv_upconv(c):
    """the four 2x2 phases in the operands' own dtype (e2eft_upconv2x_fwd)"""
    x, d, out = c.x, c.d, c.out
    lib = _lib.load()
    if not (_upconv_phases_apply(c) and lib.e2eft_upconv2x_fwd_supported(C.byref(d)) == 1):
        return None
    B, H, W, c1, cout, kh, kw, stride, hout, wout = c.geom
    wp = c.w_phase()
    assert tuple(wp.shape) == (4, cout, 4 * c1) and wp.is_contiguous() and wp.dtype == x.dtype, (wp.shape, wp.dtype)
    nbp = (B * H * W * c1 + B * hout * wout * cout + 4 * cout * 4 * c1) * x.element_size()
    with _timed("igemm", 2.0 * B * H * W * 4 * cout * 4 * c1, nbp, label="upconv2x(4 phases) B%d %dx%d %d->%d" % (B, hout, wout, c1, cout), launches=4,
                flops_nominal=2.0 * B * hout * wout * cout * 9 * c1):
        _launch_with_stats(lambda buf, nbytes, slab: lib.e2eft_upconv2x_fwd(C.byref(d), _ptr(x), _ptr(wp), _ptr(c.bias), _ptr(out), buf, nbytes, slab, _stream()),
                           out, c.want, B, hout * wout, cout)
    return out


def _conv_normed(c):
    """GroupNorm(+SiLU) applied in the convolution's operand fetch (e2eft_conv2d_fwd_normed): only the norm's statistics are finalised beforehand"""
    x, d, out = c.x, c.d, c.out
    B, H, W, cin, cout, kh, kw, stride, hout, wout = c.geom
    gamma, beta, groups, eps, silu = c.norm
    lib = _lib.load()
    # (the <= 4-output-channel route of the supported query, narrow.hip, takes neither a row vector nor a residual nor statistics: ADVICE r3)
    narrow_ok = cout > 4 or (c.rowadd is None and c.residual is None and not c.want)
    if not (NORM_FUSION_ENABLED and c.x2 is None and not c.sk and narrow_ok and lib.e2eft_conv2d_fwd_normed_supported(C.byref(d)) == 1):
        return None
    ws, coeff = groupnorm_stats(x, gamma, groups, eps)     # (a, mean) pairs; the apply pass is the convolution's operand fetch
    with _conv_timed(c, normed=True):
        _launch_with_stats(lambda buf, nbytes, slab: lib.e2eft_conv2d_fwd_normed(
            C.byref(d), _ptr(x), C.c_void_p(coeff), _ptr(beta), 1 if silu else 0, _ptr(c.w), _ptr(c.bias), _ptr(c.rowadd), _ptr(c.residual), _ptr(out), buf, nbytes, slab,
            _stream()), out, c.want, B, hout * wout, cout)
    out._e2eft_keep = ws            # (the coefficient workspace lives as long as the launch may: stream-ordered free after the output)
    return out


def _conv_norm_split(c):
    """fp32 3x3 / stride 1 / pad 1: the norm's apply pass writes the f16 split planes the convolution reads (conv2d_norm_split)"""
    B, H, W, cin, cout, kh, kw, stride, hout, wout = c.geom
    if not (c.x2 is None and not c.sk and c.up_to is None and c.rowadd is None and (kh, kw, stride) == (3, 3, 1) and c.pad == (1, 1, 1, 1)):
        return None
    r = conv2d_norm_split(c.x, c.norm, c.w, c.bias, cout, c.residual, c.alpha, c.out, c.gn_stats, s1=getattr(c.x, "_e2eft_gn", None))      # (fp32; None: nothing was launched)
    return None if r is None else r[0]


def _conv_f32split(c):
    """fp32 on the f16 matrix pipe from split planes of the input (of the concatenated input: one pair of planes)"""
    B, H, W, cin, cout, kh, kw, stride, hout, wout = c.geom
    if not (_f32split_takes(c.x.dtype, cin, c.w.shape[1], kh * kw, c.alpha, c.bias, c.up_to, c.rowadd, c.sk) and cin % 64 == 0):
        return None
    return _conv2d_f32split(c.x, c.w, c.bias, cout, c.residual, c.alpha, c.out, c.want, _conv_label(c), geom=(kh, kw, stride, c.pad), x2=c.x2)


def _conv_direct(c):
    """the implicit-GEMM kernels on the operands as they lie — split-K, with the statistics of `out`, or plain: takes every call that gets here"""
    d, out = c.d, c.out
    B, H, W, cin, cout, kh, kw, stride, hout, wout = c.geom
    lib = _lib.load()
    args = (C.byref(d), _ptr(c.x), _ptr(c.x2), _ptr(c.w), _ptr(c.bias), _ptr(c.rowadd), _ptr(c.residual), _ptr(out))
    with _conv_timed(c):
        if c.sk:   # few output tiles, long reduction: split-K (the consumer GroupNorm computes its own statistics)
            ws = torch.empty(c.sk // c.x.element_size(), dtype=c.x.dtype, device=c.x.device)
            check(lib.e2eft_conv2d_fwd_splitk(*args, _ptr(ws), c.sk, _stream()))
        elif c.want:
            _launch_with_stats(lambda buf, nbytes, slab: lib.e2eft_conv2d_fwd_gnstats(*args, buf, nbytes, slab, _stream()), out, True, B, hout * wout, cout)
        else:
            check(lib.e2eft_conv2d_fwd(*args, _stream()))
    return out


def _first_taker(c, *routes):
    for route in routes:
        out = route(c)
        if out is not None:
            return out
    return None


def conv2d(x, w_packed, bias, cout, kh, kw, stride=1, pad=(0, 0, 0, 0), x2=None, up_to=None, rowadd=None,
           residual=None, alpha=1.0, out=None, gn_stats=False, norm=None, w_phase=None, _label=None):
    """Implicit-GEMM convolution. x: [B,H,W,C1] (C1 % epc == 0), x2: optional [B,H,W,C2] fused channel concat,
    w_packed: [cout, ldw] rows = (ky,kx,c) K-contiguous, pad = (top, bottom, left, right), up_to=(hl,wl) fused
    nearest upsample, rowadd: [B,cout] per-image vector added before alpha, residual: [B,hout,wout,cout].
    norm = (gamma, beta, groups, eps, silu): the convolution of GroupNorm(+SiLU)(x) — where the library can (e2eft_conv2d_fwd_normed_supported) the
    norm is never applied as a pass of its own: its statistics are finalised and the convolution reads x through them; otherwise groupnorm() runs first."""
    _check_cuda(x, w_packed, x2, bias, rowadd, residual, out)
    B, H, W, c1 = x.shape
    hout, wout = _conv_out_hw(*((H, W) if up_to is None else up_to), kh, kw, stride, pad)
    if out is None:
        out = new_nhwc(B, hout, wout, cout, x.dtype, x.device)
    assert tuple(out.shape) == (B, hout, wout, cout), (out.shape, (B, hout, wout, cout))
    cin = c1 + (x2.shape[3] if x2 is not None else 0)
    if x2 is not None:
        assert x2.shape[:3] == x.shape[:3] and x2.dtype == x.dtype
    if residual is not None:
        assert tuple(residual.shape) == tuple(out.shape) and residual.dtype == x.dtype
    assert w_packed.dim() == 2 and w_packed.shape[0] == cout and w_packed.is_contiguous() and w_packed.dtype == x.dtype
    assert w_packed.shape[1] >= kh * kw * cin, (w_packed.shape, kh, kw, c1, cin - c1)
    if bias is not None:
        assert bias.dtype == x.dtype and bias.numel() == cout and bias.is_contiguous()
    if rowadd is not None:
        assert rowadd.dtype == x.dtype and tuple(rowadd.shape) == (B, cout) and rowadd.is_contiguous()
    d = _conv_desc(x, x2, cout, kh, kw, stride, pad, up_to, alpha, _nhwc_ld(out), _nhwc_ld(residual) if residual is not None else 0, w_packed.shape[1])
    c = SimpleNamespace(x=x, x2=x2, w=w_packed, bias=bias, rowadd=rowadd, residual=residual, out=out, d=d, geom=(B, H, W, cin, cout, kh, kw, stride, hout, wout),
                        alpha=alpha, pad=tuple(pad), up_to=up_to, norm=norm, w_phase=w_phase, label=_label, gn_stats=gn_stats,
                        want=gn_stats and GN_STATS_ENABLED and cout % 8 == 0, sk=0)
    if _first_taker(c, _conv_upconv_f32split, _conv_upconv) is not None:
        return out
    c.sk = _lib.load().e2eft_conv2d_splitk_workspace_bytes(C.byref(d)) if SPLITK_ENABLED else 0
    if norm is not None:
        if _first_taker(c, _conv_normed, _conv_norm_split) is not None:      # these read x through the norm
            return out
        # neither: the norm runs as a pass of its own, and the routes below read its output
        gamma, beta, groups, eps, silu = norm
        c.x = groupnorm(x, gamma, beta, groups, eps, silu=silu, x2=x2)      # the norm of the CONCATENATED input; its output is one tensor
        c.x2 = None
        c.d = _conv_desc(c.x, None, cout, kh, kw, stride, pad, up_to, alpha, d.ldo, d.ldr, d.ldw)
    return _first_taker(c, _conv_f32split, _conv_direct)


def _gemm_f32split(a, w, bias, residual, out, alpha, ldo, ldr):
    """fp32 nn.Linear of whole 256-row tiles: two-term f16 split planes on the f16 matrix pipe (csrc/f32split.hip; igemm5's GEMM mode), or None having launched nothing"""
    (M, K), N = a.shape, w.shape[0]
    if not ((alpha == 1.0 or bias is None) and K % 64 == 0 and M > 256 and N % 8 == 0 and w.is_contiguous() and f32split_operands_ok((a,), (out, residual, bias))):
        return None
    ds = _gemm_desc(_lib.F32, M, N, K, 2 * K, 3 * K, ldo, ldr, alpha=alpha)
    lib = _lib.load()
    if lib.e2eft_gemm_f32split_supported(C.byref(ds)) != 1:
        return None
    wsp, inv_sw = f32_split_weight(w, 1, K)
    planes, scale = f32_split2(a)
    with _timed("igemm", 6.0 * M * N * K, (M * 2 * K * 2 + N * 3 * K * 2 + M * N * 4 * (2 if residual is not None else 1)), label="gemm M%d N%d K%d f32split" % (M, N, K),
                flops_nominal=2.0 * M * N * K):
        check(lib.e2eft_gemm_f32split(C.byref(ds), _ptr(planes), _ptr(scale), _ptr(wsp), _ptr(inv_sw), _ptr(bias), _ptr(residual), _ptr(out), _stream()))
    return out


def gemm(a, w, bias=None, residual=None, out=None, alpha=1.0, bias_along_m=False, gn_rows_per_image=0):
    """out[m,n] = alpha*(sum_k a[m,k] w[n,k] + bias) + residual.  a: [M,K] view, w: [N,K] view.
    gn_rows_per_image > 0: also emit GroupNorm partial statistics of `out` (attached as out._e2eft_gn)."""
    _check_cuda(a, w, bias, residual, out)
    M, K = a.shape
    N, K2 = w.shape
    assert K == K2 and a.dtype == w.dtype
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    assert tuple(out.shape) == (M, N) and out.dtype == a.dtype
    d = _gemm_desc(dtype_id(a.dtype), M, N, K, _rows_ld(a), _rows_ld(w), _rows_ld(out), _rows_ld(residual) if residual is not None else 0, bias_along_m=bias_along_m, alpha=alpha)
    if bias is not None:
        assert bias.dtype == a.dtype and bias.is_contiguous() and bias.numel() == (M if bias_along_m else N)
    if residual is not None:
        assert tuple(residual.shape) == (M, N) and residual.dtype == a.dtype
    want = gn_rows_per_image > 0 and GN_STATS_ENABLED and N % 8 == 0 and M % gn_rows_per_image == 0 and not bias_along_m
    if a.dtype == torch.float32 and not want and not bias_along_m and _gemm_f32split(a, w, bias, residual, out, alpha, d.ldo, d.ldr) is not None:
        return out
    with _timed("igemm", 2.0 * M * N * K, (M * K + N * K + M * N * (2 if residual is not None else 1)) * a.element_size(), label="gemm M%d N%d K%d" % (M, N, K)):
        if want:
            _launch_with_stats(lambda buf, nbytes, slab: _lib.load().e2eft_gemm_gnstats(
                C.byref(d), _ptr(a), _ptr(w), _ptr(bias), _ptr(residual), _ptr(out), gn_rows_per_image, buf, nbytes, slab, _stream()), out, True, M // gn_rows_per_image, gn_rows_per_image, N)
        else:
            check(_lib.load().e2eft_gemm(C.byref(d), _ptr(a), _ptr(w), _ptr(bias), _ptr(residual), _ptr(out), _stream()))
    return out


def bgemm_raw(dtype, m, n, k, a, lda, sa, w, ldw, sw, out, ldo, so, nzo, nzi, bias=None, bias_along_m=False, alpha=1.0):
    """Batched NT GEMM on raw base tensors with explicit element strides. sa/sw/so = (outer, inner) batch strides.
    a / w / out are tensors whose data_ptr() is the z = 0 base."""
    _check_cuda(a, w, out, bias)
    d = _gemm_desc(dtype_id(dtype), m, n, k, lda, ldw, ldo, 0, (nzo, nzi), sa, sw, so, bias_along_m, alpha)
    with _timed("igemm", 2.0 * m * n * k * nzo * nzi, float(nzo * nzi) * (m * k + n * k + m * n) * dtype_size(dtype), label="bgemm z%d M%d N%d K%d" % (nzo * nzi, m, n, k)):
        check(_lib.load().e2eft_gemm(C.byref(d), _ptr(a), _ptr(w), _ptr(bias), _ptr(None), _ptr(out), _stream()))
    return out


def linear(x, weight, bias=None, residual=None, out=None, alpha=1.0, gn_rows_per_image=0):
    """nn.Linear on the last dim of x [..., K] (dense rows); weight [N, K]."""
    K = x.shape[-1]
    a = x.reshape(-1, K) if x.is_contiguous() else _as_rows(x)
    r = None
    if residual is not None:
        r = residual.reshape(-1, residual.shape[-1]) if residual.is_contiguous() else _as_rows(residual)
    N = weight.shape[0]
    o2 = None
    if out is not None:
        o2 = out.reshape(-1, N) if out.is_contiguous() else _as_rows(out)
    y = gemm(a, weight, bias, r, o2, alpha, gn_rows_per_image=gn_rows_per_image)
    res = y.reshape(*x.shape[:-1], N) if out is None else out
    st = getattr(y, "_e2eft_gn", None)
    if st is not None:
        res._e2eft_gn = st
    return res


def _as_rows(t):
    """[..., C] view with dense leading dims and a row stride -> 2-D [rows, C] as_strided view."""
    Cc = t.shape[-1]
    ld = t.stride(-2)
    rows = 1
    for s in t.shape[:-1]:
        rows *= s
    # verify leading dims are dense w.r.t. ld
    exp = ld
    for i in range(t.dim() - 2, -1, -1):
        if t.shape[i] > 1 and t.stride(i) != exp:
            raise ValueError("cannot flatten view with shape %s strides %s" % (tuple(t.shape), t.stride()))
        exp *= t.shape[i]
    return t.as_strided((rows, Cc), (ld, 1))


# ---------------------------------------------------------------------------------------------------------
def groupnorm_fwd_ws(x, gamma, beta, groups, eps, silu=False, x2=None, s1=None, s2=None, out=None):
    """GroupNorm(+SiLU) over NHWC x [B,H,W,C1] (optionally concatenated with x2 along C) -> (out, its workspace: mean / rstd live there for groupnorm_bwd).
    s1 / s2: GnStats of x / x2 emitted by their producers (statistics pass skipped for that source)."""
    _check_cuda(x, gamma, beta, x2, out)
    B, H, W, c1 = x.shape
    c2 = 0 if x2 is None else x2.shape[3]
    if out is None:
        out = torch.empty((B, H, W, c1 + c2), dtype=x.dtype, device=x.device)
    d = _gn_desc(x, x2, groups, eps, silu, _nhwc_ld(out))
    ws, nbytes = _gn_workspace(d, x.device)
    if gamma is not None:
        assert gamma.dtype == x.dtype and gamma.numel() == c1 + c2
    if not GN_STATS_ENABLED:
        s1 = s2 = None
    if x2 is None:
        s2 = None
    with _timed("groupnorm", 0.0, 2.0 * B * H * W * (c1 + c2) * x.element_size(), label="gn B%d %dx%d C%d" % (B, H, W, c1 + c2)):
        check(_lib.load().e2eft_groupnorm_fwd_pre(C.byref(d), _ptr(x), _ptr(x2), _ptr(gamma), _ptr(beta), _ptr(out), *_gn_stats_args(s1), *_gn_stats_args(s2), _ptr(ws), nbytes,
                                                  _stream()))
    return out, ws


def groupnorm(x, gamma, beta, groups, eps, silu=False, x2=None, out=None):
    """groupnorm_fwd_ws with the statistics the producers of x / x2 left on them, into `out` if given, without the workspace"""
    return groupnorm_fwd_ws(x, gamma, beta, groups, eps, silu, x2, getattr(x, "_e2eft_gn", None), getattr(x2, "_e2eft_gn", None), out)[0]


NORM_FUSION_ENABLED = True    # conv2d(norm=...): GroupNorm(+SiLU) applied inside the consuming convolution where the library supports it


def groupnorm_stats(x, gamma, groups, eps):
    """The statistics half of groupnorm() alone -> (workspace, device address of the fp32 (a, mean) pairs [B][C][2] inside it)."""
    _check_cuda(x, gamma)
    B, H, W, c1 = x.shape
    d = _gn_desc(x, None, groups, eps, False, c1)
    ws, nbytes = _gn_workspace(d, x.device, "groupnorm_stats")
    s1 = getattr(x, "_e2eft_gn", None) if GN_STATS_ENABLED else None
    lib = _lib.load()
    with _timed("groupnorm_stats", 0.0, 0.0, label="gn stats B%d %dx%d C%d" % (B, H, W, c1)):
        check(lib.e2eft_groupnorm_fwd_stats(C.byref(d), _ptr(x), C.c_void_p(0), _ptr(gamma), *_gn_stats_args(s1), C.c_void_p(0), 0, _ptr(ws), nbytes, _stream()))
    return ws, ws.data_ptr() + lib.e2eft_groupnorm_coeff_offset(C.byref(d))


def layernorm(x, gamma, beta, eps, out=None):
    _check_cuda(x, gamma, beta, out)
    Cc = x.shape[-1]
    a = x.reshape(-1, Cc) if x.is_contiguous() else _as_rows(x)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    o = out.reshape(-1, Cc) if out.is_contiguous() else _as_rows(out)
    assert gamma.dtype == x.dtype and beta.dtype == x.dtype
    check(_lib.load().e2eft_layernorm_fwd(dtype_id(x.dtype), a.shape[0], Cc, _rows_ld(a), _rows_ld(o), eps, _ptr(a), _ptr(gamma),
                                         _ptr(beta), _ptr(o), _stream()))
    return out


def geglu(h, out=None):
    """h [..., 2c] -> h[..., :c] * gelu(h[..., c:])"""
    _check_cuda(h, out)
    c2 = h.shape[-1]
    c = c2 // 2
    a = h.reshape(-1, c2) if h.is_contiguous() else _as_rows(h)
    if out is None:
        out = torch.empty((*h.shape[:-1], c), dtype=h.dtype, device=h.device)
    o = out.reshape(-1, c) if out.is_contiguous() else _as_rows(out)
    check(_lib.load().e2eft_geglu_fwd(dtype_id(h.dtype), a.shape[0], c, _rows_ld(a), _rows_ld(o), _ptr(a), _ptr(o), _stream()))
    return out


def softmax_rows_(s, n, scale, causal_nq=0):
    """in-place softmax(scale * s[r, :n]) over a 2-D [rows, lds] contiguous buffer; pad columns [n, roundup) zeroed.
    causal_nq > 0: row r is query r % causal_nq and sees keys 0 .. r % causal_nq only."""
    _check_cuda(s)
    assert s.dim() == 2 and s.is_contiguous()
    if causal_nq:
        check(_lib.load().e2eft_softmax_rows_causal(dtype_id(s.dtype), s.shape[0], n, s.shape[1], scale, causal_nq, _ptr(s), _stream()))
    else:
        check(_lib.load().e2eft_softmax_rows(dtype_id(s.dtype), s.shape[0], n, s.shape[1], scale, _ptr(s), _stream()))
    return s


def _ld3(t):
    if t.shape[2] > 1 and t.stride(2) != 1:
        raise ValueError("attention operands need unit inner stride")
    ld = t.stride(1) if t.shape[1] > 1 else max(t.shape[2], t.stride(1))
    if t.shape[0] > 1 and t.stride(0) != t.shape[1] * ld:
        raise ValueError("attention operands must be batch-dense: %s %s" % (tuple(t.shape), t.stride()))
    return ld


def _attn_desc(q, k, v, out, heads, scale, kv_nseg, kv_bmod):
    B, Nq, Wd = q.shape
    Bkv, Nk, _ = k.shape
    assert Wd == heads * 64 and k.shape[2] == Wd and v.shape == k.shape
    d = AttnDesc()
    d.dtype = dtype_id(q.dtype)
    d.batch, d.heads, d.nq, d.nk_seg = B, heads, Nq, Nk
    d.kv_nseg = kv_nseg
    d.kv_bmod = B if kv_bmod is None else kv_bmod
    assert Bkv >= d.kv_bmod * kv_nseg
    d.ldq, d.ldk, d.ldv, d.ldo = _ld3(q), _ld3(k), _ld3(v), _ld3(out)
    d.scale = scale
    return d


def attention(q, k, v, heads, scale, kv_nseg=1, kv_bmod=None, out=None, return_lse=False):
    """Fused attention, head dim 64. q: [B,Nq,heads*64] view, k/v: [Bkv,Nk,heads*64] views (row-strided).
    return_lse: also return the [B, heads, Nq] fp32 log-sum-exp the fused backward needs."""
    _check_cuda(q, k, v, out)
    B, Nq, Wd = q.shape
    Nk = k.shape[1]
    if out is None:
        out = torch.empty((B, Nq, Wd), dtype=q.dtype, device=q.device)
    d = _attn_desc(q, k, v, out, heads, scale, kv_nseg, kv_bmod)
    lse = torch.empty((B, heads, Nq), dtype=torch.float32, device=q.device) if return_lse else None
    with _timed("attn", 4.0 * B * heads * Nq * Nk * kv_nseg * 64, label="attn B%d h%d Nq%d Nk%d" % (B, heads, Nq, Nk * kv_nseg)):
        check(_lib.load().e2eft_attn_fwd_lse(C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), _stream()))
    return (out, lse) if return_lse else out


ATTN512_SPLIT_TAIL = True   # tests / A-B: without a workspace every query block runs all keys in one workgroup


def attention512(q, k, v, scale, out=None):
    """Fused attention of ONE 512-wide head (the VAE mid-block attention), fp16 / bf16.  q / k / v: [B, N, 512] views (row-strided: slices
    of one fused q|k|v projection are fine)."""
    _check_cuda(q, k, v, out)
    B, Nq, Wd = q.shape
    Nk = k.shape[1]
    assert Wd == 512 and k.shape[2] == 512 and v.shape == k.shape and k.shape[0] == B
    if out is None:
        out = torch.empty((B, Nq, 512), dtype=q.dtype, device=q.device)
    d = AttnDesc()
    d.dtype = dtype_id(q.dtype)
    d.batch, d.heads, d.nq, d.nk_seg, d.kv_nseg, d.kv_bmod = B, 1, Nq, Nk, 1, B
    d.ldq, d.ldk, d.ldv, d.ldo = _ld3(q), _ld3(k), _ld3(v), _ld3(out)
    d.scale = scale
    lib = _lib.load()
    nbytes = lib.e2eft_attn512_workspace_bytes(C.byref(d)) if ATTN512_SPLIT_TAIL else 0
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device) if nbytes else None
    with _timed("attn512", 4.0 * B * Nq * Nk * 512, label="attn512 B%d Nq%d Nk%d" % (B, Nq, Nk)):
        check(lib.e2eft_attn512_fwd(C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(ws), nbytes, _stream()))
    return out


def attention_bwd(q, k, v, out, dout, lse, heads, scale, dq, dk, dv):
    """Fused attention backward (head dim 64; fp16 / bf16 / strict fp32): writes dq / dk / dv (row-strided views shaped like q / k / v)."""
    _check_cuda(q, k, v, out, dout, lse, dq, dk, dv)
    B, Nq, Wd = q.shape
    Nk = k.shape[1]
    d = _attn_desc(q, k, v, out, heads, scale, 1, None)
    assert dout.shape == out.shape and dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    assert lse.shape == (B, heads, Nq) and lse.dtype == torch.float32 and lse.is_contiguous()
    lib = _lib.load()
    nbytes = lib.e2eft_attn_bwd_workspace_bytes(C.byref(d))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
    with _timed("attn_bwd", 14.0 * B * heads * Nq * Nk * 64, label="attn_bwd B%d h%d Nq%d Nk%d" % (B, heads, Nq, Nk)):
        check(lib.e2eft_attn_bwd(C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(dout), _ld3(dout), _ptr(lse), _ptr(dq), _ld3(dq), _ptr(dk), _ld3(dk),
                                 _ptr(dv), _ld3(dv), _ptr(ws), nbytes, _stream()))


# ---------------------------------------------------------------------------------------------------------
def nchw_to_nhwc(x, dtype=None, cpad=None, mul=1.0, add=0.0):
    """[B,C,H,W] contiguous -> NHWC [B,H,W,cpad] (zero padded channels), y = x*mul + add."""
    _check_cuda(x)
    x = x.contiguous()
    B, Cc, H, W = x.shape
    dtype = dtype or x.dtype
    cp = round_up(Cc, epc(dtype)) if cpad is None else cpad
    y = torch.empty((B, H, W, cp), dtype=dtype, device=x.device)
    check(_lib.load().e2eft_nchw_to_nhwc(dtype_id(x.dtype), dtype_id(dtype), B, Cc, H * W, cp, cp, mul, add, _ptr(x), _ptr(y), _stream()))
    return y


def nhwc_to_nchw(x, dtype=None, mul=1.0, add=0.0):
    """NHWC view [B,H,W,C] -> contiguous [B,C,H,W]"""
    _check_cuda(x)
    B, H, W, Cc = x.shape
    dtype = dtype or x.dtype
    y = torch.empty((B, Cc, H, W), dtype=dtype, device=x.device)
    check(_lib.load().e2eft_nhwc_to_nchw(dtype_id(x.dtype), dtype_id(dtype), B, Cc, H * W, _nhwc_ld(x), mul, add, _ptr(x), _ptr(y), _stream()))
    return y


def copy_scale(x, out, mul=1.0, add=0.0):
    """out[..., :] = x * mul + add for NHWC / row views of identical shape (strided channel slices allowed)."""
    _check_cuda(x, out)
    assert x.shape == out.shape and x.dtype == out.dtype
    Cc = x.shape[-1]
    xa = _as_rows(x) if x.dim() > 2 else x
    oa = _as_rows(out) if out.dim() > 2 else out
    check(_lib.load().e2eft_copy_scale(dtype_id(x.dtype), xa.shape[0], Cc, _rows_ld(xa), _rows_ld(oa), mul, add, _ptr(xa), _ptr(oa), _stream()))
    return out


def randn_fill_(dst, seed, draw, slot=0):
    """dst[..., :] = standard normals of the device generator (include/e2eft.h: Philox4x32-10 on the LOGICAL NCHW index, Box-Muller) for an NHWC view
    [B,H,W,C] (a strided channel slice allowed; the other channels of the buffer are untouched).  Same (seed, draw, slot, shape) -> same bits."""
    _check_cuda(dst)
    B, H, W, Cc = dst.shape
    check(_lib.load().e2eft_randn_fill(dtype_id(dst.dtype), B, Cc, H * W, _nhwc_ld(dst), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF, int(slot), _ptr(dst), _stream()))
    return dst


def randn_fill_at_(dst, seed, draw, slot=0):
    """`randn_fill_` with `draw` a one-element int64 DEVICE tensor read when the kernel runs (its low 32 bits): the capture-safe form — a replayed graph draws
    what the tensor holds at replay time.  Same (seed, draw value, slot, shape) -> the bits of `randn_fill_`."""
    _check_cuda(dst, draw)
    if draw.dtype != torch.int64 or draw.numel() != 1:
        raise TypeError("randn_fill_at_: draw must be a one-element int64 tensor, got %s %s" % (draw.dtype, tuple(draw.shape)))
    B, H, W, Cc = dst.shape
    check(_lib.load().e2eft_randn_fill_at(dtype_id(dst.dtype), B, Cc, H * W, _nhwc_ld(dst), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(draw), int(slot), _ptr(dst), _stream()))
    return dst


def ddim_step_(x, v, coef):
    """x = coef[0] * x + coef[1] * v in place for NHWC views [B,H,W,C] of one shape (x typically the latent channels of the UNet input); coef: fp32 DEVICE tensor
    [2], one row of `DDIMScheduler.step_coefficients` — read when the kernel runs, so a captured graph serves every step.  The arithmetic of `latent_x0`."""
    _check_cuda(x, v, coef)
    assert x.shape == v.shape and x.dtype == v.dtype, (x.shape, v.shape, x.dtype, v.dtype)
    if coef.dtype != torch.float32 or coef.numel() != 2 or not coef.is_contiguous():
        raise TypeError("ddim_step_: coef must be a contiguous fp32 tensor of two elements, got %s %s" % (coef.dtype, tuple(coef.shape)))
    xa, va = _as_rows(x), _as_rows(v)
    check(_lib.load().e2eft_ddim_step(dtype_id(x.dtype), xa.shape[0], x.shape[-1], _rows_ld(xa), _rows_ld(va), _ptr(coef), _ptr(xa), _ptr(va), _stream()))
    return x


def pyramid_noise_(dst, seed, draw, sizes, discount=0.9):
    """dst[..., :] = multi-resolution noise (training/util/noise.py:8-18): base + sum_i discount^i * bilinear_up(level_i), divided by its unbiased std over the
    whole tensor, for an NHWC view [B,H,W,C]; sizes: up to 10 (rows, cols) level sizes (host ints, passed by value: no host-to-device copy, no synchronisation)."""
    _check_cuda(dst)
    B, H, W, Cc = dst.shape
    lib = _lib.load()
    sizes = [(int(r), int(c)) for r, c in sizes]
    if len(sizes) > 10:
        raise ValueError("pyramid_noise_: at most 10 levels, got %d" % len(sizes))
    table = (C.c_int32 * max(2 * len(sizes), 2))(*[v for rc in sizes for v in rc])
    nbytes = lib.e2eft_pyramid_noise_workspace_bytes(B, Cc, H * W)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dst.device)
    check(lib.e2eft_pyramid_noise(dtype_id(dst.dtype), B, Cc, H, W, _nhwc_ld(dst), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF, float(discount), len(sizes),
                                  table, _ptr(dst), _ptr(ws), nbytes, _stream()))
    return dst


def pyramid_noise_weighted_(dst, seed, draw, sizes, timesteps, discount=0.9, timestep_div=1000.0):
    """dst[..., :] = the GeoWizard trainer's multi-resolution noise (GeoWizard/geowizard/training/train_depth_normal.py:286-296): `pyramid_noise_` with level i of
    sample b weighted by timesteps[b] / timestep_div * discount^i (include/e2eft.h states the fp32 expression), divided by the unbiased std of the whole tensor, for an
    NHWC view [B,H,W,C] (a strided channel slice allowed).  timesteps: a contiguous int64 DEVICE tensor of B elements, read when the kernel runs — nothing is copied to or
    read by the host, and a captured graph sees what the tensor holds at replay time."""
    if not isinstance(timesteps, torch.Tensor) or timesteps.dtype != torch.int64:
        raise TypeError("pyramid_noise_weighted_: timesteps must be an int64 tensor, got %s" % (timesteps.dtype if isinstance(timesteps, torch.Tensor) else type(timesteps)))
    if dst.dim() != 4:
        raise ValueError("pyramid_noise_weighted_: dst must be an NHWC view [B,H,W,C], got %s" % (tuple(dst.shape),))
    B, H, W, Cc = dst.shape
    if timesteps.numel() != B or not timesteps.is_contiguous():
        raise ValueError("pyramid_noise_weighted_: timesteps must be contiguous with one entry per sample (%d), got shape %s stride %s"
                         % (B, tuple(timesteps.shape), tuple(timesteps.stride())))
    sizes = [(int(r), int(c)) for r, c in sizes]
    if len(sizes) > 10:
        raise ValueError("pyramid_noise_weighted_: at most 10 levels, got %d" % len(sizes))
    if not float(timestep_div) > 0.0:
        raise ValueError("pyramid_noise_weighted_: timestep_div must be positive, got %r" % (timestep_div,))
    _check_cuda(dst, timesteps)
    lib = _lib.load()
    table = (C.c_int32 * max(2 * len(sizes), 2))(*[v for rc in sizes for v in rc])
    nbytes = lib.e2eft_pyramid_noise_workspace_bytes(B, Cc, H * W)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dst.device)
    check(lib.e2eft_pyramid_noise_weighted(dtype_id(dst.dtype), B, Cc, H, W, _nhwc_ld(dst), int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF, float(discount),
                                           len(sizes), table, _ptr(timesteps), float(timestep_div), _ptr(dst), _ptr(ws), nbytes, _stream()))
    return dst


PYRAMID_TABLE_WORDS = 22      # 2 + 2 * E2EFT_PYRAMID_MAX_LEVELS: {draw, n_levels, rows_0, cols_0, ..., rows_9, cols_9}


def _check_pyramid_table(what, table):
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int64 or table.numel() != PYRAMID_TABLE_WORDS or not table.is_contiguous():
        raise TypeError("%s: table must be a contiguous int64 tensor of %d elements {draw, n_levels, 10 x (rows, cols)}, got %s"
                        % (what, PYRAMID_TABLE_WORDS, "%s %s" % (table.dtype, tuple(table.shape)) if isinstance(table, torch.Tensor) else type(table)))


def pyramid_table_set_(table, draw, sizes, rows, cols):
    """table (int64 DEVICE tensor [22]) <- {draw, len(sizes), sizes..., (1, 1) for the unused levels} for an output of rows x cols: what `pyramid_noise_at_` /
    `pyramid_noise_weighted_at_` read when they run.  One one-thread launch with the values as kernel arguments — nothing is copied from the host, nothing is
    staged, nothing synchronises; a level larger than the output is refused before the launch."""
    _check_pyramid_table("pyramid_table_set_", table)
    sizes = [(int(r), int(c)) for r, c in sizes]
    if len(sizes) > 10:
        raise ValueError("pyramid_table_set_: at most 10 levels, got %d" % len(sizes))
    _check_cuda(table)
    host = (C.c_int32 * max(2 * len(sizes), 2))(*[v for rc in sizes for v in rc])
    check(_lib.load().e2eft_pyramid_table_set(_ptr(table), int(draw) & 0xFFFFFFFF, len(sizes), host, int(rows), int(cols), _stream()))
    return table


def pyramid_noise_at_(dst, seed, table, discount=0.9):
    """`pyramid_noise_` with the draw and the level sizes read on the device from `table` (`pyramid_table_set_`) when the kernel runs: the capture-safe form — a
    replayed graph draws over what the table holds at replay time.  Same table values -> the bits of `pyramid_noise_`."""
    _check_pyramid_table("pyramid_noise_at_", table)
    _check_cuda(dst, table)
    B, H, W, Cc = dst.shape
    lib = _lib.load()
    nbytes = lib.e2eft_pyramid_noise_workspace_bytes(B, Cc, H * W)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dst.device)
    check(lib.e2eft_pyramid_noise_at(dtype_id(dst.dtype), B, Cc, H, W, _nhwc_ld(dst), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(table), float(discount), _ptr(dst),
                                     _ptr(ws), nbytes, _stream()))
    return dst


def pyramid_noise_weighted_at_(dst, seed, table, timesteps, discount=0.9, timestep_div=1000.0):
    """`pyramid_noise_weighted_` with the draw and the level sizes read on the device from `table` (`pyramid_table_set_`); timesteps as there.  Same table values
    and timesteps -> the bits of `pyramid_noise_weighted_`."""
    _check_pyramid_table("pyramid_noise_weighted_at_", table)
    if not isinstance(timesteps, torch.Tensor) or timesteps.dtype != torch.int64:
        raise TypeError("pyramid_noise_weighted_at_: timesteps must be an int64 tensor, got %s" % (timesteps.dtype if isinstance(timesteps, torch.Tensor) else type(timesteps)))
    if dst.dim() != 4:
        raise ValueError("pyramid_noise_weighted_at_: dst must be an NHWC view [B,H,W,C], got %s" % (tuple(dst.shape),))
    B, H, W, Cc = dst.shape
    if timesteps.numel() != B or not timesteps.is_contiguous():
        raise ValueError("pyramid_noise_weighted_at_: timesteps must be contiguous with one entry per sample (%d), got shape %s stride %s"
                         % (B, tuple(timesteps.shape), tuple(timesteps.stride())))
    if not float(timestep_div) > 0.0:
        raise ValueError("pyramid_noise_weighted_at_: timestep_div must be positive, got %r" % (timestep_div,))
    _check_cuda(dst, table, timesteps)
    lib = _lib.load()
    nbytes = lib.e2eft_pyramid_noise_workspace_bytes(B, Cc, H * W)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dst.device)
    check(lib.e2eft_pyramid_noise_weighted_at(dtype_id(dst.dtype), B, Cc, H, W, _nhwc_ld(dst), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(table), float(discount),
                                              _ptr(timesteps), float(timestep_div), _ptr(dst), _ptr(ws), nbytes, _stream()))
    return dst


def _check_randint(what, out, high, repeat):
    if not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or not out.is_contiguous():
        raise TypeError("%s: out must be a contiguous int64 tensor" % what)
    repeat, high = int(repeat), int(high)
    if repeat < 1 or out.numel() < 1 or out.numel() % repeat:
        raise ValueError("%s: out holds %d elements, not a positive multiple of repeat = %d" % (what, out.numel(), repeat))
    if not 1 <= high <= 2 ** 31 - 1:
        raise ValueError("%s: high must be 1 .. 2^31 - 1, got %d" % (what, high))
    return out.numel() // repeat, repeat, high


def randint_fill_(out, high, seed, draw, slot=0, repeat=1):
    """out (int64, n * repeat elements) <- `repeat` copies of n integers of [0, high) from the device generator: element e takes the raw word of (seed, draw, slot,
    e) and t = (word * high) >> 32 (include/e2eft.h).  `torch.randint(0, high, (n,)).repeat(repeat)` in shape; torch's stream is not reproduced."""
    n, repeat, high = _check_randint("randint_fill_", out, high, repeat)
    _check_cuda(out)
    check(_lib.load().e2eft_randint_fill(n, repeat, high, int(seed) & 0xFFFFFFFFFFFFFFFF, int(draw) & 0xFFFFFFFF, int(slot), _ptr(out), _stream()))
    return out


def randint_fill_at_(out, high, seed, draw, slot=0, repeat=1):
    """`randint_fill_` with `draw` a one-element int64 DEVICE tensor read when the kernel runs: the capture-safe form, the integers of `randint_fill_` for the
    same value"""
    n, repeat, high = _check_randint("randint_fill_at_", out, high, repeat)
    _check_cuda(out, draw)
    if draw.dtype != torch.int64 or draw.numel() != 1:
        raise TypeError("randint_fill_at_: draw must be a one-element int64 tensor, got %s %s" % (draw.dtype, tuple(draw.shape)))
    check(_lib.load().e2eft_randint_fill_at(n, repeat, high, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(draw), int(slot), _ptr(out), _stream()))
    return out


def latent_x0(x_t, v, c_x, c_v, out=None):
    """out = c_x * x_t + c_v * v for NHWC views [B,H,W,C] of one shape (x_t typically the noise channels of the UNet input, read in place)."""
    _check_cuda(x_t, v, out)
    assert x_t.shape == v.shape and x_t.dtype == v.dtype, (x_t.shape, v.shape, x_t.dtype, v.dtype)
    if out is None:
        out = torch.empty(v.shape, dtype=v.dtype, device=v.device)
    xa, va, oa = _as_rows(x_t), _as_rows(v), _as_rows(out)
    check(_lib.load().e2eft_latent_x0(dtype_id(v.dtype), va.shape[0], v.shape[-1], _rows_ld(xa), _rows_ld(va), _rows_ld(oa), c_x, c_v, _ptr(xa), _ptr(va), _ptr(oa), _stream()))
    return out


# ---- diffusion objective of the GeoWizard trainer (csrc/diffusion.hip; train_depth_normal.py:606-609, 671, 677-682, 713-717) ----------------------------
def latent_valid_mask(val_mask, out=None):
    """val_mask bool / uint8 [B,1,H,W] or [B,H,W] (nonzero = valid) -> uint8 [B,H/8,W/8]: 1 where all 64 pixels of the 8 x 8 cell are valid
    (`~max_pool2d((~val_mask).float(), 8, 8).bool()`, :607-608)"""
    _check_cuda(val_mask, out)
    if val_mask.dim() == 4:
        if val_mask.shape[1] != 1:
            raise ValueError("latent_valid_mask: val_mask must be [B,1,H,W] or [B,H,W], got %s" % (tuple(val_mask.shape),))
        val_mask = val_mask[:, 0]
    if val_mask.dim() != 3:
        raise ValueError("latent_valid_mask: val_mask must be [B,1,H,W] or [B,H,W], got %s" % (tuple(val_mask.shape),))
    if val_mask.dtype == torch.bool:
        vm = val_mask.contiguous().view(torch.uint8)
    elif val_mask.dtype == torch.uint8:
        vm = val_mask.contiguous()
    else:
        raise TypeError("latent_valid_mask: val_mask must be bool or uint8, got %s" % val_mask.dtype)
    B, H, W = vm.shape
    if out is None:
        out = torch.empty((B, H // 8, W // 8), dtype=torch.uint8, device=vm.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (B, H // 8, W // 8), (out.dtype, out.shape)
    check(_lib.load().e2eft_latent_valid_mask(B, H, W, _ptr(vm), _ptr(out), _stream()))
    return out


def _diffusion_args(x0, noise, t, abar, y, latent_mask=None, prediction_type=None):
    """the descriptor of one call over NHWC views [R,h,w,c]: x0 and noise of one dtype, y (x_t / pred / dpred) of its own"""
    R, h, w, c = x0.shape
    assert noise.shape == x0.shape and y.shape == x0.shape and noise.dtype == x0.dtype, (x0.shape, noise.shape, y.shape, x0.dtype, noise.dtype)
    assert t.dtype == torch.int64 and t.is_contiguous() and t.numel() == R, (t.dtype, t.shape, R)
    assert abar.dtype == torch.float32 and abar.is_contiguous() and abar.dim() == 1
    d = _lib.DiffusionDesc()
    d.dtype, d.dtype_out = dtype_id(x0.dtype), dtype_id(y.dtype)
    d.rows, d.hw, d.c, d.batch = R, h * w, c, 1
    d.ldx0, d.ldn, d.ldy = _nhwc_ld(x0), _nhwc_ld(noise), _nhwc_ld(y)
    d.n_timesteps = abar.numel()
    if latent_mask is not None:
        if prediction_type not in _lib.PREDICTION_TYPES:
            raise ValueError("Unknown prediction type %s" % prediction_type)
        assert latent_mask.dtype == torch.uint8 and latent_mask.is_contiguous() and tuple(latent_mask.shape[1:]) == (h, w), (latent_mask.dtype, latent_mask.shape)
        d.batch = latent_mask.shape[0]
        d.prediction = _lib.PREDICTION_TYPES[prediction_type]
    return d


def diffusion_mix_(x0, noise, t, abar, out, kind=_lib.DIFFUSION_ADD_NOISE):
    """out[r, ..., :] = sqrt(abar[t_r]) * x0 + sqrt(1 - abar[t_r]) * noise (kind DIFFUSION_ADD_NOISE: `add_noise`, :671) or sqrt(abar[t_r]) * noise -
    sqrt(1 - abar[t_r]) * x0 (DIFFUSION_VELOCITY: `get_velocity`, :680) for NHWC views [R,h,w,c]; t int64 [R] and abar fp32 [T] on the device.  `out` may be a
    channel slice of a wider buffer (the noise channels of the UNet input) and of another dtype (rounded once).  One launch, nothing read back."""
    _check_cuda(x0, noise, t, abar, out)
    d = _diffusion_args(x0, noise, t, abar, out)
    check(_lib.load().e2eft_diffusion_mix(C.byref(d), int(kind), _ptr(t), _ptr(abar), _ptr(x0), _ptr(noise), _ptr(out), _stream()))
    return out


def masked_mse_workspace(rows, hw, c, device):
    nbytes = _lib.load().e2eft_masked_mse_workspace_bytes(rows, hw, c)
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def masked_mse_fwd(pred, x0, noise, t, abar, latent_mask, prediction_type, want_target=False, ws=None):
    """masked mean squared error of `pred` against the diffusion target (:677-682, :717) over NHWC views [R,h,w,c]; latent_mask uint8 [B,h,w], row r uses image
    r % B.  -> (loss fp32 [1], n_selected int64 [1], target fp32 [R,h,w,c] or None).  Two launches, nothing read back."""
    _check_cuda(pred, x0, noise, t, abar, latent_mask, ws)
    d = _diffusion_args(x0, noise, t, abar, pred, latent_mask, prediction_type)
    if ws is None:
        ws = masked_mse_workspace(d.rows, d.hw, d.c, pred.device)
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    nsel = torch.empty(1, dtype=torch.int64, device=pred.device)
    target = torch.empty(tuple(pred.shape), dtype=torch.float32, device=pred.device) if want_target else None
    check(_lib.load().e2eft_masked_mse_fwd(C.byref(d), _ptr(t), _ptr(abar), _ptr(pred), _ptr(x0), _ptr(noise), _ptr(latent_mask), _ptr(loss), _ptr(nsel), _ptr(target),
                                           _ptr(ws), ws.numel() * ws.element_size(), _stream()))
    return loss, nsel, target


def masked_mse_bwd(pred, x0, noise, t, abar, latent_mask, prediction_type, n_selected, grad_out, out=None):
    """dpred = grad_out * 2 * (pred - target) / n_selected on the selected elements, 0 elsewhere — NHWC [R,h,w,c] in pred's dtype; n_selected (int64 [1], from
    the forward) and grad_out (fp32 [1]) are read on the device.  One launch."""
    _check_cuda(pred, x0, noise, t, abar, latent_mask, n_selected, grad_out, out)
    d = _diffusion_args(x0, noise, t, abar, pred, latent_mask, prediction_type)
    assert n_selected.dtype == torch.int64 and grad_out.dtype == torch.float32 and grad_out.numel() == 1
    if out is None:
        out = torch.empty(tuple(pred.shape), dtype=pred.dtype, device=pred.device)
    assert out.shape == pred.shape and out.dtype == pred.dtype
    check(_lib.load().e2eft_masked_mse_bwd(C.byref(d), _ptr(t), _ptr(abar), _ptr(pred), _ptr(x0), _ptr(noise), _ptr(latent_mask), _ptr(n_selected), _ptr(grad_out),
                                           _ptr(out), _nhwc_ld(out), _stream()))
    return out


def add(a, b, out=None):
    _check_cuda(a, b, out)
    assert a.shape == b.shape and a.dtype == b.dtype
    if out is None:
        out = torch.empty(a.shape, dtype=a.dtype, device=a.device)
    Cc = a.shape[-1]
    aa, bb, oo = (_as_rows(t) if t.dim() > 2 else t for t in (a, b, out))
    check(_lib.load().e2eft_add(dtype_id(a.dtype), aa.shape[0], Cc, _rows_ld(aa), _rows_ld(bb), _rows_ld(oo), _ptr(aa), _ptr(bb), _ptr(oo), _stream()))
    return out


def timestep_embedding(t, dim, dtype):
    """t: int64 [B] device tensor -> [B, dim] = [cos | sin] (flip_sin_to_cos=True, freq_shift=0)"""
    _check_cuda(t)
    t = t.to(torch.int64).contiguous()
    out = torch.empty((t.shape[0], dim), dtype=dtype, device=t.device)
    check(_lib.load().e2eft_timestep_embedding(dtype_id(dtype), t.shape[0], dim, _ptr(t), _ptr(out), _stream()))
    return out


def silu(x):
    _check_cuda(x)
    x = x.contiguous()
    out = torch.empty_like(x)
    check(_lib.load().e2eft_silu(dtype_id(x.dtype), x.numel(), _ptr(x), _ptr(out), _stream()))
    return out


ACT_KINDS = {"quick_gelu": 0, "gelu": 1, "silu": 2, "sigmoid": 3}


def activation(x, kind):
    """y = act(x) elementwise; kind in ACT_KINDS"""
    _check_cuda(x)
    x = x.contiguous()
    out = torch.empty_like(x)
    check(_lib.load().e2eft_activation(dtype_id(x.dtype), ACT_KINDS[kind], x.numel(), _ptr(x), _ptr(out), _stream()))
    return out


def depth_head(x, to_unit, dtype=None):
    """decoder output NHWC [B,H,W,>=3 (view)] -> [B,1,H,W]: to_unit False clip(mean_c, -1, 1); True the same mapped to [0,1];
    "mean" the bare channel mean (no clip)"""
    _check_cuda(x)
    B, H, W, _ = x.shape
    dtype = dtype or x.dtype
    y = torch.empty((B, 1, H, W), dtype=dtype, device=x.device)
    mode = 2 if to_unit == "mean" else (1 if to_unit else 0)
    check(_lib.load().e2eft_depth_head(dtype_id(x.dtype), dtype_id(dtype), B * H * W, _nhwc_ld(x), mode, _ptr(x), _ptr(y), _stream()))
    return y


def normal_head(x, clamp=False, sign=1.0, dtype=None):
    """decoder output NHWC [B,H,W,>=3] -> NCHW [B,3,H,W] unit normals n/(|n|+1e-5)"""
    _check_cuda(x)
    B, H, W, _ = x.shape
    dtype = dtype or x.dtype
    y = torch.empty((B, 3, H, W), dtype=dtype, device=x.device)
    check(_lib.load().e2eft_normal_head(dtype_id(x.dtype), dtype_id(dtype), B, H * W, _nhwc_ld(x), 1 if clamp else 0, sign, _ptr(x), _ptr(y), _stream()))
    return y


def ssi_loss(pred, target, mask, return_scale_shift=False):
    """ScaleAndShiftInvariantLoss forward (training/util/loss.py:13-47). pred/target [B,1,H,W] or [B,H,W], mask bool."""
    _check_cuda(pred, target, mask)
    B = pred.shape[0]
    p = pred.reshape(B, -1).float().contiguous()
    t = target.reshape(B, -1).float().contiguous()
    m = mask.reshape(B, -1).to(torch.uint8).contiguous()
    out, ss, _ = ssi_loss_fwd_saved(p, t, m)
    return (out[0], ss) if return_scale_shift else out[0]


def angular_loss(pred, target, mask):
    """AngularLoss forward (training/util/loss.py:51-67). pred/target [B,3,H,W], mask [B,1,H,W] (channel 0 used)."""
    _check_cuda(pred, target, mask)
    B = pred.shape[0]
    p = pred.reshape(B, 3, -1).float().contiguous()
    t = target.reshape(B, 3, -1).float().contiguous()
    m = mask[:, 0].reshape(B, -1).to(torch.uint8).contiguous()
    return angular_loss_fwd_saved(p, t, m)[0][0]


# =========================================================================================================
# backward-pass kernels (include/e2eft.h "Backward pass of the E2E-FT training step"); used by autograd.py
def transpose(x, rows_pad=None, out=None):
    """x: [Z, R, C] (or [R, C]) row-strided view -> [Z, C, rows_pad] with zeros in [R, rows_pad) (rows_pad multiple of 64 by default
    so that the result is a FAST-path K operand of e2eft_gemm)."""
    _check_cuda(x, out)
    squeeze = x.dim() == 2
    if squeeze:
        x = x[None]
    Z, R, Cc = x.shape
    if Cc > 1 and x.stride(2) != 1:
        raise ValueError("transpose: unit inner stride required")
    ld = x.stride(1) if R > 1 else max(Cc, x.stride(1))
    bs = x.stride(0) if Z > 1 else R * ld
    rp = round_up(R, 64) if rows_pad is None else rows_pad
    if out is None:
        out = torch.empty((Z, Cc, rp), dtype=x.dtype, device=x.device)
    assert out.shape == (Z, Cc, rp) and out.is_contiguous()
    with _timed("transpose", 0.0, 2.0 * Z * R * Cc * x.element_size(), label="transpose z%d %dx%d" % (Z, R, Cc)):
        check(_lib.load().e2eft_transpose(dtype_id(x.dtype), Z, R, Cc, ld, bs, rp, rp, Cc * rp, _ptr(x), _ptr(out), _stream()))
    return out[0] if squeeze else out


def dgrad_weight_from_packed(pk, cout, taps, cp):
    """The dgrad operand of a convolution from its packed forward weight: pk [cout, taps*cp] (OHWI rows, 16-byte channel padding) ->
    [cp, taps*cop] with out[ci][(taps-1-t)*cop + co] = pk[co][t*cp + ci], cop = cout padded to a 16-byte multiple with zeros (include/e2eft.h,
    e2eft_conv2d_dgrad: flipped taps, channels transposed).  ONE batched e2eft_transpose: batch = tap, the output walks the taps backwards
    (negative batch stride)."""
    _check_cuda(pk)
    e = epc(pk.dtype)
    assert pk.dim() == 2 and pk.shape == (cout, taps * cp) and pk.is_contiguous() and cp % e == 0 and pk.data_ptr() % 16 == 0
    cop = round_up(cout, e)
    out = torch.empty((cp, taps * cop), dtype=pk.dtype, device=pk.device)
    last = out.data_ptr() + (taps - 1) * cop * pk.element_size()
    with _timed("transpose", 0.0, 2.0 * taps * cout * cp * pk.element_size(), label="dgrad weight %dx%d taps%d" % (cout, cp, taps)):
        check(_lib.load().e2eft_transpose(dtype_id(pk.dtype), taps, cout, cp, taps * cp, cp, cop, taps * cop, -cop, _ptr(pk), C.c_void_p(last), _stream()))
    return out


def splitk_plan(M, N, K, dtype=None, cus=256):
    """(nsplit, kc): weight-gradient GEMMs are [Cout x kh*kw*Cin] outputs contracted over 10^4..10^5 pixels — a handful of output
    tiles.  Split the contraction into nsplit chunks of kc (multiple of 64) columns so that >= ~512 workgroups exist; the
    operands are zero padded to nsplit*kc columns by their producers (transpose / im2col_t).
    fp32 (round 5): the batched GEMM runs on igemm2's 8-wave kernel — 256 x 128 tiles, ONE workgroup per CU — so what matters is whole ROUNDS of `cus`
    tiles: nsplit is the chunk count (chunks of >= 512 columns) whose tile total fills its last round best (z9 x 30 tiles = 270 on 256 CUs ran two rounds at
    53 %; 8 or 17 chunks fill theirs to 94 / 99.6 %), the smallest such count among near-ties (fewer partials for the reduction pass)."""
    if dtype == torch.float32:
        tiles = ((M + 255) // 256) * ((N + 127) // 128)
        if tiles * 1 >= cus // 2 and K < 1024:
            return 1, round_up(K, 64)
        best = None
        for ns in range(1, max(1, K // 512) + 1):
            tot = tiles * ns
            if tot > 8 * cus and best is not None:
                break
            rounds = (tot + cus - 1) // cus
            eff = tot / (rounds * cus)
            if best is None or eff > best[0] + 0.02:
                best = (eff, ns)
        want = best[1]
        kc = round_up((K + want - 1) // want, 64)
        return (K + kc - 1) // kc, kc
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    want = max(1, min((512 + tiles - 1) // tiles, K // 512))
    kc = round_up((K + want - 1) // want, 64)
    nsplit = (K + kc - 1) // kc
    return nsplit, kc


def gemm_splitk(a, w, nsplit, kc, alpha=1.0):
    """out[m,n] = alpha * sum_k a[m,k] w[n,k] for a [M, nsplit*kc], w [N, nsplit*kc]: nsplit batched partial GEMMs + a column-sum
    reduction in fp32.  Returns fp32 [M, N] (or the plain GEMM result in the operand dtype when nsplit == 1)."""
    if nsplit == 1:
        return gemm(a, w, alpha=alpha)
    M, K = a.shape
    N = w.shape[0]
    assert K == nsplit * kc and w.shape[1] == K and N % epc(a.dtype) == 0
    part = torch.empty((nsplit, M, N), dtype=a.dtype, device=a.device)
    bgemm_raw(a.dtype, M, N, kc, a, _rows_ld(a), (0, kc), w, _rows_ld(w), (0, kc), part, N, (0, M * N), 1, nsplit)
    return colsum(part.view(nsplit, M * N), groups=1, alpha=alpha).view(M, N)


def im2col_t(x, x2, kh, kw, stride, pad, up_to=None, Pp=None):
    """-> ([kh*kw*(c1+c2), Ppad] K-contiguous im2col of the conv input over the OUTPUT pixels, P, Ppad)"""
    _check_cuda(x, x2)
    d = _conv_desc(x, x2, 1, kh, kw, stride, pad, up_to, 1.0)
    P = d.batch * d.hout * d.wout
    Pp = round_up(P, 64) if Pp is None else Pp
    cin = d.c1 + d.c2
    col = torch.empty((kh * kw * cin, Pp), dtype=x.dtype, device=x.device)
    with _timed("im2col_t", 0.0, 2.0 * kh * kw * cin * Pp * x.element_size(), label="im2col_t %dx%d %d P%d" % (kh, kw, cin, P)):
        check(_lib.load().e2eft_conv2d_im2col_t(C.byref(d), _ptr(x), _ptr(x2), _ptr(col), Pp, _stream()))
    return col, P, Pp


WGRAD_DIRECT = True   # tests / A-B: False keeps every weight gradient on the transpose + im2col_t + split-K GEMM path
WGRAD_DIRECT_FP32 = True   # round 6: strict-fp32 weight gradients straight from the NHWC tensors too (csrc/wgrad.hip::wgrad32_kernel); False: the round-5 path


def _wgrad_batch_step(per_img, pixels_per_img, B):
    """images per launch of a weight gradient cut along the batch: the kernel addresses each operand through ONE 32-bit buffer descriptor (per_img: bytes of one image
    of the larger operand) and counts fewer than 2^24 output pixels"""
    return max(1, min(B, (0xFFFF0000 - 1) // max(per_img, 1), ((1 << 24) - 1) // max(pixels_per_img, 1)))


def _wgrad_split_serves(dy, x, cin, cout, kh, kw, stride, pad):
    """pure host arithmetic: does the 16-bit kernel serve the f16 split planes of this fp32 weight gradient (dY planes of pixel stride 2 c0, ONE source of cin channels
    at pixel stride 2 cin), in every launch of conv2d_wgrad's cut along the batch?  Asked before anything is split: a shape it refuses goes to wgrad32_kernel."""
    B, H, W, _ = x.shape
    c0 = dy.shape[3]
    step = _wgrad_batch_step(max(dy.shape[1] * dy.shape[2] * 2 * c0, H * W * 2 * cin) * 2, dy.shape[1] * dy.shape[2], B)
    for nb in {step, B % step or step}:
        d = _conv_desc((nb, H, W, cin, 2 * cin), None, cout, kh, kw, stride, pad, None, 1.0, dtype=_lib.F16)
        assert (d.hout, d.wout) == (dy.shape[1], dy.shape[2]), (dy.shape, d.hout, d.wout)
        if _lib.load().e2eft_conv2d_wgrad_workspace_bytes(C.byref(d), 2 * c0) == 0:
            return False
    return True


def conv2d_wgrad(dy, x, x2, cout, kh, kw, stride, pad, alpha, out=None):
    """Weight gradient straight from the NHWC tensors (csrc/wgrad.hip): dy [B,hout,wout,>=cout] (pixel-dense), x [B,H,W,c1], x2 optional second
    concat source -> fp32 [cout, kh*kw*(c1+c2)] (OHWI rows), or None when the kernel does not serve the problem (the caller falls back).
    out: a dense fp32 tensor of cout * kh*kw*(c1+c2) elements that receives the result (FlatAdamW's gradient slot: the reduction's last pass — or the kernel
    itself when it does not split — writes there, no copy / add afterwards).
    The kernel addresses each operand through ONE 32-bit buffer descriptor, so tensors of 4 GB and more (configs[2] as benchmarked: 32 images of
    576^2 x 256 channels = 5.4 GB) are cut along the batch into launches below that limit; every launch adds its split partials to the same reduction."""
    if not WGRAD_DIRECT or (dy.dtype == torch.float32 and not WGRAD_DIRECT_FP32):
        return None
    _check_cuda(dy, x, x2)
    cin = x.shape[3] + (x2.shape[3] if x2 is not None else 0)
    if (dy.dtype == torch.float32 and cin % 64 == 0 and cout % 64 == 0 and _lib.load().e2eft_get_option(_lib.OPT_F32_SPLIT) == 1
            and f32split_operands_ok((dy, x, x2)) and _wgrad_split_serves(dy, x, cin, cout, kh, kw, stride, pad)):
        # fp32 on the f16 matrix pipe (csrc/f32split.hip): dy[:, co] s_dy[co] = d0 + d1, x[:, ci] s_x[ci] = x0 + x1 (two-term f16 splits, exact to 2^-22, one power-of-two
        # scale per CHANNEL: dW[co, tap, ci] only ever multiplies column co of dY with column ci of X, so every entry keeps that precision relative to its own two
        # columns); the gradient is the sum of the 16-bit kernel's results for (d0, x0), (d0, x1), (d1, x0), scaled back by the outer product of the inverse scales in
        # one pass — three launches at the f16 rate instead of one at the fp32 rate.  (The data-gradient convolution of the same dY reduces OVER the channels: it keeps
        # its own per-tensor planes.)
        dyp, idy = f32_split2_cols(dy)
        xp, ix = f32_split2_cols(x, x2)               # (two sources: the planes of their concatenation — the 16-bit kernel then sees ONE source of c1 + c2 channels)
        c0, c1 = dy.shape[3], cin
        ts = []
        for (a_, b_) in ((dyp[..., :c0], xp[..., :c1]), (dyp[..., :c0], xp[..., c1:]), (dyp[..., c0:], xp[..., :c1])):
            t = conv2d_wgrad(a_, b_, None, cout, kh, kw, stride, pad, alpha)
            if t is None:
                raise RuntimeError("conv2d_wgrad: the 16-bit kernel refused planes that _wgrad_split_serves accepted")
            ts.append(t)
        direct = out is not None and out.data_ptr() % 16 == 0      # (a slot of the flat gradient buffer may start off a 16-byte boundary: one copy then)
        r = out.view(ts[0].shape) if direct else ts[0]
        with _timed("f32split", 0.0, 16.0 * cout * kh * kw * cin, label="wgrad finish %d x %d" % (cout, kh * kw * cin)):
            check(_lib.load().e2eft_f32_split_wgrad_finish(_ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), cout, kh * kw, cin, _ptr(idy), _ptr(ix), _ptr(r), _stream()))
        if out is not None and not direct:
            out.view(r.shape).copy_(r)
            return out.view(r.shape)
        return r
    B = x.shape[0]
    lddy = _nhwc_ld(dy)
    es = dy.element_size()
    per_img = max(dy.shape[1] * dy.shape[2] * lddy, x.shape[1] * x.shape[2] * max(_nhwc_ld(x), _nhwc_ld(x2) if x2 is not None else 0)) * es
    step = _wgrad_batch_step(per_img, dy.shape[1] * dy.shape[2], B)
    lib = _lib.load()
    parts = []
    N = kh * kw * cin
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        xs, x2s, dys = x[b0:b1], (x2[b0:b1] if x2 is not None else None), dy[b0:b1]
        d = _conv_desc(xs, x2s, cout, kh, kw, stride, pad, None, alpha)
        assert tuple(dys.shape[:3]) == (d.batch, d.hout, d.wout), (dys.shape, d.batch, d.hout, d.wout)
        nbytes = lib.e2eft_conv2d_wgrad_workspace_bytes(C.byref(d), lddy)
        if nbytes == 0:
            return None
        direct = out is not None and step >= B and nbytes == cout * N * 4      # one launch, no split: the kernel's workspace IS the result
        part = out.view(-1) if direct else torch.empty(nbytes // 4, dtype=torch.float32, device=dy.device)
        ns = C.c_int32(0)
        P = d.batch * d.hout * d.wout
        with _timed("wgrad", 2.0 * P * cout * N, (P * (cout + cin)) * es, label="wgrad %dx%ds%d P%d %d->%d" % (kh, kw, stride, P, cin, cout)):
            check(lib.e2eft_conv2d_wgrad(C.byref(d), _ptr(dys), lddy, _ptr(xs), _ptr(x2s), _ptr(part), nbytes, C.byref(ns), _stream()))
        parts.append(part.view(ns.value, cout * N))
    if len(parts) == 1 and parts[0].shape[0] == 1:
        if out is not None and parts[0].data_ptr() != out.data_ptr():
            out.view(1, -1).copy_(parts[0])
            return out.view(cout, N)
        return parts[0].view(cout, N)
    allp = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
    return colsum(allp, groups=1, out=None if out is None else out.view(1, -1)).view(cout, N)


def linear_wgrad(dy2d, x2d, alpha=1.0, out=None):
    """dW [N, K] fp32 = alpha * dy2d^T x2d for row views dy2d [M, N], x2d [M, K] (K a multiple of 64) — the 1x1 case of conv2d_wgrad; None = fall back.
    out: see conv2d_wgrad"""
    if not WGRAD_DIRECT or (dy2d.dtype == torch.float32 and not WGRAD_DIRECT_FP32) or x2d.shape[1] % 64 != 0:
        return None
    M, N = dy2d.shape
    K = x2d.shape[1]
    try:
        ldy, ldx = _rows_ld(dy2d), _rows_ld(x2d)
    except ValueError:
        return None
    if ldy % epc(dy2d.dtype) != 0 or ldx % epc(dy2d.dtype) != 0 or dy2d.data_ptr() % 16 != 0 or x2d.data_ptr() % 16 != 0:
        return None
    xv = x2d.as_strided((1, 1, M, K), (M * ldx, M * ldx, ldx, 1))
    dv = dy2d.as_strided((1, 1, M, N), (M * ldy, M * ldy, ldy, 1))
    return conv2d_wgrad(dv, xv, None, N, 1, 1, 1, (0, 0, 0, 0), alpha, out=out)


def conv2d_dgrad(dy, w_dgrad, x_shape, c2, kh, kw, stride, pad, up_to, alpha):
    """dy [B,hout,wout,cout_pad] (zero / finite pad channels), w_dgrad [cin, kh*kw*cout_pad]; x_shape = forward x [B,H,W,c1].
    Returns the gradient w.r.t. the logical (upsampled) concatenated input [B, hl, wl, c1+c2]."""
    _check_cuda(dy, w_dgrad)
    B, H, W, c1 = x_shape
    hl, wl = (H, W) if up_to is None else up_to
    cop, cin = dy.shape[3], c1 + c2
    d = _conv_desc((B, H, W, c1, c1), (c2, c2), cop, kh, kw, stride, pad, up_to, alpha, dtype=dtype_id(dy.dtype))      # (the forward's descriptor over a dense dX)
    assert (d.hout, d.wout) == (dy.shape[1], dy.shape[2])
    assert w_dgrad.shape == (cin, kh * kw * cop) and w_dgrad.is_contiguous() and w_dgrad.dtype == dy.dtype
    label = "dgrad%dx%ds%d B%d %dx%d %d->%d" % (kh, kw, stride, B, hl, wl, cop, cin)
    dx = new_nhwc(B, hl, wl, cin, dy.dtype, dy.device)
    if (_f32split_takes(dy.dtype, cop, w_dgrad.shape[1], kh * kw, alpha, None, up_to) and cop % 64 == 0 and cin % 8 == 0
            and ((kh, kw, stride, tuple(pad)) == (3, 3, 1, (1, 1, 1, 1)) or (kh, kw, stride, tuple(pad)) == (1, 1, 1, (0, 0, 0, 0)))):
        # the data gradient of a 3x3 / stride-1 / pad-1 (or 1x1) convolution IS such a convolution of dY with the flipped, transposed weights: the f16-split route of conv2d
        if _conv2d_f32split(dy, w_dgrad, None, cin, None, alpha, dx, False, label, geom=(kh, kw, 1, tuple(pad))) is not None:
            return dx
    with _timed("igemm", 2.0 * B * hl * wl * cin * kh * kw * cop, label=label):
        check(_lib.load().e2eft_conv2d_dgrad(C.byref(d), _ptr(dy), _nhwc_ld(dy), cop, _ptr(w_dgrad), w_dgrad.shape[1], _ptr(dx), _nhwc_ld(dx),
                                             _stream()))
    return dx


def colsum(x2d, groups=1, alpha=1.0, out=None):
    """x2d [rows, cols] row-strided -> fp32 [groups, cols] sums over each group of rows/groups consecutive rows (into `out`, dense fp32 [groups, cols], if given)"""
    _check_cuda(x2d, out)
    R, Cc = x2d.shape
    assert R % groups == 0
    lib = _lib.load()
    nbytes = lib.e2eft_colsum_workspace_bytes(groups, R // groups, Cc)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x2d.device)
    if out is None:
        out = torch.empty((groups, Cc), dtype=torch.float32, device=x2d.device)
    else:
        assert out.dtype == torch.float32 and tuple(out.shape) == (groups, Cc) and out.is_contiguous(), (out.dtype, out.shape, out.stride())
    check(lib.e2eft_colsum(dtype_id(x2d.dtype), groups, R // groups, Cc, _rows_ld(x2d), alpha, _ptr(x2d), _ptr(out), _ptr(ws), nbytes, _stream()))
    return out


def upsample_nearest_bwd(dy, H, W):
    """dy [B,hl,wl,C] -> [B,H,W,C]"""
    _check_cuda(dy)
    B, hl, wl, Cc = dy.shape
    dx = torch.empty((B, H, W, Cc), dtype=dy.dtype, device=dy.device)
    check(_lib.load().e2eft_upsample_nearest_bwd(dtype_id(dy.dtype), B, H, W, hl, wl, Cc, _nhwc_ld(dy), Cc, _ptr(dy), _ptr(dx), _stream()))
    return dx


def groupnorm_bwd(x, x2, gamma, beta, groups, eps, silu, dy, fwd_ws, need_dx=True, need_dparams=True, dx_add=None, dg_out=None, db_out=None):
    """-> (dx [B,H,W,C] or None, dgamma fp32 [C] or None, dbeta fp32 [C] or None); dx_add: a [B,H,W,C] gradient added into dx;
    dg_out / db_out: dense fp32 [C] tensors that receive dgamma / dbeta"""
    _check_cuda(x, x2, gamma, beta, dy, fwd_ws)
    B, H, W, c1 = x.shape
    Cc = c1 + (0 if x2 is None else x2.shape[3])
    d = _gn_desc(x, x2, groups, eps, silu, Cc)
    ws, nbytes = _gn_workspace(d, x.device, "groupnorm_bwd", bwd=True)
    dx = torch.empty((B, H, W, Cc), dtype=x.dtype, device=x.device) if need_dx else None
    for o_ in (dg_out, db_out):
        assert o_ is None or (o_.dtype == torch.float32 and tuple(o_.shape) == (Cc,) and o_.is_contiguous())
    dg = (dg_out if dg_out is not None else torch.empty(Cc, dtype=torch.float32, device=x.device)) if need_dparams else None
    db = (db_out if db_out is not None else torch.empty(Cc, dtype=torch.float32, device=x.device)) if need_dparams else None
    with _timed("groupnorm_bwd", 0.0, 5.0 * B * H * W * Cc * x.element_size(), label="gn_bwd B%d %dx%d C%d" % (B, H, W, Cc)):
        check(_lib.load().e2eft_groupnorm_bwd_add(C.byref(d), _ptr(x), _ptr(x2), _ptr(gamma), _ptr(beta), _ptr(dy), _nhwc_ld(dy), _ptr(dx_add),
                                                  _nhwc_ld(dx_add) if dx_add is not None else 0, _ptr(dx), Cc, _ptr(dg), _ptr(db), _ptr(fwd_ws), _ptr(ws), nbytes, _stream()))
    return dx, dg, db


def layernorm_bwd(x, gamma, eps, dy, need_dx=True, gb_out=None):
    """-> (dx like x or None, dgamma fp32 [C], dbeta fp32 [C]); gb_out: dense fp32 [2, C] that receives (dgamma, dbeta)"""
    _check_cuda(x, gamma, dy)
    Cc = x.shape[-1]
    a = x.reshape(-1, Cc) if x.is_contiguous() else _as_rows(x)
    g = dy.reshape(-1, Cc) if dy.is_contiguous() else _as_rows(dy)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device) if need_dx else None
    lib = _lib.load()
    nbytes = lib.e2eft_layernorm_bwd_workspace_bytes(a.shape[0], Cc)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    if gb_out is not None:
        assert gb_out.dtype == torch.float32 and tuple(gb_out.shape) == (2, Cc) and gb_out.is_contiguous()
    gb = gb_out if gb_out is not None else torch.empty((2, Cc), dtype=torch.float32, device=x.device)
    check(lib.e2eft_layernorm_bwd(dtype_id(x.dtype), a.shape[0], Cc, _rows_ld(a), _rows_ld(g), Cc, eps, _ptr(a), _ptr(gamma), _ptr(g), _ptr(dx), _ptr(gb),
                                  _ptr(ws), nbytes, _stream()))
    return dx, gb[0], gb[1]


def geglu_bwd(h, dy):
    _check_cuda(h, dy)
    c2 = h.shape[-1]
    c = c2 // 2
    a = h.reshape(-1, c2) if h.is_contiguous() else _as_rows(h)
    g = dy.reshape(-1, c) if dy.is_contiguous() else _as_rows(dy)
    dh = torch.empty(h.shape, dtype=h.dtype, device=h.device)
    check(_lib.load().e2eft_geglu_bwd(dtype_id(h.dtype), a.shape[0], c, _rows_ld(a), _rows_ld(g), c2, _ptr(a), _ptr(g), _ptr(dh), _stream()))
    return dh


def softmax_bwd_rows_(p, dp, n, scale):
    """in place on dp [rows, lds]: dp <- p * (dp - rowsum(dp*p)) * scale"""
    _check_cuda(p, dp)
    assert p.dim() == 2 and p.is_contiguous() and dp.shape == p.shape and dp.is_contiguous() and p.dtype == dp.dtype
    check(_lib.load().e2eft_softmax_bwd_rows(dtype_id(p.dtype), p.shape[0], n, p.shape[1], scale, _ptr(p), _ptr(dp), _stream()))
    return dp


def silu_bwd(x, dy):
    _check_cuda(x, dy)
    x, dy = x.contiguous(), dy.contiguous()
    dx = torch.empty_like(x)
    check(_lib.load().e2eft_silu_bwd(dtype_id(x.dtype), x.numel(), _ptr(x), _ptr(dy), _ptr(dx), _stream()))
    return dx


def depth_head_bwd(x, dy, to_unit):
    """x NHWC [B,H,W,>=3] (forward input), dy [B,1,H,W] -> dx [B,H,W,3] (view of a zero-padded buffer)"""
    _check_cuda(x, dy)
    B, H, W, _ = x.shape
    dy = dy.contiguous()
    cp = round_up(3, epc(x.dtype))
    dx = torch.empty((B, H, W, cp), dtype=x.dtype, device=x.device)
    check(_lib.load().e2eft_depth_head_bwd(dtype_id(x.dtype), dtype_id(dy.dtype), B * H * W, _nhwc_ld(x), cp, cp, 1 if to_unit else 0, _ptr(x), _ptr(dy),
                                           _ptr(dx), _stream()))
    return dx[..., :x.shape[3]] if x.shape[3] <= cp else dx


def normal_head_bwd(x, dy, clamp, sign):
    _check_cuda(x, dy)
    B, H, W, _ = x.shape
    dy = dy.contiguous()
    cp = round_up(3, epc(x.dtype))
    dx = torch.empty((B, H, W, cp), dtype=x.dtype, device=x.device)
    check(_lib.load().e2eft_normal_head_bwd(dtype_id(x.dtype), dtype_id(dy.dtype), B, H * W, _nhwc_ld(x), cp, cp, 1 if clamp else 0, sign, _ptr(x), _ptr(dy),
                                            _ptr(dx), _stream()))
    return dx[..., :x.shape[3]] if x.shape[3] <= cp else dx


def ssi_loss_fwd_saved(p, t, m):
    """p, t fp32 [B, hw] contiguous, m uint8 [B, hw] -> (loss[1], scale_shift [B,2], workspace) for ssi_loss_bwd"""
    lib = _lib.load()
    B = p.shape[0]
    nbytes = lib.e2eft_ssi_loss_workspace_bytes(B)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=p.device)
    out = torch.empty(1, dtype=torch.float32, device=p.device)
    ss = torch.empty((B, 2), dtype=torch.float32, device=p.device)
    check(lib.e2eft_ssi_loss_fwd(B, p.shape[1], _ptr(p), _ptr(t), _ptr(m), _ptr(out), _ptr(ss), _ptr(ws), nbytes, _stream()))
    return out, ss, ws


def ssi_loss_bwd(p, t, m, ss, fwd_ws, gout):
    B = p.shape[0]
    dp = torch.empty_like(p)
    lib = _lib.load()
    nbytes = lib.e2eft_ssi_loss_bwd_workspace_bytes(B)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=p.device)
    g = gout.reshape(1).float().contiguous()
    check(lib.e2eft_ssi_loss_bwd(B, p.shape[1], _ptr(p), _ptr(t), _ptr(m), _ptr(ss), _ptr(fwd_ws), _ptr(g), _ptr(dp), _ptr(ws), nbytes, _stream()))
    return dp


def angular_loss_fwd_saved(p, t, m):
    """p, t fp32 [B,3,hw], m uint8 [B,hw]"""
    lib = _lib.load()
    nbytes = lib.e2eft_angular_loss_workspace_bytes(p.shape[0])
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=p.device)
    out = torch.empty(1, dtype=torch.float32, device=p.device)
    check(lib.e2eft_angular_loss_fwd(p.shape[0], p.shape[2], _ptr(p), _ptr(t), _ptr(m), _ptr(out), _ptr(ws), nbytes, _stream()))
    return out, ws


def angular_loss_bwd(p, t, m, fwd_ws, gout):
    dp = torch.empty_like(p)
    g = gout.reshape(1).float().contiguous()
    check(_lib.load().e2eft_angular_loss_bwd(p.shape[0], p.shape[2], _ptr(p), _ptr(t), _ptr(m), _ptr(fwd_ws), _ptr(g), _ptr(dp), _stream()))
    return dp


def sumsq_workspace(g):
    """the fp64 workspace `sumsq` needs for g (a caller that keeps one passes it as ws=)"""
    nbytes = _lib.load().e2eft_sumsq_workspace_bytes(g.numel())
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=g.device)


def sumsq(g, out=None, ws=None):
    """fp64 [1] device scalar = sum g^2 over a flat fp32 buffer; fixed summation order (bit-reproducible)"""
    _check_cuda(g)
    assert g.dtype == torch.float32 and g.is_contiguous()
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=g.device)
    if ws is None:
        ws = sumsq_workspace(g)
    check(_lib.load().e2eft_sumsq(g.numel(), _ptr(g), _ptr(out), _ptr(ws), ws.numel() * ws.element_size(), _stream()))
    return out


def adamw_step_(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_sumsq=None, grad_scale=1.0, max_norm=0.0):
    _check_cuda(param, grad, exp_avg, exp_avg_sq, grad_sumsq)
    for t in (param, grad, exp_avg, exp_avg_sq):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == param.numel()
    check(_lib.load().e2eft_adamw_step(param.numel(), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), lr, beta1, beta2, eps, weight_decay, step,
                                       _ptr(grad_sumsq), grad_scale, max_norm, _stream()))
    return param


def adamw_step_guarded_(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, state, coef, grad_sumsq, grad_scale=1.0, max_norm=0.0):
    """AdamW with the step counter on the device (`state` int64 [2] = applied / skipped steps) and a skip on a non-finite gradient norm"""
    _check_cuda(param, grad, exp_avg, exp_avg_sq, state, coef, grad_sumsq)
    for t in (param, grad, exp_avg, exp_avg_sq):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == param.numel()
    assert state.dtype == torch.int64 and state.numel() == 2 and coef.dtype == torch.float32 and coef.numel() == 4 and grad_sumsq.dtype == torch.float64
    check(_lib.load().e2eft_adamw_step_guarded(param.numel(), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), lr, beta1, beta2, eps, weight_decay,
                                               _ptr(state), _ptr(coef), _ptr(grad_sumsq), grad_scale, max_norm, _stream()))
    return param


def adamw_step_guarded_at_(param, grad, exp_avg, exp_avg_sq, hyper, beta1, beta2, eps, weight_decay, state, coef, grad_sumsq, max_norm=0.0):
    """`adamw_step_guarded_` with lr and grad_scale read when the kernels run from `hyper`, a two-element fp32 DEVICE tensor {lr, grad_scale}: the capture-safe
    form — a replayed graph steps with what the tensor holds at replay time.  Same fp32 values -> the bits of `adamw_step_guarded_`."""
    _check_cuda(param, grad, exp_avg, exp_avg_sq, hyper, state, coef, grad_sumsq)
    for t in (param, grad, exp_avg, exp_avg_sq):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == param.numel()
    if hyper.dtype != torch.float32 or hyper.numel() != 2 or not hyper.is_contiguous():
        raise TypeError("adamw_step_guarded_at_: hyper must be a contiguous two-element fp32 tensor {lr, grad_scale}, got %s %s" % (hyper.dtype, tuple(hyper.shape)))
    assert state.dtype == torch.int64 and state.numel() == 2 and coef.dtype == torch.float32 and coef.numel() == 4 and grad_sumsq.dtype == torch.float64
    check(_lib.load().e2eft_adamw_step_guarded_at(param.numel(), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(hyper), beta1, beta2, eps,
                                                  weight_decay, _ptr(state), _ptr(coef), _ptr(grad_sumsq), max_norm, _stream()))
    return param


def adamw_groups(groups):
    """[(begin, end, lr, beta1, beta2, eps, weight_decay), ...] -> the host table `e2eft_adamw_step_groups` reads (a ctypes array of `_lib.AdamwGroup`; a table
    built once may be passed again and again).  Ranges and counts are checked by the library."""
    if isinstance(groups, C.Array) and groups._type_ is _lib.AdamwGroup:
        return groups
    return (_lib.AdamwGroup * len(groups))(*[_lib.AdamwGroup(int(b), int(e), lr, b1, b2, eps, wd) for b, e, lr, b1, b2, eps, wd in groups])


def _check_adamw_groups(param, grad, exp_avg, exp_avg_sq, table, state, coef, grad_sumsq):
    for t in (param, grad, exp_avg, exp_avg_sq):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == param.numel()
    assert state.dtype == torch.int64 and state.numel() == 2 and grad_sumsq.dtype == torch.float64
    assert coef.dtype == torch.float32 and coef.is_contiguous() and coef.numel() >= 2 + 2 * len(table), "coef: fp32 [2 + 2 * n_groups]"


def adamw_step_groups_(param, grad, exp_avg, exp_avg_sq, groups, state, coef, grad_sumsq, grad_scale=1.0, max_norm=0.0):
    """`adamw_step_guarded_` over parameter groups: `groups` = [(begin, end, lr, beta1, beta2, eps, weight_decay), ...] (or `adamw_groups(...)` of it), up to 8
    ascending ranges of the flat buffers with their own hyper-parameters; one clip factor, one guard, one step counter.  coef: fp32 [2 + 2 * n_groups]."""
    _check_cuda(param, grad, exp_avg, exp_avg_sq, state, coef, grad_sumsq)
    table = adamw_groups(groups)
    _check_adamw_groups(param, grad, exp_avg, exp_avg_sq, table, state, coef, grad_sumsq)
    check(_lib.load().e2eft_adamw_step_groups(param.numel(), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), table, len(table), _ptr(state),
                                              _ptr(coef), _ptr(grad_sumsq), grad_scale, max_norm, _stream()))
    return param


def adamw_step_groups_at_(param, grad, exp_avg, exp_avg_sq, groups, hyper, state, coef, grad_sumsq, max_norm=0.0):
    """`adamw_step_groups_` with grad_scale and every group's lr read when the kernels run from `hyper`, an fp32 DEVICE tensor {grad_scale, lr[0], ...,
    lr[n_groups - 1]} (the lr of `groups` is ignored): the capture-safe form.  Same fp32 words -> the bits of `adamw_step_groups_`."""
    _check_cuda(param, grad, exp_avg, exp_avg_sq, hyper, state, coef, grad_sumsq)
    table = adamw_groups(groups)
    _check_adamw_groups(param, grad, exp_avg, exp_avg_sq, table, state, coef, grad_sumsq)
    if hyper.dtype != torch.float32 or hyper.numel() != 1 + len(table) or not hyper.is_contiguous():
        raise TypeError("adamw_step_groups_at_: hyper must be a contiguous fp32 tensor of 1 + n_groups = %d elements {grad_scale, lr per group}, got %s %s"
                        % (1 + len(table), hyper.dtype, tuple(hyper.shape)))
    check(_lib.load().e2eft_adamw_step_groups_at(param.numel(), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), table, len(table), _ptr(hyper),
                                                 _ptr(state), _ptr(coef), _ptr(grad_sumsq), max_norm, _stream()))
    return param


def ema_step_(shadow, param, one_minus_decay):
    """shadow -= one_minus_decay * (shadow - param) over flat fp32 buffers (diffusers EMAModel.step; csrc/bwd.hip ema_kernel)"""
    _check_cuda(shadow, param)
    assert shadow.dtype == param.dtype == torch.float32 and shadow.is_contiguous() and param.is_contiguous() and shadow.numel() == param.numel()
    check(_lib.load().e2eft_ema_step(shadow.numel(), _ptr(shadow), _ptr(param), float(one_minus_decay), _stream()))
    return shadow


def ema_step_at_(shadow, param, one_minus_decay):
    """`ema_step_` with 1 - decay read on the device from a one-element fp32 tensor when the kernel runs: the capture-safe form, the bits of `ema_step_` for
    the same fp32 value"""
    if not isinstance(one_minus_decay, torch.Tensor) or one_minus_decay.dtype != torch.float32 or one_minus_decay.numel() != 1:
        raise TypeError("ema_step_at_: one_minus_decay must be a one-element fp32 tensor, got %r" % (one_minus_decay,))
    _check_cuda(shadow, param, one_minus_decay)
    assert shadow.dtype == param.dtype == torch.float32 and shadow.is_contiguous() and param.is_contiguous() and shadow.numel() == param.numel()
    check(_lib.load().e2eft_ema_step_at(shadow.numel(), _ptr(shadow), _ptr(param), _ptr(one_minus_decay), _stream()))
    return shadow


def cast_(x, y, mul=1.0, accumulate=False):
    """y <- (y if accumulate else 0) + x*mul with dtype conversion; flat contiguous buffers"""
    _check_cuda(x, y)
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    check(_lib.load().e2eft_cast(dtype_id(x.dtype), dtype_id(y.dtype), x.numel(), mul, 1 if accumulate else 0, _ptr(x), _ptr(y), _stream()))
    return y


# ---------------------------------------------------------------------------------------------------------
# pre- / post-processing of the pipelines' __call__ (csrc/prepost.hip)
def resample_bilinear_aa(x, size, xtab, ytab, round_u8=False, mul=1.0, add=0.0):
    """torch's antialiased bilinear resize of planar images: x [P, h0, w0] uint8 or fp32 (device, contiguous) -> fp32 [P, h, w];
    xtab / ytab = (bounds int32 [out, 2], weights fp32 [out, ksize]) device tables (pipeline.aa_bilinear_tables); round_u8: round to the
    uint8 grid first; then v * mul + add."""
    _check_cuda(x, xtab[0], xtab[1], ytab[0], ytab[1])
    assert x.dim() == 3 and x.is_contiguous() and x.dtype in (torch.uint8, torch.float32)
    P, h0, w0 = x.shape
    h, w = size
    mid = torch.empty((P, h0, w), dtype=torch.float32, device=x.device)
    out = torch.empty((P, h, w), dtype=torch.float32, device=x.device)
    check(_lib.load().e2eft_resample_bilinear_aa(P, h0, w0, h, w, 1 if x.dtype == torch.uint8 else 0, _ptr(x), _ptr(xtab[0]), _ptr(xtab[1]), xtab[1].shape[1],
                                                 _ptr(ytab[0]), _ptr(ytab[1]), ytab[1].shape[1], 1 if round_u8 else 0, mul, add, _ptr(mid), _ptr(out), _stream()))
    return out


def minmax_unit(x):
    """(x - min) / (max - min) over the whole fp32 tensor (zeros when max == min)"""
    _check_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    lib = _lib.load()
    nbytes = lib.e2eft_minmax_unit_workspace_bytes()
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    check(lib.e2eft_minmax_unit(x.numel(), _ptr(x), _ptr(out), _ptr(None), _ptr(ws), nbytes, _stream()))
    return out


def minmax_unit_batched(x, return_minmax=False):
    """minmax_unit per image of a contiguous fp32 [B, ...] batch in one launch sequence: out[b] holds the bits minmax_unit(x[b]) gives (zeros where an
    image is constant); return_minmax: also the fp32 [B, 2] (min, max) table.  No host synchronisation."""
    _check_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 1, "minmax_unit_batched: need a contiguous fp32 [B, ...] batch"
    B = x.shape[0]
    lib = _lib.load()
    nbytes = lib.e2eft_minmax_unit_batched_workspace_bytes(B)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    out = torch.empty_like(x)
    mm = torch.empty((B, 2), dtype=torch.float32, device=x.device) if return_minmax else None
    check(lib.e2eft_minmax_unit_batched(B, x.numel() // B if B else 0, _ptr(x), _ptr(out), _ptr(mm), _ptr(ws), nbytes, _stream()))
    return (out, mm) if return_minmax else out


# ---------------------------------------------------------------------------------------------------------
# test-time ensembling (csrc/ensemble.hip): x is the fp32 [N, ...] stack of the N predictions of one image
def _ens_stack(x):
    _check_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 2, "ensemble: need a contiguous fp32 [N, ...] stack"
    n = x.shape[0]
    lib = _lib.load()
    nbytes = lib.e2eft_ensemble_workspace_bytes(n)
    if nbytes == 0:
        raise RuntimeError("ensemble: %s" % lib.e2eft_last_error().decode())
    return n, x.numel() // n, torch.empty(nbytes // 8, dtype=torch.float64, device=x.device), nbytes


def ensemble_minmax(x):
    """[N, 2] (min, max) of every image of the stack"""
    n, npix, ws, nbytes = _ens_stack(x)
    out = torch.empty((n, 2), dtype=torch.float32, device=x.device)
    check(_lib.load().e2eft_ensemble_minmax(n, npix, _ptr(x), _ptr(out), _ptr(ws), nbytes, _stream()))
    return out


def ensemble_gram(x):
    """fp64 (gram [N, N] = sum_p x_i x_j, sums [N] = sum_p x_i)"""
    n, npix, ws, nbytes = _ens_stack(x)
    gram = torch.empty((n, n), dtype=torch.float64, device=x.device)
    sums = torch.empty(n, dtype=torch.float64, device=x.device)
    check(_lib.load().e2eft_ensemble_gram(n, npix, _ptr(x), _ptr(gram), _ptr(sums), _ptr(ws), nbytes, _stream()))
    return gram, sums


def ensemble_depth_reduce(x, scale, shift, use_mean=False, want_images=True):
    """a_i = x_i * scale_i + shift_i -> (pred, uncertainty, minmax [2]); pred / uncertainty are None when want_images is False"""
    n, npix, ws, nbytes = _ens_stack(x)
    _check_cuda(scale, shift)
    assert scale.dtype == torch.float32 and shift.dtype == torch.float32 and scale.numel() == n and shift.numel() == n
    pred = torch.empty(x.shape[1:], dtype=torch.float32, device=x.device) if want_images else None
    unc = torch.empty(x.shape[1:], dtype=torch.float32, device=x.device) if want_images else None
    minmax = torch.empty(2, dtype=torch.float32, device=x.device)
    check(_lib.load().e2eft_ensemble_depth_reduce(n, npix, _ptr(x), _ptr(scale.contiguous()), _ptr(shift.contiguous()), 1 if use_mean else 0,
                                                  _ptr(pred), _ptr(unc), _ptr(minmax), _ptr(ws), nbytes, _stream()))
    return pred, unc, minmax


def ensemble_depth_finish_(pred, unc, minmax):
    """in place: pred = (pred - min) / (max - min), unc /= (max - min)"""
    _check_cuda(pred, unc, minmax)
    assert pred.dtype == torch.float32 and pred.is_contiguous() and (unc is None or (unc.is_contiguous() and unc.numel() == pred.numel()))
    check(_lib.load().e2eft_ensemble_depth_finish(pred.numel(), _ptr(minmax), _ptr(pred), _ptr(unc), _stream()))
    return pred, unc


def ensemble_normals(x):
    """x [N, 3, H, W] -> (unit vectors [N, 3, H, W], fp64 [N] summed angular error to the mean direction)"""
    n, npix3, ws, nbytes = _ens_stack(x)
    assert x.dim() == 4 and x.shape[1] == 3
    unit = torch.empty_like(x)
    err = torch.empty(n, dtype=torch.float64, device=x.device)
    check(_lib.load().e2eft_ensemble_normals(n, npix3 // 3, _ptr(x), _ptr(unit), _ptr(err), _ptr(ws), nbytes, _stream()))
    return unit, err


# ---------------------------------------------------------------------------------------------------------
# training-sample preparation (csrc/dataprep.hip)
def masked_quantiles(depth, near, far, q_lo=0.02, q_hi=0.98):
    """depth [B, ...] fp32 -> [B, 4] = (q_lo quantile, q_hi quantile, number of valid pixels, ok) over near < depth < far"""
    _check_cuda(depth)
    assert depth.dtype == torch.float32 and depth.is_contiguous() and depth.dim() >= 2
    B = depth.shape[0]
    lib = _lib.load()
    nbytes = lib.e2eft_masked_quantiles_workspace_bytes(B)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=depth.device)
    out = torch.empty((B, 4), dtype=torch.float32, device=depth.device)
    check(lib.e2eft_masked_quantiles(B, depth.numel() // B, _ptr(depth), near, far, q_lo, q_hi, _ptr(out), _ptr(ws), nbytes, _stream()))
    return out


def prepare_sample(rgb01, depth, normal01, near, far, quantiles):
    """rgb01 / normal01 [B,3,H,W] in [0,1], depth [B,1,H,W] metres, quantiles [B,4] -> (rgb, depth3, metric, normals, val_mask bool)"""
    _check_cuda(rgb01, depth, normal01, quantiles)
    B, _, H, W = rgb01.shape
    for t in (rgb01, depth, normal01, quantiles):
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert tuple(depth.shape) == (B, 1, H, W) and tuple(normal01.shape) == (B, 3, H, W) and tuple(quantiles.shape) == (B, 4)
    dev = rgb01.device
    rgb, depth3, normals = torch.empty_like(rgb01), torch.empty_like(rgb01), torch.empty_like(rgb01)
    metric = torch.empty_like(depth)
    mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev)
    check(_lib.load().e2eft_prepare_sample(B, H * W, _ptr(rgb01), _ptr(depth), _ptr(normal01), near, far, _ptr(quantiles), _ptr(rgb), _ptr(depth3),
                                           _ptr(metric), _ptr(normals), _ptr(mask), _stream()))
    return rgb, depth3, metric, normals, mask.bool()


def align_normals_u8(normal_u8, depth, inv_k):
    """Hypersim's camera-facing fix (load.py:185-204,225-232): normal_u8 uint8 [B,H,W,3], depth fp32 [B,H,W] metres, inv_k = 9 floats (row-major inverse
    intrinsics, host) -> uint8 [B,H,W,3]"""
    _check_cuda(normal_u8, depth)
    assert normal_u8.dtype == torch.uint8 and normal_u8.is_contiguous() and normal_u8.dim() == 4 and normal_u8.shape[-1] == 3
    B, H, W, _ = normal_u8.shape
    assert depth.dtype == torch.float32 and depth.is_contiguous() and tuple(depth.shape) == (B, H, W)
    ik = (C.c_double * 9)(*[float(v) for v in inv_k])
    out = torch.empty_like(normal_u8)
    check(_lib.load().e2eft_align_normals_u8(B, H, W, _ptr(normal_u8), _ptr(depth), ik, _ptr(out), _stream()))
    return out


# ------------------------------------------------------------------------------------------------------------
# sample augmentation (csrc/dataaug.hip) and evaluation metrics (csrc/evalmetrics.hip)
def aug_resample_bilinear_u8(img, size, xtab, ytab, flip=None, invert_x_on_flip=False):
    """img uint8 [B,H0,W0,3] -> fp32 [B,3,h,w] in [0,1]: PIL-exact bilinear resize + ToTensor; xtab / ytab = (bounds int32 [out,2], coef int32 [out,k])"""
    _check_cuda(img, xtab[0], xtab[1], ytab[0], ytab[1], flip)
    B, H0, W0, c = img.shape
    assert c == 3 and img.dtype == torch.uint8 and img.is_contiguous()
    h, w = size
    mid = torch.empty((B, H0, w, 3), dtype=torch.uint8, device=img.device)
    out = torch.empty((B, 3, h, w), dtype=torch.float32, device=img.device)
    check(_lib.load().e2eft_aug_resample_bilinear_u8(B, H0, W0, h, w, _ptr(img), _ptr(flip), 1 if invert_x_on_flip else 0, _ptr(xtab[0]), _ptr(xtab[1]),
                                                     xtab[1].shape[1], _ptr(ytab[0]), _ptr(ytab[1]), ytab[1].shape[1], _ptr(mid), _ptr(out), _stream()))
    return out


def aug_gather(img, ymap, xmap, flip=None, invert_x_on_flip=False):
    """index-table gather (nearest resize / crop) with the synchronised flip: fp32 [B,H0,W0] -> [B,h,w], or uint8 [B,H0,W0,3] -> fp32 [B,3,h,w] / 255"""
    _check_cuda(img, ymap, xmap, flip)
    h, w = ymap.numel(), xmap.numel()
    lib = _lib.load()
    if img.dtype == torch.uint8:
        B, H0, W0, c = img.shape
        assert c == 3 and img.is_contiguous()
        out = torch.empty((B, 3, h, w), dtype=torch.float32, device=img.device)
        check(lib.e2eft_aug_gather_u8(B, H0, W0, h, w, _ptr(img), _ptr(ymap), _ptr(xmap), _ptr(flip), 1 if invert_x_on_flip else 0, _ptr(out), _stream()))
        return out
    B, H0, W0 = img.shape
    assert img.dtype == torch.float32 and img.is_contiguous()
    out = torch.empty((B, h, w), dtype=torch.float32, device=img.device)
    check(lib.e2eft_aug_gather_f32(B, H0, W0, h, w, _ptr(img), _ptr(ymap), _ptr(xmap), _ptr(flip), _ptr(out), _stream()))
    return out


def depth_eval(pred, gt, mask, disparity=False, align_max_res=0, min_depth=1e-3, max_depth=80.0, return_aligned=False):
    """pred, gt fp32 [B,H,W], mask bool / uint8 [B,H,W] -> metrics fp32 [B,12] (see include/e2eft.h) [, aligned prediction [B,H,W]]"""
    _check_cuda(pred, gt, mask)
    B, H, W = pred.shape
    pred, gt = pred.float().contiguous(), gt.float().contiguous()
    mask = mask.to(torch.uint8).contiguous()
    lib = _lib.load()
    nws = lib.e2eft_depth_eval_workspace_bytes(B)
    ws = torch.empty(((nws + 7) // 8,), dtype=torch.float64, device=pred.device)
    out = torch.empty((B, 12), dtype=torch.float32, device=pred.device)
    aligned = torch.empty_like(pred) if return_aligned else None
    check(lib.e2eft_depth_eval(B, H, W, _ptr(pred), _ptr(gt), _ptr(mask), 1 if disparity else 0, int(align_max_res or 0), float(min_depth), float(max_depth),
                               _ptr(out), _ptr(aligned), _ptr(ws), nws, _stream()))
    return (out, aligned) if return_aligned else out


def normal_eval_workspace(device):
    """one workspace for e2eft_normal_eval_update / _finalize (16-byte aligned, reused by every call of an accumulator)"""
    n = _lib.load().e2eft_normal_eval_workspace_bytes()
    return torch.empty(((n + 15) // 16 * 2,), dtype=torch.float64, device=device), n


def normal_eval_update(pred, gt, mask, err, offset, totals, ws, nws):
    """pred, gt fp32 [B,3,H,W] (any element strides), mask uint8 [B,H,W] (any strides) or None -> errors into err[offset : offset + B*H*W]
    (+inf where the mask is 0); the update's totals are added to `totals` (int64 [9], see include/e2eft.h)"""
    _check_cuda(pred, gt, mask, err, totals, ws)
    assert pred.dtype == torch.float32 and gt.dtype == torch.float32 and err.dtype == torch.float32 and totals.dtype == torch.int64
    assert pred.dim() == 4 and pred.shape == gt.shape and pred.shape[1] == 3, (pred.shape, gt.shape)
    B, _, H, W = pred.shape
    d = _lib.NormalEvalDesc()
    d.batch, d.height, d.width = B, H, W
    d.pred_stride[:] = list(pred.stride())
    d.gt_stride[:] = list(gt.stride())
    if mask is not None:
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == (B, H, W), (mask.dtype, mask.shape)
        d.mask_stride[:] = list(mask.stride())
    check(_lib.load().e2eft_normal_eval_update(C.byref(d), _ptr(pred), _ptr(gt), _ptr(mask), _ptr(err), int(offset), err.numel(), _ptr(totals),
                                               _ptr(ws), nws, _stream()))


def normal_eval_finalize(err, count, totals, ws, nws, out=None):
    """-> fp64 [9]: mean, median, rmse, a1..a5, n over err[:count] and the totals (include/e2eft.h)"""
    _check_cuda(err, totals, ws)
    if out is None:
        out = torch.empty((9,), dtype=torch.float64, device=totals.device)
    check(_lib.load().e2eft_normal_eval_finalize(_ptr(err) if count else C.c_void_p(0), int(count), _ptr(totals), _ptr(out), _ptr(ws), nws, _stream()))
    return out


_D2NT_FORMATS = {"f32": (_lib.D2NT_F32, torch.float32), "u16": (_lib.D2NT_U16, torch.uint16), "u8": (_lib.D2NT_U8, torch.uint8)}


def depth_to_normals(depth, intrinsics, refine=True, out_format="f32", depth_scale=1.0, out=None):
    """the D2NT translator (csrc/d2nt.hip, include/e2eft.h e2eft_depth_to_normals): depth fp32 [B,H,W] (or [H,W]), intrinsics fp32 (fx, fy, cx, cy)
    as a device tensor [B,4] or [4] (one camera for the batch) -> channels-last [B,H,W,3] normals: "f32", the file's "u16" or the loader's "u8"
    (its high byte).  refine: v3 (MRF refinement) / v2.  Z = depth * depth_scale in fp32 before anything else."""
    if out_format not in _D2NT_FORMATS:
        raise ValueError("out_format must be one of %s, got %r" % (sorted(_D2NT_FORMATS), out_format))
    fmt, odt = _D2NT_FORMATS[out_format]
    squeeze = depth.dim() == 2
    d = depth[None] if squeeze else depth
    assert d.dim() == 3 and d.dtype == torch.float32, (tuple(depth.shape), depth.dtype)
    d = d.contiguous()
    B, H, W = d.shape
    if not isinstance(intrinsics, torch.Tensor):
        intrinsics = torch.tensor([float(v) for v in intrinsics], dtype=torch.float32, device=d.device)
    k = intrinsics.to(torch.float32)
    if k.dim() == 1:
        assert k.numel() == 4, tuple(k.shape)
        k = k[None].expand(B, 4)
    assert tuple(k.shape) == (B, 4), (tuple(k.shape), B)
    k = k.contiguous()
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=odt, device=d.device)
    assert out.dtype == odt and tuple(out.shape) == (B, H, W, 3) and out.is_contiguous(), (out.dtype, tuple(out.shape))
    _check_cuda(d, k, out)
    desc = _lib.D2ntDesc()
    desc.batch, desc.height, desc.width, desc.refine, desc.out_format, desc.depth_scale = B, H, W, 1 if refine else 0, fmt, float(depth_scale)
    check(_lib.load().e2eft_depth_to_normals(C.byref(desc), _ptr(d), _ptr(k), _ptr(out), _stream()))
    return out[0] if squeeze else out


_HYPERSIM_DEPTH = {"u16": (_lib.HYPERSIM_DEPTH_U16, torch.uint16), "f32": (_lib.HYPERSIM_DEPTH_F32, torch.float32)}
HYPERSIM_RECORD_FIELDS = ("invalid_ratio", "rgb_mean", "rgb_std", "rgb_min", "rgb_max", "depth_mean", "depth_std", "depth_min", "depth_max",
                          "zero_ids", "nan_brightness", "n_valid", "percentile", "scale")


def hypersim_scale_numerator():
    """hypersim_util.py:41-44: np.power(0.8, inv_gamma) with inv_gamma = 1.0 / (1.0 / 2.2), as this host's numpy computes it (once)"""
    import numpy as np
    return float(np.power(0.8, 1.0 / (1.0 / 2.2)))


def hypersim_preprocess(color, distance, entity_id, focal=886.81, depth_format="u16", out=None):
    """raw Hypersim frames -> what preprocess_hypersim.py stores (csrc/hypersimprep.hip, include/e2eft.h e2eft_hypersim_preprocess): color [B,H,W,3] and
    distance [B,H,W] fp16 or fp32, entity_id int32 [B,H,W] (or one frame without the batch axis) -> (rgb_u8 uint8 [B,H,W,3] tone-mapped, depth [B,H,W]
    planar: "u16" the file's millimetres / "f32" metres as the training loader reads the file back, record fp64 [B,16]: HYPERSIM_RECORD_FIELDS).
    out = (rgb_u8, depth, record) to write into existing tensors.  No host synchronisation."""
    if depth_format not in _HYPERSIM_DEPTH:
        raise ValueError("depth_format must be one of %s, got %r" % (sorted(_HYPERSIM_DEPTH), depth_format))
    fmt, odt = _HYPERSIM_DEPTH[depth_format]
    squeeze = entity_id.dim() == 2
    c, d, e = (color[None], distance[None], entity_id[None]) if squeeze else (color, distance, entity_id)
    if c.dim() != 4 or c.shape[-1] != 3 or tuple(d.shape) != tuple(c.shape[:3]) or tuple(e.shape) != tuple(c.shape[:3]):
        raise ValueError("hypersim_preprocess: color [B,H,W,3], distance and entity_id [B,H,W]; got %s, %s, %s" % (tuple(color.shape), tuple(distance.shape), tuple(entity_id.shape)))
    for name, t in (("color", c), ("distance", d)):
        if t.dtype not in (torch.float16, torch.float32):
            raise TypeError("hypersim_preprocess: %s must be float16 or float32, got %s" % (name, t.dtype))
    if e.dtype != torch.int32:
        raise TypeError("hypersim_preprocess: entity_id must be int32, got %s" % e.dtype)
    c, d, e = c.contiguous(), d.contiguous(), e.contiguous()
    B, H, W = e.shape
    dev = c.device
    if out is None:
        out = (torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev), torch.empty((B, H, W), dtype=odt, device=dev),
               torch.empty((B, _lib.HYPERSIM_RECORD), dtype=torch.float64, device=dev))
    rgb, depth, rec = out
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (B, H, W, 3) and rgb.is_contiguous(), (rgb.dtype, tuple(rgb.shape))
    assert depth.dtype == odt and tuple(depth.shape) == (B, H, W) and depth.is_contiguous(), (depth.dtype, tuple(depth.shape))
    assert rec.dtype == torch.float64 and tuple(rec.shape) == (B, _lib.HYPERSIM_RECORD) and rec.is_contiguous(), (rec.dtype, tuple(rec.shape))
    _check_cuda(c, d, e, rgb, depth, rec)
    desc = _lib.HypersimDesc()
    desc.batch, desc.height, desc.width, desc.color_dtype, desc.distance_dtype, desc.depth_format = B, H, W, _lib.dtype_id(c.dtype), _lib.dtype_id(d.dtype), fmt
    desc.focal, desc.scale_numerator = float(focal), hypersim_scale_numerator()
    lib = _lib.load()
    nbytes = lib.e2eft_hypersim_preprocess_workspace_bytes(C.byref(desc))
    if nbytes == 0:
        raise RuntimeError(lib.e2eft_last_error().decode())
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=dev)
    check(lib.e2eft_hypersim_preprocess(C.byref(desc), _ptr(c), _ptr(d), _ptr(e), _ptr(rgb), _ptr(depth), _ptr(rec), _ptr(ws), nbytes, _stream()))
    return (rgb[0], depth[0], rec[0]) if squeeze else (rgb, depth, rec)


_GT_DTYPES = {torch.uint16: _lib.GT_U16, torch.int32: _lib.GT_I32, torch.float32: _lib.GT_F32}


def depth_gt_prepare(raw, divisor=1.0, min_depth=0.0, max_depth=float("inf"), crop=None, window=None, inf_to_zero=False, ext_mask=None, count=True, out=None):
    """decoded benchmark ground truth -> evaluation inputs (csrc/evalprep.hip, include/e2eft.h e2eft_depth_gt_prepare): raw [B,H0,W0] (or one raster
    [H0,W0]) uint16, int32 or float32 -> (depth fp32 [B,h,w] = float(double(raw) / divisor), valid mask bool [B,h,w], n_valid int32 [B] or None).
    crop = (top, left, h, w) inside the raster (None: all of it); window = (y0, y1, x0, x1) in output coordinates, clamped to the output here as a
    slice would be (None: no evaluation window); inf_to_zero: +inf -> 0 before the range test; ext_mask uint8 / bool [B,H0,W0]: the mask is
    ext_mask != 0 alone, cropped like raw.  out = (depth, mask uint8, n_valid) to write into existing tensors.  No host synchronisation."""
    squeeze = raw.dim() == 2
    r = raw[None] if squeeze else raw
    if r.dim() != 3:
        raise ValueError("depth_gt_prepare: raw must be [H,W] or [B,H,W]; got %s" % (tuple(raw.shape),))
    if r.dtype not in _GT_DTYPES:
        raise TypeError("depth_gt_prepare: raw must be uint16, int32 or float32, got %s" % r.dtype)
    r = r.contiguous()
    B, H0, W0 = r.shape
    top, left, h, w = (0, 0, H0, W0) if crop is None else (int(v) for v in crop)
    if top < 0 or left < 0 or h <= 0 or w <= 0 or top + h > H0 or left + w > W0:
        raise ValueError("depth_gt_prepare: crop %d x %d at (%d, %d) lies outside the %d x %d raster" % (h, w, top, left, H0, W0))
    y0, y1, x0, x1 = (0, h, 0, w) if window is None else (int(v) for v in window)
    y0, y1, x0, x1 = min(max(y0, 0), h), min(max(y1, 0), h), min(max(x0, 0), w), min(max(x1, 0), w)
    y1, x1 = max(y1, y0), max(x1, x0)
    e = None
    if ext_mask is not None:
        e = ext_mask[None] if ext_mask.dim() == 2 else ext_mask
        if e.dtype not in (torch.uint8, torch.bool):
            raise TypeError("depth_gt_prepare: ext_mask must be uint8 or bool, got %s" % e.dtype)
        if tuple(e.shape) != (B, H0, W0):
            raise ValueError("depth_gt_prepare: ext_mask %s does not match raw %s" % (tuple(ext_mask.shape), tuple(raw.shape)))
        e = e.contiguous()
        e = e.view(torch.uint8) if e.dtype == torch.bool else e
    dev = r.device
    if out is None:
        out = (torch.empty((B, h, w), dtype=torch.float32, device=dev), torch.empty((B, h, w), dtype=torch.uint8, device=dev),
               torch.empty((B,), dtype=torch.int32, device=dev) if count else None)
    depth, mask, nv = out
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (B, h, w) and depth.is_contiguous(), (depth.dtype, tuple(depth.shape))
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (B, h, w) and mask.is_contiguous(), (mask.dtype, tuple(mask.shape))
    assert nv is None or (nv.dtype == torch.int32 and tuple(nv.shape) == (B,) and nv.is_contiguous()), (nv.dtype, tuple(nv.shape))
    _check_cuda(r, e, depth, mask, nv)
    desc = _lib.DepthGtDesc()
    desc.batch, desc.h0, desc.w0, desc.raw_dtype, desc.divisor, desc.inf_to_zero = B, H0, W0, _GT_DTYPES[r.dtype], float(divisor), 1 if inf_to_zero else 0
    desc.crop_top, desc.crop_left, desc.crop_h, desc.crop_w = top, left, h, w
    desc.min_depth, desc.max_depth = float(min_depth), float(max_depth)
    desc.win_y0, desc.win_y1, desc.win_x0, desc.win_x1, desc.use_ext_mask = y0, y1, x0, x1, 0 if e is None else 1
    check(_lib.load().e2eft_depth_gt_prepare(C.byref(desc), _ptr(r), _ptr(e), _ptr(depth), _ptr(mask), _ptr(nv), _stream()))
    mb = mask.view(torch.bool)
    return (depth[0], mb[0], nv) if squeeze else (depth, mb, nv)


_NORMAL_GT_DTYPES = {torch.uint8: _lib.NORMAL_GT_U8, torch.float32: _lib.NORMAL_GT_F32}


def normal_gt_prepare(raw, out=None):
    """decoded benchmark normals -> evaluation inputs (csrc/normalprep.hip, include/e2eft.h e2eft_normal_gt_prepare): raw [B,H,W,3] (or one raster
    [H,W,3]), R, G, B interleaved, uint8 (a PNG: mask = r + g + b > 0, normal = u8 / 255 * 2 - 1 in fp32) or float32 (an EXR: mask = |n| > 0.5, the
    values pass through bit for bit) -> (normal fp32 [B,3,H,W], mask bool [B,1,H,W], n_valid int32 [B]).  out = (normal, mask uint8, n_valid) to
    write into existing tensors.  No host synchronisation."""
    squeeze = raw.dim() == 3
    r = raw[None] if squeeze else raw
    if r.dim() != 4 or r.shape[-1] != 3:
        raise ValueError("normal_gt_prepare: raw must be [H,W,3] or [B,H,W,3]; got %s" % (tuple(raw.shape),))
    if r.dtype not in _NORMAL_GT_DTYPES:
        raise TypeError("normal_gt_prepare: raw must be uint8 or float32, got %s" % r.dtype)
    if r.numel() == 0:
        raise ValueError("normal_gt_prepare: empty raster %s" % (tuple(raw.shape),))
    r = r.contiguous()
    B, H, W, _ = r.shape
    dev = r.device
    if out is None:
        out = (torch.empty((B, 3, H, W), dtype=torch.float32, device=dev), torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev),
               torch.empty((B,), dtype=torch.int32, device=dev))
    normal, mask, nv = out
    assert normal.dtype == torch.float32 and tuple(normal.shape) == (B, 3, H, W) and normal.is_contiguous(), (normal.dtype, tuple(normal.shape))
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (B, 1, H, W) and mask.is_contiguous(), (mask.dtype, tuple(mask.shape))
    assert nv.dtype == torch.int32 and tuple(nv.shape) == (B,) and nv.is_contiguous(), (nv.dtype, tuple(nv.shape))
    desc = _lib.NormalGtDesc()
    desc.batch, desc.height, desc.width, desc.raw_dtype = B, H, W, _NORMAL_GT_DTYPES[r.dtype]
    with on_device_of(r):
        _check_cuda(r, normal, mask, nv)
        check(_lib.load().e2eft_normal_gt_prepare(C.byref(desc), _ptr(r), _ptr(normal), _ptr(mask), _ptr(nv), _stream()))
    mb = mask.view(torch.bool)
    return (normal[0], mb[0], nv[0]) if squeeze else (normal, mb, nv)


_RGB_LAYOUTS = {"hwc": _lib.RGB_HWC, "chw": _lib.RGB_CHW}


def dsine_rgb_requantize(rgb_u8, layout="hwc", out=None, workspace=None):
    """the image DSINE's benchmark mode hands to the pipeline (csrc/normalprep.hip, include/e2eft.h e2eft_dsine_rgb_requantize): rgb_u8 uint8 [B,H,W,3]
    (or one image [H,W,3]) as decoded -> normalised with the ImageNet constants, stretched to the tensor's own minimum and maximum over all channels
    and truncated to uint8 again (test.py:59-65; NOT the identity: every channel is stretched differently).  layout "hwc": [B,H,W,3], what
    Image.fromarray takes; "chw": [B,3,H,W], what the pipelines accept as a tensor.  An image with one single normalised value gives zeros (the
    reference divides by zero).  out: an existing uint8 tensor of the output's shape; workspace: int32 [6 * B] (allocated when None; pass one under
    graph capture to keep it out of the graph's pool).  No host synchronisation."""
    if layout not in _RGB_LAYOUTS:
        raise ValueError("dsine_rgb_requantize: layout must be one of %s, got %r" % (sorted(_RGB_LAYOUTS), layout))
    squeeze = rgb_u8.dim() == 3
    r = rgb_u8[None] if squeeze else rgb_u8
    if r.dim() != 4 or r.shape[-1] != 3:
        raise ValueError("dsine_rgb_requantize: rgb_u8 must be [H,W,3] or [B,H,W,3]; got %s" % (tuple(rgb_u8.shape),))
    if r.dtype != torch.uint8:
        raise TypeError("dsine_rgb_requantize: rgb_u8 must be uint8, got %s" % r.dtype)
    if r.numel() == 0:
        raise ValueError("dsine_rgb_requantize: empty image %s" % (tuple(rgb_u8.shape),))
    r = r.contiguous()
    B, H, W, _ = r.shape
    dev = r.device
    shape = (B, H, W, 3) if layout == "hwc" else (B, 3, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    o = out[None] if squeeze and out.dim() == 3 else out
    assert o.dtype == torch.uint8 and tuple(o.shape) == shape and o.is_contiguous(), (o.dtype, tuple(o.shape))
    if o.data_ptr() == r.data_ptr():
        raise ValueError("dsine_rgb_requantize: out must not be the input")
    if workspace is None:
        workspace = torch.empty((_lib.DSINE_RGB_WS_INTS * B,), dtype=torch.int32, device=dev)
    assert workspace.dtype == torch.int32 and workspace.numel() >= _lib.DSINE_RGB_WS_INTS * B and workspace.is_contiguous(), (workspace.dtype, tuple(workspace.shape))
    desc = _lib.DsineRgbDesc()
    desc.batch, desc.height, desc.width, desc.out_layout = B, H, W, _RGB_LAYOUTS[layout]
    with on_device_of(r):
        _check_cuda(r, o, workspace)
        check(_lib.load().e2eft_dsine_rgb_requantize(C.byref(desc), _ptr(r), _ptr(o), _ptr(workspace), _stream()))
    return o[0] if squeeze else o
