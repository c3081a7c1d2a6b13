"""Memory containment of the libe2eft kernels (tests/containment.py): every op runs twice, once per fill (0xFF: NaN in every float type, 0x00: zero).  In each run
every tensor operand the Python entry accepts as a view IS a guarded view (inputs, residuals, out=), and torch.empty & co. hand out tensors full of the fill, so
workspaces, partial-sum slabs, pad columns and self-allocated outputs start as NaN / as zero.  Asserted per case:
  (a) the output is finite and within the tolerance of the family's own parity test against the same fp64 CPU reference;
  (b) the outputs of the two runs are torch.equal (identical layout and addresses);
  (c) the guard bands of every guarded buffer, inputs included, still hold the fill, outside the allowed write set;
  (d) the kernel the case is meant to reach took the launch.  The library names a launch (ops._last_kernel(), e2eft_debug_*_launches) for igemm2 / igemm5 / igemm6,
      narrow.hip, convin.hip, the fp32 split routes and the two fp32 attention kernels: those cases assert the name (operand path and wave count of igemm2 included).
      Where it names nothing, the route is asserted by what the host layer can observe, or (d) CANNOT be asserted and the case says only that the entry point ran:
        split-K convolution        e2eft_conv2d_splitk_workspace_bytes > 0 for the descriptor that is launched
        fused-norm convolution     out._e2eft_keep (the coefficient workspace) is attached
        statistics epilogues       out._e2eft_gn is attached
        weight gradients           conv2d_wgrad / linear_wgrad return a tensor (None = the direct kernel refused) and, with out=, the slot's own address; WHICH of wgrad.hip's
                                   tile shapes or whether the fp32 planes or wgrad32_kernel ran is set by OPT_F32_SPLIT but not observable
        folded cross-attention     the module's _fold_cache is filled
        16-bit attention (OPT_ATTN_DMA 0 / 1), attention512 (split tail on / off), attention_bwd in 16-bit, the norms, softmax, GEGLU, layout, elementwise, optimizer,
        loss, resize, data, ensemble and evaluation kernels: one kernel family per entry point and no tag — not assertable; an ignored option would pass unseen here
        (tests/test_attn_dma_gpu.py compares the two DMA settings with each other).

ALLOWED WRITES beyond the logical extent — exactly what include/e2eft.h documents, each asserted to hold the documented value.  In every case below the documented pad
lies inside the buffer the entry point itself takes or allocates as ONE dense tensor, so the guard bands of the cases stay "logical extent only" and the pad is an
output of its own that must be all zero:
  e2eft_transpose        "out[z][c][r] = ... 0 for rows <= r < rows_pad"                       zeros in [rows, rows_pad) of the dense [Z, C, rows_pad] output
  e2eft_conv2d_im2col_t  "im2col_t writes zeros in [P, ldcol)"                                 zeros in [P, ldcol) of the dense [K, ldcol] output
  e2eft_softmax_rows, e2eft_softmax_rows_causal, e2eft_softmax_bwd_rows
                         "The pad columns [n, roundup(n, 16 bytes)) of every row are written as zeros"  zeros there in the dense [rows, lds] buffer of s and of dp; these
                         columns hold the fill going in.  (The header said this for none of the three; the sentence was added with this module: the kernels' behaviour.)
  e2eft_nchw_to_nhwc     "channels zero-padded from c to cpad"                                 zeros in [c, cpad) of the (poisoned) output
  e2eft_*_head_bwd       "cpad >= 3 channels written (zeros beyond 3)"                         zeros in [3, cpad) of the (poisoned) output
  e2eft_randn_fill, e2eft_pyramid_noise   "channels c..ldy untouched"                          no exception at all: guarded channel slices, bands intact
Every other case allows the logical extent only.

No output is exempt from (b): no reduction of csrc/ goes through floating-point atomics (the losses and sumsq sum per-block partials in a fixed order).
The atomicAdd calls of csrc/ are integer and exact: the histograms of dataprep.hip, normaleval.hip and hypersimprep.hip, the valid-pixel counts of evalprep.hip and
normalprep.hip, and the per-frame statistics of hypersimprep.hip (unsigned 64-bit sums next to atomicMin / atomicMax)."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from containment import FILLS, check_two_fills, guarded, poisoned_allocations
from util import DTYPES, TOL as TOL_FOLD, assert_close, pack_conv_weight, q, rel_err, to_nchw

pytestmark = pytest.mark.gpu
HALF = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def ops(dev):
    from diffusion_e2e_ft_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L(dev):
    from diffusion_e2e_ft_amd import _lib
    lib = _lib.load()
    for n in ("e2eft_debug_patch_launches", "e2eft_debug_persistent_launches", "e2eft_debug_thin_launches"):
        getattr(lib, n).restype = ctypes.c_long
    return _lib


def _g(seed):
    return torch.Generator().manual_seed(seed)


class Guards(list):
    """the guarded operands of one run: inp() an input (data inside, fill around), out() an output (fill everywhere)"""

    def __init__(self, dtype, dev, fill, ld_unit=None):
        super().__init__()
        self.dtype, self.dev, self.fill, self.ld_unit = dtype, dev, fill, ld_unit

    def inp(self, t, dtype=None, **kw):
        dtype = dtype or self.dtype
        kw.setdefault("ld_unit", self.ld_unit)
        b, v = guarded(t.shape, dtype, self.dev, self.fill, data=t.to(dtype).to(self.dev), **kw)
        self.append([b, v, None])
        return v

    def out(self, shape, dtype=None, allowed=None, **kw):
        kw.setdefault("ld_unit", self.ld_unit)
        b, v = guarded(shape, dtype or self.dtype, self.dev, self.fill, **kw)
        self.append([b, v, allowed])
        return v

    def flat(self, n, dtype=torch.float32, misalign=False, data=None):
        """a dense slot of n elements inside a guarded flat buffer (FlatAdamW's gradient / parameter slots), 16-byte aligned or one element off"""
        unit = 16 // torch.empty(0, dtype=dtype).element_size()
        b, v = guarded((1, n), dtype, self.dev, self.fill, data=None if data is None else data.view(1, n), col0=unit + (1 if misalign else 0), rows_before=1, rows_after=1, cols_after=4096)
        self.append([b, v, None])
        return v.view(-1)


def nhwc_cpu(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _closer(ref, dtype, what, scale=1.0):
    def check(name, t):
        r = ref[name] if isinstance(ref, dict) else ref
        s = scale[name] if isinstance(scale, dict) else scale
        assert_close(t.float().cpu() if t.dtype != torch.float64 else t.cpu(), r.float() if t.dtype != torch.float64 else r, dtype, "%s %s" % (what, name), scale=s)
    return check


# ================================================================================================ GEMM
# (M, N, K, epilogue): one row past a 128-row tile + ragged N + a K tail of 8; 2.3 tiles with the bias along m; a K of whole 64-/32-element k-tiles (the FAST operand path)
GEMM_CASES = [(129, 72, 72, "bias+residual"), (300, 200, 136, "bias_along_m"), (129, 72, 128, "bias+residual")]


def _gemm_case(ops, dev, dtype, M, N, K, epi, expect):
    g = _g(M * 7 + N)
    a, w = q(torch.randn(M, K, generator=g), dtype), q(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    along_m = epi == "bias_along_m"
    bias = q(torch.randn(M if along_m else N, generator=g), dtype)
    res = None if along_m else q(torch.randn(M, N, generator=g), dtype)
    ref = a.double() @ w.double().t() + (bias.double()[:, None] if along_m else bias.double())
    ref = (ref if along_m else 0.5 * ref + res.double()).float()

    def run(fill):
        gs = Guards(dtype, dev, fill)
        av, wv, ov = gs.inp(a), gs.inp(w), gs.out((M, N))
        rv = None if res is None else gs.inp(res)
        ops.gemm(av, wv, bias.to(dtype).to(dev), rv, out=ov, alpha=1.0 if along_m else 0.5, bias_along_m=along_m)
        assert expect in ops._last_kernel(), (ops._last_kernel(), expect)
        return dict(out=ov), gs

    check_two_fills(run, _closer(ref, dtype, "gemm"), what="gemm %s %s %s" % ((M, N, K), epi, expect))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("waves", [4, 8])
def test_gemm(ops, L, dev, dtype, general, waves):
    tname = {torch.float32: "float", torch.float16: "_Float16", torch.bfloat16: "__bf16"}[dtype]
    with L.option(L.OPT_IGEMM_GENERAL_OPERANDS, general), L.option(L.OPT_IGEMM2_WAVES, waves), L.option(L.OPT_PERSISTENT, 0):
        for (M, N, K, epi) in GEMM_CASES:
            fast = (K % (128 // dtype.itemsize) == 0) and not general
            _gemm_case(ops, dev, dtype, M, N, K, epi, "igemm2_kernel<%s, 0, %s, %d>" % (tname, "true" if fast else "false", waves))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_gn_statistics_and_consuming_groupnorm(ops, L, dev, dtype):
    """ops.linear(gn_rows_per_image=...) at M = 256, N = 72 into a guarded output, then the GroupNorm that consumes the (poisoned, then written) partial statistics"""
    g = _g(17)
    B, H, W, K, N, groups = 2, 16, 8, 64, 72, 9
    t, wl = q(torch.randn(B, H, W, K, generator=g), dtype), q(torch.randn(N, K, generator=g) / 8, dtype)
    res = q(torch.randn(B, H, W, N, generator=g), dtype)
    ga, be = q(1 + 0.3 * torch.randn(N, generator=g), dtype), q(0.3 * torch.randn(N, generator=g), dtype)
    lin = (t.double() @ wl.double().t() + res.double()).float()

    def run(fill):
        gs = Guards(dtype, dev, fill)
        tv, rv, ov, yv = gs.inp(t), gs.inp(res), gs.out((B, H, W, N)), gs.out((B, H, W, N))
        lo = ops.linear(tv, wl.to(dtype).to(dev), residual=rv, out=ov, gn_rows_per_image=H * W)
        assert getattr(lo, "_e2eft_gn", None) is not None and "igemm2_kernel" in ops._last_kernel(), "no statistics emitted"
        ops.groupnorm(lo, ga.to(dtype).to(dev), be.to(dtype).to(dev), groups, 1e-6, False, out=yv)
        return dict(linear=ov, partial=lo._e2eft_gn.partial, gn=yv), gs

    def check(name, o):
        if name == "linear":
            assert_close(o.float().cpu(), lin, dtype, "linear")

    got = check_two_fills(run, check, what="gemm gnstats")
    # the norm of the tensor that was written (as tests/test_ops_gpu.py::test_groupnorm_with_producer_statistics)
    refl = F.group_norm(got["linear"].float().cpu().permute(0, 3, 1, 2).double(), groups, ga.double(), be.double(), 1e-6).float()
    assert_close(to_nchw(got["gn"]), refl, dtype, "groupnorm on gemm statistics", scale=1.5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bgemm_into_a_guarded_score_buffer(ops, dev, dtype):
    """tests/test_ops_gpu.py::test_bgemm (Nk = 77 in rows of 80) with head-strided guarded operands and a guarded [B, heads, N, .] score buffer"""
    g = _g(5)
    B, H, N, Nk, D = 2, 3, 150, 77, 64
    qq, kk = q(torch.randn(B, N, H * D, generator=g), dtype), q(torch.randn(B, Nk, H * D, generator=g), dtype)
    ref = torch.einsum("bnhd,bmhd->bhnm", qq.view(B, N, H, D).double(), kk.view(B, Nk, H, D).double()).float()

    def run(fill):
        gs = Guards(dtype, dev, fill)
        qv, kv, sv = gs.inp(qq), gs.inp(kk), gs.out((B, H, N, Nk))
        ldq, ldk, lds = qv.stride(1), kv.stride(1), sv.stride(2)
        ops.bgemm_raw(dtype, N, Nk, D, qv, ldq, (N * ldq, D), kv, ldk, (Nk * ldk, D), sv, lds, (H * N * lds, N * lds), B, H)
        assert "igemm2_kernel" in ops._last_kernel()
        return dict(S=sv), gs

    check_two_fills(run, _closer(ref, dtype, "bgemm"), what="bgemm")


# (M, N, K, bias, residual): tests/test_persistent_gpu.py's smallest GEMM with a ragged N tile and the whole epilogue
@pytest.mark.parametrize("dtype", HALF)
def test_gemm_persistent(ops, L, dev, dtype):
    M, N, K = 4096, 320, 320
    g = _g(M + N + K)
    a, w = q(torch.randn(M, K, generator=g), dtype), q(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    b, r = q(torch.randn(N, generator=g), dtype), q(torch.randn(M, N, generator=g), dtype)
    ref = (a.double() @ w.double().t() + b.double() + r.double()).float()

    def run(fill):
        gs = Guards(dtype, dev, fill)
        av, wv, rv, ov = gs.inp(a), gs.inp(w), gs.inp(r), gs.out((M, N))
        n0 = L.load().e2eft_debug_persistent_launches()
        ops.gemm(av, wv, b.to(dtype).to(dev), rv, out=ov)
        assert L.load().e2eft_debug_persistent_launches() - n0 == 1 and "igemm5_kernel" in ops._last_kernel(), ops._last_kernel()
        return dict(out=ov), gs

    with L.option(L.OPT_PERSISTENT_GRID, 8), L.option(L.OPT_PERSISTENT_MIN_QROUNDS, 8), L.option(L.OPT_PERSISTENT, 1):
        check_two_fills(run, _closer(ref, dtype, "persistent gemm"), what="persistent gemm")


def test_gemm_f32split(ops, L, dev):
    """tests/test_f32split_gpu.py's ragged nn.Linear (1100 rows = 4.3 tiles of 256): the split planes of a guarded A, a guarded residual and output"""
    M, N, K = 1100, 320, 320
    g = _g(M + N + K)
    a = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, K, generator=g))
    w, b, r = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ref = (a.double() @ w.double().t() + b.double() + r.double()).float()

    def run(fill):
        gs = Guards(torch.float32, dev, fill, ld_unit=8)        # (igemm5's vector epilogue takes rows of whole 32 bytes: ldo % 8, ldr % 8)
        av, rv, ov = gs.inp(a), gs.inp(r), gs.out((M, N))
        ops.gemm(av, w.to(dev), b.to(dev), rv, out=ov)
        assert "f32split" in ops._last_kernel() and "igemm5" in ops._last_kernel(), ops._last_kernel()
        return dict(out=ov), gs

    with L.option(L.OPT_PERSISTENT_GRID, 8), L.option(L.OPT_F32_SPLIT, 1):
        check_two_fills(run, _closer(ref, torch.float32, "f32split gemm"), what="f32split gemm")


# ================================================================================================ convolution forward
def _conv_ref(x, x2, w, b, k, stride, pad, up_to, ra, rs, alpha):
    xin = x if x2 is None else torch.cat([x, x2], dim=1)
    if up_to is not None:
        xin = F.interpolate(xin, size=up_to, mode="nearest")
    xin = F.pad(xin, (pad[2], pad[3], pad[0], pad[1]))
    ref = F.conv2d(xin.double(), w.double(), None if b is None else b.double(), stride=stride).float()
    if ra is not None:
        ref = ref + ra[:, :, None, None]
    ref = ref * alpha
    if rs is not None:
        ref = ref + rs
    return ref


def _conv_case(ops, L, dev, dtype, B, Ci, Co, H, W, k=3, stride=1, pad=(1, 1, 1, 1), up_to=None, c2=0, rowadd=False, residual=False, alpha=1.0, bias=True, norm=False,
               gn_stats=False, kernel=None, counter=None, splitk=False, phases=False, scale=1.0, what="conv", dense_x=False, ld_unit=None):
    """one convolution: the input a channel slice of a three times wider buffer, second source / residual / output channel slices of wider buffers.  dense_x: the
    input dense inside a guarded flat buffer (csrc/convin.hip takes 8-channel pixels of 16 bytes, ldx = 8, only)"""
    g = _g(B * 1000 + H * 10 + Ci + Co + W + k)
    x = q(torch.randn(B, Ci, H, W, generator=g) * (2.0 if norm else 1.0) + (0.7 if norm else 0.0), dtype)
    x2 = q(torch.randn(B, c2, H, W, generator=g), dtype) if c2 else None
    w = q(torch.randn(Co, Ci + c2, k, k, generator=g) / ((Ci + c2) * k * k) ** 0.5, dtype)
    b = q(torch.randn(Co, generator=g), dtype) if bias else None
    ra = q(torch.randn(B, Co, generator=g), dtype) if rowadd else None
    nrm = None
    xr = x
    if norm:
        gamma, beta = q(torch.randn(Ci, generator=g) * 0.3 + 1.0, dtype), q(torch.randn(Ci, generator=g) * 0.5, dtype)
        xr = q(F.silu(F.group_norm(x.double(), 32, gamma.double(), beta.double(), 1e-5)).float(), dtype)      # (tests/test_fused_norm_conv_gpu.py: the normalised tensor is rounded once)
    ref0 = _conv_ref(xr, x2, w, b, k, stride, pad, up_to, ra, None, alpha)
    rs = q(torch.randn(ref0.shape, generator=g), dtype) if residual else None
    ref = ref0 if rs is None else ref0 + rs
    wd, bd = pack_conv_weight(w, dtype, dev), (None if b is None else b.to(dtype).to(dev))
    wph = None
    if phases:
        from diffusion_e2e_ft_amd import autograd as ag
        conv = torch.nn.Conv2d(Ci, Co, 3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        conv = conv.float().to(dev)
        wph = lambda: ag.phase_conv_weight(conv, dtype)

    def run(fill):
        gs = Guards(dtype, dev, fill, ld_unit=ld_unit)
        xv = gs.flat(x.numel(), dtype=dtype, data=nhwc_cpu(x).reshape(-1)).view(B, H, W, Ci) if dense_x else gs.inp(nhwc_cpu(x), col0=Ci, cols_after=Ci)
        x2v = None if x2 is None else gs.inp(nhwc_cpu(x2))
        rv = None if rs is None else gs.inp(nhwc_cpu(rs))
        ov = gs.out(tuple(nhwc_cpu(ref).shape))
        if norm:
            nrm = (gamma.to(dtype).to(dev), beta.to(dtype).to(dev), 32, 1e-5, True)
        if splitk:
            d = ops._conv_desc(xv, x2v, Co, k, k, stride, pad, up_to, alpha, ldo=ov.stride(2))
            assert L.load().e2eft_conv2d_splitk_workspace_bytes(ctypes.byref(d)) > 0, "this shape is expected to be split"
        n0 = counter() if counter else 0
        y = ops.conv2d(xv, wd, bd, Co, k, k, stride, pad, x2=x2v, up_to=up_to, rowadd=None if ra is None else ra.to(dtype).to(dev), residual=rv, alpha=alpha, out=ov,
                       gn_stats=gn_stats, norm=nrm if norm else None, w_phase=wph)
        tag = ops._last_kernel()
        for part in ([kernel] if isinstance(kernel, str) else (kernel or [])):
            assert part in tag, "%s: expected %s, the launch was %s" % (what, kernel, tag)
        if counter:
            assert counter() - n0 >= 1, "%s: the kernel under test did not take the launch (%s)" % (what, tag)
        if norm:
            assert getattr(y, "_e2eft_keep", None) is not None, "%s: the fused-norm route was not taken" % what
        outs = dict(out=ov)
        if gn_stats:
            assert getattr(y, "_e2eft_gn", None) is not None, "%s: no statistics emitted" % what
            outs["partial"] = y._e2eft_gn.partial
        return outs, gs

    def check(name, t):
        if name == "out":
            assert_close(to_nchw(t), ref, dtype, what, scale=scale)

    return check_two_fills(run, check, what="%s %s" % (what, (B, Ci, c2, Co, H, W, k, stride)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_forward(ops, L, dev, dtype):
    c = lambda *a, **kw: _conv_case(ops, L, dev, dtype, *a, **kw)
    with L.option(L.OPT_F32_SPLIT, 0), L.option(L.OPT_PERSISTENT, 0):      # igemm2 for all three dtypes (the other kernels have their own tests below)
        _conv_forward_cases(c)


def _conv_forward_cases(c):
    c(2, 32, 48, 17, 13, kernel="igemm2_kernel", what="3x3")
    c(2, 24, 48, 17, 13, c2=40, rowadd=True, residual=True, alpha=0.7, kernel="igemm2_kernel", what="3x3 two sources")
    c(2, 32, 32, 16, 16, stride=2, pad=(0, 1, 0, 1), kernel="igemm2_kernel", what="stride 2 pads (0, 1, 0, 1)")
    c(2, 64, 96, 9, 11, k=1, pad=(0, 0, 0, 0), residual=True, kernel="igemm2_kernel", what="1x1")
    c(1, 64, 32, 6, 5, up_to=(12, 10), kernel="igemm2_kernel", what="fused nearest upsample")
    c(1, 32, 32, 8, 10, up_to=(15, 20), kernel="igemm2_kernel", what="fused nearest upsample to a forced size")
    c(2, 256, 128, 12, 12, rowadd=True, residual=True, alpha=0.5, splitk=True, scale=2, kernel="igemm2_kernel", what="split-K")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mfma", [0, 1])
def test_conv_narrow_output(ops, L, dev, dtype, mfma):
    """cout = 4 on csrc/narrow.hip (>= 16k pixels): the output a 4-channel slice — an 8-byte row in 16-bit — of a wider buffer"""
    with L.option(L.OPT_NARROW_MFMA, mfma):
        name = "conv3x3_narrow_mfma_kernel" if (mfma and dtype != torch.float32) else "conv3x3_narrow_kernel"
        _conv_case(ops, L, dev, dtype, 2, 32, 4, 100, 90, alpha=0.7, kernel=name, what="narrow")
        _conv_case(ops, L, dev, dtype, 1, 72, 1, 131, 127, kernel="conv3x3_narrow_kernel", what="narrow one channel")


@pytest.mark.parametrize("dtype", HALF)
def test_conv_fused_groupnorm(ops, L, dev, dtype):
    """conv2d(norm=...): the coefficient workspace of groupnorm_stats is poisoned; igemm6's NORM variant and narrow.hip's"""
    with L.option(L.OPT_PERSISTENT_GRID, 8):
        _conv_case(ops, L, dev, dtype, 2, 128, 128, 32, 64, norm=True, gn_stats=True, scale=2.0, kernel="igemm6_kernel", counter=L.load().e2eft_debug_patch_launches, what="fused norm")
        _conv_case(ops, L, dev, dtype, 17, 128, 64, 8, 32, norm=True, residual=True, bias=False, scale=2.0, kernel="igemm6_kernel", what="fused norm one tile per image")
        _conv_case(ops, L, dev, dtype, 1, 64, 4, 160, 128, norm=True, scale=2.0, kernel="conv3x3_narrow", what="fused norm conv_out")


@pytest.mark.parametrize("dtype", HALF)
def test_conv_persistent_kernels(ops, L, dev, dtype):
    """the smallest eligible cases of tests/test_persistent_gpu.py (igemm5), test_patch_conv_gpu.py / test_patch_conv_2x2_gpu.py (igemm6) and test_thin_conv_gpu.py
    (convin.hip) on an 8-workgroup grid"""
    lib = L.load()
    with L.option(L.OPT_PERSISTENT_GRID, 8), L.option(L.OPT_PERSISTENT_MIN_QROUNDS, 8):
        with L.option(L.OPT_PATCH_CONV, 0):
            _conv_case(ops, L, dev, dtype, 1, 128, 128, 64, 64, rowadd=True, residual=True, alpha=0.7, kernel="igemm5_kernel", counter=lib.e2eft_debug_persistent_launches, what="igemm5 3x3")
            _conv_case(ops, L, dev, dtype, 1, 256, 136, 64, 64, k=1, pad=(0, 0, 0, 0), rowadd=True, kernel="igemm5_kernel", counter=lib.e2eft_debug_persistent_launches,
                       what="igemm5 1x1 ragged N")
        _conv_case(ops, L, dev, dtype, 2, 128, 128, 32, 64, gn_stats=True, kernel="igemm6_kernel", counter=lib.e2eft_debug_patch_launches, what="igemm6")
        _conv_case(ops, L, dev, dtype, 17, 128, 128, 8, 32, rowadd=True, kernel="igemm6_kernel", counter=lib.e2eft_debug_patch_launches, what="igemm6 one tile per image")
        _conv_case(ops, L, dev, dtype, 1, 64, 320, 96, 96, c2=64, residual=True, kernel="igemm6_kernel", counter=lib.e2eft_debug_patch_launches, what="igemm6 two sources ragged N")
        _conv_case(ops, L, dev, dtype, 6, 128, 320, 8, 32, up_to=(16, 64), phases=True, kernel=", false, false, 2>", counter=lib.e2eft_debug_patch_launches, what="igemm6 2x2 phases")
        thin = dict(kernel="conv_thin_in_kernel", counter=lib.e2eft_debug_thin_launches, dense_x=True)
        _conv_case(ops, L, dev, dtype, 2, 8, 128, 32, 64, what="thin input", **thin)
        _conv_case(ops, L, dev, dtype, 17, 8, 128, 8, 32, what="thin input one tile per image", **thin)
        _conv_case(ops, L, dev, dtype, 3, 8, 136, 16, 96, bias=False, what="thin input ragged N", **thin)


def test_conv_f32split(ops, L, dev):
    """the fp32 split route (csrc/f32split.hip) on the halo-patch kernel and on igemm5, including the 1620-pixel case whose last 256-row tile is ragged"""
    dtype = torch.float32
    with L.option(L.OPT_PERSISTENT_GRID, 8), L.option(L.OPT_F32_SPLIT, 1):
        # (ld_unit 8: the persistent kernels' vector epilogue takes rows of whole 32 bytes, ldo % 8 and ldr % 8 in fp32 elements too)
        _conv_case(ops, L, dev, dtype, 1, 64, 128, 16, 64, gn_stats=True, kernel=["f32split", "igemm6"], ld_unit=8, what="f32split igemm6")
        _conv_case(ops, L, dev, dtype, 5, 128, 128, 18, 18, residual=True, kernel=["f32split", "igemm5"], ld_unit=8, what="f32split igemm5 1620 pixels")
        _conv_case(ops, L, dev, dtype, 2, 64, 192, 32, 64, stride=2, bias=False, kernel=["f32split", "igemm5"], ld_unit=8, what="f32split stride 2")


DGRAD_CASES = [dict(name="3x3", B=2, H=10, W=12, c1=16, co=24, k=3, s=1, p=1), dict(name="s2", B=2, H=12, W=10, c1=16, co=16, k=3, s=2, p=1),
               dict(name="conv_out", B=2, H=8, W=8, c1=32, co=4, k=3, s=1, p=1)]      # tests/test_bwd_gpu.py CONV_CASES: stride 1, stride 2, and one with pad channels in dY


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c["name"] for c in DGRAD_CASES])
def test_conv_dgrad(ops, dev, dtype, case):
    """e2eft_conv2d_dgrad: dY a guarded view whose pad channels (documented: "dy pad channels must be finite") hold finite random data, everything else the fill"""
    c = case
    g = _g(len(c["name"]) * 13 + c["c1"])
    B, H, W, ci, co, k, s, p = c["B"], c["H"], c["W"], c["c1"], c["co"], c["k"], c["s"], c["p"]
    e = 16 // dtype.itemsize
    cop = (co + e - 1) // e * e
    w = q(torch.randn(co, ci, k, k, generator=g) / math.sqrt(ci * k * k), dtype)
    ho, wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = q(torch.randn(B, cop, ho, wo, generator=g), dtype)           # channels [co, cop): the finite pad
    xr = torch.zeros(B, ci, H, W, dtype=torch.double, requires_grad=True)
    F.conv2d(xr, w.double(), None, s, p).backward(dy[:, :co].double())
    wpad = F.pad(w, (0, 0, 0, 0, 0, 0, 0, cop - co))                 # co padded with zeros
    wd = wpad.permute(1, 2, 3, 0).flip(1, 2).reshape(ci, k * k * cop).contiguous().to(dtype).to(dev)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        dyv = gs.inp(nhwc_cpu(dy))
        dx = ops.conv2d_dgrad(dyv, wd, (B, H, W, ci), 0, k, k, s, (p, p, p, p), None, 0.5)
        return dict(dx=dx), gs

    check_two_fills(run, lambda n, t: assert_close(to_nchw(t), 0.5 * xr.grad.float(), dtype, "dgrad", scale=2), what="dgrad %s" % c["name"])


# ================================================================================================ weight gradients
WGRAD_CASES = [(3, 13, 11, 320, 0, 128, 3), (2, 16, 16, 64, 64, 320, 1), (1, 72, 72, 64, 0, 64, 3)]
WGRAD_TOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2, torch.float32: 2e-5}      # tests/test_wgrad_gpu.py


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,c1,c2,Co,k", WGRAD_CASES)
@pytest.mark.parametrize("slot", ["none", "aligned", "off by 4 bytes"])
def test_conv_wgrad(ops, L, dev, dtype, B, H, W, c1, c2, Co, k, slot):
    g = _g(H * 7 + Co + k)
    x1 = torch.randn(B, c1, H, W, generator=g).to(dtype)
    x2 = torch.randn(B, c2, H, W, generator=g).to(dtype) if c2 else None
    pad = k // 2
    dy = (torch.randn(B, Co, H, W, generator=g) * 0.1).to(dtype)
    xin = x1.float() if x2 is None else torch.cat([x1, x2], dim=1).float()
    w = torch.zeros(Co, c1 + c2, k, k, requires_grad=True)
    F.conv2d(xin, w, None, stride=1, padding=pad).backward(dy.float())
    want = w.grad.permute(0, 2, 3, 1).reshape(Co, -1)
    n = want.numel()

    def run(fill):
        gs = Guards(dtype, dev, fill)
        dyv, xv = gs.inp(nhwc_cpu(dy)), gs.inp(nhwc_cpu(x1), col0=c1, cols_after=c1)
        x2v = None if x2 is None else gs.inp(nhwc_cpu(x2))
        out = None if slot == "none" else gs.flat(n, misalign=slot != "aligned")
        got = ops.conv2d_wgrad(dyv, xv, x2v, Co, k, k, 1, (pad, pad, pad, pad), 1.0, out=out)
        assert got is not None and got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape), "the direct kernel refused the case"
        assert out is None or got.data_ptr() == out.data_ptr()
        return dict(dw=got), gs

    def check(name, t):
        e = rel_err(t, want)
        assert e <= WGRAD_TOL[dtype], e

    for split in ((1, 0) if dtype == torch.float32 else (1,)):      # fp32: the f16 split-plane route and wgrad32_kernel
        with L.option(L.OPT_F32_SPLIT, split):
            check_two_fills(run, check, what="wgrad f32split=%d" % split)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slot", ["none", "aligned", "off by 4 bytes"])
def test_linear_wgrad_of_the_middle_qkv_slice(ops, L, dev, dtype, slot):
    """dY the middle slice of a q | k | v buffer whose other slices are the fill"""
    g = _g(3)
    M, N, K = 2 * 77 * 5, 128, 320
    x = torch.randn(M, K, generator=g).to(dtype)
    dy = (torch.randn(M, N, generator=g) * 0.1).to(dtype)
    want = 0.5 * (dy.double().t() @ x.double()).float()

    def run(fill):
        gs = Guards(dtype, dev, fill)
        dyv, xv = gs.inp(dy, col0=N, cols_after=N), gs.inp(x)
        out = None if slot == "none" else gs.flat(N * K, misalign=slot != "aligned")
        got = ops.linear_wgrad(dyv, xv, 0.5, out=out)
        assert got is not None and tuple(got.shape) == (N, K)
        assert out is None or got.data_ptr() == out.data_ptr()
        return dict(dw=got), gs

    def check(name, t):
        e = rel_err(t, want)
        assert e <= WGRAD_TOL[dtype], e

    for split in ((1, 0) if dtype == torch.float32 else (1,)):
        with L.option(L.OPT_F32_SPLIT, split):
            check_two_fills(run, check, what="linear wgrad f32split=%d" % split)


# ================================================================================================ norms, softmax, GEGLU
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,H,W,c2,silu", [(64, 9, 7, 0, True), (24, 9, 7, 40, True)])
def test_groupnorm(ops, dev, dtype, C, H, W, c2, silu):
    g = _g(C + H)
    B = 2
    x = q(torch.randn(B, C + c2, H, W, generator=g) * 2 + torch.randn(1, C + c2, 1, 1, generator=g), dtype)
    ga, be = q(1 + 0.3 * torch.randn(C + c2, generator=g), dtype), q(0.3 * torch.randn(C + c2, generator=g), dtype)
    ref = F.silu(F.group_norm(x.double(), 32, ga.double(), be.double(), 1e-5)).float()

    def run(fill):
        gs = Guards(dtype, dev, fill)
        xn = nhwc_cpu(x)
        xv = gs.inp(xn[..., :C])
        x2v = gs.inp(xn[..., C:]) if c2 else None
        ov = gs.out((B, H, W, C + c2))
        ops.groupnorm(xv, ga.to(dtype).to(dev), be.to(dtype).to(dev), 32, 1e-5, silu, x2=x2v, out=ov)
        return dict(out=ov), gs

    check_two_fills(run, lambda n, t: assert_close(to_nchw(t), ref, dtype, "groupnorm", scale=1.5), what="groupnorm")


@pytest.mark.parametrize("dtype", DTYPES)
def test_groupnorm_with_producer_statistics_from_a_guarded_conv(ops, dev, dtype):
    g = _g(16 * 3 + 128)
    B, H, W, Ci, Co = 3, 16, 16, 64, 128
    x = q(torch.randn(B, Ci, H, W, generator=g) + 0.5, dtype)
    w = q(torch.randn(Co, Ci, 3, 3, generator=g) / (Ci * 9) ** 0.5, dtype)
    b = q(torch.randn(Co, generator=g), dtype)
    res = q(torch.randn(B, Co, H, W, generator=g), dtype)
    ga, be = q(1 + 0.3 * torch.randn(Co, generator=g), dtype), q(0.3 * torch.randn(Co, generator=g), dtype)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        xv, rv, cv, yv = gs.inp(nhwc_cpu(x)), gs.inp(nhwc_cpu(res)), gs.out((B, H, W, Co)), gs.out((B, H, W, Co))
        conv_out = ops.conv2d(xv, pack_conv_weight(w, dtype, dev), b.to(dtype).to(dev), Co, 3, 3, 1, (1, 1, 1, 1), residual=rv, out=cv, gn_stats=True)
        assert getattr(conv_out, "_e2eft_gn", None) is not None, "statistics were not emitted"
        ops.groupnorm(conv_out, ga.to(dtype).to(dev), be.to(dtype).to(dev), 32, 1e-5, True, out=yv)
        return dict(conv=cv, gn=yv), gs

    got = check_two_fills(run, what="groupnorm on producer statistics")
    assert_close(to_nchw(got["conv"]), _conv_ref(x, None, w, b, 3, 1, (1, 1, 1, 1), None, None, res, 1.0), dtype, "conv")
    ref = F.silu(F.group_norm(to_nchw(got["conv"]).double(), 32, ga.double(), be.double(), 1e-5)).float()
    assert_close(to_nchw(got["gn"]), ref, dtype, "groupnorm on producer statistics", scale=1.5)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,W,c1,c2,silu", [(2, 9, 7, 64, 0, True), (2, 8, 8, 24, 40, True)])
def test_groupnorm_backward_with_dx_add(ops, dev, dtype, B, H, W, c1, c2, silu):
    g = _g(c1 + c2 + H)
    C = c1 + c2
    x = q(torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3, dtype)
    ga, be = q(1 + 0.2 * torch.randn(C, generator=g), dtype), q(0.2 * torch.randn(C, generator=g), dtype)
    dy, dadd = q(torch.randn(B, C, H, W, generator=g), dtype), q(torch.randn(B, C, H, W, generator=g), dtype)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, ga, be))
    F.silu(F.group_norm(xr, 32, gr, br, 1e-5)).backward(dy)
    ref = dict(dx=nhwc_cpu(xr.grad + dadd), dgamma=gr.grad, dbeta=br.grad)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        xn = nhwc_cpu(x)
        xv = gs.inp(xn[..., :c1])
        x2v = gs.inp(xn[..., c1:]) if c2 else None
        dyv, av = gs.inp(nhwc_cpu(dy)), gs.inp(nhwc_cpu(dadd))
        dg, db = gs.flat(C), gs.flat(C, misalign=True)
        gd, bd = ga.to(dtype).to(dev), be.to(dtype).to(dev)
        _, ws = ops.groupnorm_fwd_ws(xv, gd, bd, 32, 1e-5, silu=silu, x2=x2v)
        dx, dg2, db2 = ops.groupnorm_bwd(xv, x2v, gd, bd, 32, 1e-5, silu, dyv, ws, dx_add=av, dg_out=dg, db_out=db)
        return dict(dx=dx, dgamma=dg2, dbeta=db2), gs

    check_two_fills(run, _closer(ref, dtype, "groupnorm bwd", scale=dict(dx=3, dgamma=4, dbeta=4)), what="groupnorm bwd")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C", [(9, 640), (333, 320)])
def test_layernorm(ops, dev, dtype, rows, C):
    g = _g(rows)
    x = q(torch.randn(rows, C, generator=g) * 3 + 1, dtype)
    ga, be = q(1 + 0.3 * torch.randn(C, generator=g), dtype), q(0.3 * torch.randn(C, generator=g), dtype)
    ref = F.layer_norm(x.double(), (C,), ga.double(), be.double(), 1e-5).float()

    def run(fill):
        gs = Guards(dtype, dev, fill)
        xv, ov = gs.inp(x), gs.out((rows, C))
        ops.layernorm(xv, ga.to(dtype).to(dev), be.to(dtype).to(dev), 1e-5, out=ov)
        return dict(out=ov), gs

    check_two_fills(run, _closer(ref, dtype, "layernorm", scale=1.5), what="layernorm")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C", [(74, 320), (27, 1280)])
def test_layernorm_backward(ops, dev, dtype, rows, C):
    """74 x 320: the two-stage reduction of dgamma / dbeta (partial sums in the poisoned workspace); 27 x 1280: a single stage"""
    g = _g(C)
    x = q(torch.randn(rows, C, generator=g) * 2 + 0.5, dtype)
    ga, be = q(1 + 0.2 * torch.randn(C, generator=g), dtype), q(0.2 * torch.randn(C, generator=g), dtype)
    dy = q(torch.randn(rows, C, generator=g), dtype)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, ga, be))
    F.layer_norm(xr, (C,), gr, br, 1e-5).backward(dy)
    ref = dict(dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        xv, dyv = gs.inp(x), gs.inp(dy)
        gb = gs.flat(2 * C).view(2, C)
        dx, dg, db = ops.layernorm_bwd(xv, ga.to(dtype).to(dev), 1e-5, dyv, gb_out=gb)
        return dict(dx=dx, dgamma=dg, dbeta=db), gs

    check_two_fills(run, _closer(ref, dtype, "layernorm bwd", scale=dict(dx=3, dgamma=4, dbeta=4)), what="layernorm bwd")


@pytest.mark.parametrize("dtype", DTYPES)
def test_geglu_forward_and_backward_on_slices(ops, dev, dtype):
    g = _g(11)
    rows, C = 300, 256
    h = q(torch.randn(rows, 2 * C, generator=g) * 2, dtype)
    dy = q(torch.randn(rows, C, generator=g), dtype)
    hr = h.clone().requires_grad_(True)
    y = hr[:, :C] * F.gelu(hr[:, C:])
    y.backward(dy)
    ref = dict(out=y.detach(), dh=hr.grad)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        hv, dyv, ov = gs.inp(h), gs.inp(dy), gs.out((rows, C))
        ops.geglu(hv, out=ov)
        return dict(out=ov, dh=ops.geglu_bwd(hv, dyv)), gs

    check_two_fills(run, _closer(ref, dtype, "geglu", scale=dict(out=1, dh=2)), what="geglu")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,nq", [(1, 0), (77, 0), (4100, 0), (1, 1), (77, 77), (130, 130), (4100, 8)])
def test_softmax_rows_and_backward(ops, dev, dtype, n, nq):
    """in place on a dense [rows, npad] buffer inside a guarded flat allocation.  Only [:, :n] holds data: the pad columns [n, npad) of the scores, of p and of dp hold
    the FILL going in (a pad column read without a mask would show as NaN) and must come out as zeros (include/e2eft.h, e2eft_softmax_rows / _causal / _bwd_rows).
    nq > 0: the causal form, row r sees keys 0 .. r % nq.  (4100, 8): the causal mask on the several-sweeps path of long rows — nq bounds the visible keys, so the
    rows are mostly masked; (4100, 0) is the same path with every key live."""
    g = _g(n)
    e = 16 // dtype.itemsize
    npad = (n + e - 1) // e * e
    rows = 2 * nq if nq else 37
    s = q(torch.randn(rows, n, generator=g) * 4, dtype)
    dp = q(torch.randn(rows, n, generator=g), dtype)
    sc = s.double() * 0.125
    if nq:
        keep = torch.arange(n)[None, :] <= (torch.arange(rows) % nq)[:, None]
        sc = sc.masked_fill(~keep, float("-inf"))
    ref_p = torch.softmax(sc, dim=-1).float()

    def run(fill):
        gs = Guards(dtype, dev, fill)

        def padded(data):          # dense [rows, npad] in a guarded flat buffer: data in [:, :n], the fill in [n, npad)
            b = gs.flat(rows * npad, dtype=dtype).view(rows, npad)
            b[:, :n] = data.to(dtype).to(dev)
            return b

        buf = padded(s)
        ops.softmax_rows_(buf, n, 0.125, causal_nq=nq)
        pb, dbuf = padded(buf[:, :n]), padded(dp)
        ops.softmax_bwd_rows_(pb, dbuf, n, 0.125)
        return dict(p=buf[:, :n], pad=buf[:, n:], ds=dbuf[:, :n], ds_pad=dbuf[:, n:]), gs

    pq = q(ref_p, dtype).double()
    ref_ds = (pq * (dp.double() - (dp.double() * pq).sum(-1, keepdim=True)) * 0.125).float()

    def check(name, t):
        if name == "p":
            assert_close(t.float().cpu(), ref_p, dtype, "softmax")
        elif name.endswith("pad"):
            assert t.numel() == 0 or t.float().abs().max().item() == 0, "%s: columns [n, roundup) must be zero" % name
        else:
            assert_close(t.float().cpu(), ref_ds, dtype, "softmax bwd", scale=2)

    check_two_fills(run, check, what="softmax n=%d nq=%d" % (n, nq))


# ================================================================================================ attention
def _attn_ref(qq, kk, vv, heads, scale):
    sp = lambda t: t.reshape(t.shape[0], t.shape[1], heads, -1).transpose(1, 2).double()
    o = F.scaled_dot_product_attention(sp(qq), sp(kk), sp(vv), scale=scale)
    s = torch.einsum("bhqd,bhkd->bhqk", sp(qq), sp(kk)) * scale
    return o.transpose(1, 2).reshape(qq.shape).float(), (torch.logsumexp(s, dim=-1) / math.log(2.0)).float()


def _attention_case(ops, dev, dtype, N, Nk, expect=None, heads=3, B=2):
    g = _g(N + Nk)
    C = heads * 64
    qq, kk, vv = (q(torch.randn(B, n, C, generator=g), dtype) for n in (N, Nk, Nk))
    ref_o, ref_lse = _attn_ref(qq, kk, vv, heads, 64 ** -0.5)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        qv = gs.inp(qq, cols_after=C)                                         # [q | fill]
        kvv = gs.inp(torch.cat([kk, vv], dim=2), col0=C, cols_after=C)        # [fill | k | v | fill]
        ov = gs.out((B, N, C))
        _, lse = ops.attention(qv, kvv[..., :C], kvv[..., C:], heads, 64 ** -0.5, out=ov, return_lse=True)
        if expect:
            assert expect in ops._last_kernel(), (expect, ops._last_kernel())
        return dict(out=ov, lse=lse), gs

    def check(name, t):
        assert_close(t.float().cpu(), ref_o if name == "out" else ref_lse, dtype, "attention " + name, scale=1.5)

    check_two_fills(run, check, what="attention %s" % ((N, Nk),))


ATTN_SHAPES = [(130, 64), (200, 1), (128, 129)]


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("dma", [0, 1])
@pytest.mark.parametrize("N,Nk", ATTN_SHAPES)
def test_attention(ops, L, dev, dtype, dma, N, Nk):
    with L.option(L.OPT_ATTN_DMA, dma):
        _attention_case(ops, dev, dtype, N, Nk)


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("N,Nk", ATTN_SHAPES)
def test_attention_fp32(ops, L, dev, split, N, Nk):
    with L.option(L.OPT_F32_SPLIT_ATTN, split):
        _attention_case(ops, dev, torch.float32, N, Nk, expect="attn_f32split_fwd_kernel" if split else "attn32_fwd_kernel")


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_joint_segments(ops, dev, dtype):
    """kv_nseg = 2, kv_bmod = B / 2 (tests/test_ops_gpu.py::test_attention_joint): both halves attend to both halves' keys"""
    g = _g(33)
    Bh, heads, N = 2, 2, 144
    C = heads * 64
    qq, kk, vv = (q(torch.randn(2 * Bh, N, C, generator=g), dtype) for _ in range(3))
    kj = torch.cat([torch.cat([kk[:Bh], kk[Bh:]], dim=1)] * 2, dim=0)
    vj = torch.cat([torch.cat([vv[:Bh], vv[Bh:]], dim=1)] * 2, dim=0)
    ref, _ = _attn_ref(qq, kj, vj, heads, 64 ** -0.5)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        qkv = gs.inp(torch.cat([qq, kk, vv], dim=2), cols_after=C)       # [q | k | v | fill]
        ov = gs.out((2 * Bh, N, C))
        ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, 64 ** -0.5, kv_nseg=2, kv_bmod=Bh, out=ov)
        return dict(out=ov), gs

    check_two_fills(run, _closer(ref, dtype, "joint attention", scale=1.5), what="joint attention")


@pytest.mark.parametrize("dtype", HALF)
@pytest.mark.parametrize("split_tail", [True, False])
def test_attention512(ops, dev, dtype, split_tail):
    """N = 144 with and without the split-tail workspace (poisoned)"""
    g = _g(144 * 8)
    B, N = 2, 144
    qq, kk, vv = (torch.randn(B, N, 512, generator=g).to(dtype).float() for _ in range(3))
    ref, _ = _attn_ref(qq, kk, vv, 1, 512 ** -0.5)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        qkv = gs.inp(torch.cat([qq, kk, vv], dim=2), cols_after=512)
        ov = gs.out((B, N, 512))
        ops.attention512(qkv[..., :512], qkv[..., 512:1024], qkv[..., 1024:], 512 ** -0.5, out=ov)
        return dict(out=ov), gs

    saved, ops.ATTN512_SPLIT_TAIL = ops.ATTN512_SPLIT_TAIL, split_tail
    try:
        check_two_fills(run, _closer(ref, dtype, "attention512"), what="attention512")
    finally:
        ops.ATTN512_SPLIT_TAIL = saved


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,Nk", [(100, 100), (129, 257)])
def test_attention_backward_into_slices_of_one_buffer(ops, dev, dtype, N, Nk):
    g = _g(N + Nk)
    B, heads = 2, 2
    C = heads * 64
    qq, kk, vv = (q(torch.randn(B, n, C, generator=g), dtype) for n in (N, Nk, Nk))
    do = q(torch.randn(B, N, C, generator=g), dtype)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (qq, kk, vv))
    sp = lambda t: t.view(B, -1, heads, 64).transpose(1, 2)
    (torch.softmax(sp(qr) @ sp(kr).transpose(-1, -2) * 0.125, -1) @ sp(vr)).transpose(1, 2).reshape(B, N, C).backward(do)
    ref = dict(dq=qr.grad, dk=kr.grad, dv=vr.grad)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        qv, kvv, dov = gs.inp(qq), gs.inp(torch.cat([kk, vv], dim=2), cols_after=C), gs.inp(do)
        ov = gs.out((B, N, C))
        _, lse = ops.attention(qv, kvv[..., :C], kvv[..., C:], heads, 0.125, out=ov, return_lse=True)
        if N == Nk:
            all3 = gs.out((B, N, 3 * C), cols_after=C)     # [dq | dk | dv | fill]: one guarded buffer
            dqv, dkv = all3[..., :C], all3[..., C:]
        else:
            dqv, dkv = gs.out((B, N, C)), gs.out((B, Nk, 2 * C), cols_after=C)         # [dq | fill], [dk | dv | fill]
        ops.attention_bwd(qv, kvv[..., :C], kvv[..., C:], ov, dov, lse, heads, 0.125, dqv, dkv[..., :C], dkv[..., C:])
        return dict(dq=dqv, dk=dkv[..., :C], dv=dkv[..., C:]), gs

    check_two_fills(run, _closer(ref, dtype, "attention bwd", scale=3), what="attention bwd %s" % ((N, Nk),))


# ================================================================================================ layout, elementwise, optimizer
@pytest.mark.parametrize("dtype", DTYPES)
def test_transpose_and_im2col_t(ops, dev, dtype):
    g = _g(77 + 128)
    Z, R, C = 3, 77, 72
    x = torch.randn(Z, R, C, generator=g).to(dtype)
    rp = 128

    def run(fill):
        gs = Guards(dtype, dev, fill)
        xv = gs.inp(x)
        ov = gs.flat(Z * C * rp, dtype=dtype).view(Z, C, rp)
        ops.transpose(xv, rows_pad=rp, out=ov)
        return dict(t=ov), gs

    def check(name, t):
        assert torch.equal(t[:, :, :R].cpu(), x.transpose(1, 2)) and t[:, :, R:].float().abs().max().item() == 0      # zeros in [rows, rows_pad)

    check_two_fills(run, check, what="transpose")
    B, H, W, c1, c2 = 1, 12, 10, 8, 24
    xi = torch.randn(B, c1 + c2, H, W, generator=g).to(dtype)
    u = F.unfold(F.pad(xi.float(), (1, 1, 1, 1)), (3, 3))
    refc = u.view(B, c1 + c2, 9, -1).permute(2, 1, 0, 3).reshape(9 * (c1 + c2), -1)

    def run2(fill):
        gs = Guards(dtype, dev, fill)
        xn = nhwc_cpu(xi)
        x1v, x2v = gs.inp(xn[..., :c1]), gs.inp(xn[..., c1:])
        col, P, Pp = ops.im2col_t(x1v, x2v, 3, 3, 1, (1, 1, 1, 1))
        assert P == B * H * W and Pp > P
        return dict(col=col), gs

    def check2(name, t):
        P = B * H * W
        assert torch.equal(t[:, :P].float().cpu(), refc) and t[:, P:].float().abs().max().item() == 0                   # zeros in [P, ldcol)

    check_two_fills(run2, check2, what="im2col_t")


@pytest.mark.parametrize("dtype", DTYPES)
def test_colsum_upsample_bwd_copy_add(ops, dev, dtype):
    g = _g(4)
    x = q(torch.randn(6 * 50, 72, generator=g), dtype)
    dyu = q(torch.randn(2, 16, 9, 11, generator=g), dtype)
    xin = torch.zeros(2, 16, 5, 6, requires_grad=True)
    F.interpolate(xin, size=(9, 11), mode="nearest").backward(dyu)
    a, b = q(torch.randn(2, 5, 6, 16, generator=g), dtype), q(torch.randn(2, 5, 6, 16, generator=g), dtype)
    a4 = q(torch.randn(2, 5, 6, 4, generator=g), dtype)
    ref = dict(colsum=0.5 * x.view(6, 50, 72).sum(1), colsum_view=x[:, 8:24].sum(0, keepdim=True), up=nhwc_cpu(xin.grad), copy=a * 0.18215, copy4=a4 * -0.99766725, add=a + b)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        xv, dyv, av, bv, a4v = gs.inp(x), gs.inp(nhwc_cpu(dyu)), gs.inp(a), gs.inp(b), gs.inp(a4)
        cs = gs.flat(6 * 72, misalign=True).view(6, 72)
        co, c4, ad = gs.out(a.shape), gs.out(a4.shape), gs.out(a.shape)
        ops.colsum(xv, groups=6, alpha=0.5, out=cs)
        ops.copy_scale(av, co, mul=0.18215)
        ops.copy_scale(a4v, c4, mul=-0.99766725)
        ops.add(av, bv, out=ad)
        return dict(colsum=cs, colsum_view=ops.colsum(xv[:, 8:24], groups=1), up=ops.upsample_nearest_bwd(dyv, 5, 6), copy=co, copy4=c4, add=ad), gs

    def check(name, t):
        assert_close(t.float().cpu(), ref[name].float(), torch.float32 if name.startswith("colsum") else dtype, name, scale=10 if name.startswith("colsum") else 1)

    check_two_fills(run, check, what="colsum / upsample_bwd / copy_scale / add")


@pytest.mark.parametrize("dtype", DTYPES)
def test_heads_and_layout(ops, dev, dtype):
    """nchw_to_nhwc writes zeros in [c, cpad); the head backward kernels write cpad >= 3 channels, zeros beyond 3 (include/e2eft.h): their buffers are poisoned"""
    g = _g(51)
    x = q(torch.randn(2, 3, 9, 11, generator=g) * 0.8, dtype)
    dy1, dy3 = torch.randn(2, 1, 9, 11, generator=g), torch.randn(2, 3, 9, 11, generator=g)
    xr = x.clone().requires_grad_(True)
    torch.clamp(xr.mean(dim=1, keepdim=True), -1, 1).backward(q(dy1, dtype))
    ref_d = xr.grad.clone()
    xr = x.clone().requires_grad_(True)
    torch.clamp(xr / (torch.norm(xr, p=2, dim=1, keepdim=True) + 1e-5), -1, 1).backward(q(dy3, dtype))
    ref = dict(nhwc=x * 2 - 0.5, depth=(torch.clip(x.mean(dim=1, keepdim=True), -1, 1) + 1) / 2,
               normal=-torch.clamp(x / (torch.norm(x, p=2, dim=1, keepdim=True) + 1e-5), -1, 1), back=x, ddepth=ref_d, dnormal=xr.grad)

    def run(fill):
        gs = Guards(dtype, dev, fill)
        y = ops.nchw_to_nhwc(x.to(dev), dtype=dtype, mul=2.0, add=-0.5)
        xv = gs.inp(nhwc_cpu(x))                                             # a 3-channel view, pixel stride ld
        dd = ops.depth_head_bwd(xv, dy1.to(dtype).to(dev), False)
        dn = ops.normal_head_bwd(xv, dy3.to(dtype).to(dev), True, 1.0)
        full = lambda t: t.as_strided((2, 9, 11, t.stride(2)), t.stride(), t.storage_offset())
        return dict(nhwc=y[..., :3], nhwc_pad=y[..., 3:], depth=ops.depth_head(xv, to_unit=True, dtype=torch.float32), normal=ops.normal_head(xv, clamp=True, sign=-1.0, dtype=torch.float32),
                    back=ops.nhwc_to_nchw(xv, dtype=torch.float32), ddepth=dd, ddepth_pad=full(dd)[..., 3:], dnormal=dn, dnormal_pad=full(dn)[..., 3:]), gs

    def check(name, t):
        if name.endswith("_pad"):
            assert t.numel() > 0 and t.float().abs().max().item() == 0, "%s: the channels up to cpad must be zero" % name
        elif name in ("nhwc", "ddepth", "dnormal"):
            assert_close(to_nchw(t), ref[name], dtype, name, scale=dict(nhwc=1, ddepth=2, dnormal=3)[name])
        else:
            assert_close(t.float().cpu(), ref[name], torch.float32, name, scale=4 if name != "back" else 1)

    check_two_fills(run, check, what="heads / layout")


@pytest.mark.parametrize("tail", [1, 2, 3])
def test_flat_optimizer_kernels_on_the_interior_of_a_guarded_buffer(ops, dev, tail):
    """ema_step_, adamw_step_, cast_ and sumsq on n = 4 k + tail elements: a float4 body must not spill over the end.  adamw_step_, cast_ and sumsq take any fp32
    pointer and also run one element off the 16-byte boundary; e2eft_ema_step asks for 16-byte aligned buffers and gets them"""
    g = _g(8 + tail)
    n = 10004 + tail
    p0, gr, sh = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.01, torch.randn(n, generator=g)
    refp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([refp], lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    refp.grad = gr.clone()
    torch.nn.utils.clip_grad_norm_([refp], 1.0)
    opt.step()
    ss_ref = float((gr.double() ** 2).sum())
    ref = dict(p=refp.detach(), ema=sh - 0.1 * (sh - p0), cast=gr.to(torch.bfloat16).float(), acc=1 + 2 * gr)

    for mis in (False, True):
        def run(fill):
            gs = Guards(torch.float32, dev, fill)
            p, gd, m, v = gs.flat(n, misalign=mis, data=p0), gs.flat(n, misalign=mis, data=gr), gs.flat(n, misalign=mis, data=torch.zeros(n)), gs.flat(n, misalign=mis, data=torch.zeros(n))
            shv, pv = gs.flat(n, data=sh), gs.flat(n, data=p0)
            ops.ema_step_(shv, pv, 0.1)
            ss = ops.sumsq(gd)
            ops.adamw_step_(p, gd, m, v, 3e-3, 0.9, 0.999, 1e-8, 1e-2, 1, grad_sumsq=ss, grad_scale=1.0, max_norm=1.0)
            y = gs.flat(n, dtype=torch.bfloat16, misalign=mis)
            ops.cast_(gd, y)
            acc = gs.flat(n, misalign=mis, data=torch.ones(n))
            ops.cast_(gd, acc, mul=2.0, accumulate=True)
            return dict(p=p, ema=shv, sumsq=ss, cast=y, acc=acc), gs

        def check(name, t):
            if name == "sumsq":
                assert abs(t.item() - ss_ref) < 1e-6 * ss_ref
            elif name == "cast":
                assert torch.equal(t.float().cpu(), ref[name])
            else:
                assert rel_err(t, ref[name]) < 2e-6, (name, rel_err(t, ref[name]))

        check_two_fills(run, check, what="flat optimizer kernels misaligned=%s" % mis)


# ================================================================================================ entries that allocate their dense outputs themselves: poison only
def test_losses_forward_and_backward_poisoned(ops, dev):
    from oracle.losses_ref import angular_loss_ref, ssi_loss_ref
    g = _g(61)
    B, H, W = 3, 40, 56
    tgt = torch.rand(B, 1, H, W, generator=g) * 2 - 1
    pred = 0.6 * tgt + 0.2 + 0.05 * torch.randn(B, 1, H, W, generator=g)
    mask = torch.rand(B, 1, H, W, generator=g) > 0.05
    mask[2] = False
    nrm = F.normalize(torch.randn(B, 3, H, W, generator=g), dim=1)
    nt = F.normalize(nrm + 0.3 * torch.randn(B, 3, H, W, generator=g), dim=1)
    pr, nr = pred.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
    ref_s, ref_a = ssi_loss_ref(pr, tgt, mask), angular_loss_ref(nr, nt, mask)
    (3.0 * ref_s).backward()
    ref_a.backward()

    def run(fill):
        p, t, m = pred.to(dev).view(B, -1), tgt.to(dev).view(B, -1), mask.to(dev).view(B, -1).to(torch.uint8)
        loss, ss, ws = ops.ssi_loss_fwd_saved(p, t, m)
        dp = ops.ssi_loss_bwd(p, t, m, ss, ws, torch.full((1,), 3.0, device=dev))
        n_, nt_ = nrm.to(dev).view(B, 3, -1), nt.to(dev).view(B, 3, -1)
        la, wsa = ops.angular_loss_fwd_saved(n_, nt_, m)
        dn = ops.angular_loss_bwd(n_, nt_, m, wsa, torch.ones(1, device=dev))
        return dict(ssi=loss, ssi_dpred=dp, angular=la, angular_dpred=dn, ssi_public=ops.ssi_loss(pred.to(dev), tgt.to(dev), mask.to(dev)).reshape(1),
                    angular_public=ops.angular_loss(nrm.to(dev), nt.to(dev), mask.to(dev)).reshape(1)), []

    def check(name, t):      # tests/test_ops_gpu.py::test_losses, tests/test_bwd_gpu.py::test_loss_gradients_match_reference_fixture
        if name.startswith("ssi") and not name.endswith("dpred"):
            assert abs(t.item() - ref_s.item()) <= 2e-5 * max(1.0, abs(ref_s.item())), (name, t.item(), ref_s.item())
        elif name.startswith("angular") and not name.endswith("dpred"):
            assert abs(t.item() - ref_a.item()) <= 2e-5, (name, t.item(), ref_a.item())
        elif name == "ssi_dpred":
            assert rel_err(t.view(B, 1, H, W), pr.grad) < 2e-4
        else:
            assert rel_err(t.view(B, 3, H, W), nr.grad) < 2e-4

    check_two_fills(run, check, what="losses")


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_attention_through_the_score_buffer_poisoned(dev, dtype):
    """autograd.attention with the GEMM + softmax backward (FLASH_BACKWARD off): the [B, heads, N, nkp] score / probability buffers with their pad columns are poisoned"""
    from diffusion_e2e_ft_amd import autograd as ag
    g = _g(100 + 77)
    B, N, Lk, heads = 2, 100, 77, 2
    C = heads * 64
    qq, kv, do = q(torch.randn(B, N, C, generator=g), dtype), q(torch.randn(B, Lk, 2 * C, generator=g), dtype), q(torch.randn(B, N, C, generator=g), dtype)
    qr, kr = qq.clone().requires_grad_(True), kv.clone().requires_grad_(True)
    sp = lambda t: t.view(B, -1, heads, 64).transpose(1, 2)
    o = (torch.softmax(sp(qr) @ sp(kr[..., :C]).transpose(-1, -2) * 0.125, -1) @ sp(kr[..., C:])).transpose(1, 2).reshape(B, N, C)
    o.backward(do)
    ref = dict(out=o.detach(), dq=qr.grad, dkv=kr.grad)

    def run(fill):
        qd, kd = qq.to(dtype).to(dev).requires_grad_(True), kv.to(dtype).to(dev).requires_grad_(True)
        out = ag.attention(qd, kd, heads, 0.125)
        out.backward(do.to(dtype).to(dev))
        return dict(out=out.detach(), dq=qd.grad, dkv=kd.grad), []

    saved, ag.FLASH_BACKWARD = ag.FLASH_BACKWARD, False
    try:
        check_two_fills(run, _closer(ref, dtype, "autograd attention", scale=dict(out=1.5, dq=3, dkv=3)), what="autograd attention (GEMM + softmax backward)")
    finally:
        ag.FLASH_BACKWARD = saved


def test_resize_and_minmax_poisoned(ops, dev):
    """pipeline.resize_device (the `mid` image of the two-pass resamplers is a poisoned torch.empty) at the smallest cases of tests/test_prepost_gpu.py; ops.minmax_unit"""
    from diffusion_e2e_ft_amd.pipeline import resize_device
    g = _g(37 + 200)
    img = torch.randint(0, 256, (3, 37, 53), generator=g, dtype=torch.uint8)
    f = torch.rand(3, 61, 45, generator=g)
    x = torch.randn(70, 90, generator=g) * 3 + 5
    want = F.interpolate(img[None].float(), size=(11, 200), mode="bilinear", antialias=True, align_corners=False)[0]
    want_c = F.interpolate(f[None], size=(224, 224), mode="bicubic", antialias=True, align_corners=False)[0]
    iy = torch.tensor([min(int(i * (1.0 / (224 / 61))), 60) for i in range(224)])
    ix = torch.tensor([min(int(i * (1.0 / (224 / 45))), 44) for i in range(224)])

    def run(fill):
        return dict(bilinear=resize_device(img.to(dev), (11, 200)), bicubic=resize_device(f.to(dev), (224, 224), kind="bicubic"),
                    nearest=resize_device(f.to(dev), (224, 224), kind="nearest"), minmax=ops.minmax_unit(x.to(dev))), []

    def check(name, t):
        t = t.cpu()
        if name == "bilinear":
            assert (t - want).abs().max().item() <= 2e-4
        elif name == "bicubic":
            assert (t - want_c).abs().max().item() <= 4e-6
        elif name == "nearest":
            assert torch.equal(t, f[:, iy][:, :, ix])
        else:
            assert torch.equal(t, (x - x.min()) / (x.max() - x.min()))

    check_two_fills(run, check, what="resize / minmax")


def test_sample_preparation_and_augmentation_poisoned(ops, dev):
    """csrc/dataprep.hip (histogram workspaces) and csrc/dataaug.hip at the smallest cases of tests/test_data_gpu.py"""
    import numpy as np
    from PIL import Image
    from oracle import dataprep_ref
    from diffusion_e2e_ft_amd.data import NEAR_FAR, augment_hypersim, augment_vkitti, prepare_batch
    from test_data_gpu import _decoded_batch, _depth
    near, far = 1e-5, 65.0
    d = torch.stack([_depth(100, 1000 + i, k) for i, k in enumerate(["smooth", "ties", "wide"])])
    H, W, B = 6, 8, 4
    g = _g(H)
    rgb, nrm = torch.rand(B, 3, H, W, generator=g), torch.rand(B, 3, H, W, generator=g)
    depth = torch.stack([_depth(H * W, 7 + i, k).view(1, H, W) for i, k in enumerate(["smooth", "ties", "wide", "smooth"])])
    depth[3] = 3.0
    r8, d8, n8 = _decoded_batch(3, 77, 101, 5)
    flips = [True, False, True]
    rk, dk, nk = _decoded_batch(2, 375, 1242, 7)

    def run(fill):
        out = prepare_batch(rgb.to(dev), depth.to(dev), nrm.to(dev), "hypersim")
        r01, dd, n01 = augment_hypersim(torch.from_numpy(r8).to(dev), torch.from_numpy(d8).to(dev), torch.from_numpy(n8).to(dev), size=(48, 64), flip=flips)
        k01, kd, kn = augment_vkitti(torch.from_numpy(rk).to(dev), torch.from_numpy(dk).to(dev), torch.from_numpy(nk).to(dev), flip=[False, True])
        outs = dict(quantiles=ops.masked_quantiles(d.to(dev), near, far), aug_rgb=r01, aug_depth=dd, aug_normals=n01, kitti_rgb=k01, kitti_depth=kd, kitti_normals=kn)
        outs.update({"batch_" + k: out[k] for k in ("rgb", "val_mask", "metric", "depth", "normals")})
        return outs, []

    def check(name, t):
        t = t.cpu()
        if name == "quantiles":
            for b in range(3):
                valid = d[b][(d[b] > near) & (d[b] < far)]
                lo, hi = torch.quantile(valid, 0.02), torch.quantile(valid, 0.98)
                assert int(t[b, 2]) == valid.numel() and abs(float(t[b, 0]) - float(lo)) <= 1e-6 * max(1.0, abs(float(lo))) and abs(float(t[b, 1]) - float(hi)) <= 1e-6 * max(1.0, abs(float(hi)))
        elif name.startswith("batch_"):
            k = name[6:]
            for b in range(B):
                ref = dataprep_ref.prepare_sample_ref(rgb[b], depth[b], nrm[b], *NEAR_FAR["hypersim"])[k]
                if k in ("rgb", "val_mask"):
                    assert torch.equal(t[b], ref)
                else:
                    assert torch.allclose(t[b], ref, rtol=1e-6 if k == "metric" else 0, atol=dict(metric=1e-6, depth=4e-6, normals=1e-6)[k])
        elif name.startswith("aug_"):
            want = []
            for b in range(3):
                src = dict(aug_rgb=r8, aug_depth=d8, aug_normals=n8)[name][b]
                im = Image.fromarray(src, mode="F") if name == "aug_depth" else Image.fromarray(src)
                if flips[b]:
                    im = im.transpose(Image.FLIP_LEFT_RIGHT)
                    if name == "aug_normals":
                        a = np.array(im)
                        a[:, :, 0] = 255 - a[:, :, 0]
                        im = Image.fromarray(a)
                if name == "aug_depth":
                    want.append(np.asarray(im.resize((64, 48), resample=Image.NEAREST))[None])
                else:
                    want.append(np.asarray(im.resize((64, 48), resample=Image.BILINEAR)).astype(np.float32).transpose(2, 0, 1) / 255.0)
            assert np.array_equal(t.numpy(), np.stack(want))
        else:
            top, left = 375 - 352, int((1242 - 1216) / 2)
            for b, flip in enumerate([False, True]):
                src = dict(kitti_rgb=rk, kitti_depth=dk, kitti_normals=nk)[name][b]
                if flip:
                    src = src[:, ::-1].copy()
                    if name == "kitti_normals":
                        src[:, :, 0] = 255 - src[:, :, 0]
                src = src[top:top + 352, left:left + 1216]
                assert np.array_equal(t[b].numpy(), src[None] if name == "kitti_depth" else src.astype(np.float32).transpose(2, 0, 1) / 255.0)

    check_two_fills(run, check, what="dataprep / dataaug")


def test_ensemble_kernels_poisoned(ops, dev):
    """csrc/ensemble.hip at the smallest cases of tests/test_ensemble_gpu.py: fixed-order reductions, bit-equal between the fills"""
    import golden_cases as gc
    from oracle import ensemble_ref
    x = gc.ensemble_depth_stack(n=2, H=7, W=5, seed=52)
    x3 = gc.ensemble_depth_stack(n=3, H=37, W=53, seed=63)
    g = _g(3)
    s, t0 = torch.rand(3, generator=g) + 0.5, torch.randn(3, generator=g) * 0.3
    al = x3 * s.view(-1, 1, 1) + t0.view(-1, 1, 1)
    med = al.median(0).values
    mad = (al - med).abs().median(0).values
    xn = gc.ensemble_normal_stack(n=3, H=17, W=29, seed=39)
    unit_ref, err_ref = ensemble_ref.normals_error_sums_ref(xn)

    def run(fill):
        gram, sums = ops.ensemble_gram(x.to(dev))
        pred, unc, mm = ops.ensemble_depth_reduce(x3.to(dev), s.to(dev), t0.to(dev), use_mean=False)
        pm, um, _ = ops.ensemble_depth_reduce(x3.to(dev), s.to(dev), t0.to(dev), use_mean=True)
        unit, err = ops.ensemble_normals(xn.to(dev))
        fin_p, fin_u = pred.clone(), unc.clone()
        ops.ensemble_depth_finish_(fin_p, fin_u, mm)
        return dict(minmax=ops.ensemble_minmax(x.to(dev)), gram=gram, sums=sums, median=pred, mad=unc, mm=mm, mean=pm, std=um, unit=unit, err=err, fin_p=fin_p, fin_u=fin_u), []

    def check(name, t):
        t = t.cpu()
        flat = x.reshape(2, -1)
        rng = med.max() - med.min()
        if name == "minmax":
            assert torch.equal(t[:, 0], flat.min(1).values) and torch.equal(t[:, 1], flat.max(1).values)
        elif name == "gram":
            assert torch.allclose(t, flat.double() @ flat.double().T, rtol=1e-12, atol=0)
        elif name == "sums":
            assert torch.allclose(t, flat.double().sum(1), rtol=1e-12, atol=1e-12)
        elif name in ("median", "mad", "fin_p", "fin_u"):
            assert torch.equal(t, dict(median=med, mad=mad, fin_p=(med - med.min()) / rng, fin_u=mad / rng)[name])
        elif name == "mm":
            assert float(t[0]) == float(med.min()) and float(t[1]) == float(med.max())
        elif name == "mean":
            assert torch.allclose(t, al.mean(0), rtol=1e-6, atol=1e-6)
        elif name == "std":
            assert torch.allclose(t, al.std(0), rtol=1e-4, atol=1e-6)
        elif name == "unit":
            assert torch.allclose(t, unit_ref, rtol=0, atol=2e-6)
        else:
            assert torch.allclose(t, err_ref, rtol=1e-5)

    check_two_fills(run, check, what="ensemble")


@pytest.mark.parametrize("shape", [(2, 2), (33, 130)])
def test_depth_to_normals_poisoned(ops, dev, shape):
    """csrc/d2nt.hip at the minimal and the ragged case of tests/test_d2nt_gpu.py::test_ragged_and_minimal_sizes (exact against the restatement)"""
    import numpy as np
    import d2nt_ref
    rng = np.random.default_rng(shape[0] * 10007 + shape[1])
    dm = d2nt_ref.cm_to_metres(d2nt_ref.vkitti_like_depth_cm(rng, *shape))
    ref = {r: d2nt_ref.depth_to_normals(dm, d2nt_ref.VKITTI_K, r, power=d2nt_ref.correctly_rounded_power) for r in (False, True)}

    def run(fill):
        d = torch.from_numpy(np.ascontiguousarray(dm)).to(dev)
        k = torch.tensor(np.asarray(d2nt_ref.VKITTI_K, dtype=np.float32), device=dev)
        return {"%s %d" % (f, r): ops.depth_to_normals(d, k, refine=r, out_format=f, depth_scale=100.0) for r in (False, True) for f in ("f32", "u16", "u8")}, []

    def check(name, t):
        f, r = name.split()
        want = ref[bool(int(r))]
        assert np.array_equal(t.cpu().numpy(), want["normal"].astype(np.float32) if f == "f32" else want[f]), name

    check_two_fills(run, check, what="depth_to_normals %s" % (shape,))


@pytest.mark.parametrize("kind", ["u16", "i32"])
def test_depth_gt_prepare_poisoned(dev, kind):
    """csrc/evalprep.hip at the ragged 17 x 33 case of tests/test_depth_benchmark_gpu.py::test_kernel_on_ragged_shapes, checked by that file's own comparison with the
    restatement (bit-exact depth, mask and valid-pixel count: the count is an integer atomicAdd into a buffer the wrapper allocates)"""
    import numpy as np
    from test_depth_benchmark_gpu import _check, _raster
    shape = (17, 33)
    rng = np.random.default_rng(shape[0] * 131 + shape[1])
    raw = _raster(rng, kind, shape)
    ext = rng.integers(0, 3, (2,) + shape).astype(np.uint8)
    res = {}
    for fill in FILLS:
        with poisoned_allocations(fill):
            res[fill] = (_check(raw, dev, (kind, "plain", fill), divisor=1000.0, min_depth=1e-3, max_depth=10.0)
                         + _check(raw[None].repeat(2, 0), dev, (kind, "ext", fill), divisor=1000.0, min_depth=0.6, max_depth=350.0, ext_mask=ext)
                         + _check(raw, dev, (kind, "crop", fill), divisor=256.0, min_depth=1e-5, max_depth=80.0, crop=(1, 1, shape[0] - 2, shape[1] - 2), window=(0, 1, 1, 2)))
    for a, b in zip(res[FILLS[0]], res[FILLS[1]]):
        assert (a is None and b is None) or (np.isfinite(a).all() and np.array_equal(a, b))


def test_normal_gt_prepare_and_dsine_requantize_poisoned(ops, dev):
    """csrc/normalprep.hip against the reference's recordings (tests/test_normal_benchmark_gpu.py, first dataset): bit-exact normals, mask, valid-pixel count (an integer
    atomicAdd into a buffer the wrapper allocates) and requantized image, under both fills"""
    import normal_benchmark_fixture as nfx
    from test_normal_benchmark_gpu import GOLD, _raw_normal, _same_bits
    name = nfx.NAMES[0]
    rec = GOLD["datasets"][name]["samples"][0]

    def run(fill):
        normal, mask, nv = ops.normal_gt_prepare(torch.from_numpy(_raw_normal(name, 0)).to(dev))
        outs = dict(normal=normal, mask=mask.view(torch.uint8), count=nv.reshape(1))
        for layout in ("hwc", "chw"):
            outs["img_" + layout] = ops.dsine_rgb_requantize(torch.from_numpy(nfx.image(name, 0)).to(dev), layout=layout)
        return outs, []

    def check(name_, t):
        if name_ == "count":
            assert int(t) == int(rec["normal_mask"].sum())
        else:
            want = dict(normal=rec["normal"], mask=rec["normal_mask"], img_chw=rec["img_u8"], img_hwc=rec["img_u8"].permute(1, 2, 0).contiguous())[name_]
            assert _same_bits(t, want), name_

    check_two_fills(run, check, what="normal_gt_prepare / dsine_rgb_requantize")


def test_depth_eval_poisoned(dev):
    """ops.depth_eval through evaluate.depth_metrics at the first case of tests/test_eval_gpu.py (tests/golden/eval_golden.pt: the reference's functions), every
    alignment setting: the fp64 normal-equation sums and metric accumulators live in buffers the wrapper allocates.  Fixed-order reductions: bit-equal between the fills."""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    try:
        from make_eval_golden import CASES, NAMES, SETTINGS, eval_case
    finally:
        sys.path.pop(0)
    from diffusion_e2e_ft_amd import evaluate
    gold = torch.load(os.path.join(here, "golden", "eval_golden.pt"), weights_only=False)
    pred, gt, mask = eval_case(**CASES[0])

    def run(fill):
        outs = {}
        for si, s in enumerate(SETTINGS):
            out = evaluate.depth_metrics(pred.to(dev), gt.to(dev), mask.to(dev), alignment=s["alignment"], min_depth=1e-3, max_depth=80.0, alignment_max_res=s["max_res"],
                                         return_aligned=True)
            outs.update({"%d %s" % (si, k): v for k, v in out.items() if isinstance(v, torch.Tensor)})
        return outs, []

    def check(name, t):
        si, key = name.split(" ", 1)
        want = gold[(0, int(si))]
        if key == "scale":
            assert abs(t.item() - want["scale"]) <= 2e-4 * abs(want["scale"]) + 1e-6
        elif key == "shift":
            assert abs(t.item() - want["shift"]) <= 2e-4 * abs(want["shift"]) + 2e-4
        elif key in NAMES:
            w = want["metrics"][list(NAMES).index(key)].item()
            assert abs(t.item() - w) <= 1e-4 * abs(w) + 1e-5, (name, t.item(), w)
        elif key == "aligned":
            a = t[0].cpu()[::7, ::5]
            assert ((a - want["aligned_sample"]).abs() / want["aligned_sample"].abs().clamp_min(1e-3)).max().item() < 5e-4

    got = check_two_fills(run, check, what="depth_eval")
    assert all("%d %s" % (si, k) in got for si in range(len(SETTINGS)) for k in list(NAMES) + ["scale", "shift", "aligned"])


def test_normal_eval_update_and_finalize_poisoned(dev):
    """ops.normal_eval_update / normal_eval_finalize through evaluate.NormalMetricAccumulator at the first case of tests/test_normal_eval_gpu.py (the reference's
    recorded errors and metrics): error buffer, totals and the radix-select histogram workspace (integer atomicAdd, csrc/normaleval.hip) are allocated by the host layer"""
    from test_normal_eval_cpu import GOLD
    from test_normal_eval_gpu import _check_against_reference
    from diffusion_e2e_ft_amd import evaluate
    c = GOLD["cases"][0]
    res = {}

    def run(fill):
        pred, gt, mask = c["pred"].to(dev), c["gt"].to(dev), c["mask"].to(dev)
        acc = evaluate.NormalMetricAccumulator(capacity=1000)
        acc.update(pred, gt, mask)
        res[fill] = acc.result()
        _check_against_reference(res[fill], acc.errors(), c["errors"], c["metrics"], c["n"], "fill 0x%02X" % fill)
        return dict(errors=acc.errors(), metrics=acc.result_tensor(), error_map=evaluate.normal_error(pred, gt)), []

    check_two_fills(run, what="normal_eval")
    assert res[FILLS[0]] == res[FILLS[1]]


@pytest.mark.parametrize("shape", [(1, 1), (33, 130)])
def test_hypersim_preprocess_poisoned(ops, dev, shape):
    """csrc/hypersimprep.hip at the minimal and a ragged case of tests/test_hypersim_prep_gpu.py::test_ragged_shapes_against_restatement, against the float64 restatement
    (tests/hypersim_prep_ref.py).  The percentile histogram and the per-frame statistics are integer atomics (atomicAdd / atomicMin / atomicMax on unsigned 32- and
    64-bit words, the one at the end of the statistics pass included) into a workspace the wrapper allocates: exact, so every output is bit-equal between the fills."""
    import numpy as np
    import hypersim_prep_ref as hpr
    rng = np.random.default_rng(shape[0] * 10007 + shape[1])
    H, W = shape
    color = (rng.random((H, W, 3)) ** 2 * 2.5 * (0.1 + rng.random())).astype(np.float16)
    dist = (0.3 + rng.random((H, W)) * 20.0).astype(np.float32)
    ids = rng.integers(1, 99, (H, W)).astype(np.int32)
    ids[rng.random((H, W)) < (0.2 if H > 1 else 0.0)] = -1
    ref = hpr.preprocess(color, dist, ids)

    def run(fill):
        c, d, e = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (color, dist, ids))
        rgb, u16, rec = ops.hypersim_preprocess(c, d, e, depth_format="u16")
        rgb2, f32, rec2 = ops.hypersim_preprocess(c, d, e, depth_format="f32")
        return dict(rgb=rgb, u16=u16, record=rec, rgb2=rgb2, f32=f32, record2=rec2), []

    def check(name, t):
        a = t.cpu().numpy()
        if name.startswith("rgb"):
            hpr.check_u8(a, ref, name)
        elif name == "u16":
            assert np.array_equal(a, ref["u16"])
        elif name == "f32":
            assert np.array_equal(a.view(np.uint32), ref["depth_f32"].view(np.uint32))
        else:
            hpr.check_record(a, ref["record"], name)
            assert a[14] == 0.0 and a[15] == 0.0

    check_two_fills(run, check, what="hypersim_preprocess %s" % (shape,))


# ================================================================================================ noise kernels, folded cross-attention
NOISE_FILL_BAR, NOISE_PYRAMID_BAR = 3.5e-6, 1.5e-5      # tests/test_noise_gpu.py


@pytest.mark.parametrize("shape,sizes", [((2, 4, 9, 12), ((9, 12), (4, 6), (2, 3), (1, 1))), ((2, 3, 5, 7), ((5, 7), (2, 3), (1, 1)))])
def test_noise_kernels_write_their_channels_only(ops, dev, shape, sizes):
    """randn_fill_, pyramid_noise_ (include/e2eft.h: "channels c..ldy untouched"; its workspace is poisoned) and latent_x0 on guarded channel slices, fp32, the
    float4 path (c = 4, hw % 4 = 0) and the element-wise one, against tests/noise_ref.py"""
    import noise_ref
    seed = 0x5EED0123456789AB
    B, C, H, W = shape
    ref = dict(randn=noise_ref.normal_grid(seed, 3, 0, shape), pyramid=noise_ref.pyramid(seed, 9, shape, list(sizes), 0.9))
    g = _g(H)
    xt, v = torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, C, generator=g)

    def run(fill):
        gs = Guards(torch.float32, dev, fill)
        rv, pv, xv, vv, ov = gs.out((B, H, W, C)), gs.out((B, H, W, C)), gs.inp(xt), gs.inp(v), gs.out((B, H, W, C))
        ops.randn_fill_(rv, seed, 3, slot=0)
        ops.pyramid_noise_(pv, seed, 9, sizes, 0.9)
        ops.latent_x0(xv, vv, 0.6, -0.8, out=ov)
        return dict(randn=rv, pyramid=pv, x0=ov), gs

    def check(name, t):
        if name == "x0":
            assert_close(t.float().cpu(), 0.6 * xt - 0.8 * v, torch.float32, "latent_x0")
        else:
            err = (t.permute(0, 3, 1, 2).double().cpu() - ref[name]).abs().max().item()
            assert err <= (NOISE_FILL_BAR if name == "randn" else NOISE_PYRAMID_BAR), (name, err)

    check_two_fills(run, check, what="noise kernels %s" % (shape,))


@pytest.mark.parametrize("dtype", DTYPES)
def test_folded_cross_attention_poisoned(dev, dtype):
    """modules.Attention._fold (two-token shared context: two GEMMs and a row kernel instead of the attention kernel) at the smallest case of
    tests/test_cross_attn_fold_gpu.py, against that file's float64 restatement; its fold operands and intermediate rows are allocated by the module.  (That file uses
    neither kv_nseg nor kv_bmod: those are covered by test_attention_joint_segments above.)"""
    from diffusion_e2e_ft_amd import modules as M
    from test_cross_attn_fold_gpu import _ref
    heads, C, N, B = 5, 320, 300, 2
    torch.manual_seed(heads)
    att = M.Attention(C, heads=heads, cross_attention_dim=1024).to(dev, dtype).eval()
    g = _g(C)
    x, res = torch.randn(B, N, C, generator=g).to(dev, dtype), torch.randn(B, N, C, generator=g).to(dev, dtype)
    ctx1 = (0.5 * torch.randn(1, 2, 1024, generator=g)).to(dev, dtype)
    want = _ref(att, x.float(), ctx1.float(), res.float()).float()

    def run(fill):
        att.__dict__.pop("_fold_cache", None)            # the fold itself is rebuilt under this fill
        with torch.no_grad():
            y = att(x, M.CtxCond(ctx1.expand(B, -1, -1).contiguous(), None, shared=True, src=ctx1), residual=res)
        assert att.__dict__.get("_fold_cache") is not None, "the folded route was not taken"
        return dict(y=y), []

    tol = 1e-5 if dtype == torch.float32 else TOL_FOLD[dtype]

    def check(name, t):
        assert rel_err(t, want) <= tol, rel_err(t, want)

    check_two_fills(run, check, what="folded cross-attention")
