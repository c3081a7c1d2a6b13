"""Every forward route of the implicit-GEMM family (igemm2 / igemm5 / igemm6 / convin / narrow, the split-K finish, the upsampler phases, the fp32 split-plane route) on
the integer-valued cases of tests/conv_exact_cases.py: the output must EQUAL the float64 reference bit for bit — summation order, tile shape, MFMA form and the split of K
cannot matter when every product and partial sum is an integer below 2^24 — so one dropped k chunk, one wrong border tap, a neighbour's bias in a ragged N tile or an
epilogue term rounded through the output type fails the case that holds it, with the channels / image rows / 256-row tiles of the wrong entries in the message.

Per case three variants (conv_exact_cases): base (bias + rowadd + residual + alpha 0.5 where the route takes them), large (accumulators in [2^12, 2^16], alpha 2^-6;
where the case's shortest reduction can reach 2^12) and round1 (alpha 0.7 + a fractional residual: one rounding, a derived per-element bound).  Deliberate arithmetic
contracts are modelled, not tolerated: split-K's per-tap-row partials rounded to the output type (X.splitk_expect), the split-plane route's three-block sum without
x1 w1 (X.split_planes).  A variant a route declines (the upsampler phases take alpha = 1 only, the thin-input kernel no residual, ...) falls through inside the
library and must still be exact on whichever kernel took it; the tag asserted then is the fall-through's.

Routes are forced in process with the scoped _lib.option(...) and proved by e2eft_debug_last_kernel(); the last test prints route x dtype x variant counts and requires
every route of the family among the asserted tags."""
import contextlib
import ctypes
import re

import pytest
import torch
import torch.nn.functional as TF

import conv_exact_cases as X
from util import nhwc, pack_conv_weight

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
HALF, ALL = (F16, BF16), (F16, BF16, F32)
TNAME = {F16: "_Float16", BF16: "__bf16", F32: "float"}
SEEN = {}            # (route, dtype name, variant) -> cases compared
TAGS = set()         # every kernel tag a comparison was made under
NOT_APPLICABLE = {}  # (route, variant) -> cases whose shortest reduction cannot reach 2^12


@contextlib.contextmanager
def options(**kw):
    """scoped e2eft_set_option for several keys: persistent_grid=8 -> _lib.OPT_PERSISTENT_GRID"""
    from diffusion_e2e_ft_amd import _lib
    with contextlib.ExitStack() as st:
        for k, v in kw.items():
            st.enter_context(_lib.option(getattr(_lib, "OPT_" + k.upper()), v))
        yield


@contextlib.contextmanager
def no_host_splitk():
    """ops.conv2d without its split-K plan: a long reduction on few tiles stays one launch of the route under test"""
    from diffusion_e2e_ft_amd import ops
    old, ops.SPLITK_ENABLED = ops.SPLITK_ENABLED, False
    try:
        yield
    finally:
        ops.SPLITK_ENABLED = old


def _sync():
    """torch.cuda.synchronize(); a device fault ends the session here — nothing more is launched on a device that reported one"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error, stopping the session: %s" % e, returncode=3)


def last_kernel():
    from diffusion_e2e_ft_amd import _lib
    fn = _lib.load().e2eft_debug_last_kernel
    fn.restype = ctypes.c_char_p
    return fn().decode()


def _dev(t, dtype, dev):
    return None if t is None else t.to(torch.float32).to(dtype).to(dev)


def _nhwc(t, dtype, dev):
    return None if t is None else nhwc(t.float(), dtype, dev)


def _note(route, dtype, variant, tag):
    SEEN[(route, TNAME[dtype], variant)] = SEEN.get((route, TNAME[dtype], variant), 0) + 1
    TAGS.add(tag)


def _want(tag_re, variant):
    return tag_re[variant] if isinstance(tag_re, dict) else tag_re


def conv_call(c, dtype, dev, views=False, w_phase=None):
    """ops.conv2d on the case's operands.  views: x and the output are channel slices of wider buffers (pixel strides beyond the channel counts); returns (out, the rest of
    the output buffer, which must stay zero)."""
    from diffusion_e2e_ft_amd import ops
    x, x2 = _nhwc(c.x, dtype, dev), _nhwc(c.x2, dtype, dev)
    w = pack_conv_weight(c.w.float(), dtype, dev)
    out, rest = None, None
    if views:
        B, H, W, c1 = x.shape
        e = ops.epc(dtype)
        wide = torch.full((B, H, W, c1 + 2 * e), 3.0, dtype=dtype, device=dev)      # neighbours a wrong stride would read: not small integers' zeros
        wide[..., e: e + c1] = x
        x = wide[..., e: e + c1]
        hout, wout = ops._conv_out_hw(*((H, W) if c.up_to is None else c.up_to), c.k, c.k, c.stride, c.pad)
        obuf = torch.zeros((B, hout, wout, c.cout + 2 * e), dtype=dtype, device=dev)
        out, rest = obuf[..., e: e + c.cout], (obuf[..., :e], obuf[..., e + c.cout:])
    y = ops.conv2d(x, w, _dev(c.bias, dtype, dev), c.cout, c.k, c.k, c.stride, c.pad, x2=x2, up_to=c.up_to, rowadd=_dev(c.rowadd, dtype, dev),
                   residual=_nhwc(c.residual, dtype, dev), alpha=c.alpha, out=out, w_phase=w_phase)
    _sync()
    if rest is not None:
        assert all(float(r.abs().max()) == 0 for r in rest), "%s: wrote outside its channel slice" % c.name
    return y


def run_conv(dev, route, dtype, opts, tag_re, geom, variants=X.VARIANTS, views=False, expect=None, phases=False, host_splitk=True):
    """one geometry, every variant: build the case on the CPU, run it under `opts`, assert the kernel tag (a regex; a dict per variant where a variant falls through)
    and compare.  expect(c): the route's own arithmetic contract in place of c.expect.  phases: offer the four phase weights of the 2x upsampler."""
    for variant in variants:
        c = X.exact_conv_case(dtype, variant=variant, **geom)
        if c is None:
            NOT_APPLICABLE[(route, variant)] = NOT_APPLICABLE.get((route, variant), 0) + 1
            continue
        with options(**opts), (contextlib.nullcontext() if host_splitk else no_host_splitk()):
            y = conv_call(c, dtype, dev, views=views, w_phase=_phase_weights(c, dtype, dev) if phases else None)
            tag = last_kernel()
        assert re.search(_want(tag_re, variant), tag), "%s [%s]: ran on %s, expected %s" % (c.name, route, tag, _want(tag_re, variant))
        X.check("%s [%s, %s] on %s" % (c.name, route, TNAME[dtype], tag), y, c, expect=None if expect is None or variant == "round1" else expect(c))
        _note(route, dtype, variant, tag)


def _phase_weights(c, dtype, dev):
    from diffusion_e2e_ft_amd import autograd as AG
    conv = torch.nn.Conv2d(c.w.shape[1], c.w.shape[0], 3, padding=1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(c.w.float())
    conv = conv.to(dev)
    return lambda: AG.phase_conv_weight(conv, dtype)


def gemm_call(c, dtype, dev, views=False):
    from diffusion_e2e_ft_amd import ops
    a, w = _dev(c.a, dtype, dev), _dev(c.w, dtype, dev)
    out, rest = None, None
    if views:
        M, K = a.shape
        N = w.shape[0]
        big = torch.full((M, 3 * K), 3.0, dtype=dtype, device=dev)
        big[:, K: 2 * K] = a
        a = big[:, K: 2 * K]
        obuf = torch.zeros((M, 2 * N), dtype=dtype, device=dev)
        out, rest = obuf[:, N:], obuf[:, :N]
    y = ops.gemm(a, w, _dev(c.bias, dtype, dev), _dev(c.residual, dtype, dev), out=out, alpha=c.alpha, bias_along_m=c.bias_along_m)
    _sync()
    if rest is not None:
        assert float(rest.abs().max()) == 0, "%s: wrote outside its column slice" % c.name
    return y


def run_gemm(dev, route, dtype, opts, tag_re, geom, variants=X.VARIANTS, views=False):
    for variant in variants:
        c = X.exact_gemm_case(dtype, variant=variant, **geom)
        if c is None:
            NOT_APPLICABLE[(route, variant)] = NOT_APPLICABLE.get((route, variant), 0) + 1
            continue
        with options(**opts):
            y = gemm_call(c, dtype, dev, views=views)
            tag = last_kernel()
        assert re.search(_want(tag_re, variant), tag), "%s [%s]: ran on %s, expected %s" % (c.name, route, tag, _want(tag_re, variant))
        X.check("%s [%s, %s] on %s" % (c.name, route, TNAME[dtype], tag), y, c)
        _note(route, dtype, variant, tag)


def _ids(cases):
    return [c[0] for c in cases]


# ================================================================================================================================================== igemm2
NO_PERS = dict(persistent=0, f32_split=0)      # igemm5 / igemm6 / convin off; fp32 on v_mfma_f32_32x32x2_f32


def _i2(dtype, mode, fast, nw):
    return r"^igemm2_kernel<%s, %d, %s, %d>$" % (TNAME[dtype], mode, "true" if fast else "false", nw)


def _fast(dtype, geom):
    """igemm2 / igemm5's FAST operand path: whole k-tiles (64 16-bit, 32 fp32 elements) per source"""
    bk = 32 if dtype == F32 else 64
    if "K" in geom:
        return geom["K"] % bk == 0
    return geom["c1"] % bk == 0 and geom.get("c2", 0) % bk == 0


# name, geometry, views
IGEMM2_CONV = [
    ("3x3 ragged M and N, image border inside a tile", dict(B=2, H=17, W=13, c1=64, cout=72, rowadd=True, residual=True, alpha=0.5), False),
    ("3x3 K=1728, four images per tile", dict(B=5, H=8, W=8, c1=192, cout=136, rowadd=True, residual=True, alpha=0.5), False),
    ("3x3 cin 72: no whole k-tile", dict(B=2, H=12, W=12, c1=72, cout=64, rowadd=True, residual=True, alpha=0.5), False),
    ("3x3 cout 20: the scalar epilogue", dict(B=2, H=11, W=9, c1=64, cout=20, rowadd=True, residual=True, alpha=0.5), False),
    ("stride 2", dict(B=2, H=15, W=17, c1=64, cout=32, stride=2, rowadd=True, residual=True, alpha=0.5), False),
    ("stride 2, asymmetric pads", dict(B=2, H=16, W=16, c1=128, cout=32, stride=2, pad=(0, 1, 0, 1), residual=True), False),
    ("fused 2x nearest upsample", dict(B=2, H=8, W=8, c1=128, cout=32, up_to=(16, 16), rowadd=True, alpha=0.5), False),
    ("fused upsample 8x10 -> 15x20", dict(B=1, H=8, W=10, c1=64, cout=32, up_to=(15, 20), residual=True), False),
    ("two sources 64 + 64", dict(B=2, H=10, W=10, c1=64, c2=64, cout=64, rowadd=True, residual=True, alpha=0.5), False),
    ("1x1 on two sources 64 + 32", dict(B=2, H=9, W=11, c1=64, c2=32, cout=96, k=1, residual=True), False),
    ("strided input and output views", dict(B=2, H=12, W=12, c1=128, cout=72, rowadd=True, residual=True, alpha=0.5), True),
]
# every case on 8- and 4-wave tiles; a case whose channels allow the FAST operands also with E2EFT_OPT_IGEMM_GENERAL_OPERANDS
IGEMM2_CONV_RUNS = [(case, dtype, nw, general) for case in IGEMM2_CONV for dtype in ALL for nw in (8, 4) for general in ((0, 1) if _fast(dtype, case[1]) else (0,))]


@pytest.mark.parametrize("case,dtype,nw,general", IGEMM2_CONV_RUNS, ids=["%s-%s-%dw%s" % (c[0], TNAME[d], n, "-general" if g else "") for c, d, n, g in IGEMM2_CONV_RUNS])
def test_igemm2_conv(dev, case, dtype, nw, general):
    name, geom, views = case
    fast = _fast(dtype, geom) and not general
    run_conv(dev, "igemm2 %s %d-wave" % ("FAST" if fast else "general", nw), dtype, dict(NO_PERS, igemm2_waves=nw, igemm_general_operands=general),
             _i2(dtype, 1, fast, nw), geom, views=views)


IGEMM2_GEMM = [
    ("129 x 129 x 72: ragged M, N, K tail", dict(M=129, N=129, K=72, bias=True, residual=True, alpha=0.5), False),
    ("129 x 129 x 72, bias along m", dict(M=129, N=129, K=72, bias=True, bias_along_m=True), False),
    ("300 x 200 x 512", dict(M=300, N=200, K=512, bias=True, residual=True, alpha=0.5), False),
    ("column-slice views", dict(M=200, N=96, K=128, bias=True, residual=False), True),
]


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: TNAME[d])
@pytest.mark.parametrize("nw", [8, 4])
@pytest.mark.parametrize("case", IGEMM2_GEMM, ids=_ids(IGEMM2_GEMM))
def test_igemm2_gemm(dev, dtype, nw, case):
    name, geom, views = case
    fast = _fast(dtype, geom)
    run_gemm(dev, "igemm2 gemm %s %d-wave" % ("FAST" if fast else "general", nw), dtype, dict(NO_PERS, igemm2_waves=nw), _i2(dtype, 0, fast, nw), geom, views=views)
    if fast:
        run_gemm(dev, "igemm2 gemm general %d-wave" % nw, dtype, dict(NO_PERS, igemm2_waves=nw, igemm_general_operands=1), _i2(dtype, 0, False, nw), geom, views=views)


def _bgemm(dev, dtype, route, opts, tag_re, B, H, N, Nk, D, variants):
    """attention-shaped batched GEMM with head strides: S[b, h] = alpha Q[b, :, h] K[b, :, h]^T, operands [B, N, H * D] read in place, output rows padded to 16 bytes"""
    from diffusion_e2e_ft_amd import ops
    e = ops.epc(dtype)
    nkp = ops.round_up(Nk, e)
    for variant in variants:
        # (K = 64 without a bias: 3/4 of the entries non-zero, so that few of the short sums cancel to zero)
        c = X.exact_gemm_case(dtype, N, Nk, D, bias=False, alpha=0.5, variant=variant, batch=(B, H), density=0.75 if D < 128 else None)
        if c is None:
            NOT_APPLICABLE[(route, variant)] = NOT_APPLICABLE.get((route, variant), 0) + 1
            continue
        q_ = _dev(c.a.permute(0, 2, 1, 3).reshape(B, N, H * D), dtype, dev)
        k_ = _dev(c.w.permute(0, 2, 1, 3).reshape(B, Nk, H * D), dtype, dev)
        S = torch.zeros(B, H, N, nkp, dtype=dtype, device=dev)
        with options(**opts):
            ops.bgemm_raw(dtype, N, Nk, D, q_, H * D, (N * H * D, D), k_, H * D, (Nk * H * D, D), S, nkp, (H * N * nkp, N * nkp), B, H, alpha=c.alpha)
            _sync()
            tag = last_kernel()
        assert re.search(tag_re, tag), "%s [%s]: ran on %s" % (c.name, route, tag)
        assert float(S[..., Nk:].abs().max()) == 0 if nkp > Nk else True, "%s: wrote the pad columns" % c.name
        X.check("%s [%s, %s] on %s" % (c.name, route, TNAME[dtype], tag), S[..., :Nk].contiguous(), c)
        _note(route, dtype, variant, tag)


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: TNAME[d])
def test_igemm2_batched_gemm_with_head_strides(dev, dtype):
    _bgemm(dev, dtype, "igemm2 batched gemm", dict(NO_PERS), _i2(dtype, 0, True, 4), 2, 3, 150, 77, 64, X.VARIANTS)
    _bgemm(dev, dtype, "igemm2 batched gemm", dict(NO_PERS), _i2(dtype, 0, True, 4), 1, 2, 130, 64, 512, X.VARIANTS)      # K = 512: the large-sum variant exists


def _dgrad(dev, dtype, route, opts, tag_re, B, H, W, cin, cout, variants=X.VARIANTS, stride=2):
    from diffusion_e2e_ft_amd import ops
    for variant in variants:
        c = X.exact_dgrad_case(dtype, B, H, W, cin, cout, stride=stride, variant=variant, alpha=0.5)
        if c is None:
            NOT_APPLICABLE[(route, variant)] = NOT_APPLICABLE.get((route, variant), 0) + 1
            continue
        with options(**opts):
            dx = ops.conv2d_dgrad(_nhwc(c.dy, dtype, dev), _dev(c.w_dgrad, dtype, dev), (B, H, W, cin), 0, 3, 3, stride, (1, 1, 1, 1), None, c.alpha)
            _sync()
            tag = last_kernel()
        assert re.search(tag_re, tag), "%s [%s]: ran on %s" % (c.name, route, tag)
        X.check("%s [%s, %s] on %s" % (c.name, route, TNAME[dtype], tag), dx, c)
        _note(route, dtype, variant, tag)


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: TNAME[d])
@pytest.mark.parametrize("nw", [8, 4])
def test_igemm2_zero_insertion_dgrad(dev, dtype, nw):
    _dgrad(dev, dtype, "igemm2 zero-insertion dgrad", dict(NO_PERS, igemm2_waves=nw), _i2(dtype, 1, True, nw), 2, 16, 16, 64, 128)
    _dgrad(dev, dtype, "igemm2 zero-insertion dgrad", dict(NO_PERS, igemm2_waves=nw, igemm_general_operands=1), _i2(dtype, 1, False, nw), 2, 14, 18, 72, 128)
    _dgrad(dev, dtype, "igemm2 zero-insertion dgrad", dict(NO_PERS, igemm2_waves=nw), _i2(dtype, 1, True, nw), 1, 10, 14, 64, 320)      # (320 gradient channels: a pixel under ONE tap carries the large-sum variant)


# ================================================================================================================================================== igemm5
PERS5 = dict(persistent_grid=8, patch_conv=0)      # eight workgroups: small problems are eligible; the halo-patch kernel stands aside


def _i5(dtype, mode, res):
    return r"^igemm5_kernel<%s, %d, %s>$" % (TNAME[dtype], mode, "true" if res else "false")


def _i5v(dtype, mode, res):
    """per variant: the large-sum variant carries no residual"""
    return {"base": _i5(dtype, mode, res), "round1": _i5(dtype, mode, res), "large": _i5(dtype, mode, False)}


# name, geometry, kernel mode (0: a 1x1 / stride-1 convolution is a plain GEMM), residual
IGEMM5_CONV = [
    ("9 k-tiles, 27 tiles on 8 workgroups, ragged N tile", dict(B=1, H=48, W=48, c1=64, cout=320, residual=True, alpha=0.5), 1, True),
    ("two sources 64 + 128", dict(B=4, H=16, W=16, c1=64, c2=128, cout=128, rowadd=True, alpha=0.5), 1, False),
    ("four images per tile", dict(B=16, H=8, W=8, c1=128, cout=128, residual=True, alpha=0.5), 1, True),
    ("stride 2", dict(B=4, H=32, W=32, c1=64, cout=136, stride=2, rowadd=True, residual=True, alpha=0.5), 1, True),
    ("fused 2x nearest upsample", dict(B=1, H=16, W=16, c1=128, cout=128, up_to=(32, 32), rowadd=True, residual=True, alpha=0.5), 1, True),
    ("2x2 taps, pads (1, 0, 0, 1)", dict(B=4, H=16, W=16, c1=128, cout=128, k=2, pad=(1, 0, 0, 1), rowadd=True, alpha=0.5), 1, False),
    ("1x1: 3 k-tiles", dict(B=1, H=32, W=32, c1=192, cout=128, k=1, residual=True, alpha=0.5), 0, True),
    ("1x1: 4 k-tiles, 8 columns in the second N tile", dict(B=1, H=32, W=32, c1=256, cout=136, k=1, rowadd=True, alpha=0.5), 0, False),
    ("1x1: 5 k-tiles", dict(B=1, H=32, W=48, c1=320, cout=128, k=1, residual=True), 0, True),
]


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
@pytest.mark.parametrize("case", IGEMM5_CONV, ids=_ids(IGEMM5_CONV))
def test_igemm5_conv(dev, dtype, case):
    name, geom, gemm_mode, res = case
    run_conv(dev, "igemm5", dtype, PERS5, _i5v(dtype, gemm_mode, res), geom)


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
def test_igemm5_declines_a_row_vector_with_several_images_per_tile(dev, dtype):
    """64 rows per image and a per-image row vector: igemm5 declines (its row vector is one per tile), igemm2 takes the launch — and must be exact as well"""
    run_conv(dev, "igemm5 declined -> igemm2", dtype, PERS5, r"^igemm2_kernel<", dict(B=16, H=8, W=8, c1=128, cout=128, rowadd=True, residual=True, alpha=0.5),
             variants=("base", "round1"))


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
def test_igemm5_gemm_and_batched_gemm(dev, dtype):
    run_gemm(dev, "igemm5 gemm", dtype, PERS5, _i5v(dtype, 0, True), dict(M=1024, N=320, K=320, bias=True, residual=True, alpha=0.5))
    run_gemm(dev, "igemm5 gemm", dtype, PERS5, _i5(dtype, 0, False), dict(M=1024, N=136, K=192, bias=True, alpha=0.5))
    _bgemm(dev, dtype, "igemm5 batched gemm", PERS5, _i5(dtype, 0, False), 2, 3, 512, 256, 320, X.VARIANTS)


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
def test_igemm5_zero_insertion_dgrad(dev, dtype):
    _dgrad(dev, dtype, "igemm5 zero-insertion dgrad", PERS5, _i5(dtype, 1, False), 4, 32, 32, 64, 128)
    _dgrad(dev, dtype, "igemm5 zero-insertion dgrad", PERS5, _i5(dtype, 1, False), 4, 16, 32, 128, 320)      # (320 gradient channels: a pixel under ONE tap carries the large-sum variant)


# ================================================================================================================================================== igemm6
def _i6(dtype, form, res, taps=3, nrm=False):
    if taps == 2:
        return r"^igemm6_kernel<%s, %sfalse, false, 2>$" % (TNAME[dtype], "m16, " if form == 2 else "")
    if form == 2:
        return r"^igemm6_kernel<%s, m16, %s, false>$" % (TNAME[dtype], "true" if res else "false")
    return r"^igemm6_kernel<%s, %s, %s>$" % (TNAME[dtype], "true" if res else "false", "true" if nrm else "false")


def _i6v(dtype, form, res, **kw):
    return {"base": _i6(dtype, form, res, **kw), "round1": _i6(dtype, form, res, **kw), "large": _i6(dtype, form, False, **kw)}


# name, geometry, residual, the host would split K (long reduction on few tiles)
IGEMM6_CONV = [
    ("2 chunks, four tiles", dict(B=2, H=16, W=32, c1=128, cout=128, rowadd=True, residual=True, alpha=0.5), True, False),
    ("3 chunks, 12 tiles on 8 workgroups, ragged N tile", dict(B=1, H=32, W=32, c1=192, cout=320, residual=True, alpha=0.5), True, False),
    ("two sources 64 + 64: the switch after one chunk", dict(B=2, H=16, W=32, c1=64, c2=64, cout=136, rowadd=True, alpha=0.5), False, False),
    ("two sources 128 + 64: the switch after two chunks of three", dict(B=2, H=16, W=32, c1=128, c2=64, cout=128, residual=True), True, False),
    ("two sources 64 + 128", dict(B=3, H=16, W=32, c1=64, c2=128, cout=128, rowadd=True, residual=True, alpha=0.5), True, False),
    ("one tile row per image", dict(B=2, H=8, W=128, c1=128, cout=128, rowadd=True, residual=True, alpha=0.5), True, False),
    ("one tile per image, five images", dict(B=5, H=8, W=32, c1=128, cout=128, rowadd=True, residual=True, alpha=0.5), True, False),
    ("5 chunks", dict(B=4, H=16, W=32, c1=320, cout=136, rowadd=True, alpha=0.5), False, True),
    ("fused 2x nearest upsample", dict(B=2, H=8, W=16, c1=128, cout=128, up_to=(16, 32), rowadd=True, residual=True, alpha=0.5), True, False),
]


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
@pytest.mark.parametrize("form", [1, 2], ids=["32x32x16", "16x16x32"])
@pytest.mark.parametrize("case", IGEMM6_CONV, ids=_ids(IGEMM6_CONV))
def test_igemm6_conv(dev, dtype, form, case):
    name, geom, res, splits = case
    run_conv(dev, "igemm6 %s" % ("16x16x32" if form == 2 else "32x32x16"), dtype, dict(persistent_grid=8, patch_mfma=form), _i6v(dtype, form, res), geom,
             host_splitk=not splits)


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
def test_igemm6_source_switch_inside_a_chunk_falls_through(dev, dtype):
    """96 + 32 channels: the second source would start inside a 64-channel chunk; neither persistent kernel takes it, igemm2's general operands do"""
    run_conv(dev, "igemm6 declined -> igemm2", dtype, dict(persistent_grid=8), r"^igemm2_kernel<%s, 1, false, " % TNAME[dtype],
             dict(B=2, H=16, W=32, c1=96, c2=32, cout=128, rowadd=True, residual=True, alpha=0.5))


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
@pytest.mark.parametrize("form", [1, 2], ids=["32x32x16", "16x16x32"])
@pytest.mark.parametrize("pt,pl", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_igemm6_2x2_taps_every_phase_padding(dev, dtype, form, pt, pl):
    run_conv(dev, "igemm6 2x2 %s" % ("16x16x32" if form == 2 else "32x32x16"), dtype, dict(persistent_grid=8, patch_mfma=form), _i6(dtype, form, False, taps=2),
             dict(B=2, H=16, W=32, c1={(1, 1): 192, (1, 0): 256, (0, 1): 128, (0, 0): 320}[(pt, pl)], cout=128 + 8 * pl, k=2, pad=(pt, 1 - pt, pl, 1 - pl), rowadd=True, alpha=0.5))      # (320 channels: one tap of a corner pixel carries the large-sum variant)


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
@pytest.mark.parametrize("geom", [dict(B=2, H=16, W=32, c1=128, cout=128, bias=True, rowadd=True, residual=True, alpha=0.5),
                                  dict(B=5, H=8, W=32, c1=192, cout=64, bias=False, rowadd=False, residual=False, alpha=1.0)], ids=["2 chunks", "one tile per image, 3 chunks"])
def test_igemm6_fused_norm_operand(dev, dtype, geom):
    """e2eft_conv2d_fwd_normed with a hand-made coefficient buffer: (a, mean) = (1 or 2, an integer) per image and channel, integer beta, no SiLU — the operand the
    kernel forms in its fetch is again a small integer (conv_exact_cases: |n| <= 4, zeros exact), padding rows stay zero AFTER the map"""
    from diffusion_e2e_ft_amd import _lib, ops
    lib = _lib.load()
    for variant in ("base", "round1"):
        c = X.exact_conv_case(dtype, variant=variant, norm=True, **geom)
        x, w = _nhwc(c.x, dtype, dev), pack_conv_weight(c.w.float(), dtype, dev)
        coeff = c.coeff.to(torch.float32).to(dev).contiguous()
        beta, bias, rowadd, res = _dev(c.beta, dtype, dev), _dev(c.bias, dtype, dev), _dev(c.rowadd, dtype, dev), _nhwc(c.residual, dtype, dev)
        B, H, W, c1 = x.shape
        out = torch.empty((B, H, W, c.cout), dtype=dtype, device=dev)
        with options(persistent_grid=8):
            d = ops._conv_desc(x, None, c.cout, 3, 3, 1, (1, 1, 1, 1), None, c.alpha, c.cout, c.cout if res is not None else 0, w.shape[1])
            assert lib.e2eft_conv2d_fwd_normed_supported(ctypes.byref(d)) == 1
            _lib.check(lib.e2eft_conv2d_fwd_normed(ctypes.byref(d), ops._ptr(x), ops._ptr(coeff), ops._ptr(beta), 0, ops._ptr(w), ops._ptr(bias), ops._ptr(rowadd), ops._ptr(res),
                                                   ops._ptr(out), None, 0, None, ops._stream()))
            _sync()
            tag = last_kernel()
        assert re.search(_i6(dtype, 1, res is not None, nrm=True), tag), tag
        X.check("%s [fused norm, %s] on %s" % (c.name, TNAME[dtype], tag), out, c)
        _note("igemm6 fused norm", dtype, variant, tag)


# ================================================================================================================================================== convin, narrow
@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
@pytest.mark.parametrize("geom", [dict(B=4, H=32, W=32, cout=128), dict(B=2, H=16, W=96, cout=136), dict(B=17, H=8, W=32, cout=64)], ids=["16 tiles", "ragged N tile", "one tile per image"])
def test_thin_input_conv(dev, dtype, geom):
    """convin.hip: eight input channels, bias and alpha only (K = 72: no large-sum variant)"""
    run_conv(dev, "convin", dtype, dict(persistent_grid=8), r"^conv_thin_in_kernel<%s>$" % TNAME[dtype], dict(geom, c1=8, alpha=0.5))
    # a residual is not the kernel's: the launch falls through
    run_conv(dev, "convin declined", dtype, dict(persistent_grid=8), r"^igemm2_kernel<", dict(geom, c1=8, residual=True, alpha=0.5), variants=("base",))


NARROW = [("128 -> 3", dict(B=1, H=128, W=128, c1=128, cout=3)), ("72 -> 1: a partial chunk", dict(B=1, H=131, W=127, c1=72, cout=1)),
          ("96 -> 2: a 64- and a 32-channel chunk", dict(B=2, H=64, W=130, c1=96, cout=2)), ("32 -> 4", dict(B=1, H=128, W=128, c1=32, cout=4)),
          ("8 -> 3", dict(B=1, H=128, W=130, c1=8, cout=3))]


@pytest.mark.parametrize("dtype,mfma", [(F16, 1), (BF16, 1), (F16, 0), (BF16, 0), (F32, 1)], ids=["_Float16-mfma", "__bf16-mfma", "_Float16-packed dot", "__bf16-packed dot", "float"])
@pytest.mark.parametrize("case", NARROW, ids=_ids(NARROW))
def test_narrow_output_conv(dev, dtype, mfma, case):
    """narrow.hip: 1 to 4 output channels; fp32 (v_fma), packed dot products, MFMA 16x16x32 (Cin % 32 == 0); bias and alpha only"""
    name, geom = case
    form = "_mfma" if (dtype != F32 and mfma and geom["c1"] % 32 == 0) else ""
    route = "narrow fp32" if dtype == F32 else ("narrow mfma" if form else "narrow packed dot")
    run_conv(dev, route, dtype, dict(narrow_mfma=mfma, f32_split=0), r"^conv3x3_narrow%s_kernel$" % form, dict(geom, alpha=0.5))


# ================================================================================================================================================== split-K
@pytest.mark.parametrize("dtype", ALL, ids=lambda d: TNAME[d])
@pytest.mark.parametrize("geom", [dict(B=2, H=12, W=12, c1=256, cout=128), dict(B=1, H=9, W=9, c1=128, c2=128, cout=320), dict(B=2, H=24, W=24, c1=256, cout=128, stride=2)],
                         ids=["2x12x12x256->128", "two sources", "stride 2"])
def test_conv_split_k(dev, dtype, geom):
    """e2eft_conv2d_fwd_splitk: one partial per row of filter taps, ROUNDED to the output type, summed in fp32 by splitk_finish_kernel with the whole epilogue — a
    deliberate contract (X.splitk_expect); with small integers the partials are exact and the result equals the plain reference as well"""
    from diffusion_e2e_ft_amd import _lib, ops
    probe = ops._conv_desc((geom["B"], geom["H"], geom["W"], geom["c1"], geom["c1"]), (geom["c2"], geom["c2"]) if geom.get("c2") else None, geom["cout"], 3, 3,
                           geom.get("stride", 1), (1, 1, 1, 1), None, 1.0, ldo=geom["cout"], ldw=9 * (geom["c1"] + geom.get("c2", 0)), dtype=_lib.dtype_id(dtype))
    assert _lib.load().e2eft_conv2d_splitk_workspace_bytes(ctypes.byref(probe)) > 0, "this shape is expected to be split"
    full = dict(geom, rowadd=True, residual=True, alpha=0.5)
    run_conv(dev, "split-K", dtype, dict(f32_split=0), r"^igemm2_kernel<%s, 1, true, " % TNAME[dtype], full, expect=X.splitk_expect)
    c = X.exact_conv_case(dtype, variant="base", **full)
    X.assert_exact("split-K model vs plain reference", X.splitk_expect(c), c.expect)


# ================================================================================================================================================== upsampler
def _upconv(dev, dtype, route, opts, phase_tag, geom):
    """e2eft_upconv2x_fwd through ops.conv2d(w_phase=...): four 2x2 phases of the low-resolution input against upsample-then-3x3 — exact, the phase weights are sums
    of at most four integers.  The route takes alpha = 1 without row vector or residual: the base variant (bias only) runs the phases, the others the fused-upsample
    3x3 form on whichever kernel takes that."""
    geom = dict(geom, up_to=(2 * geom["H"], 2 * geom["W"]))
    run_conv(dev, route, dtype, opts, phase_tag, dict(geom, alpha=1.0), variants=("base",), phases=True)
    run_conv(dev, route + " declined", dtype, opts, r"^igemm[256]_kernel<", dict(geom, alpha=0.5, rowadd=True), phases=True)


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
def test_upsampler_phases_on_igemm6(dev, dtype):
    _upconv(dev, dtype, "upconv2x on igemm6 2x2", dict(persistent_grid=8, patch_mfma=1), _i6(dtype, 1, False, taps=2), dict(B=4, H=16, W=32, c1=128, cout=256))
    _upconv(dev, dtype, "upconv2x on igemm6 2x2", dict(persistent_grid=8, patch_mfma=2), _i6(dtype, 2, False, taps=2), dict(B=8, H=8, W=32, c1=192, cout=200))


@pytest.mark.parametrize("dtype", HALF, ids=lambda d: TNAME[d])
def test_upsampler_phases_on_igemm5_out_seg_layout(dev, dtype):
    opts = dict(persistent_grid=8, patch_conv_2x2=0)
    _upconv(dev, dtype, "upconv2x on igemm5 (out_seg)", opts, _i5(dtype, 1, False), dict(B=2, H=32, W=32, c1=64, cout=256))
    _upconv(dev, dtype, "upconv2x on igemm5 (out_seg)", opts, _i5(dtype, 1, False), dict(B=3, H=16, W=48, c1=128, cout=320))      # segments of 48: tiles cross them


@pytest.mark.parametrize("dtype", ALL, ids=lambda d: TNAME[d])
def test_upsampler_phases_on_igemm2(dev, dtype):
    """fp32, and widths that are no multiple of 16: the phases run as four igemm2 launches that place every row by division"""
    geom = dict(B=8, H=24, W=24, c1=64, cout=128) if dtype != F32 else dict(B=4, H=32, W=32, c1=32, cout=64)
    _upconv(dev, dtype, "upconv2x on igemm2", dict(persistent_grid=8, f32_split=0), r"^igemm2_kernel<%s, 1, true, " % TNAME[dtype], geom)


# ================================================================================================================================================== fp32 split planes
SPLIT = dict(persistent_grid=8, f32_split=1)


@pytest.mark.parametrize("planes", [False, True], ids=["integers", "two planes"])
@pytest.mark.parametrize("case", [("igemm6", dict(B=2, H=16, W=32, c1=128, cout=128), r"^igemm6_kernel<_Float16, true, false, 3, f32split>$"),
                                  ("igemm6 two sources", dict(B=2, H=16, W=32, c1=64, c2=64, cout=136), r"^igemm6_kernel<_Float16, true, false, 3, f32split>$"),
                                  ("igemm5", dict(B=2, H=16, W=48, c1=128, cout=128), r"^igemm5_kernel<_Float16, 1, true, f32split>$"),
                                  ("igemm5 ragged last tile", dict(B=5, H=18, W=18, c1=64, cout=64), r"^igemm5_kernel<_Float16, 1, true, f32split>$")], ids=lambda c: c[0])
def test_f32_split_plane_conv(dev, planes, case):
    """fp32 convolutions from two-term f16 planes: x0 w0 + x0 w1 + x1 w0, x1 w1 dropped by design.  Integer inputs leave the second plane empty; x = a + b 2^-13,
    w = c + d 2^-13 fill it exactly, and sum ac + 2^-13 sum (ad + bc) is exact in fp32.  The route takes a bias only with alpha = 1 and no row vector."""
    name, geom, tag_re = case
    route = "f32split conv on " + name.split()[0]
    variants = ("base", "round1") if planes else X.VARIANTS
    run_conv(dev, route, F32, SPLIT, tag_re, dict(geom, bias=True, residual=True, alpha=1.0, planes=planes), variants=[v for v in variants if v != "round1"])
    run_conv(dev, route, F32, SPLIT, tag_re, dict(geom, bias=False, residual=True, alpha=0.5, planes=planes), variants=variants)


@pytest.mark.parametrize("planes", [False, True], ids=["integers", "two planes"])
def test_f32_split_plane_gemm(dev, planes):
    tag_re = r"^igemm5_kernel<_Float16, 0, true, f32split>$"
    variants = ("base",) if planes else ("base", "large")
    run_gemm(dev, "f32split gemm", F32, SPLIT, tag_re, dict(M=1024, N=320, K=320, bias=True, residual=True, alpha=1.0, planes=planes), variants=variants)
    run_gemm(dev, "f32split gemm", F32, SPLIT, tag_re, dict(M=1100, N=136, K=512, bias=False, residual=True, alpha=0.5, planes=planes), variants=variants)


@pytest.mark.parametrize("case", [("igemm6", dict(B=2, H=16, W=32, c1=128, cout=128), r"^igemm6_kernel<_Float16, true, false, 2, f32split>$"),
                                  ("igemm5", dict(B=4, H=16, W=16, c1=128, cout=64), r"^igemm5_kernel<_Float16, 1, true, f32split>$")], ids=lambda c: c[0])
def test_f32_split_plane_upsampler(dev, case):
    """e2eft_upconv2x_fwd_f32split.  Integer inputs; and a two-plane INPUT with integer weights — a phase weight is a sum of up to four weights, and a sum of
    c + d 2^-13 terms whose integer parts cancel would put d into the first weight plane, where the x1 w0 product keeps what the construction assumes dropped."""
    name, geom, tag_re = case
    run_conv(dev, "f32split upconv2x on " + name, F32, SPLIT, tag_re, dict(geom, alpha=1.0, up_to=(2 * geom["H"], 2 * geom["W"])), variants=("base",), phases=True)
    c = X.exact_conv_case(F32, variant="base", up_to=(2 * geom["H"], 2 * geom["W"]), **geom)
    g = X.gen(5)
    c.x = c.x + (c.x != 0) * X.integers(c.x.shape, -1, 1, g) * X.PLANE_EPS
    x0, x1, s = X.split_planes(c.x)
    assert torch.equal((x0 + x1) / s, c.x)                                   # both planes together hold x exactly: with integer weights nothing is dropped
    ref = TF.conv2d(TF.interpolate(c.x, scale_factor=2.0, mode="nearest"), c.w, c.bias, padding=1)
    expect = ref.float().permute(0, 2, 3, 1).contiguous()
    assert torch.equal(expect.double().permute(0, 3, 1, 2), ref)
    with options(**SPLIT):
        y = conv_call(c, F32, dev, w_phase=_phase_weights(c, F32, dev))
        tag = last_kernel()
    assert re.search(tag_re, tag), tag
    X.assert_exact("%s two-plane input [f32split upconv2x] on %s" % (c.name, tag), y, expect)
    _note("f32split upconv2x on " + name, F32, "base", tag)


# ================================================================================================================================================== coverage
REQUIRED = {
    "igemm2 FAST, 8 waves": r"^igemm2_kernel<\w+, 1, true, 8>", "igemm2 FAST, 4 waves": r"^igemm2_kernel<\w+, 1, true, 4>",
    "igemm2 general, 8 waves": r"^igemm2_kernel<\w+, 1, false, 8>", "igemm2 general, 4 waves": r"^igemm2_kernel<\w+, 1, false, 4>",
    "igemm2 fp32": r"^igemm2_kernel<float, ", "igemm2 GEMM": r"^igemm2_kernel<\w+, 0, ",
    "igemm5 conv": r"^igemm5_kernel<(_Float16|__bf16), 1, (true|false)>", "igemm5 GEMM": r"^igemm5_kernel<(_Float16|__bf16), 0, (true|false)>",
    "igemm6 32x32x16": r"^igemm6_kernel<(_Float16|__bf16), (true|false), false>", "igemm6 16x16x32": r"^igemm6_kernel<(_Float16|__bf16), m16, (true|false), false>",
    "igemm6 2x2": r"^igemm6_kernel<(_Float16|__bf16), false, false, 2>", "igemm6 2x2 16x16x32": r"^igemm6_kernel<(_Float16|__bf16), m16, false, false, 2>",
    "igemm6 fused norm": r"^igemm6_kernel<(_Float16|__bf16), (true|false), true>",
    "convin": r"^conv_thin_in_kernel<", "narrow": r"^conv3x3_narrow_kernel$", "narrow MFMA": r"^conv3x3_narrow_mfma_kernel$",
    "f32split igemm6 3x3": r"^igemm6_kernel<_Float16, true, false, 3, f32split>", "f32split igemm6 2x2": r"^igemm6_kernel<_Float16, true, false, 2, f32split>",
    "f32split igemm5 conv": r"^igemm5_kernel<_Float16, 1, true, f32split>", "f32split igemm5 GEMM": r"^igemm5_kernel<_Float16, 0, true, f32split>",
}
REQUIRED_ROUTES = ("split-K", "upconv2x on igemm6 2x2", "upconv2x on igemm5 (out_seg)", "upconv2x on igemm2", "narrow fp32", "narrow packed dot", "narrow mfma",
                   "igemm2 zero-insertion dgrad", "igemm5 zero-insertion dgrad", "igemm2 batched gemm", "igemm5 batched gemm")


def test_every_route_was_compared(dev, request):
    """prints route x dtype x variant -> cases compared; when the whole file ran, every route of the family must be among the asserted kernel tags"""
    routes = sorted({k[0] for k in SEEN})
    print("\n%-44s %-9s %6s %6s %6s" % ("route", "dtype", "base", "large", "round1"))
    for r in routes:
        for dt in ("_Float16", "__bf16", "float"):
            n = [SEEN.get((r, dt, v), 0) for v in X.VARIANTS]
            if any(n):
                print("%-44s %-9s %6d %6d %6d" % (r, dt, *n))
    for (r, v), n in sorted(NOT_APPLICABLE.items()):
        print("no %s variant (shortest reduction below 320 terms): %s x %d" % (v, r, n))
    print("%d kernel tags: %s" % (len(TAGS), sorted(TAGS)))
    if request.config.getoption("keyword") or any("::" in a for a in request.config.args):
        return          # a selection of this file's tests: the table above is what it covered
    missing = [name for name, pat in REQUIRED.items() if not any(re.search(pat, t) for t in TAGS)]
    missing += [r for r in REQUIRED_ROUTES if r not in routes]
    assert not missing, "no comparison ran on: %s" % missing
