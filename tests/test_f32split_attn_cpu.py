"""Host side of the split-operand fp32 attention route (csrc/attn_f32split.hip): option 15 (E2EFT_OPT_F32_SPLIT_ATTN, off by default) and the pure host
arithmetic of e2eft_attn_f32split_supported.  No GPU."""
import ctypes as C

import pytest

from diffusion_e2e_ft_amd import _lib


def _desc(B, heads, N, Nk, dtype=0, kv_nseg=1, kv_bmod=None):
    d = _lib.AttnDesc()
    d.dtype = dtype
    d.batch, d.heads, d.nq, d.nk_seg = B, heads, N, Nk
    d.kv_nseg = kv_nseg
    d.kv_bmod = B if kv_bmod is None else kv_bmod
    d.ldq = d.ldk = d.ldv = d.ldo = heads * 64
    d.scale = 0.125
    return d


@pytest.fixture
def split_on():
    _lib.set_option(_lib.OPT_F32_SPLIT_ATTN, 1)
    try:
        yield _lib.load()
    finally:
        _lib.set_option(_lib.OPT_F32_SPLIT_ATTN, 0)


def test_option_defaults_to_off_and_round_trips():
    lib = _lib.load()
    assert _lib.OPT_F32_SPLIT_ATTN == 15
    assert lib.e2eft_get_option(15) == 0
    try:
        _lib.set_option(15, 1)
        assert lib.e2eft_get_option(15) == 1
        _lib.set_option(15, 0)
        assert lib.e2eft_get_option(15) == 0
        with pytest.raises(RuntimeError):
            _lib.set_option(15, 2)
    finally:
        _lib.set_option(15, 0)
    assert lib.e2eft_version() == 119


def test_supported_is_zero_with_the_option_off():
    lib = _lib.load()
    assert lib.e2eft_get_option(15) == 0
    for shape in ((2, 5, 144, 144), (1, 5, 200, 77), (2, 3, 576, 2)):
        for bwd in (0, 1):
            assert lib.e2eft_attn_f32split_supported(C.byref(_desc(*shape)), bwd) == 0


@pytest.mark.parametrize("shape", [(2, 5, 144, 144), (1, 5, 200, 77), (2, 3, 576, 2), (16, 5, 5184, 5184), (16, 20, 81, 81), (1, 1, 1, 1)])
def test_supported_shapes_forward_and_backward(split_on, shape):
    for bwd in (0, 1):
        assert split_on.e2eft_attn_f32split_supported(C.byref(_desc(*shape)), bwd) == 1


def test_declined_descriptors(split_on):
    lib = split_on
    for dtype in (1, 2):                                                  # fp16, bf16
        for bwd in (0, 1):
            assert lib.e2eft_attn_f32split_supported(C.byref(_desc(2, 5, 144, 144, dtype=dtype)), bwd) == 0
    assert lib.e2eft_attn_f32split_supported(None, 0) == 0 and lib.e2eft_attn_f32split_supported(None, 1) == 0
    assert lib.e2eft_attn_f32split_supported(C.byref(_desc(2, 5, 0, 144)), 0) == 0      # no geometry: the entry point rejects it
    # DESIGN.md §3 "fp32 attention from f16 splits": GeoWizard's joint keys (kv_nseg = 2) are declined and stay on attn32.hip
    for bwd in (0, 1):
        assert lib.e2eft_attn_f32split_supported(C.byref(_desc(4, 2, 200, 200, kv_nseg=2, kv_bmod=2)), bwd) == 0
    # the backward has no form with a key batch that differs from the query batch (e2eft_attn_bwd rejects it)
    assert lib.e2eft_attn_f32split_supported(C.byref(_desc(4, 2, 200, 77, kv_bmod=2)), 0) == 1
    assert lib.e2eft_attn_f32split_supported(C.byref(_desc(4, 2, 200, 77, kv_bmod=2)), 1) == 0


def test_workspace_answer_does_not_depend_on_the_option():
    lib = _lib.load()
    d = _desc(2, 5, 144, 144)
    off = lib.e2eft_attn_bwd_workspace_bytes(C.byref(d))
    try:
        _lib.set_option(15, 1)
        on = lib.e2eft_attn_bwd_workspace_bytes(C.byref(d))
    finally:
        _lib.set_option(15, 0)
    assert off == 2 * 5 * 144 * 4 and on == off      # the route shares attn32's D = rowsum(dO o O) pass and needs nothing else
