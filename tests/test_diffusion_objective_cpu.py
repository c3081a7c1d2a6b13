"""The diffusion objective of the GeoWizard trainer without a GPU: the entry points of csrc/diffusion.hip refuse bad arguments before any device call (through
e2eft_last_error), the workspace query, the host layer's refusals, and the CPU restatement (tests/diffusion_objective_ref.py) against itself in float64."""
import ctypes
import inspect

import pytest
import torch

import diffusion_objective_ref as ref


def _lib():
    from diffusion_e2e_ft_amd import _lib
    return _lib, _lib.load()


def _desc(_lib, **kw):
    d = _lib.DiffusionDesc()
    d.dtype, d.dtype_out, d.prediction, d.rows, d.hw, d.c, d.batch, d.ldx0, d.ldn, d.ldy, d.n_timesteps = 0, 0, 1, 4, 99, 4, 2, 4, 4, 8, 1000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _p():
    buf = ctypes.create_string_buffer(64)
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_latent_valid_mask_arguments():
    _, lib = _lib()
    buf, p = _p()
    assert lib.e2eft_latent_valid_mask(2, 64, 64, None, p, None) == 1 and b"null" in lib.e2eft_last_error()
    assert lib.e2eft_latent_valid_mask(2, 64, 64, p, None, None) == 1
    assert lib.e2eft_latent_valid_mask(2, 60, 64, p, p, None) == 1 and b"multiples of 8" in lib.e2eft_last_error()      # H not a multiple of 8
    assert lib.e2eft_latent_valid_mask(2, 64, 68, p, p, None) == 1 and b"multiples of 8" in lib.e2eft_last_error()
    assert lib.e2eft_latent_valid_mask(0, 64, 64, p, p, None) == 1


def test_diffusion_mix_arguments():
    _lib_, lib = _lib()
    buf, p = _p()
    ok = _desc(_lib_)
    assert lib.e2eft_diffusion_mix(None, 0, p, p, p, p, p, None) == 1
    for missing in range(5):
        args = [p] * 5
        args[missing] = None
        assert lib.e2eft_diffusion_mix(ctypes.byref(ok), 0, *args, None) == 1 and b"null" in lib.e2eft_last_error(), missing
    assert lib.e2eft_diffusion_mix(ctypes.byref(_desc(_lib_, ldy=3)), 0, p, p, p, p, p, None) == 1 and b"smaller than c" in lib.e2eft_last_error()      # ldy < c
    assert lib.e2eft_diffusion_mix(ctypes.byref(_desc(_lib_, ldx0=2)), 0, p, p, p, p, p, None) == 1
    assert lib.e2eft_diffusion_mix(ctypes.byref(_desc(_lib_, dtype=3)), 0, p, p, p, p, p, None) == 1 and b"dtype" in lib.e2eft_last_error()           # unknown dtype
    assert lib.e2eft_diffusion_mix(ctypes.byref(_desc(_lib_, dtype_out=-1)), 0, p, p, p, p, p, None) == 1 and b"dtype" in lib.e2eft_last_error()
    assert lib.e2eft_diffusion_mix(ctypes.byref(ok), 2, p, p, p, p, p, None) == 1 and b"kind" in lib.e2eft_last_error()
    assert lib.e2eft_diffusion_mix(ctypes.byref(_desc(_lib_, n_timesteps=0)), 0, p, p, p, p, p, None) == 1
    assert lib.e2eft_diffusion_mix(ctypes.byref(_desc(_lib_, rows=1 << 20, hw=1 << 10, c=4)), 0, p, p, p, p, p, None) == 1


def test_masked_mse_arguments_and_workspace():
    _lib_, lib = _lib()
    buf, p = _p()
    ok = _desc(_lib_)
    need = lib.e2eft_masked_mse_workspace_bytes(ok.rows, ok.hw, ok.c)
    fwd = lambda d, a=None, ws=need: lib.e2eft_masked_mse_fwd(ctypes.byref(d), *(a or [p] * 10), ws, None)      # noqa: E731
    bwd = lambda d, a=None, ld=4: lib.e2eft_masked_mse_bwd(ctypes.byref(d), *(a or [p] * 9), ld, None)           # noqa: E731
    # NULL pointers (out_target, argument 8 of the forward, is optional and checked by the GPU tests)
    for missing in (0, 1, 2, 3, 4, 5, 6, 7, 9):
        args = [p] * 10
        args[missing] = None
        assert fwd(ok, args) == 1 and b"null" in lib.e2eft_last_error(), missing
    for missing in range(9):
        args = [p] * 9
        args[missing] = None
        assert bwd(ok, args) == 1 and b"null" in lib.e2eft_last_error(), missing
    assert lib.e2eft_masked_mse_fwd(None, *([p] * 10), need, None) == 1 and lib.e2eft_masked_mse_bwd(None, *([p] * 9), 4, None) == 1
    for f in (fwd, bwd):
        assert f(_desc(_lib_, ldy=3)) == 1 and b"smaller than c" in lib.e2eft_last_error()                # ldy < c
        assert f(_desc(_lib_, dtype=7)) == 1 and b"dtype" in lib.e2eft_last_error()                       # unknown dtype
        assert f(_desc(_lib_, prediction=2)) == 1 and b"Unknown prediction type" in lib.e2eft_last_error()    # `sample`: the trainer refuses it (:682)
        assert f(_desc(_lib_, prediction=-1)) == 1 and b"Unknown prediction type" in lib.e2eft_last_error()
        assert f(_desc(_lib_, batch=0)) == 1
    assert bwd(ok, ld=3) == 1 and b"lddp" in lib.e2eft_last_error()
    # a workspace one byte short is refused with code 2, before any device call
    assert need > 0
    assert fwd(ok, ws=need - 1) == 2 and b"workspace" in lib.e2eft_last_error()
    # the query: 0 for an empty problem, monotone in every argument
    q = lib.e2eft_masked_mse_workspace_bytes
    assert q(0, 99, 4) == 0 and q(4, 0, 4) == 0 and q(4, 99, 0) == 0 and q(-1, 99, 4) == 0
    sizes = [q(r, hw, 4) for r, hw in ((1, 1), (1, 64), (4, 64), (4, 99), (4, 4800), (8, 4800), (64, 4800), (256, 19200))]
    assert sizes[0] == 16 and sizes == sorted(sizes) and sizes[-1] > sizes[0], sizes
    assert [q(4, 99, c) for c in (1, 4, 5, 8, 9)] == sorted(q(4, 99, c) for c in (1, 4, 5, 8, 9))


def test_scheduler_methods_have_no_cpu_fallback():
    from diffusion_e2e_ft_amd.scheduler import DDPMScheduler
    s = DDPMScheduler()
    x, n, t = torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 8, 8), torch.tensor([0, 999])
    assert list(inspect.signature(s.add_noise).parameters) == ["original_samples", "noise", "timesteps"]            # diffusers' argument order
    assert list(inspect.signature(s.get_velocity).parameters) == ["sample", "noise", "timesteps"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.add_noise(x, n, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.get_velocity(x, n, t)


def test_host_layer_signatures_and_refusals():
    from diffusion_e2e_ft_amd import training, ops
    sig = inspect.signature(training.geowizard_diffusion_loss)
    assert list(sig.parameters) == ["unet", "vae", "batch", "imgs_embed", "domain", "noise_scheduler", "noise_type", "generator", "noise", "timesteps",
                                    "prediction_type", "return_parts"]
    assert sig.parameters["noise_type"].default == "gaussian" and sig.parameters["domain"].default == "indoor"
    sig = inspect.signature(training.geowizard_e2e_ft_loss)
    assert list(sig.parameters)[-3:] == ["noise_type", "generator", "noise"] and sig.parameters["noise_type"].default == "zeros"
    msg = training.GEOWIZARD_PYRAMID_MESSAGE
    assert "t / 1000" in msg and "286-296" in msg and "e2eft_pyramid_noise" in msg and "not built" in msg
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.latent_valid_mask(torch.ones(1, 1, 8, 8, dtype=torch.bool))


def test_restatement_agrees_with_itself_in_float64():
    """add_noise / get_velocity / the masked MSE of the restatement, fp32 against float64 on the same fp32 inputs: three roundings per mixed value (2^-24 each,
    relative to the larger product), and a mean of non-negative terms"""
    from oracle import pipeline_ref
    g = torch.Generator().manual_seed(3)
    abar = pipeline_ref.alphas_cumprod()
    x0, nz, pred = (torch.randn(4, 4, 9, 11, generator=g) for _ in range(3))
    t = torch.tensor([0, 999, 500, 1])
    a64 = abar.double()
    for fn in (ref.add_noise_ref, ref.get_velocity_ref):
        lo, hi = fn(abar, x0, nz, t), fn(a64, x0.double(), nz.double(), t)
        assert lo.dtype == torch.float32 and hi.dtype == torch.float64
        scale = x0.abs().double() + nz.abs().double()
        assert float(((lo.double() - hi).abs() / scale).max()) <= 4 * 2.0 ** -24
    # the restatement's root is the correctly rounded one: its square brackets the argument between the squares of its two fp32 neighbours' midpoints
    r = ref.root(abar)
    assert r.dtype == torch.float32
    lo = (r.double() + torch.nextafter(r, torch.zeros_like(r)).double()) / 2
    hi = (r.double() + torch.nextafter(r, torch.full_like(r, 2.0)).double()) / 2
    assert bool(((lo * lo <= a64) & (a64 <= hi * hi)).all())
    off = int((abar ** 0.5 != r).sum()), int((abar.sqrt() != r).sum())
    print("this host's fp32 `** 0.5` / sqrt differ from the correctly rounded root at %d / %d of %d schedule entries" % (off + (abar.numel(),)))
    assert ref.target_ref(abar, x0, nz, t, "epsilon") is nz
    with pytest.raises(ValueError, match="Unknown prediction type"):
        ref.target_ref(abar, x0, nz, t, "sample")
    vm = ref.objective_mask()
    lm = ref.latent_mask_ref(vm)
    assert tuple(int(m.sum()) for m in lm[:, 0]) == ref.SELECTED_CELLS
    lm911 = torch.rand(2, 1, 9, 11, generator=g) > 0.3
    tgt = ref.get_velocity_ref(abar, x0, nz, t)
    loss, n = ref.masked_mse_ref(pred, tgt, lm911)
    loss64, n64 = ref.masked_mse_ref(pred.double(), tgt.double(), lm911)
    sel = lm911.repeat(2, 4, 1, 1)
    want = ((pred.double() - tgt.double())[sel] ** 2).mean()
    assert n == n64 == int(sel.sum()) and abs(float(loss) - float(want)) <= 2.0 ** -20 * float(want)
    assert ref.masked_mse_ref(pred, tgt, torch.zeros(2, 1, 9, 11, dtype=torch.bool)) == (torch.zeros(()), 0)
