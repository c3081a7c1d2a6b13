"""Pin the CPU oracle (oracle/unet_ref.py, vae_ref.py, pipeline_ref.py) to the REFERENCE'S OWN SOURCE.

The reference vendors diffusers' UNet composition code (GeoWizard/geowizard/models/{unet_2d_condition,unet_2d_blocks,transformer_2d,
attention}.py) and holds the pipeline / training glue (Marigold/marigold/marigold_pipeline.py, geowizard_pipeline.py, training/train.py).
These tests import and execute those files in place (tests/refimport.py; third-party LEAF modules come from tests/stubs, which is the
only part that stays "restated from the published diffusers 0.30.2 definitions") and assert that

  * the oracle's functional UNet / VAE equal the reference wiring on the same seeded state dict (loaded strict=True: the key sets
    agree) — SD-v2 and GeoWizard configurations, forced-upsample sizes, per-sample timesteps, 77-token context, joint attention;
  * the oracle's pipeline / training-step restatements equal the reference's `single_infer` / step body run from source;
  * the committed fixtures are what the reference's code produces today: tests/golden/refwiring_golden.pt is regenerated and compared,
    and the oracle-made tests/golden/model_golden.pt / train_golden.pt (which every GPU parity test checks the HIP path against) agree
    with the reference wiring to fp32 round-off.
Where the reference tree is absent the same assertions run against what its code produced when the fixtures were made
(tests/golden/refwiring_golden*.pt, tests/golden/reference_pins.pt); where it is present, the fixtures are also checked against it."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import golden_cases as gc  # noqa: E402
import make_reference_pins as pins  # noqa: E402
import make_refwiring_golden  # noqa: E402
import refimport  # noqa: E402
from oracle import config, pipeline_ref, synth, unet_ref, vae_ref  # noqa: E402

LIVE = refimport.reference_available()
TOL = 1e-5      # fp32 round-off between two orderings of the same arithmetic (measured 2e-6)


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def ref():
    """the reference's modules, imported from its source; None where the tree is absent (the recorded results stand in)"""
    if not LIVE:
        yield None
        return
    with refimport.reference_modules() as r:
        yield r


@pytest.fixture(scope="module")
def gen():
    return make_refwiring_golden


@pytest.fixture(scope="module")
def fx():
    return make_refwiring_golden.load_fixture()


def test_reference_unet_loads_oracle_state_dict_strictly():
    """key set and shapes of oracle.unet_param_shapes == the reference constructor's parameters (SD-v2 shape AND the full-size config)"""
    want = pins.pinned("unet_keys")
    for name in ("TINY_UNET", "TINY_GEOWIZARD_UNET", "SD2_UNET"):
        assert want[name] == {k: tuple(v) for k, v in unet_ref.unet_param_shapes(getattr(config, name)).items()}, name
    assert want["SD2_UNET_numel"] == 865_922_244


def test_reference_vae_blocks_load_oracle_state_dict_strictly():
    want = pins.pinned("vae_keys")
    for name, n in (("TINY_VAE", None), ("SD_VAE", 83_653_863)):
        assert want[name] == {k: tuple(v) for k, v in vae_ref.vae_param_shapes(getattr(config, name)).items()}, name
        if n:
            assert want[name + "_numel"] == n


@pytest.mark.parametrize("hw,batch,ctx_len,per_sample_t", pins.UNET_CASES)
def test_oracle_unet_equals_reference_wiring(hw, batch, ctx_len, per_sample_t):
    """unet_2d_condition.py:845-1221 incl. the forced-upsample path (:920-930,1185-1186) for latent sizes not divisible by 8"""
    want = pins.pinned("unet_wiring")[pins.UNET_CASES.index((hw, batch, ctx_len, per_sample_t))]
    x, ctx = gc.unet_inputs(hw, batch=batch, ctx_len=ctx_len, seed=8)
    t = torch.tensor([999, 500, 1][:batch]) if per_sample_t else 999
    with torch.no_grad():
        got = unet_ref.unet_forward(gc.tiny_unet_sd(), config.TINY_UNET, x, t, ctx)
    assert rel(got, want) < TOL


def test_oracle_joint_attention_equals_reference_processor():
    """GeoWizard: XFormersJointAttnProcessor (attention.py:425-513) installed the way the reference installs it
    (enable_xformers_memory_efficient_attention -> CustomJointAttention.set_use_memory_efficient_attention_xformers), class embedding"""
    pin = pins.pinned("joint_attention")
    assert "XFormersJointAttnProcessor" in pin["processors"]
    want = pin["out"]
    x, ctx, cls = gc.geo_unet_inputs()
    with torch.no_grad():
        got = unet_ref.unet_forward(gc.tiny_geo_sd(), config.TINY_GEOWIZARD_UNET, x, 999, ctx, class_labels=cls)
        plain = unet_ref.unet_forward(gc.tiny_geo_sd(), dict(config.TINY_GEOWIZARD_UNET, joint_attention=False), x, 999, ctx, class_labels=cls)
    assert rel(got, want) < TOL
    assert rel(plain, want) > 1e-3          # the joint keys matter: the test would notice a processor that was not installed


def test_oracle_vae_equals_reference_blocks():
    want = pins.pinned("vae_blocks")
    rgb, z = gc.vae_inputs()
    sd = gc.tiny_vae_sd()
    with torch.no_grad():
        assert rel(vae_ref.quant_conv(sd, vae_ref.encoder_forward(sd, config.TINY_VAE, rgb)), want["moments"]) < TOL
        assert rel(vae_ref.decoder_forward(sd, config.TINY_VAE, vae_ref.post_quant_conv(sd, z)), want["dec"]) < TOL


def test_oracle_pipeline_equals_reference_single_infer_source(ref, gen, fx):
    """marigold_pipeline.py:372-538 run from source (depth, normals, 2-step DDIM; recorded: refwiring_golden.pt) vs oracle.pipeline_ref"""
    cases = gen.marigold_cases(ref) if ref is not None else fx["marigold"]
    rgb, ctx = synth.synth_inputs(1, 64, 96, 2, 128, seed=3)
    usd, vsd = gc.tiny_unet_sd(), gc.tiny_vae_sd()
    with torch.no_grad():
        d = pipeline_ref.single_infer_ref(usd, config.TINY_UNET, vsd, config.TINY_VAE, rgb, ctx)
        n = pipeline_ref.single_infer_ref(usd, config.TINY_UNET, vsd, config.TINY_VAE, rgb, ctx, normals=True)
        lat = torch.zeros(1, 4, 8, 12)
        d2 = pipeline_ref.marigold_multistep_ref(usd, config.TINY_UNET, vsd, config.TINY_VAE, rgb, ctx, lat, 2)
    assert rel(d, cases["depth"]["out"]) < TOL
    assert rel(n, cases["normals"]["out"]) < 5 * TOL
    assert rel(d2, cases["depth_2step"]["out"]) < TOL
    # the caller's view of the modules: exactly these accesses, in this order
    assert [e["path"] for e in cases["depth"]["trace"]] == ["vae.encoder", "vae.quant_conv", "unet", "vae.post_quant_conv", "vae.decoder"]
    call = cases["depth"]["trace"][2]
    assert list(call["kwargs"]) == ["encoder_hidden_states"] and call["args"]["__seq__"][1]["__tensor__"].dim() == 0   # t: 0-dim int64 tensor


def test_oracle_geowizard_equals_reference_single_infer_source(ref, gen, fx):
    case = gen.geowizard_case(ref) if ref is not None else fx["geowizard"]
    rgb, emb = gc.geo_pipe_inputs()
    with torch.no_grad():
        d, n = pipeline_ref.geowizard_infer_ref(gc.tiny_geo_sd(), config.TINY_GEOWIZARD_UNET, gc.tiny_vae_sd(), config.TINY_VAE,
                                                rgb[:1], emb[:1], "indoor")
    # unit normals: x / (|x| + 1e-5) amplifies round-off where |x| is small.  Against the recorded result (another host's fp32 convolutions)
    # the normals get the bound of the unit-normal estimate below (measured 2.2e-5 - 3.8e-5 across thread counts on one host, 5.7e-5 on another)
    assert rel(d, case["depth"]) < TOL and rel(n, case["normal"]) < (5 * TOL if ref is not None else 2e-4)


@pytest.fixture(scope="module")
def ref_train_cases(ref, gen, fx):
    return gen.train_cases(ref) if ref is not None else fx["train"]


@pytest.mark.parametrize("modality", ["depth", "normals"])
def test_oracle_train_step_equals_reference_step_body_source(ref_train_cases, modality):
    """training/train.py:472-566 run line for line; loss and ALL 686 UNet gradients vs torch autograd over the oracle"""
    case = ref_train_cases[modality]
    want = gc.train_grads(modality)
    assert abs(float(want["loss"]) - float(case["loss"])) < 1e-5 * abs(float(case["loss"]))
    assert rel(want["estimate"], case["estimate"]) < (TOL if modality == "depth" else 2e-4)   # unit normals: x / (|x| + 1e-5) amplifies round-off where |x| is small
    assert set(want["grad_norms"]) == set(case["grad_norms"])
    worst = max(abs(want["grad_norms"][k] - v) / max(v, 1e-12) for k, v in case["grad_norms"].items() if v > 1e-8)
    assert worst < 1e-3, worst
    for k, g in case["grads"].items():
        assert rel(want["grads"][k], g) < 2e-4, k


def test_committed_fixtures_are_what_the_reference_produces(ref, gen, fx):
    """refwiring_golden*.pt is reproducible from the reference's code (where its tree is present), and the oracle-made model / train goldens
    agree with it"""
    now = gen.model_cases(ref) if ref is not None else fx["model"]
    for k, v in now.items():
        assert rel(fx["model"][k], v) < 1e-6, k
    old = torch.load(os.path.join(HERE, "golden", "model_golden.pt"), weights_only=False)
    assert rel(old["unet_16x16"]["out"], now["unet_16x16"]) < TOL and rel(old["unet_20x12"]["out"], now["unet_20x12"]) < TOL
    assert rel(old["unet_ctx77"]["out"], now["unet_ctx77"]) < TOL and rel(old["geo_unet"]["out"], now["geo_unet"]) < TOL
    assert rel(old["vae"]["moments"], now["vae_moments"]) < TOL and rel(old["vae"]["dec"], now["vae_dec"]) < TOL
    tr_old = torch.load(os.path.join(HERE, "golden", "train_golden.pt"), weights_only=False)
    for m in ("depth", "normals"):
        assert abs(float(tr_old[m]["loss"]) - float(fx["train"][m]["loss"])) < 1e-5 * abs(float(fx["train"][m]["loss"]))
        for k, g in fx["train"][m]["grads"].items():
            assert rel(tr_old[m]["grads"][k], g) < 2e-4, (m, k)
    if ref is not None:
        cases = gen.marigold_cases(ref)
        for k in ("depth", "normals", "depth_2step"):
            assert rel(fx["marigold"][k]["out"], cases[k]["out"]) < 1e-6
