"""`MarigoldPipeline` surface (Marigold/marigold/marigold_pipeline.py:113-538) over the libe2eft UNet / VAE, plus the
batched GeoWizard joint depth+normal inference (GeoWizard/geowizard/models/geowizard_pipeline.py:252-344).

Same component slots (unet, vae, scheduler, text_encoder, tokenizer), same `__call__` keyword arguments, same
`single_infer / encode_rgb / decode_depth / decode_normal` methods and `MarigoldDepthOutput` fields.  Host-side image
pre/post-processing (resize, colourising) is SURVEY.md §8f "next"; it runs in torch on the host as in the reference.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops
from .modules import to_nchw_view


@dataclass
class MarigoldDepthOutput:
    depth_np: Optional[np.ndarray]
    depth_colored: object
    uncertainty: Optional[np.ndarray]
    normal_np: Optional[np.ndarray]
    normal_colored: object


@dataclass
class DepthNormalPipelineOutput:          # geowizard_pipeline.py:37-57
    depth_np: np.ndarray
    depth_colored: object
    normal_np: np.ndarray
    normal_colored: object
    uncertainty: Optional[np.ndarray]


class _LatentPipeline:
    """What both pipelines own: the unet / vae / scheduler slots, `dtype` / `device`, the VAE round trip with the latent scale factors, the one-step
    schedule, the DDIM update and the hipGraph cache."""
    rgb_latent_scale_factor = 0.18215    # marigold_pipeline.py:134
    depth_latent_scale_factor = 0.18215  # marigold_pipeline.py:135

    _graphs = None

    def __init__(self, unet, vae, scheduler):
        self.unet, self.vae, self.scheduler = unet, vae, scheduler

    # ---- DiffusionPipeline-like surface (Marigold/run.py:274-290) ----
    @property
    def dtype(self):
        return self.unet.dtype

    @property
    def device(self):
        return self.unet.device

    # ---- marigold_pipeline.py:481-498 ----
    @ops.device_scoped
    @torch.no_grad()
    def encode_rgb(self, rgb_in):
        h = self.vae.encoder(rgb_in)
        moments = self.vae.quant_conv(h)
        mean = moments[:, : moments.shape[1] // 2]  # torch.chunk(moments, 2, dim=1)[0]
        return _scaled(mean, self.rgb_latent_scale_factor)

    def _decode(self, latent):
        z = self.vae.post_quant_conv(_scaled(latent, 1.0 / self.depth_latent_scale_factor))
        return self.vae.decoder(z)

    def _one_step_schedule(self):
        """(t_dev [1], sb) of the one-step setting: x0 = -sb * model_output (by prediction_type); sb comes from the host copy of the timestep, no device read-back"""
        self.scheduler.set_timesteps(1, device=self.device)
        return self.scheduler.timesteps[:1], -self.scheduler.zero_latent_x0_scale(self.scheduler.timesteps_host[0])

    def _ddim_step(self, v, t_host, latent, last):
        """one scheduler step from the host copy of the timestep (no device synchronisation per step); the last step hands back the predicted x0
        (marigold_pipeline.py:466-468, geowizard_pipeline.py:332-336)"""
        step = self.scheduler.step(v, t_host, latent)
        return step.pred_original_sample if last else step.prev_sample

    def enable_hip_graphs(self, enabled=True):
        """Replay the one-step zero-latent `single_infer` from a hipGraph captured per key (Marigold: input shape, dtype, modality, context; GeoWizard: batch
        shape, dtype, domain, embedding source): ~1.4k launches per batch become one graph launch, which removes the host-side gaps on the small UNet levels
        (at 2 GeoWizard images per step the CLIP tower is launch-bound as well).  Every other step count or start the device can produce inside a capture
        (zeros, an explicit latent, gaussian from a `noise.DeviceNoise`) runs through `_denoise`: a head, ONE step and a tail graph per key, the DDIM update fused
        into the step graph; a `torch.Generator` and "pyramid" keep the host-driven loop.  Weights are baked in by address: call this again after changing them
        (load_state_dict, .to(), an optimizer step)."""
        self._graphs = {} if enabled else None
        return self

    def _replay(self, key, static, keep, fn):
        """`fn(*static)` replayed from the graph cached under key + the weight state.  static: the tensors copied into the graph's own input buffers before
        every replay (a None passes through); keep: tensors the graph reads in place — the entry keeps them alive, an address in `key` or baked into the graph
        must not be handed to another tensor while the entry lives; fn: only device work on the current stream, returns a tensor or a tuple of tensors."""
        from . import autograd as F
        w0 = self.unet.conv_in.weight
        weights = (F.PARAM_EPOCH, w0.data_ptr(), w0._version)
        key = key + (weights,)
        ent = self._graphs.get(key)
        if ent is None:
            # a new weight state makes every graph captured for an older one unreachable — drop them (validation during training would otherwise grow the
            # cache by one graph + its static buffers per step)
            for k in [k for k in self._graphs if k[-1] != weights]:
                del self._graphs[k]
            fn(*static)                      # eager pass: fills the packed-weight caches (and the folded cross-attention of a kept context)
            torch.cuda.synchronize()
            s_in = tuple(None if t is None else t.clone() for t in static)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                s_out = fn(*s_in)
            ent = self._graphs[key] = (g, s_in, s_out, (w0, keep))
        g, s_in, s_out, _ = ent
        for s, t in zip(s_in, static):
            if s is not None:
                s.copy_(t)
        g.replay()
        return s_out.clone() if isinstance(s_out, torch.Tensor) else tuple(o.clone() for o in s_out)

    # ---- multi-step inference with the DDIM update fused on the device ----
    _dn_copies = 1        # row blocks of the UNet input that share the rgb latent and the initial noise (GeoWizard: a depth block and a normal block)

    def _fused_denoise(self, num_inference_steps, noise, generator):
        """does this call run through `_denoise`?  Graphs on, not the one-step zeros case (its own captured path), and a start the device can produce inside a
        capture: zeros, an explicit latent, or gaussian from a `noise.DeviceNoise`.  A `torch.Generator` and "pyramid" keep the host-driven loop."""
        if self._graphs is None:
            return False
        if isinstance(noise, torch.Tensor):
            return True
        if noise == "zeros":
            return num_inference_steps != 1
        from .noise import DeviceNoise
        return noise == "gaussian" and isinstance(generator, DeviceNoise)

    def _denoise(self, rgb, num_inference_steps, noise, generator=None, captured=True, rows=None, img_embed=None, **mode):
        """Multi-step DDIM inference as three pieces over one set of static buffers per key, each piece a hipGraph when `captured`:
          head  VAE encode -> the rgb latent into channels 0:C of the persistent UNet input `xin`, the initial latent into C:2C (a memset, a copy of the explicit
                tensor, or `noise.randn_at` reading the draw from the device), the context / class embedding;
          step  ONE graph for every step of every schedule: the UNet on `xin` at `t`, then `ops.ddim_step_` in place on xin[..., C:].  Its inputs `t` (int64 [1])
                and `coef` ([2]) are refreshed before each replay by device-to-device copies from `scheduler.timesteps[i:i+1]` and row i of
                `scheduler.step_coefficients`; the host loop is n times (two tiny copies + one graph launch) and reads nothing back;
          tail  decode + head from xin[..., C:], which holds the predicted x0 after the last step (the table's last row).
        The key leaves the step count out: three steps and four steps share the graphs.  A generator's seed is a launch argument of the head graph (its draw
        counter is not: `noise.set_draw`), so a generator with another seed recaptures the entry in place — keep one generator per pipeline.  rows: encode ONE image (rgb [1,3,H,W]) and broadcast its latent into
        `rows` rows — the members of an ensemble (the encoder is batch-invariant bit for bit, tests/test_multistep_graph_gpu.py).  captured=False issues the same
        launches eagerly on fresh buffers (and needs no graph cache): the capture can then be checked bit for bit, apart from the arithmetic.
        Everything stays on the current stream; the graphs have no parallel branches."""
        from . import autograd as F
        from . import noise as N
        device, dt = self.device, self.dtype
        rgb = rgb.to(device=device, dtype=dt)
        n = int(num_inference_steps)
        self.scheduler.set_timesteps(n, device=device)
        table = self.scheduler.step_coefficients(n, device)
        B = rgb.shape[0] if rows is None else int(rows)
        if rows is not None and rgb.shape[0] != 1:
            raise ValueError("_denoise: rows= broadcasts ONE encoded image, got %d" % rgb.shape[0])
        kind = "tensor" if isinstance(noise, torch.Tensor) else noise
        if kind == "gaussian" and not isinstance(generator, N.DeviceNoise):
            raise TypeError("_denoise: noise='gaussian' needs a noise.DeviceNoise generator")
        if kind not in ("tensor", "zeros", "gaussian"):
            raise ValueError("_denoise: noise must be 'zeros', 'gaussian' or a tensor, got %s" % (noise,))
        seed = generator.seed if kind == "gaussian" else None
        if img_embed is not None:
            img_embed = img_embed.to(device=device, dtype=dt)
        ent = None
        if captured:
            if self._graphs is None:
                raise RuntimeError("_denoise(captured=True) needs enable_hip_graphs()")
            w0 = self.unet.conv_in.weight
            weights = (F.PARAM_EPOCH, w0.data_ptr(), w0._version)
            key = ("denoise", tuple(rgb.shape), B, dt, kind, None if img_embed is None else tuple(img_embed.shape)) + self._dn_key(mode) + (weights,)
            ent = self._graphs.get(key)
            if ent is not None and ent["seed"] != seed:      # the seed travels by value: another generator seed is another head graph, which REPLACES this one
                ent = None
        if ent is None:
            ent = self._dn_entry(rgb, B, kind, seed, img_embed, mode)
        st = ent["static"]
        st["rgb"].copy_(rgb)
        if img_embed is not None:
            st["embed"].copy_(img_embed)
        if kind == "tensor":
            if tuple(noise.shape) != tuple(st["noise"].permute(0, 3, 1, 2).shape):
                raise ValueError("_denoise: the explicit latent must be %s, got %s" % (tuple(st["noise"].permute(0, 3, 1, 2).shape), tuple(noise.shape)))
            st["noise"].copy_(noise.to(device=device, dtype=dt).permute(0, 2, 3, 1))
        elif kind == "gaussian":
            N.set_draw(st["draw"], generator)
        timesteps = self.scheduler.timesteps
        if captured and "graphs" not in ent:
            for k in [k for k in self._graphs if k[-1] != weights]:      # as _replay: graphs of an older weight state are unreachable
                del self._graphs[k]
            st["t"].copy_(timesteps[:1])
            st["coef"].copy_(table[0])
            self._dn_step(ent, *self._dn_head(ent))      # eager pass: fills the packed-weight caches
            self._dn_tail(ent)
            torch.cuda.synchronize()
            graphs = [torch.cuda.CUDAGraph() for _ in range(3)]
            with torch.cuda.graph(graphs[0]):
                cond = self._dn_head(ent)
            with torch.cuda.graph(graphs[1]):
                self._dn_step(ent, *cond)
            with torch.cuda.graph(graphs[2]):
                out = self._dn_tail(ent)
            # the folded cross-attention the step graph reads in place (modules.Attention._fold keeps ONE entry per layer; another context would free it)
            folds = [m.__dict__.get("_fold_cache") for m in self.unet.modules() if "_fold_cache" in m.__dict__]
            ent["graphs"], ent["cond"], ent["out"], ent["alive"] = graphs, cond, out, (w0, folds)
            self._graphs[key] = ent
        if captured:
            g_head, g_step, g_tail = ent["graphs"]
            g_head.replay()
        else:
            cond = self._dn_head(ent)
        for i in range(n):
            st["t"].copy_(timesteps[i:i + 1])
            st["coef"].copy_(table[i])
            if captured:
                g_step.replay()
            else:
                self._dn_step(ent, *cond)
        if captured:
            g_tail.replay()
            out = ent["out"]
        else:
            out = self._dn_tail(ent)
        return out.clone() if isinstance(out, torch.Tensor) else tuple(o.clone() for o in out)

    def _dn_entry(self, rgb, B, kind, seed, img_embed, mode):
        """the static buffers and constants of one `_denoise` key.  Data only: an entry must not refer back to the pipeline (a closure over `self` would), or
        pipeline -> graph cache -> entry -> pipeline is a reference cycle, the graphs are then destroyed by the cyclic collector whenever it runs — and a graph
        destroyed in the middle of a LATER stream capture aborts the process."""
        device, dt = rgb.device, rgb.dtype
        _, C, h, w = self.encode_rgb(rgb).shape      # (the latent's shape; warms the encoder up as well)
        st = {"rgb": torch.empty_like(rgb), "embed": None if img_embed is None else torch.empty_like(img_embed),
              "noise": torch.empty((B, h, w, C), dtype=dt, device=device) if kind == "tensor" else None,
              "draw": torch.zeros(1, dtype=torch.int64, device=device), "t": torch.zeros(1, dtype=torch.int64, device=device),
              "coef": torch.zeros(2, dtype=torch.float32, device=device)}
        return {"static": st, "xin": torch.zeros((self._dn_copies * B, h, w, 2 * C), dtype=dt, device=device), "consts": self._dn_setup(B, dt, device, mode),
                "seed": seed, "kind": kind, "rows": B, "mode": dict(mode)}

    # the three pieces of `_denoise` over an entry: only device work on the current stream (capturable)
    def _dn_head(self, ent):
        from . import noise as N
        st, xin, B, kind = ent["static"], ent["xin"], ent["rows"], ent["kind"]
        C = xin.shape[-1] // 2
        lat = self.encode_rgb(st["rgb"]).permute(0, 2, 3, 1)
        for r in range(self._dn_copies):
            blk = xin[r * B:(r + 1) * B]
            if lat.shape[0] == B:
                ops.copy_scale(lat, blk[..., :C])
            else:                                   # ONE encoded image broadcast into the rows of an ensemble batch
                for j in range(B):
                    ops.copy_scale(lat, blk[j:j + 1, ..., :C])
        first = xin[:B, ..., C:]
        if kind == "zeros":
            xin[..., C:].zero_()
        else:
            if kind == "tensor":
                ops.copy_scale(st["noise"], first)
            else:
                N.randn_at(first, ent["seed"], st["draw"])
            for r in range(1, self._dn_copies):      # the SAME initial noise for every row block (geowizard_pipeline.py:271)
                ops.copy_scale(first, xin[r * B:(r + 1) * B, ..., C:])
        return self._dn_context(st["rgb"], st["embed"], ent["consts"], B)

    def _dn_step(self, ent, ctx, cls):
        xin = ent["xin"]
        v = self.unet(to_nchw_view(xin), ent["static"]["t"], encoder_hidden_states=ctx, class_labels=cls).sample
        ops.ddim_step_(xin[..., xin.shape[-1] // 2:], v.permute(0, 2, 3, 1), ent["static"]["coef"])

    def _dn_tail(self, ent):
        xin = ent["xin"]
        return self._dn_decode(xin[..., xin.shape[-1] // 2:].permute(0, 3, 1, 2), ent["rows"], ent["mode"])


class MarigoldPipeline(_LatentPipeline):
    def __init__(self, unet, vae, scheduler, text_encoder=None, tokenizer=None):
        super().__init__(unet, vae, scheduler)
        self.text_encoder, self.tokenizer = text_encoder, tokenizer
        self.empty_text_embed = None

    def to(self, *args, **kwargs):
        self.unet.to(*args, **kwargs)
        self.vae.to(*args, **kwargs)
        if self.text_encoder is not None:
            self.text_encoder.to(*args, **kwargs)
        if self.empty_text_embed is not None:
            self.empty_text_embed = self.empty_text_embed.to(*args, **kwargs)
        return self

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, unet=None, vae=None, scheduler=None, text_encoder=None, tokenizer=None,
                        variant=None, torch_dtype=None, **kw):
        """MarigoldPipeline.from_pretrained(ckpt, unet=..., vae=..., ...) (Marigold/run.py:274-282) on a diffusers-format directory
        (unet/, vae/, scheduler/, text_encoder/).  As in diffusers, components handed in are used as they are; `variant` and
        `torch_dtype` only shape the ones loaded here.  No tokenizer is needed (clip.empty_prompt_ids)."""
        import os
        from .clip import CLIPTextModel
        from .scheduler import DDIMScheduler
        from .unet import UNet2DConditionModel
        from .vae import AutoencoderKL
        root = pretrained_model_name_or_path
        if unet is None:
            unet = UNet2DConditionModel.from_pretrained(root, subfolder="unet", torch_dtype=torch_dtype, variant=variant)
        if vae is None:
            vae = AutoencoderKL.from_pretrained(root, subfolder="vae", torch_dtype=torch_dtype, variant=variant)
        if scheduler is None:
            scheduler = DDIMScheduler.from_pretrained(root, subfolder="scheduler")
        if text_encoder is None and os.path.isdir(os.path.join(root, "text_encoder")):
            text_encoder = CLIPTextModel.from_pretrained(root, subfolder="text_encoder", torch_dtype=torch_dtype, variant=variant)
        return cls(unet, vae, scheduler, text_encoder, tokenizer)

    def save_pretrained(self, save_directory, **kw):
        """diffusers layout: model_index.json + one sub-folder per component (training/train.py:612-630 saves the UNet this way)"""
        import json
        import os
        os.makedirs(save_directory, exist_ok=True)
        index = {"_class_name": "MarigoldPipeline"}
        for name in ("unet", "vae", "scheduler", "text_encoder"):
            comp = getattr(self, name)
            if comp is not None and hasattr(comp, "save_pretrained"):
                comp.save_pretrained(os.path.join(save_directory, name))
                index[name] = ["diffusion_e2e_ft_amd", type(comp).__name__]
        with open(os.path.join(save_directory, "model_index.json"), "w") as f:
            json.dump(index, f, indent=2)

    def enable_xformers_memory_efficient_attention(self):
        return None  # fused attention is the only path

    # ---- marigold_pipeline.py:356-369 ----
    def encode_empty_text(self):
        if self.text_encoder is None:
            raise RuntimeError("no text encoder: set pipe.empty_text_embed ([1, L, cross_attention_dim]) explicitly")
        if self.tokenizer is not None:
            ids = self.tokenizer("", padding="do_not_pad", max_length=self.tokenizer.model_max_length, truncation=True,
                                 return_tensors="pt").input_ids.to(self.device)
        else:   # the empty prompt is <|startoftext|><|endoftext|> in every CLIP vocabulary: no tokenizer files needed
            from .clip import empty_prompt_ids
            ids = empty_prompt_ids("do_not_pad").to(self.device)
        self.empty_text_embed = self.text_encoder(ids)[0].to(self.dtype)

    # ---- marigold_pipeline.py:501-519 ----
    @ops.device_scoped
    @torch.no_grad()
    def decode_depth(self, depth_latent):
        """the channel mean of the decoded image, NOT clipped (the reference clips in single_infer, :475-477)"""
        stacked = self._decode(depth_latent)
        return ops.depth_head(stacked.permute(0, 2, 3, 1), to_unit="mean")

    # ---- marigold_pipeline.py:522-538 ----
    @ops.device_scoped
    @torch.no_grad()
    def decode_normal(self, normal_latent):
        return self._decode(normal_latent)

    # ---- marigold_pipeline.py:372-478 ----
    @ops.device_scoped
    @torch.no_grad()
    def single_infer(self, rgb_in, num_inference_steps, show_pbar=False, noise="gaussian", normals=False, generator=None):
        device, dt = self.device, self.dtype
        rgb_in = rgb_in.to(device=device, dtype=dt)
        if isinstance(noise, str) and noise == "zeros" and num_inference_steps == 1:
            # E2E-FT path (x_t = 0, one step): no host synchronisation anywhere, optionally replayed from a captured hipGraph
            t_dev, sb, ctx = self._one_step()
            if self._graphs is None:
                return self._e2e_ft_zero_latent(rgb_in, t_dev, sb, ctx, normals)
            # the context is part of the key by IDENTITY (address + version; the entry keeps the tensor alive): the graph reads it in place and bakes what the
            # cross-attention layers derived from it (modules.Attention._fold) — a changed embedding is another graph, not a copy into a static buffer
            key = (tuple(rgb_in.shape), rgb_in.dtype, bool(normals), tuple(ctx.shape), float(sb), ctx.data_ptr(), ctx._version)
            return self._replay(key, (rgb_in, t_dev), ctx, lambda r, t: self._e2e_ft_zero_latent(r, t, sb, ctx, normals))
        if self._fused_denoise(num_inference_steps, noise, generator):
            return self._denoise(rgb_in, num_inference_steps, noise, generator, normals=normals)
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        rgb_latent = self.encode_rgb(rgb_in)  # [B,4,h,w] logical NCHW
        B, C = rgb_latent.shape[:2]
        xin = _unet_input(rgb_latent)
        # a DeviceNoise generator draws straight into channels 4:8 of the input buffer (noise.py): no host tensor, no copy; "zeros": they are zero already
        latent = _initial_latent(noise, generator, rgb_latent, "Unknown noise type: %s", dst=xin[..., C:])
        if latent is not None and not _device_noise(noise, generator):
            ops.copy_scale(latent.permute(0, 2, 3, 1).contiguous(), xin[..., C:])
        if self.empty_text_embed is None:
            self.encode_empty_text()
        ctx = self.empty_text_embed.to(device=device, dtype=dt).repeat(B, 1, 1)
        for i, (t, t_host) in enumerate(zip(self.scheduler.timesteps, self.scheduler.timesteps_host)):
            v = self.unet(to_nchw_view(xin), t, encoder_hidden_states=ctx).sample
            cur = latent if latent is not None else torch.zeros(tuple(rgb_latent.shape), dtype=dt, device=device)
            latent = self._ddim_step(v, t_host, cur, i == num_inference_steps - 1)
            ops.copy_scale(latent.permute(0, 2, 3, 1).contiguous(), xin[..., C:])
        return self._decode_head(latent, normals)

    # ---- the pieces `_denoise` asks its pipeline for ----
    def _dn_key(self, mode):
        if self.empty_text_embed is None:
            self.encode_empty_text()
        ctx = self._empty_ctx(self.device, self.dtype)      # by identity, as the one-step graphs key it (the step graph reads what is derived from it in place)
        return (bool(mode.get("normals", False)), tuple(ctx.shape), ctx.data_ptr(), ctx._version)

    def _dn_setup(self, B, dt, device, mode):
        if self.empty_text_embed is None:
            self.encode_empty_text()
        src = self._empty_ctx(device, dt)
        return {"src": src, "ctx": src.repeat(B, 1, 1)}                     # the context single_infer's host-driven loop hands to the UNet

    def _dn_context(self, rgb, embed, consts, B):
        return consts["ctx"], None

    def _dn_decode(self, x0, B, mode):
        return self._decode_head(x0, mode.get("normals", False))

    def _one_step(self):
        """(t_dev, sb, ctx) of the E2E-FT path: the one-step schedule and the empty-prompt context (encoded on first use)"""
        t_dev, sb = self._one_step_schedule()
        if self.empty_text_embed is None:
            self.encode_empty_text()
        return t_dev, sb, self._empty_ctx(self.device, self.dtype)

    def _decode_head(self, x0, normals):
        if normals:
            return ops.normal_head(self._decode(x0).permute(0, 2, 3, 1), clamp=False)
        return ops.depth_head(self._decode(x0).permute(0, 2, 3, 1), to_unit=True)   # clip(mean_c, -1, 1) -> (x+1)/2  (:518,476-477)

    def _zero_latent_x0(self, rgb_in, t_dev, sb, ctx1, marks=None):
        """encode -> UNet on [rgb latent | zeros] at t -> x0 = -sqrt(1 - abar_t) * v (marigold_pipeline.py:457-465, train.py:509-512).  Only device work on the
        current stream: safe inside a hipGraph capture.  marks: optional list that receives three recorded events (start, after encode, after UNet)."""
        _mark(marks)
        xin = _unet_input(self.encode_rgb(rgb_in))
        _mark(marks)
        v = self.unet(to_nchw_view(xin), t_dev, encoder_hidden_states=ctx1.expand(xin.shape[0], -1, -1)).sample
        x0 = _scaled(v, -sb)
        _mark(marks)
        return x0

    def _e2e_ft_zero_latent(self, rgb_in, t_dev, sb, ctx1, normals, marks=None):
        """_zero_latent_x0 -> decode -> head, capturable like it.  marks: optional list that receives four recorded events (start, after encode, after UNet,
        end) for stage timing."""
        out = self._decode_head(self._zero_latent_x0(rgb_in, t_dev, sb, ctx1, marks), normals)
        _mark(marks)
        return out

    @ops.device_scoped
    @torch.no_grad()
    def predict_latent(self, rgb_in):
        """the predicted x0 LATENT of the one-step zero-latent path ([B,4,h/8,w/8], logical NCHW): encode -> UNet at the scheduler's first timestep -> x0, i.e.
        `single_infer` without the decoder — the quantity BASELINE.json states parity on ("within 1e-3 relative fp32 on the depth/normal latent")"""
        return self._zero_latent_x0(rgb_in.to(device=self.device, dtype=self.dtype), *self._one_step())

    @ops.device_scoped
    @torch.no_grad()
    def stage_times_ms(self, rgb_in, normals=False, repeats=3):
        """{"vae_encode", "unet", "vae_decode"}: mean milliseconds per batch of the three stages of the E2E-FT path (HIP events on the
        launch stream; SURVEY.md §8(d) asks for the UNet-only rate next to the full path)."""
        rgb_in = rgb_in.to(device=self.device, dtype=self.dtype)
        t_dev, sb, ctx = self._one_step()
        tot = [0.0, 0.0, 0.0]
        for _ in range(repeats):
            marks = []
            self._e2e_ft_zero_latent(rgb_in, t_dev, sb, ctx, normals, marks=marks)
            torch.cuda.synchronize()
            for i in range(3):
                tot[i] += marks[i].elapsed_time(marks[i + 1])
        return dict(zip(("vae_encode", "unet", "vae_decode"), (v / repeats for v in tot)))

    def _empty_ctx(self, device, dt):
        """the empty-prompt embedding on `device` in `dt` as ONE stable tensor per (source tensor state, device, dtype): the UNet's cross-attention layers key their
        folded form on it (modules.Attention._fold) and a captured hipGraph reads it in place — a fresh `.to()` copy per call would rebuild both every call"""
        src = self.empty_text_embed
        if src.device == device and src.dtype == dt:
            return src
        key = (src.data_ptr(), src._version, str(device), dt)
        hit = self.__dict__.get("_ctx_dev")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_ctx_dev"] = (key, src.to(device=device, dtype=dt), src)      # (src kept alive: its address is part of the key)
        return hit[1]

    def _unit_range(self, rgb):
        return (rgb / 255.0 * 2.0 - 1.0).to(self.dtype)

    # ---- marigold_pipeline.py:158-353 ----
    @ops.device_scoped
    @torch.no_grad()
    def __call__(self, input_image, denoising_steps=10, ensemble_size=10, processing_res=768, match_input_res=True,
                 resample_method="bilinear", batch_size=0, color_map="Spectral", show_progress_bar=True, ensemble_kwargs=None,
                 noise="gaussian", normals=False, generator=None):
        """generator: a `torch.Generator` (host / torch RNG, as before) or a `noise.DeviceNoise` — then noise="gaussian" / "pyramid" is drawn on the device,
        once per ensemble batch, directly in the UNet's input buffer"""
        assert processing_res >= 0 and ensemble_size >= 1
        rgb = _image_chw(input_image)
        input_size = rgb.shape
        on_dev = resample_method == "bilinear" and self.device.type == "cuda"      # pre / post-processing on the device (csrc/prepost.hip)
        if on_dev:
            rgb = rgb.to(self.device)
        if processing_res > 0:
            rgb = resize_max_res(rgb, processing_res, resample_method)
        rgb_norm = self._unit_range(rgb)
        assert rgb_norm.min() >= -1.0 and rgb_norm.max() <= 1.0
        bs = batch_size if batch_size > 0 else find_batch_size(ensemble_size, max(rgb_norm.shape[1:]), self.dtype)   # :254-261
        preds = []
        if ensemble_size > 1 and self._fused_denoise(denoising_steps, noise, generator):
            # the members of a batch share ONE encode: the rgb latent is broadcast into the rows of the UNet input (the encoder is batch-invariant bit for bit)
            for s in range(0, ensemble_size, bs):
                preds.append(self._denoise(rgb_norm[None], denoising_steps, noise, generator, rows=min(bs, ensemble_size - s), normals=normals))
        else:
            dup = torch.stack([rgb_norm] * ensemble_size)
            for s in range(0, ensemble_size, bs):
                preds.append(self.single_infer(dup[s:s + bs], denoising_steps, show_progress_bar, noise=noise, normals=normals, generator=generator))
        preds = torch.cat(preds, dim=0).float().squeeze()
        if ensemble_size > 1:   # marigold_pipeline.py:293-297 (E2E-FT checkpoints are run with ensemble_size=1)
            from .ensemble import ensemble_depths, ensemble_normals
            pred, pred_uncert = ensemble_normals(preds) if normals else ensemble_depths(preds, **(ensemble_kwargs or {}))
        else:
            pred, pred_uncert = preds, None
        size = tuple(input_size[-2:]) if match_input_res else None
        if on_dev:        # predict_batch's tails on the one image; the clip is numpy's below, on the host as in the torch branch: no launch for it
            pred = (_post_normals(pred[None], size, "bilinear", renorm=True, clamp=False) if normals else _post_depth(pred, size, "bilinear", clamp=False))[0]
        else:
            if normals:
                pred = pred / (torch.norm(pred, p=2, dim=0, keepdim=True) + 1e-5)
            else:
                mn, mx = torch.min(pred), torch.max(pred)
                pred = torch.zeros_like(pred) if mx == mn else (pred - mn) / (mx - mn)
            if size is not None and tuple(pred.shape[-2:]) != size:
                p4 = pred[None] if normals else pred[None, None]
                p4 = torch.nn.functional.interpolate(p4, size=size, mode=resample_method, antialias=resample_method != "nearest",
                                                     **({} if resample_method == "nearest" else {"align_corners": False}))
                pred = p4[0] if normals else p4[0, 0]
        pred = pred.cpu().numpy()
        if not normals:
            pred = pred.clip(0, 1)
            colored = _to_pil(colorize_depth(pred, color_map)) if color_map is not None else None          # :326-336
            return MarigoldDepthOutput(depth_np=pred, depth_colored=colored, uncertainty=pred_uncert, normal_np=None, normal_colored=None)
        pred = pred.clip(-1.0, 1.0)
        colored = _to_pil(np.moveaxis((((pred + 1) / 2) * 255).astype(np.uint8), 0, -1))                     # :338-341
        return MarigoldDepthOutput(depth_np=None, depth_colored=None, uncertainty=pred_uncert, normal_np=pred, normal_colored=colored)

    @ops.device_scoped
    @torch.no_grad()
    def predict_batch(self, images, processing_res=768, match_input_res=True, resample_method="bilinear", normals=False, denoising_steps=1,
                      noise="zeros", generator=None):
        """`__call__` with ensemble_size = 1 for a whole batch, device tensors in and out (an addition to the reference's surface).
        images: uint8 [B,3,H,W] (host or device; moved to the pipeline's device once) or a list of PIL images of ONE size.  Returns fp32 depth [B,H',W'] in
        [0,1], or with normals=True fp32 normals [B,3,H',W'] in [-1,1]; H',W' is the input size when match_input_res, else the processing size (as single_infer
        returns it: the VAE keeps whole 8-pixel latents).
        The steps are `__call__`'s on the batch: resize_max_res when processing_res > 0, / 255 * 2 - 1, ONE single_infer on [B,...], then per image min-max to
        [0,1] (ops.minmax_unit_batched) — normals: pred / (|pred| + 1e-5) over the channels —, resize back, clip.  Every resample_method ("bilinear", "bicubic",
        "nearest") runs through resize_device(kind=...) on the device, before and after the model.  No host synchronisation with a device input and the
        default one-step zero-noise setting: no host read of a tensor value (uint8 input cannot leave [-1,1], so `__call__`'s range assert has nothing to
        check), no .cpu().  There is no ensemble_size: ensembling stays with `__call__`."""
        if processing_res < 0:
            raise ValueError("processing_res must be >= 0, got %s" % (processing_res,))
        if resample_method not in ("bilinear", "bicubic", "nearest"):
            raise ValueError("Unknown resampling method: %s" % resample_method)
        rgb = _uint8_batch(images, self.device)
        size = tuple(rgb.shape[-2:]) if match_input_res else None
        if processing_res > 0:
            rgb = _resize_max_res_batch(rgb, processing_res, resample_method)
        pred = self.single_infer(self._unit_range(rgb), denoising_steps, False, noise=noise, normals=normals, generator=generator)
        return _post_normals(pred, size, resample_method, renorm=True) if normals else _post_depth(pred, size, resample_method)


def _image_chw(input_image):
    """`__call__`'s input_image, a tensor ([3,H,W] once squeezed) or a PIL image -> [3,H,W] in 0..255 (uint8 from PIL)"""
    if isinstance(input_image, torch.Tensor):
        rgb = input_image.squeeze()
    else:  # PIL image
        rgb = torch.from_numpy(np.asarray(input_image.convert("RGB"))).permute(2, 0, 1)
    assert rgb.dim() == 3 and rgb.shape[0] == 3, "Wrong input shape %s, expected [rgb, H, W]" % (tuple(rgb.shape),)
    return rgb


def _post_depth(depth, size, kind, clamp=True):
    """predictions [.., h, w] of B images -> fp32 [B,H,W]: per image min-max to [0,1] (ops.minmax_unit_batched: zeros where an image is constant), resize back
    to `size` (None: keep) through resize_device(kind=...), clamp (left out for a caller that clips on the host).  No host synchronisation."""
    h, w = depth.shape[-2:]
    depth = ops.minmax_unit_batched(depth.float().reshape(-1, h, w).contiguous())
    if size is not None and (h, w) != tuple(size):
        depth = resize_device(depth, size, kind=kind)
    return depth.clamp(0.0, 1.0) if clamp else depth


def _post_normals(normal, size, kind, renorm, clamp=True):
    """normals [B,3,h,w] -> fp32 [B,3,H,W]: renorm: pred / (|pred| + 1e-5) over the channels; resize back to `size` (None: keep) through
    resize_device(kind=...), clamp (left out for a caller that clips on the host).  No host synchronisation."""
    normal = normal.float()
    if renorm:
        normal = normal / (torch.norm(normal, p=2, dim=1, keepdim=True) + 1e-5)
    h, w = normal.shape[-2:]
    if size is not None and (h, w) != tuple(size):
        normal = resize_device(normal.reshape(-1, h, w), size, kind=kind).reshape(normal.shape[:-2] + tuple(size))
    return normal.clamp(-1.0, 1.0).contiguous() if clamp else normal


def _mark(marks):
    if marks is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append(e)


def _unet_input(rgb_latent, copies=1):
    """UNet input buffer [copies * B,h,w,2C] NHWC from the rgb latent [B,C,h,w]: channels 0:C the rgb latent in each of the `copies` row blocks (GeoWizard: a
    depth block and a normal block), C:2C the current latent, zero here ("this order is important", marigold_pipeline.py:447-449)"""
    B, C, h, w = rgb_latent.shape
    xin = torch.zeros((copies * B, h, w, 2 * C), dtype=rgb_latent.dtype, device=rgb_latent.device)
    for r in range(copies):
        ops.copy_scale(rgb_latent.permute(0, 2, 3, 1), xin[r * B:(r + 1) * B, ..., :C])
    return xin


def _initial_latent(noise, generator, rgb_latent, unknown, dst=None):
    """the initial latent [B,C,h,w] that `noise` names, None for "zeros".  A DeviceNoise generator (noise.py) draws into `dst`, an NHWC [B,h,w,C] view (a
    fresh buffer when None), and the result is its NCHW view; every other draw is torch's.  unknown: the caller's error text for any other `noise`."""
    if isinstance(noise, torch.Tensor):          # an explicit initial latent [B,4,h,w] (tests, reproducibility across devices)
        return noise.to(device=rgb_latent.device, dtype=rgb_latent.dtype)
    B, C, h, w = rgb_latent.shape
    if _device_noise(noise, generator):
        from . import noise as N
        if dst is None:
            dst = torch.empty((B, h, w, C), dtype=rgb_latent.dtype, device=rgb_latent.device)
        return to_nchw_view(N.noise_into(noise, dst, generator))
    if noise == "gaussian":
        return torch.randn((B, C, h, w), device=rgb_latent.device, dtype=rgb_latent.dtype, generator=generator)
    if noise == "pyramid":
        return pyramid_noise_like(rgb_latent)
    if noise == "zeros":
        return None
    raise ValueError(unknown % noise)


def _uint8_batch(images, device):
    """predict_batch's input -> uint8 [B,3,H,W] on `device`: a uint8 [B,3,H,W] tensor (one .to), or a list of PIL images of one size (stacked on the host, one copy)"""
    if isinstance(images, torch.Tensor):
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3 or images.shape[0] == 0:
            raise ValueError("predict_batch: expected a uint8 [B,3,H,W] tensor, got %s %s" % (images.dtype, tuple(images.shape)))
        return images.to(device).contiguous()
    arrays = [np.asarray(im.convert("RGB")) for im in images]
    if not arrays:
        raise ValueError("predict_batch: no images")
    sizes = [a.shape[:2] for a in arrays]
    if len(set(sizes)) != 1:
        raise ValueError("predict_batch: the images of a batch must have one size, got (H, W) = %s" % ", ".join(str(s) for s in sorted(set(sizes))))
    return torch.from_numpy(np.ascontiguousarray(np.stack(arrays).transpose(0, 3, 1, 2))).to(device)


def _resize_max_res_batch(rgb, max_edge_resolution, resample_method="bilinear"):
    """resize_max_res for a uint8 [B,3,H,W] device batch: the B * 3 planes in one call of the table-driven resampler, rounded back to uint8 as
    torchvision does for an integer image"""
    B, C, H, W = rgb.shape
    f = min(max_edge_resolution / W, max_edge_resolution / H)
    nw, nh = int(W * f), int(H * f)
    return resize_device(rgb.reshape(B * C, H, W), (nh, nw), round_u8=True, kind=resample_method).to(rgb.dtype).reshape(B, C, nh, nw)


def _device_noise(noise, generator):
    """noise="gaussian" / "pyramid" with a noise.DeviceNoise generator: drawn on the device.  Any other generator (None, a torch.Generator) keeps torch's path."""
    from .noise import DeviceNoise
    return isinstance(noise, str) and noise in ("gaussian", "pyramid") and isinstance(generator, DeviceNoise)


def find_batch_size(ensemble_size, input_res, dtype):
    """Marigold/marigold/util/batchsize.py:26-81 for this GPU: the reference looks its inference batch size up in a table measured on 10-80 GB
    cards; 288 GB of HBM3E holds any ensemble the pipeline is run with (activations are ~1.3 GB per 768x768 fp16 image), so the table has
    one row per resolution class and the reference's rounding rule is kept (a batch larger than half the ensemble but smaller than
    it is cut to ceil(ensemble / 2) so that the two passes are balanced)."""
    import math
    table = [(512, 128, 64), (768, 64, 32), (1024, 32, 16), (1 << 30, 8, 4)]        # (max resolution, fp16/bf16 images, fp32 images)
    for res, bs16, bs32 in table:
        if input_res <= res:
            bs = bs32 if dtype == torch.float32 else bs16
            break
    if bs > ensemble_size:
        bs = ensemble_size
    elif bs > math.ceil(ensemble_size / 2) and bs < ensemble_size:
        bs = math.ceil(ensemble_size / 2)
    return bs


def colorize_depth(depth, cmap="Spectral"):
    """[H,W] depth in [0,1] -> uint8 [H,W,3] through a matplotlib colour map (what marigold_pipeline.py:326-334 hands to PIL)"""
    import matplotlib
    rgba = matplotlib.colormaps[cmap](np.clip(depth, 0.0, 1.0), bytes=False)
    return (rgba[..., :3] * 255).astype(np.uint8)


def _to_pil(hwc_uint8):
    from PIL import Image
    return Image.fromarray(hwc_uint8)


def _scaled(x, mul):
    """y = x * mul for a logical-NCHW tensor, computed by libe2eft into NHWC storage; returns a logical-NCHW view."""
    xv = x.permute(0, 2, 3, 1)
    try:
        ops._nhwc_ld(xv)
    except ValueError:
        xv = xv.contiguous()
    out = torch.empty(xv.shape, dtype=x.dtype, device=x.device)
    ops.copy_scale(xv, out, mul=mul)
    return out.permute(0, 3, 1, 2)


_AA_TABLES = {}       # (in, out, kind, device) -> device tables: a handful of shapes per process; cached so that a hipGraph capture (whose eager warm-up pass fills
                       # this like the packed-weight caches) contains no host -> device copy


def aa_tables(in_size, out_size, device, kind="bilinear"):
    key = (int(in_size), int(out_size), kind, str(device))
    hit = _AA_TABLES.get(key)
    if hit is None:
        if len(_AA_TABLES) > 256:
            _AA_TABLES.clear()
        hit = _AA_TABLES[key] = _aa_tables(in_size, out_size, device, kind)
    return hit


def cv2_nearest_indices(in_size, out_size):
    """cv2.resize(..., interpolation=INTER_NEAREST) along one dimension (geowizard_pipeline.py:205; OpenCV imgproc/resize.cpp `resizeNN`): the scale is formed in
    DOUBLE as fx = out / in, ifx = 1 / fx, and output i reads min(floor(i * ifx), in - 1).  (torch's "nearest" forms in / out in float32: for non-dyadic ratios the
    two differ by one source pixel at exact-boundary positions, so the device path and the host path both use THIS table.)  -> int32 [out]"""
    ifx = 1.0 / (float(out_size) / float(in_size))
    return np.minimum(np.floor(np.arange(out_size, dtype=np.float64) * ifx).astype(np.int64), in_size - 1).astype(np.int32)


def _aa_tables(in_size, out_size, device, kind="bilinear"):
    """aten `_compute_indices_min_size_weights_aa` (UpSampleKernel.cpp), align_corners = False, in aten's float32 arithmetic: (bounds int32 [out, 2] = (first tap,
    tap count), weights fp32 [out, ksize]) — what `F.interpolate(mode=kind, antialias=True)` applies along one dimension.  kind "bilinear": the triangle filter
    (support 1); "bicubic": Keys' cubic with a = -0.5 (support 2) — aten's antialiased bicubic is Pillow's resize (`Image.resize` of a float image, default
    BICUBIC: the resize-back of GeoWizard's `__call__`, geowizard_pipeline.py:201-203) and torchvision's `resize(..., BICUBIC, antialias=True)` (the CLIP image
    preprocessing, geowizard_pipeline.py:236-245); "nearest": one tap at cv2.INTER_NEAREST's source index (`cv2_nearest_indices`, geowizard_pipeline.py:205).
    Built on the host (a few hundred numbers), consumed by e2eft_resample_bilinear_aa (a separable table-driven resampler: the filter lives in the table)."""
    f32 = np.float32
    scale = f32(in_size) / f32(out_size)
    if kind == "nearest":
        idx = cv2_nearest_indices(in_size, out_size)
        bounds = np.stack([idx, np.ones_like(idx)], axis=1).astype(np.int32)
        return torch.from_numpy(bounds).to(device), torch.ones((out_size, 1), dtype=torch.float32, device=device)
    base = {"bilinear": f32(1.0), "bicubic": f32(2.0)}[kind]

    def filt(x):
        x = np.abs(x)
        if kind == "bilinear":
            return np.maximum(f32(0.0), f32(1.0) - x).astype(np.float32)
        a = f32(-0.5)
        near = ((a + f32(2.0)) * x - (a + f32(3.0))) * x * x + f32(1.0)
        far = (((x - f32(5.0)) * x + f32(8.0)) * x - f32(4.0)) * a
        return np.where(x < 1.0, near, np.where(x < 2.0, far, f32(0.0))).astype(np.float32)

    support = f32(base * scale) if scale >= 1.0 else base
    invscale = f32(1.0) / scale if scale >= 1.0 else f32(1.0)
    ksize = int(np.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    weights = np.zeros((out_size, ksize), dtype=np.float32)
    for i in range(out_size):
        center = scale * f32(i + 0.5)
        xmin = max(int(center - support + f32(0.5)), 0)
        xsize = min(int(center + support + f32(0.5)), in_size) - xmin
        j = np.arange(xsize, dtype=np.float32)
        wv = filt((j + f32(xmin) - center + f32(0.5)) * invscale)
        tot = f32(0.0)
        for v in wv:                       # aten sums sequentially in float32
            tot = f32(tot + v)
        if tot != 0:
            wv = (wv / tot).astype(np.float32)
        bounds[i] = (xmin, xsize)
        weights[i, :xsize] = wv
    return torch.from_numpy(bounds).to(device), torch.from_numpy(weights).to(device)


def aa_bilinear_tables(in_size, out_size, device):
    return aa_tables(in_size, out_size, device, "bilinear")


def resize_device(img, size, round_u8=False, mul=1.0, add=0.0, kind="bilinear"):
    """antialiased bilinear (default) / antialiased bicubic / nearest resize of a planar [P,H,W] device tensor (uint8 or fp32) by libe2eft (csrc/prepost.hip)
    -> fp32 [P,h,w]"""
    H, W = img.shape[-2:]
    h, w = size
    x = img.contiguous() if img.dtype == torch.uint8 else img.float().contiguous()
    return ops.resample_bilinear_aa(x, (h, w), aa_tables(W, w, img.device, kind), aa_tables(H, h, img.device, kind), round_u8=round_u8, mul=mul, add=add)


def resize_max_res(img, max_edge_resolution, resample_method="bilinear"):
    """Marigold/marigold/util/image_util.py:79-108 — keep aspect ratio, longer edge = max_edge_resolution.  A device tensor is resized by the
    library's antialiased-bilinear kernels, a host tensor by torch (the reference's own path)."""
    assert img.dim() == 3
    H, W = img.shape[-2:]
    f = min(max_edge_resolution / W, max_edge_resolution / H)
    nw, nh = int(W * f), int(H * f)
    if img.is_cuda and resample_method == "bilinear":
        out = resize_device(img, (nh, nw), round_u8=not img.is_floating_point())
        return out if img.is_floating_point() else out.to(img.dtype)
    kw = {} if resample_method == "nearest" else {"align_corners": False}
    out = torch.nn.functional.interpolate(img[None].float(), size=(nh, nw), mode=resample_method,
                                          antialias=resample_method != "nearest", **kw)[0]
    if not img.is_floating_point():       # torchvision resizes integer images in float and rounds back (uint8 from pil_to_tensor, :227)
        out = out.round().clamp(0, 255).to(img.dtype)
    return out


def pyramid_noise_like(x, discount=0.9):
    """Multi-resolution noise for the non-default `noise="pyramid"` setting (training/util/noise.py:8-18, marigold_pipeline.py:76-86): white
    noise plus bilinearly upsampled white noise of successively (cumulatively) shrunk grids, weighted discount^level, rescaled to unit
    std.  Host RNG; draws `random.random()` and `torch.randn` in the reference's order (tests/test_host_logic.py pins it to the
    reference's function)."""
    import random
    n, ch, rows, cols = x.shape
    upsample = torch.nn.Upsample(size=(rows, cols), mode="bilinear")
    total = torch.randn_like(x)
    for level in range(10):
        shrink = (random.random() * 2 + 2) ** level
        rows, cols = max(1, int(rows / shrink)), max(1, int(cols / shrink))
        total += upsample(torch.randn(n, ch, rows, cols).to(x)) * discount ** level
        if rows == 1 or cols == 1:
            break
    return total / total.std()


class DepthNormalEstimationPipeline(_LatentPipeline):
    """GeoWizard joint depth + normal single-step inference, batched (rows [depth x B ; normal x B]) as in
    GeoWizard/geowizard/training/train_depth_normal.py:687-704; per-image semantics of geowizard_pipeline.py:252-344.
    `image_encoder` (clip.CLIPVisionModelWithProjection, geowizard_pipeline.py:76-86) is optional: without it pass `img_embed`
    [B,1,X] to single_infer directly."""

    def __init__(self, unet, vae, scheduler, image_encoder=None, feature_extractor=None):
        super().__init__(unet, vae, scheduler)
        self.image_encoder, self.feature_extractor = image_encoder, feature_extractor
        self.img_embed = None                      # geowizard_pipeline.py:86

    def _clip_constants(self):
        """(size, mean [3,1,1], std [3,1,1]) of the CLIP preprocessor, resident on the device (no host->device copy per image)"""
        from .clip import CLIP_IMAGE_MEAN, CLIP_IMAGE_STD
        fe = self.feature_extractor
        key = (str(self.device), id(fe))
        if getattr(self, "_clip_key", None) != key:
            mean = tuple(fe.image_mean) if fe is not None else CLIP_IMAGE_MEAN
            std = tuple(fe.image_std) if fe is not None else CLIP_IMAGE_STD
            size = fe.crop_size["height"] if fe is not None else self.image_encoder.config["image_size"]
            self._clip_const = (size, torch.tensor(mean, device=self.device, dtype=torch.float32)[:, None, None],
                                torch.tensor(std, device=self.device, dtype=torch.float32)[:, None, None])
            self._clip_key = key
        return self._clip_const

    @ops.device_scoped
    @torch.no_grad()
    def encode_img_embed(self, rgb):
        """geowizard_pipeline.py:232-248 (__encode_img_embed): CLIP image embedding [B,1,X] of rgb in [-1,1]; resize + normalisation
        constants come from `feature_extractor` when one is given (image_mean / image_std / crop_size), else CLIP's defaults."""
        from .clip import preprocess_for_clip
        assert self.image_encoder is not None, "DepthNormalEstimationPipeline was built without an image_encoder: pass img_embed"
        size, mean, std = self._clip_constants()
        x = preprocess_for_clip(rgb.to(device=self.device, dtype=self.dtype), size, mean, std)
        return self.image_encoder(x).image_embeds.unsqueeze(1).to(self.dtype)

    @staticmethod
    def class_embedding(batch, domain, dtype, device):
        geo = torch.tensor([[0.0, 1.0], [1.0, 0.0]], dtype=torch.float32).repeat_interleave(batch, 0)
        dom = {"indoor": [1.0, 0.0, 0.0], "outdoor": [0.0, 1.0, 0.0], "object": [0.0, 0.0, 1.0]}[domain]
        dom = torch.tensor([dom], dtype=torch.float32).repeat(2 * batch, 1)
        emb = torch.cat([torch.sin(geo), torch.cos(geo), torch.sin(dom), torch.cos(dom)], dim=-1)  # 10 constants, host
        return emb.to(device=device, dtype=dtype)

    def _unit_range(self, rgb):
        return (rgb.float() / 255.0 * 2.0 - 1.0).clamp(-1.0, 1.0).to(self.dtype)

    def _decode_heads(self, geo, B):
        """joint latent [depth x B ; normal x B] -> (depth [B,1,H,W] in [0,1], unit normals [B,3,H,W], sign flipped: geowizard_pipeline.py:341-342)"""
        depth = ops.depth_head(self._decode(geo[:B]).permute(0, 2, 3, 1), to_unit=True)
        normal = ops.normal_head(self._decode(geo[B:]).permute(0, 2, 3, 1), clamp=False, sign=-1.0)
        return depth, normal

    # ---- the pieces `_denoise` asks its pipeline for ----
    _dn_copies = 2

    def _dn_key(self, mode):
        return (mode.get("domain", "indoor"),)

    def _dn_setup(self, B, dt, device, mode):
        return {"cls": self.class_embedding(B, mode.get("domain", "indoor"), dt, device)}

    def _dn_context(self, rgb, embed, consts, B):
        e = self.encode_img_embed(rgb) if embed is None else embed
        if e.shape[0] != B:                                   # one encoded image broadcast over the rows of an ensemble batch
            e = e.repeat(B, 1, 1)
        return e.to(rgb.dtype).repeat(2, 1, 1), consts["cls"]

    def _dn_decode(self, x0, B, mode):
        return self._decode_heads(x0, B)

    def _device_path(self, rgb, img_embed, t_dev, sb, cls):
        """everything after the host-side setup; only device work on the current stream (capturable)"""
        if img_embed is None:
            img_embed = self.encode_img_embed(rgb)
        B = rgb.shape[0]
        xin = _unet_input(self.encode_rgb(rgb), copies=2)      # geo latent half stays zero
        ctx = img_embed.to(rgb.dtype).repeat(2, 1, 1)
        v = self.unet(to_nchw_view(xin), t_dev.repeat(2 * B), encoder_hidden_states=ctx, class_labels=cls).sample
        return self._decode_heads(_scaled(v, -sb), B)

    @torch.no_grad()
    def _multi_step(self, rgb, img_embed, cls, num_inference_steps, noise, generator):
        """geowizard_pipeline.py:266-343 for the pre-E2E-FT checkpoints: DDIM over the joint geometry latent (the SAME initial noise for
        the depth and the normal row of an image, :271), host launches only."""
        B = rgb.shape[0]
        if img_embed is None:
            img_embed = self.encode_img_embed(rgb)
        self.scheduler.set_timesteps(num_inference_steps, device=rgb.device)
        rgb_latent = self.encode_rgb(rgb)
        C = rgb_latent.shape[1]
        geo = _initial_latent(noise, generator, rgb_latent, "Invalid noise type: %s")
        if geo is None:
            geo = torch.zeros(tuple(rgb_latent.shape), device=rgb.device, dtype=rgb.dtype)
        geo = geo.repeat(2, 1, 1, 1)
        xin = _unet_input(rgb_latent, copies=2)
        ctx = img_embed.to(rgb.dtype).repeat(2, 1, 1)
        for i, (t, t_host) in enumerate(zip(self.scheduler.timesteps, self.scheduler.timesteps_host)):
            ops.copy_scale(geo.permute(0, 2, 3, 1).contiguous(), xin[..., C:])
            v = self.unet(to_nchw_view(xin), t.repeat(2 * B), encoder_hidden_states=ctx, class_labels=cls).sample
            geo = self._ddim_step(v, t_host, geo, i == num_inference_steps - 1)
        return self._decode_heads(geo, B)

    @ops.device_scoped
    @torch.no_grad()
    def single_infer(self, input_rgb, num_inference_steps=1, domain="indoor", show_pbar=False, noise="zeros", img_embed=None, generator=None):
        """Positional order of the reference (geowizard_pipeline.py:252-258: input_rgb, num_inference_steps, domain, show_pbar, noise).
        The CLIP embedding [B,1,X] comes from `img_embed=`, else from `self.img_embed` when a caller has set it as the reference's
        `__call__` does (:222,283-284), else from the image encoder.  Defaults are the E2E-FT setting (one step, zeros)."""
        if isinstance(num_inference_steps, torch.Tensor):        # older call form single_infer(rgb, img_embed[, domain])
            img_embed, num_inference_steps = num_inference_steps, 1
        if img_embed is None:
            img_embed = self.img_embed
        device, dt = self.device, self.dtype
        rgb = input_rgb.to(device=device, dtype=dt)
        B = rgb.shape[0]
        if num_inference_steps != 1 or isinstance(noise, torch.Tensor) or noise != "zeros":
            if self._fused_denoise(num_inference_steps, noise, generator):
                return self._denoise(rgb, num_inference_steps, noise, generator, img_embed=img_embed, domain=domain)
            cls = self.class_embedding(B, domain, dt, device)
            return self._multi_step(rgb, None if img_embed is None else img_embed.to(device=device, dtype=dt), cls, num_inference_steps, noise, generator)
        t_dev, sb = self._one_step_schedule()
        ck = (B, domain, dt, str(device))
        if getattr(self, "_cls_key", None) != ck:
            self._cls, self._cls_key = self.class_embedding(B, domain, dt, device), ck
        cls = self._cls
        if img_embed is not None:
            img_embed = img_embed.to(device=device, dtype=dt)
        if self._graphs is None:
            return self._device_path(rgb, img_embed, t_dev, sb, cls)
        # the class embedding is a function of key fields (batch, domain, dtype); the graph reads it in place, so the entry keeps it alive
        key = (tuple(rgb.shape), dt, domain, None if img_embed is None else tuple(img_embed.shape), float(sb))
        return self._replay(key, (rgb, img_embed, t_dev), cls, lambda r, e, t: self._device_path(r, e, t, sb, cls))

    # ---- geowizard_pipeline.py:88-230 ----
    @ops.device_scoped
    @torch.no_grad()
    def __call__(self, input_image, denoising_steps=1, ensemble_size=1, processing_res=768, match_input_res=True, batch_size=0,
                 domain="indoor", color_map="Spectral", show_progress_bar=False, ensemble_kwargs=None, noise="zeros"):
        """Host orchestration of the joint prediction: resize -> [-1,1] -> `ensemble_size` passes -> depth / normal ensembling ->
        min-max -> resize back.  Defaults are the E2E-FT setting (denoising_steps = 1, noise = "zeros": every pass identical, ensembling
        is a no-op); the reference's own defaults for the original checkpoints are 10 steps, 10 members, gaussian noise.  Resampling runs in torch (the reference goes
        through PIL / cv2 on the host: bicubic for depth, nearest for normals) and the colourised images are left to the caller."""
        assert processing_res >= 0 and ensemble_size >= 1 and denoising_steps >= 1
        rgb = _image_chw(input_image)
        size = tuple(rgb.shape[-2:]) if match_input_res else None
        rgb = rgb.to(self.device)
        if processing_res > 0:
            rgb = resize_max_res(rgb, processing_res)
        rgb_norm = self._unit_range(rgb)
        bs = batch_size if batch_size > 0 else 1
        fused = ensemble_size > 1 and self._fused_denoise(denoising_steps, noise, None)
        dup = None if fused else torch.stack([rgb_norm] * ensemble_size)
        depths, normals = [], []
        for s0 in range(0, ensemble_size, bs):
            if fused:      # the members of a batch share ONE encode (MarigoldPipeline.__call__)
                d, n = self._denoise(rgb_norm[None], denoising_steps, noise, rows=min(bs, ensemble_size - s0), img_embed=self.img_embed, domain=domain)
            else:
                d, n = self.single_infer(dup[s0:s0 + bs], domain=domain, num_inference_steps=denoising_steps, noise=noise)
            depths.append(d)
            normals.append(n)
        depth_preds = torch.cat(depths, 0).float().squeeze(1)         # [N, H, W]
        normal_preds = torch.cat(normals, 0).float()                  # [N, 3, H, W]
        uncert = None
        if ensemble_size > 1:
            from .ensemble import ensemble_depths, ensemble_normals
            depth_pred, uncert = ensemble_depths(depth_preds, **(ensemble_kwargs or {}))
            normal_pred = ensemble_normals(normal_preds)[0]
        else:
            depth_pred, normal_pred = depth_preds[0], normal_preds[0]
        # geowizard_pipeline.py:201-205: Pillow's resize of the float depth (default BICUBIC = the antialiased Keys cubic, a = -0.5) and cv2.INTER_NEAREST for
        # the normals — through the table-driven resampler of csrc/prepost.hip.  The predictions are device tensors: single_infer moves its input to the
        # device and every libe2eft op refuses host tensors (ops._check_cuda), the ensembling ones included
        depth_pred = _post_depth(depth_pred, size, "bicubic")[0]
        normal_pred = _post_normals(normal_pred[None], size, "nearest", renorm=False)[0]
        if match_input_res:
            normal_pred = normal_pred.permute(1, 2, 0).contiguous()      # the reference returns HWC normals after its cv2 resize (:205)
        return DepthNormalPipelineOutput(depth_np=depth_pred.cpu().numpy().astype(np.float32), depth_colored=None,
                                         normal_np=normal_pred.cpu().numpy().astype(np.float32), normal_colored=None, uncertainty=uncert)

    @ops.device_scoped
    @torch.no_grad()
    def predict_batch(self, images, processing_res=768, match_input_res=True, domain="indoor", denoising_steps=1, noise="zeros"):
        """`__call__` with ensemble_size = 1 for a whole batch, device tensors in and out (an addition to the reference's surface).
        images: uint8 [B,3,H,W] (host or device; moved to the pipeline's device once) or a list of PIL images of ONE size.  Returns (depth fp32 [B,H',W'] in
        [0,1], normals fp32 [B,3,H',W'] in [-1,1]); H',W' is the input size when match_input_res, else the processing size.  The normals are PLANAR here,
        as MarigoldPipeline.predict_batch returns them — `__call__` returns them HWC when match_input_res is set, as the reference does.
        The steps are `__call__`'s on the batch: resize_max_res when processing_res > 0, / 255 * 2 - 1, ONE single_infer on [B,...] (2 * B UNet rows), per image
        min-max of the depth (ops.minmax_unit_batched), bicubic resize back for the depth and nearest for the normals, clamps.  The CLIP embedding is
        `self.img_embed` ([B,1,X]) when set, else the image encoder's for the batch.  No host synchronisation with a device input and the default one-step
        zero-noise setting.  There is no ensemble_size: ensembling stays with `__call__`."""
        if processing_res < 0 or denoising_steps < 1:
            raise ValueError("processing_res must be >= 0 and denoising_steps >= 1, got %s, %s" % (processing_res, denoising_steps))
        rgb = _uint8_batch(images, self.device)
        size = tuple(rgb.shape[-2:]) if match_input_res else None
        if processing_res > 0:
            rgb = _resize_max_res_batch(rgb, processing_res)
        d, n = self.single_infer(self._unit_range(rgb), domain=domain, num_inference_steps=denoising_steps, noise=noise)
        return _post_depth(d, size, "bicubic"), _post_normals(n, size, "nearest", renorm=False)
