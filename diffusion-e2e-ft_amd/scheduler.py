"""DDIM scheduler surface used by the pipelines (diffusers DDIMScheduler semantics; scaled_linear betas,
v_prediction, trailing spacing — Marigold/run.py:157-162, training/train.py:509-518,613-617)."""
import numpy as np
import torch

from .unet import Config


class SchedulerOutput:
    def __init__(self, prev_sample, pred_original_sample):
        self.prev_sample = prev_sample
        self.pred_original_sample = pred_original_sample


class DDIMScheduler:
    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 prediction_type="v_prediction", timestep_spacing="trailing", steps_offset=1, clip_sample=False,
                 set_alpha_to_one=False, thresholding=False):
        if beta_schedule != "scaled_linear":
            raise NotImplementedError(beta_schedule)
        self.config = Config(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                             beta_schedule=beta_schedule, prediction_type=prediction_type, timestep_spacing=timestep_spacing,
                             steps_offset=steps_offset, clip_sample=clip_sample, set_alpha_to_one=set_alpha_to_one,
                             thresholding=thresholding)
        self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))

    config_name = "scheduler_config.json"

    @classmethod
    def from_pretrained(cls, path, subfolder=None, **overrides):
        """DDIMScheduler.from_pretrained(ckpt, timestep_spacing=..., subfolder="scheduler") (Marigold/run.py:272): diffusers'
        scheduler_config.json, keyword overrides win, unknown keys (trained_betas, rescale_betas_zero_snr, ...) are ignored"""
        import inspect
        import json
        import os
        d = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(d, cls.config_name)) as f:
            cfg = json.load(f)
        cfg.update(overrides)
        known = set(inspect.signature(cls.__init__).parameters) - {"self"}
        return cls(**{k: v for k, v in cfg.items() if k in known})

    def save_pretrained(self, save_directory, **kw):
        import json
        import os
        os.makedirs(save_directory, exist_ok=True)
        cfg = dict(self.config)
        cfg["_class_name"] = type(self).__name__
        with open(os.path.join(save_directory, self.config_name), "w") as f:
            json.dump(cfg, f, indent=2)

    def _spaced(self, n):
        """the n timesteps of the configured spacing, descending (a float numpy array of whole numbers)"""
        T = self.config.num_train_timesteps
        sp = self.config.timestep_spacing
        if sp == "trailing":
            return np.round(np.arange(T, 0, -T / n)) - 1
        if sp == "leading":
            return (np.arange(0, n) * (T // n)).round()[::-1].copy() + self.config.steps_offset
        if sp == "linspace":
            return np.linspace(0, T - 1, n).round()[::-1].copy()
        raise ValueError(sp)

    def set_timesteps(self, num_inference_steps, device=None):
        n = num_inference_steps
        self.num_inference_steps = n
        ts = self._spaced(n)
        self.timesteps_host = [int(v) for v in ts]           # host copy: reading a timestep must not synchronise with the device
        key = (tuple(self.timesteps_host), str(device))
        if getattr(self, "_ts_key", None) != key:            # same schedule as last call: keep the device tensor (no H2D per image)
            self.timesteps = torch.from_numpy(ts.astype(np.int64)).to(device)
            self._ts_key = key

    def x0_coefficients(self, t):
        """(sqrt(abar_t), sqrt(1 - abar_t)) as python floats computed in fp32 like the reference (train.py:509-512)."""
        ac = self.alphas_cumprod[int(t)]
        return float(ac ** 0.5), float((1 - ac) ** 0.5)

    def zero_latent_x0_scale(self, t):
        """c with x0 = c * model_output when x_t = 0 (the E2E-FT recipe, training/train.py:480-518): the scheduler's own
        `prediction_type` decides — v_prediction -sqrt(1 - abar_t), epsilon -sqrt(1 - abar_t) / sqrt(abar_t), sample 1 — as in step().
        clip_sample / thresholding configurations are refused rather than silently ignored by the fused single-step paths."""
        if self.config.clip_sample or self.config.thresholding:
            raise NotImplementedError("the fused single-step path does not clip / threshold x0 (scheduler config clip_sample=%s, thresholding=%s)"
                                      % (self.config.clip_sample, self.config.thresholding))
        sa, sb = self.x0_coefficients(t)
        pt = self.config.prediction_type
        if pt == "v_prediction":
            return -sb
        if pt == "epsilon":
            return -sb / sa
        if pt == "sample":
            return 1.0
        raise ValueError("Unknown prediction type %s" % pt)

    def x0_coefficients_for(self, t):
        """(c_x, c_v) with x0 = c_x * x_t + c_v * model_output for ANY x_t (training/train.py:509-518, as in step()): v_prediction
        (sqrt(abar_t), -sqrt(1 - abar_t)), epsilon (1 / sqrt(abar_t), -sqrt(1 - abar_t) / sqrt(abar_t)), sample (0, 1).  c_v is
        `zero_latent_x0_scale(t)`; clip_sample / thresholding configurations are refused in the same way."""
        c_v = self.zero_latent_x0_scale(t)
        sa, _ = self.x0_coefficients(t)
        pt = self.config.prediction_type
        return {"v_prediction": sa, "epsilon": 1.0 / sa, "sample": 0.0}[pt], c_v

    def step_coefficients_f64(self, num_inference_steps):
        """float64 [n, 2] host tensor: row i < n - 1 is (c_x, c_v) with `step(model_output, t_i, x_t).prev_sample = c_x * x_t + c_v * model_output`, row n - 1 gives
        `pred_original_sample` (what the pipelines decode after the last step).  With eta = 0 and no clipping the step is linear in (x_t, model_output); with
        sa = sqrt(abar_t), sb = sqrt(1 - abar_t), sp = sqrt(abar_prev), sq = sqrt(1 - abar_prev), from the values step() reads (the fp32 table entries widened):
            v_prediction  (sp sa + sq sb,  sq sa - sp sb)        epsilon  (sp / sa,  sq - sp sb / sa)        sample  (sq / sb,  sp - sq sa / sb)
        and the last row is `x0_coefficients_for` in float64.  clip_sample / thresholding configurations are refused as `zero_latent_x0_scale` refuses them."""
        if self.config.clip_sample or self.config.thresholding:
            raise NotImplementedError("the fused multi-step path does not clip / threshold x0 (scheduler config clip_sample=%s, thresholding=%s)"
                                      % (self.config.clip_sample, self.config.thresholding))
        n = int(num_inference_steps)
        pt = self.config.prediction_type
        if pt not in ("v_prediction", "epsilon", "sample"):
            raise ValueError("Unknown prediction type %s" % pt)
        rows = []
        for i, t in enumerate(int(v) for v in self._spaced(n)):
            a_t = self.alphas_cumprod[t].item()
            sa, sb = a_t ** 0.5, (1 - a_t) ** 0.5
            if i == n - 1:
                rows.append({"v_prediction": (sa, -sb), "epsilon": (1.0 / sa, -sb / sa), "sample": (0.0, 1.0)}[pt])
                continue
            prev_t = t - self.config.num_train_timesteps // n
            a_prev = (self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod).item()
            sp, sq = a_prev ** 0.5, (1 - a_prev) ** 0.5
            rows.append({"v_prediction": (sp * sa + sq * sb, sq * sa - sp * sb), "epsilon": (sp / sa, sq - sp * sb / sa),
                         "sample": (sq / sb, sp - sq * sa / sb)}[pt])
        return torch.tensor(rows, dtype=torch.float64)

    def step_coefficients(self, num_inference_steps, device=None):
        """`step_coefficients_f64` rounded once to fp32, on `device`: [n, 2], row i is what `ops.ddim_step_` reads at step i.  Kept per (schedule, device) as
        `timesteps` is: no host-to-device copy per image."""
        c = self.config
        key = (int(num_inference_steps), str(device), c.prediction_type, c.timestep_spacing, c.steps_offset, c.num_train_timesteps)
        cache = self.__dict__.setdefault("_coef_cache", {})
        tab = cache.get(key)
        if tab is None:
            if len(cache) > 64:
                cache.clear()
            tab = self.step_coefficients_f64(num_inference_steps).to(torch.float32)
            tab = cache[key] = (tab if device is None else tab.to(device)).contiguous()
        return tab

    def step(self, model_output, timestep, sample, eta=0.0, **kw):
        """DDIM step for epsilon / sample / v_prediction with eta = 0 (elementwise torch ops on tiny latents; the
        pipelines' fused path uses ops.copy_scale instead)."""
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t].item()
        a_prev = (self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod).item()
        b_t = 1 - a_t
        pt = self.config.prediction_type
        if pt == "epsilon":
            x0 = (sample - b_t ** 0.5 * model_output) / a_t ** 0.5
            eps = model_output
        elif pt == "sample":
            x0 = model_output
            eps = (sample - a_t ** 0.5 * x0) / b_t ** 0.5
        elif pt == "v_prediction":
            x0 = a_t ** 0.5 * sample - b_t ** 0.5 * model_output
            eps = a_t ** 0.5 * model_output + b_t ** 0.5 * sample
        else:
            raise ValueError(pt)
        if self.config.clip_sample or self.config.thresholding:
            raise NotImplementedError("clip_sample / thresholding are not implemented (SD-v2 / Marigold / GeoWizard schedulers set neither)")
        prev = a_prev ** 0.5 * x0 + (1 - a_prev) ** 0.5 * eps
        return SchedulerOutput(prev, x0)


class DDPMScheduler(DDIMScheduler):
    """The name the training script loads, reads and saves (training/train.py:25,292,461,480,511-524,613-617): `DDPMScheduler.from_pretrained(ckpt,
    subfolder="scheduler"[, timestep_spacing="trailing"])`, `.alphas_cumprod`, `.config.num_train_timesteps / prediction_type / thresholding /
    clip_sample`, and at the end of training `StableDiffusionPipeline(..., scheduler=DDPMScheduler.from_pretrained(..., timestep_spacing="trailing"))
    .save_pretrained(out)` which writes scheduler/scheduler_config.json.  The E2E-FT step never calls the scheduler's stochastic `step()`: it only
    needs the noise schedule (identical to DDIM's: scaled_linear betas, diffusers scheduling_ddpm.py) and the config, so this is the same object
    under the reference's class name; `save_pretrained` records `_class_name: DDPMScheduler` as diffusers would.  SD-v2 ships `clip_sample: false`;
    a checkpoint that sets it (DDPM's diffusers default is true) is refused by the fused single-step path exactly like DDIM's (zero_latent_x0_scale).

    The diffusion objective of the GeoWizard trainer (GeoWizard/geowizard/training/train_depth_normal.py:671,680) also calls `add_noise` and `get_velocity`:
    both take diffusers' argument order and run on device tensors through e2eft_diffusion_mix (one launch, per-row timesteps read on the device)."""

    def alphas_cumprod_on(self, device):
        """the fp32 alphas_cumprod table on `device`: uploaded once per (scheduler, device) and kept"""
        cache = self.__dict__.setdefault("_abar_dev", {})
        key = str(torch.device(device))
        tab = cache.get(key)
        if tab is None:
            tab = cache[key] = self.alphas_cumprod.to(device=device, dtype=torch.float32).contiguous()
        return tab

    def _mix(self, x0, noise, timesteps, kind):
        from . import ops
        ops._check_cuda(x0, noise, timesteps)
        if x0.dim() != 4 or x0.shape != noise.shape or x0.dtype != noise.dtype:
            raise ValueError("expected two [R,C,h,w] tensors of one dtype, got %s %s and %s %s" % (tuple(x0.shape), x0.dtype, tuple(noise.shape), noise.dtype))
        t = timesteps.to(torch.int64).reshape(-1).contiguous()
        if t.numel() != x0.shape[0]:
            raise ValueError("expected one timestep per row: %d timesteps for %d rows" % (t.numel(), x0.shape[0]))
        from .autograd import _nhwc_view
        R, Cc, h, w = x0.shape
        out = torch.empty((R, h, w, Cc), dtype=x0.dtype, device=x0.device)
        ops.diffusion_mix_(_nhwc_view(x0), _nhwc_view(noise), t, self.alphas_cumprod_on(x0.device), out, kind)
        return out.permute(0, 3, 1, 2)

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers `DDPMScheduler.add_noise`: sqrt(abar_t) * original_samples + sqrt(1 - abar_t) * noise per row (logical NCHW in, logical NCHW out)"""
        from ._lib import DIFFUSION_ADD_NOISE
        return self._mix(original_samples, noise, timesteps, DIFFUSION_ADD_NOISE)

    def get_velocity(self, sample, noise, timesteps):
        """diffusers `DDPMScheduler.get_velocity`: sqrt(abar_t) * noise - sqrt(1 - abar_t) * sample per row"""
        from ._lib import DIFFUSION_VELOCITY
        return self._mix(sample, noise, timesteps, DIFFUSION_VELOCITY)

    def step(self, *a, **kw):
        raise NotImplementedError("ancestral DDPM sampling is not on the E2E-FT path (training/train.py reads the schedule only; inference uses DDIMScheduler)")
