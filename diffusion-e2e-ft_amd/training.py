"""Host side of the E2E-FT training step (training/train.py:470-568), built on the libe2eft forward/backward kernels.

  e2e_ft_loss        — the step's forward half: frozen VAE encode -> zeros latent -> UNet @ t=999 -> x0 -> frozen VAE decode ->
                       depth / normal head -> ScaleAndShiftInvariantLoss / AngularLoss   (train.py:472-556)
  FlatAdamW          — clip_grad_norm_ + torch.optim.AdamW semantics (train.py:346-353,561-566) on ONE flat fp32 parameter
                       buffer: parameters and their .grad are views of two big allocations, so the data-parallel gradient
                       exchange is a handful of large RCCL all-reduces over contiguous slices (no bucket copies), launched
                       from autograd hooks while the rest of the backward is still running, and the update is one launch.
  GroupedFlatAdamW   — FlatAdamW over up to 8 parameter groups with their own lr / betas / eps / weight decay, still one update launch
                       (GeoWizard/geowizard/training/train_depth_normal.py:428-444; geowizard_param_groups restates its split)
  IterExponential    — training/util/lr_scheduler.py:10-36
  replace_unet_conv_in — training/util/unet_prep.py:6-20

The reference wraps the UNet in DDP via accelerate; here one process per GPU (torchrun) calls FlatAdamW.step(), which waits for
the outstanding all-reduces.  xGMI is point-to-point, so few large collectives (default 4 byte-sized slices of the 3.46 GB
gradient, the last-finishing one the smallest) keep all seven links busy; the first slice to finish its backward (the up blocks)
starts its exchange while the down blocks are still computing.
"""
import math
import weakref

import torch
import torch.distributed as dist

from . import autograd as F
from . import ops


class IterExponential:
    """lr multiplier: linear warm-up, then exp decay to final_ratio at total_iter_length (lr_scheduler.py:10-36)"""

    def __init__(self, total_iter_length, final_ratio, warmup_steps=0):
        self.total_length = total_iter_length
        self.effective_length = total_iter_length - warmup_steps
        self.final_ratio = final_ratio
        self.warmup_steps = warmup_steps

    def __call__(self, n_iter):
        if n_iter < self.warmup_steps:
            return 1.0 * n_iter / self.warmup_steps
        if n_iter >= self.total_length:
            return self.final_ratio
        return math.exp((n_iter - self.warmup_steps) / self.effective_length * math.log(self.final_ratio))


def replace_unet_conv_in(unet, repeat=2):
    """4 -> 8 input channels: repeat the weight on Cin, halve weight and bias (unet_prep.py:6-20)"""
    w = unet.conv_in.weight.detach().clone().repeat(1, repeat, 1, 1) / repeat
    b = unet.conv_in.bias.detach().clone() / repeat
    old = unet.conv_in
    new = type(old)(old.in_channels * repeat, old.out_channels, kernel_size=old.kernel_size, stride=old.stride, padding=old.padding)
    new = new.to(device=w.device, dtype=w.dtype)
    with torch.no_grad():
        new.weight.copy_(w)
        new.bias.copy_(b)
    unet.conv_in = new
    unet.config["in_channels"] = old.in_channels * repeat


# ------------------------------------------------------------------------------------------------------------
def encode_image(vae, image):
    """train.py:233-237"""
    h = vae.encoder(image)
    moments = vae.quant_conv(h)
    latent, _ = torch.chunk(moments, 2, dim=1)
    return latent


NOISE_TYPES = ("zeros", "gaussian", "pyramid", None)      # training/train.py:57-63 (`--noise_type`; unset = a UNet without noise channels)


def e2e_ft_loss(unet, vae, batch, empty_encoding, modality="depth", noise_scheduler=None, return_estimate=False, noise_type="zeros", generator=None,
                noise=None):
    """Forward half of one micro-step (train.py:472-556) at t = 999 (the E2E-FT recipe).
    batch: rgb [b,3,H,W] in [-1,1], val_mask [b,1,H,W] bool, metric [b,1,H,W] / normals [b,3,H,W].  Returns the scalar loss
    (device tensor with a grad_fn through the decoder and the UNet).  `unet` may be wrapped (DistributedDataParallel by
    `accelerator.prepare`, train.py:369): attributes are read from `.module`, the forward goes through the wrapper.
    noise_type (train.py:483-499): "zeros" (default: the zeros latent, x0 = c * model_pred), "gaussian" / "pyramid" (drawn on the device by
    `generator`, a noise.DeviceNoise, straight into channels 4:8 of the UNet input; x0 by the scheduler's prediction_type from that x_t), None
    (a 4-channel UNet fed the rgb latent alone).  noise: an explicit x_t [b,4,h,w] instead of a drawn one (tests, reproducibility across devices).
    The drawn settings are not capture-safe (noise.py): a replayed graph repeats its noise — except "gaussian" with a `noise.DrawAt` generator, whose draw is read
    on the device (what CapturedTrainStep hands in)."""
    if noise_type not in NOISE_TYPES:
        raise ValueError("Unknown noise type %s" % noise_type)
    core = getattr(unet, "module", unet)
    with ops.on_device_of(next(core.parameters())):
        return _e2e_ft_loss(unet, core, vae, batch, empty_encoding, modality, noise_scheduler, return_estimate, noise_type, generator, noise)


def _e2e_ft_loss(unet, core, vae, batch, empty_encoding, modality, noise_scheduler, return_estimate, noise_type="zeros", generator=None, noise=None):
    dev = core.device
    dt = getattr(core, "compute_dtype", core.dtype)
    if noise_type is None:
        if noise is not None:
            raise ValueError("noise_type=None feeds the UNet no noise channels: an explicit `noise` has nowhere to go")
        if core.config["in_channels"] != 4:
            raise ValueError("noise_type=None needs a UNet whose conv_in takes the 4 rgb-latent channels alone; this one has in_channels=%s "
                             "(replace_unet_conv_in doubles them for the other noise types)" % core.config["in_channels"])
    with torch.no_grad():
        rgb_latents = encode_image(vae, batch["rgb"].to(device=dev, dtype=dt)) * vae.config.scaling_factor
    val_mask = batch["val_mask"].bool().to(dev)
    b = rgb_latents.shape[0]
    timesteps = torch.full((b,), 999, device=dev, dtype=torch.long)
    ctx = empty_encoding.to(device=dev, dtype=dt).repeat(b, 1, 1)
    if noise_scheduler is None:
        from .scheduler import DDIMScheduler
        noise_scheduler = DDIMScheduler()
    x_t = None              # NHWC view of the noise channels when x_t != 0
    if noise_type is None:
        unet_input = rgb_latents
    elif noise is None and noise_type == "zeros":
        noisy = torch.zeros_like(rgb_latents)
        unet_input = torch.cat((rgb_latents, noisy), dim=1).contiguous(memory_format=torch.channels_last)
    else:
        # UNet input buffer [b,h,w,8] NHWC: channels 0:4 the rgb latent, 4:8 x_t, written in place (no concat, no layout copy)
        _, C, h, w = rgb_latents.shape
        xin = torch.empty((b, h, w, 2 * C), dtype=dt, device=dev)
        ops.copy_scale(F._nhwc_view(rgb_latents), xin[..., :C])
        x_t = xin[..., C:]
        if noise is not None:
            if tuple(noise.shape) != (b, C, h, w):
                raise ValueError("noise must be [%d,%d,%d,%d], got %s" % (b, C, h, w, tuple(noise.shape)))
            ops.copy_scale(F._nhwc_view(noise.to(device=dev, dtype=dt)), x_t)
        else:
            from . import noise as N
            if not isinstance(generator, N.DeviceNoise):
                raise TypeError("noise_type=%r draws on the device: pass generator=noise.DeviceNoise(seed)" % noise_type)
            N.noise_into(noise_type, x_t, generator)
        unet_input = xin.permute(0, 3, 1, 2)
    model_pred = unet(unet_input, timesteps, ctx, return_dict=False)[0]
    sf = vae.config.scaling_factor
    if x_t is None:
        # x_t = 0: x0 = c * model_pred with c by the scheduler's prediction_type (v: -sqrt(1 - alpha_prod), train.py:509-518), then / scaling_factor (:528)
        x0 = model_pred * (noise_scheduler.zero_latent_x0_scale(999) / sf)
    else:
        c_x, c_v = noise_scheduler.x0_coefficients_for(999)
        x0 = F.latent_x0(model_pred, x_t, c_x / sf, c_v / sf)
    est = vae.decoder(vae.post_quant_conv(x0))                     # [b,3,H,W] logical NCHW, NHWC memory
    est_nhwc = est.permute(0, 2, 3, 1)
    if modality == "depth":
        cur = F.depth_head(est_nhwc, to_unit=False)                # mean over channels, clamp(-1, 1)  (:531-533)
        loss = F.ssi_loss(cur, batch["metric"].to(device=dev), val_mask)
    elif modality == "normals":
        cur = F.normal_head(est_nhwc, clamp=True)                  # x / (|x| + 1e-5), clamp  (:535-538)
        loss = F.angular_loss(cur, batch["normals"].to(device=dev), val_mask)
    else:
        raise ValueError("Unknown modality %s" % modality)
    return (loss, cur) if return_estimate else loss


def geowizard_class_embedding(batch, domain, dtype, device):
    """hybrid switcher + domain class, rows [depth (b); normal (b)]  (train_depth_normal.py:684-700).  A function of its arguments alone: kept per
    (batch, domain, dtype, device), so that a call inside a stream capture (CapturedTrainStep, after its eager first step) copies nothing from the host.
    The result is shared: read it, do not write it."""
    key = (int(batch), domain, dtype, str(device))
    hit = _CLASS_EMBEDDINGS.get(key)
    if hit is None:
        if len(_CLASS_EMBEDDINGS) >= 16:
            _CLASS_EMBEDDINGS.clear()
        hit = _CLASS_EMBEDDINGS[key] = _geowizard_class_embedding(batch, domain, dtype, device)
    return hit


_CLASS_EMBEDDINGS = {}


def _geowizard_class_embedding(batch, domain, dtype, device):
    geo =torch.tensor([[0.0, 1.0], [1.0, 0.0]], dtype=torch.float32, device=device).repeat_interleave(batch, 0)
    dom = {"indoor": [1.0, 0.0, 0.0], "outdoor": [0.0, 1.0, 0.0], "object": [0.0, 0.0, 1.0]}[domain]
    dom = torch.tensor([dom], dtype=torch.float32, device=device).repeat(2 * batch, 1)
    return torch.cat([torch.sin(geo), torch.cos(geo), torch.sin(dom), torch.cos(dom)], dim=-1).to(dtype)


GEOWIZARD_PYRAMID_MESSAGE = ("noise_type='pyramid' is not built for the GeoWizard trainer: its multi-resolution noise weights every level per sample by t / 1000 "
                             "(GeoWizard/geowizard/training/train_depth_normal.py:286-296), which is a different function from e2eft_pyramid_noise "
                             "(training/util/noise.py:8-18, no timestep weight); the trainer's own function is noise_type='geowizard_pyramid' "
                             "(e2eft_pyramid_noise_weighted): map the trainer's `--noise_type pyramid` to that name")
GEOWIZARD_NOISE_TYPES = ("zeros", "gaussian", "pyramid", "geowizard_pyramid")      # "pyramid" is known and refused (GEOWIZARD_PYRAMID_MESSAGE)


def _geowizard_noise(noise_type, generator, noise, rows, C, h, w, dt, dev, timesteps=None):
    """the geometry noise [2b,4,h,w] of the GeoWizard trainer (train_depth_normal.py:656-663) as an NHWC tensor [2b,h,w,4]: an explicit `noise`, zeros,
    standard normals drawn on the device by a noise.DeviceNoise (:661-662), or — "geowizard_pyramid" — the trainer's `pyramid_noise_like(geo_latents, timesteps)`
    (:286-296, called at :658-659) drawn on the device from the doubled int64 device `timesteps` [2b], which are read there and never by the host"""
    if noise_type == "pyramid":
        raise ValueError(GEOWIZARD_PYRAMID_MESSAGE)
    if noise is not None:
        if tuple(noise.shape) != (rows, C, h, w):
            raise ValueError("noise must be [%d,%d,%d,%d], got %s" % (rows, C, h, w, tuple(noise.shape)))
        return F._nhwc_view(noise.to(device=dev, dtype=dt))
    if noise_type == "zeros":
        return torch.zeros((rows, h, w, C), dtype=dt, device=dev)
    if noise_type == "gaussian":
        from . import noise as N
        if not isinstance(generator, N.DeviceNoise):
            raise TypeError("noise_type='gaussian' draws on the device: pass generator=noise.DeviceNoise(seed)")
        return N.randn_into(torch.empty((rows, h, w, C), dtype=dt, device=dev), generator)
    if noise_type == "geowizard_pyramid":
        from . import noise as N
        if not isinstance(generator, N.DeviceNoise):
            raise TypeError("noise_type='geowizard_pyramid' draws on the device: pass generator=noise.DeviceNoise(seed)")
        return N.geowizard_pyramid_noise_into(torch.empty((rows, h, w, C), dtype=dt, device=dev), generator, timesteps)
    raise ValueError("Unknown noise type %s" % noise_type)


def geowizard_e2e_ft_loss(unet, vae, batch, imgs_embed, domain="indoor", depth_scale=0.5, normal_scale=1.0, return_parts=False, noise_type="zeros", generator=None,
                          noise=None):
    """Forward half of the GeoWizard E2E-FT micro-step (GeoWizard/geowizard/training/train_depth_normal.py:597-768, --e2e_ft, zeros
    noise): the UNet runs the doubled batch [depth rows; normal rows] with cross-domain joint self-attention and the class
    embedding, the frozen decoder decodes both halves, loss = 0.5 * SSI(depth) + 1.0 * angular(normals vs -GT).
    imgs_embed: CLIP image embeddings [b,1,768] (an input here).
    noise_type (:656-668): "zeros" (default), "gaussian" (drawn on the device by `generator`, a noise.DeviceNoise) or an explicit `noise` [2b,4,h,w]: x_t = noise
    (:668) goes into channels 4:8 of the UNet input and x0 comes from that x_t.  "geowizard_pyramid" (also a noise.DeviceNoise) is the trainer's own
    `--noise_type pyramid`: `pyramid_noise_like(geo_latents, timesteps)` (:286-296, called at :658-659) with the constant 999 timesteps of :651-652, every level
    weighted by 999 / 1000; its level sizes come from numpy's global stream as in the reference.  The name "pyramid" itself is refused: in this package it means
    training/util/noise.py's unweighted function (GEOWIZARD_PYRAMID_MESSAGE)."""
    core = getattr(unet, "module", unet)
    with ops.on_device_of(next(core.parameters())):
        return _geowizard_e2e_ft_loss(unet, core, vae, batch, imgs_embed, domain, depth_scale, normal_scale, return_parts, noise_type, generator, noise)


def _geowizard_e2e_ft_loss(unet, core, vae, batch, imgs_embed, domain, depth_scale, normal_scale, return_parts, noise_type="zeros", generator=None, noise=None):
    dev = core.device
    dt = getattr(core, "compute_dtype", core.dtype)
    if noise_type not in GEOWIZARD_NOISE_TYPES:
        raise ValueError("Unknown noise type %s" % noise_type)
    if noise_type == "pyramid":
        raise ValueError(GEOWIZARD_PYRAMID_MESSAGE)
    with torch.no_grad():
        rgb_latents = encode_image(vae, batch["rgb"].to(device=dev, dtype=dt)) * vae.config.scaling_factor
    val_mask = batch["val_mask"].bool().to(dev)
    b = rgb_latents.shape[0]
    timesteps = torch.full((2 * b,), 999, device=dev, dtype=torch.long)
    ctx = imgs_embed.to(device=dev, dtype=dt).repeat(2, 1, 1)
    cls = geowizard_class_embedding(b, domain, dt, dev)
    from .scheduler import DDIMScheduler
    sf = vae.config.scaling_factor
    if noise is None and noise_type == "zeros":
        noisy = torch.zeros_like(rgb_latents).repeat(2, 1, 1, 1)
        unet_input = torch.cat((rgb_latents.repeat(2, 1, 1, 1), noisy), dim=1).contiguous(memory_format=torch.channels_last)
        noise_pred = unet(unet_input, timesteps, ctx, class_labels=cls, return_dict=False)[0]
        x0 = noise_pred * (DDIMScheduler().zero_latent_x0_scale(999) / sf)
    else:
        # x_t = noise (:668) in channels 4:8 of the [2b,h,w,8] UNet input, x0 from that x_t by the scheduler's prediction type
        _, C, h, w = rgb_latents.shape
        xin = torch.empty((2 * b, h, w, 2 * C), dtype=dt, device=dev)
        lat = F._nhwc_view(rgb_latents)
        ops.copy_scale(lat, xin[:b, ..., :C])
        ops.copy_scale(lat, xin[b:, ..., :C])
        x_t = xin[..., C:]
        ops.copy_scale(_geowizard_noise(noise_type, generator, noise, 2 * b, C, h, w, dt, dev, timesteps), x_t)      # (:651-652: all 999 under --e2e_ft)
        noise_pred = unet(xin.permute(0, 3, 1, 2), timesteps, ctx, class_labels=cls, return_dict=False)[0]
        c_x, c_v = DDIMScheduler().x0_coefficients_for(999)
        x0 = F.latent_x0(noise_pred, x_t, c_x / sf, c_v / sf)
    est = vae.decoder(vae.post_quant_conv(x0)).permute(0, 2, 3, 1)          # NHWC view [2b,H,W,3]
    depth = F.depth_head(est[:b], to_unit=False)
    normal = F.normal_head(est[b:], clamp=True)
    ssi = F.ssi_loss(depth, batch["metric"].to(device=dev), val_mask)
    ang = F.angular_loss(normal, batch["normals"].to(device=dev) * -1, val_mask)     # GeoWizard trains on inverted normals (:611,751)
    loss = ssi * depth_scale + ang * normal_scale
    return (loss, ssi, ang) if return_parts else loss


def geowizard_diffusion_loss(unet, vae, batch, imgs_embed, domain="indoor", noise_scheduler=None, noise_type="gaussian", generator=None, noise=None,
                             timesteps=None, prediction_type=None, return_parts=False):
    """Forward half of the GeoWizard DIFFUSION-objective micro-step (GeoWizard/geowizard/training/train_depth_normal.py:598-717 WITHOUT --e2e_ft): one frozen VAE
    encode of [rgb; depth; -normals] (:611,634-638), per-sample timesteps `randint(0, T, (b,)).repeat(2)` (:651), geometry noise (:656-663), `add_noise` written
    straight into channels 4:8 of the UNet input (:671,704), the UNet over the doubled batch [depth rows; normal rows] with the class embedding (:684-709), and the
    mean squared error against the target of the prediction type over the latent cells whose 8 x 8 pixels are all valid (:606-609,677-682,713-717).  The objective's
    own arithmetic is five launches of csrc/diffusion.hip and synchronises nothing with the host.
    batch: rgb [b,3,H,W], depth [b,3,H,W] (the normalised depth on three channels), normals [b,3,H,W], val_mask [b,1,H,W]; H and W multiples of 8.
    noise_scheduler: a scheduler.DDPMScheduler (default: a fresh one); prediction_type overrides its config's (:674-676), "epsilon" or "v_prediction".
    noise_type: "gaussian" (drawn on the device by `generator`, a noise.DeviceNoise), "zeros", an explicit `noise` [2b,4,h,w], or "geowizard_pyramid" — the trainer's
    own `--noise_type pyramid`, `pyramid_noise_like(geo_latents, timesteps)` (:286-296, called at :658-659): drawn by the same kind of generator straight after the
    doubled timesteps exist, level i of row r weighted by timesteps[r] / 1000 * 0.9^i on the device (no read-back), level sizes from numpy's global stream as in the
    reference; it then goes through add_noise and the masked MSE as "gaussian" does.  The name "pyramid" is refused (GEOWIZARD_PYRAMID_MESSAGE).
    timesteps: int64 [b] instead of drawn ones (drawn on the device from torch's generator, no read-back).
    timesteps may also be a noise.DeviceNoise: the timesteps are then drawn by IT (`noise.randint_into`, the counter-based `randint(0, T, (b,)).repeat(2)`) BEFORE
    the noise draw instead of by `torch.randint`; usually the same object as `generator`, which then advances twice per call.  Capture-safe with a `noise.DrawAt`
    (training.CapturedTrainStepAt).  None keeps `torch.randint`.
    No selected cell: the loss is 0 and its gradient is zero everywhere, as e2e_ft_loss does for an all-invalid batch (the reference skips the term, :714).
    Returns the loss; return_parts: (loss, n_selected int64 [1], target fp32 [2b,4,h,w], x_t [2b,4,h,w])."""
    core = getattr(unet, "module", unet)
    with ops.on_device_of(next(core.parameters())):
        return _geowizard_diffusion_loss(unet, core, vae, batch, imgs_embed, domain, noise_scheduler, noise_type, generator, noise, timesteps, prediction_type,
                                         return_parts)


def _geowizard_diffusion_loss(unet, core, vae, batch, imgs_embed, domain, noise_scheduler, noise_type, generator, noise, timesteps, prediction_type, return_parts):
    dev = core.device
    dt = getattr(core, "compute_dtype", core.dtype)
    if noise_type not in GEOWIZARD_NOISE_TYPES:
        raise ValueError("Unknown noise type %s" % noise_type)
    if noise_type == "pyramid":
        raise ValueError(GEOWIZARD_PYRAMID_MESSAGE)
    if noise_scheduler is None:
        from .scheduler import DDPMScheduler
        noise_scheduler = DDPMScheduler()
    pt = prediction_type if prediction_type is not None else noise_scheduler.config.prediction_type
    if pt not in ("epsilon", "v_prediction"):
        raise ValueError("Unknown prediction type %s" % pt)
    rgb = batch["rgb"].to(device=dev, dtype=dt)
    b = rgb.shape[0]
    with torch.no_grad():
        images = torch.cat((rgb, batch["depth"].to(device=dev, dtype=dt), batch["normals"].to(device=dev, dtype=dt) * -1), dim=0)
        latents = F._nhwc_view(encode_image(vae, images) * vae.config.scaling_factor)       # [3b,h,w,4]: rgb | depth | normal rows
    _, h, w, C = latents.shape
    rgb_latents, geo_latents = latents[:b], latents[b:]                                     # geo rows [depth (b); normal (b)] (:639)
    latent_mask = ops.latent_valid_mask(batch["val_mask"].to(dev))                          # [b,h,w]; row r reads image r % b (:609)
    if tuple(latent_mask.shape[1:]) != (h, w):
        raise ValueError("val_mask gives %s latent cells, the latents are %s" % (tuple(latent_mask.shape[1:]), (h, w)))
    T = noise_scheduler.config.num_train_timesteps
    from . import noise as N
    if isinstance(timesteps, N.DeviceNoise):
        timesteps = N.randint_into(torch.empty((2 * b,), dtype=torch.long, device=dev), T, timesteps, repeat=2)      # (:651, already doubled)
    else:
        if timesteps is None:
            timesteps = torch.randint(0, T, (b,), device=dev)
        elif timesteps.numel() != b:
            raise ValueError("timesteps must hold one entry per image (%d), got %d" % (b, timesteps.numel()))
        timesteps = timesteps.to(device=dev, dtype=torch.long).reshape(b).repeat(2)
    nz = _geowizard_noise(noise_type, generator, noise, 2 * b, C, h, w, dt, dev, timesteps)      # (:656-663; the weighted pyramid reads the doubled timesteps on the device)
    abar = noise_scheduler.alphas_cumprod_on(dev)
    xin = torch.empty((2 * b, h, w, 2 * C), dtype=dt, device=dev)
    ops.copy_scale(rgb_latents, xin[:b, ..., :C])
    ops.copy_scale(rgb_latents, xin[b:, ..., :C])
    x_t = ops.diffusion_mix_(geo_latents, nz, timesteps, abar, xin[..., C:])
    ctx = imgs_embed.to(device=dev, dtype=dt).repeat(2, 1, 1)
    cls = geowizard_class_embedding(b, domain, dt, dev)
    noise_pred = unet(xin.permute(0, 3, 1, 2), timesteps, ctx, class_labels=cls, return_dict=False)[0]
    out = F.masked_mse(noise_pred, geo_latents, nz, timesteps, abar, latent_mask, pt, want_target=return_parts)
    if not return_parts:
        return out[0]
    return out[0], out[1], out[2].permute(0, 3, 1, 2), x_t.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------
class FlatAdamW(torch.optim.Optimizer):
    """`torch.optim.AdamW` + `clip_grad_norm_` (training/train.py:346-353,561-566) over ONE flat fp32 buffer, with the data-parallel
    gradient all-reduce overlapped with the backward.

    A real `torch.optim.Optimizer`: one `param_groups` entry whose `lr` is live (so `LambdaLR(optimizer, IterExponential(...))` of
    train.py:356-357 drives it), `state[p] = {"step", "exp_avg", "exp_avg_sq"}` per parameter (views of the flat moment buffers and of
    the device-side step counter), `state_dict()` / `load_state_dict()` in torch's own format (`accelerator.save_state / load_state`,
    train.py:417-440,578-599, and checkpoints written by `torch.optim.AdamW` load here and vice versa), `zero_grad(set_to_none=...)`,
    `step(closure=None)`.

    What is flat: the storage of every trainable Parameter is moved into `self.flat_param` (diffusers-layout views: `state_dict()` of the
    model keeps working), `.grad` is pre-bound to views of `self.flat_grad`, so autograd accumulates straight into the exchange buffer,
    the exchange is a handful of large RCCL all-reduces over contiguous slices (no bucket copies) launched from autograd hooks while the
    rest of the backward is still running, and clip + update are one `sumsq` and one `adamw` launch.

    external_grad_sync=True: somebody else averages the gradients across ranks (a DistributedDataParallel wrap by `accelerator.prepare`,
    train.py:369) — no hooks, no division by the world size here.
    Non-finite gradient norm: the step is skipped on the device, the bias-correction step does not advance, `skipped_steps()` counts it
    (e2eft_adamw_step_guarded, include/e2eft.h).

    direct_grads=True (default): `zero_grad()` leaves every `.grad` None (torch's own default) instead of clearing the flat buffer, and the backward kernels of
    the libe2eft autograd Functions write a parameter's FIRST gradient of an optimizer step straight into its slot of `flat_grad` (autograd.grad_sink): the
    tensor autograd then stores as `.grad` is a view of the exchange buffer, no AccumulateGrad add per parameter, no 3.5 GB memset per step.  Later gradients of the
    same step (gradient accumulation) are accumulated by autograd in place as before; gradients that arrive any other way are adopted (copied) into their slot by
    the hook / `step()`; slots that received nothing are zeroed there.  Scope of the sink: `loss.backward()` accumulating into `.grad`, gradients cleared by
    `zero_grad()` (this optimizer's or the model's, set_to_none=True).  The tensor such a backward hands to autograd is a VIEW of the exchange buffer that later
    steps overwrite in place: do not keep it across steps (`torch.autograd.grad(...)` results, hooks that retain the gradient, a `retain_graph` second backward —
    use direct_grads=False for those)."""

    def __init__(self, params, lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=1.0, n_slices=4,
                 process_group=None, external_grad_sync=False, direct_grads=True):
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) != 1:
                raise ValueError("FlatAdamW updates one flat buffer with one set of hyper-parameters: pass a single parameter group")
            group0 = dict(params[0])
            plist = [p for p in group0.pop("params") if p.requires_grad]
            lr, betas, eps, weight_decay = group0.get("lr", lr), group0.get("betas", betas), group0.get("eps", eps), group0.get("weight_decay", weight_decay)
        else:
            plist = [p for p in params if p.requires_grad]
        self._init_flat(plist, plist, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), max_grad_norm, n_slices, process_group,
                        external_grad_sync, direct_grads)

    def _init_flat(self, plist, torch_params, defaults, max_grad_norm, n_slices, process_group, external_grad_sync, direct_grads):
        """everything behind the argument parsing: `plist` in the flat buffer's order, `torch_params` what `torch.optim.Optimizer` is built from (the same list, or
        GroupedFlatAdamW's group dicts over the same parameters in the same order)"""
        if not plist:
            raise ValueError("no trainable parameters")
        dev = plist[0].device
        for p in plist:
            if p.dtype != torch.float32:
                raise TypeError("FlatAdamW keeps fp32 master parameters; got %s" % p.dtype)
            if p.device != dev:
                raise ValueError("FlatAdamW: all parameters must live on one device")
        torch.optim.Optimizer.__init__(self, torch_params, defaults)
        self.params = plist
        self.max_grad_norm = max_grad_norm
        self.offsets, n = [], 0
        for p in self.params:
            self.offsets.append(n)
            n += (p.numel() + 7) // 8 * 8                     # keep every view 16-byte aligned in the 16-bit twin too (autograd.FlatShadow): 32 bytes here
        self.numel = n
        # Convolution weights are stored in the order the kernels read them — OHWI, i.e. the Parameter becomes a channels_last view of its slot (same values, same
        # logical OIHW shape: state_dict / save_pretrained / copy_ see no difference) — so that with 16-bit compute the packed weight of every convolution is a
        # slice of ONE flat cast of this buffer (autograd.FlatShadow) and the weight gradient, which the kernels produce in OHWI order, is accumulated without a
        # permuting copy.
        self._ohwi = [p.dim() == 4 and p.shape[2] * p.shape[3] > 1 for p in plist]
        with ops.on_device_of(plist[0]):
            self.flat_param = torch.zeros(n, dtype=torch.float32, device=dev)
            self.flat_grad = torch.zeros(n, dtype=torch.float32, device=dev)
            self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
            self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
            self._sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
            self._sumsq_ws = ops.sumsq_workspace(self.flat_grad)             # per-block partials of the gradient norm, sized once
            self._steps = torch.zeros(2, dtype=torch.int64, device=dev)      # {applied, skipped} — advanced by the update kernel itself
            self._coef = torch.zeros(4, dtype=torch.float32, device=dev)
            with torch.no_grad():
                self.shadow = F.FlatShadow(self.flat_param)
                for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                    view = self._slot(self.flat_param, i)
                    view.copy_(p.data)
                    p.data = view
                    p.grad = self._slot(self.flat_grad, i)
                    p._e2eft_flat = (self.shadow, o)
                    p._e2eft_gslot = (weakref.ref(self), i)      # (weak: the tag must not tie the optimizer's buffers into a reference cycle with its parameters)
                self.shadow.register(self.params, self.offsets)
        self.direct_grads = bool(direct_grads)
        self._claimed = [False] * len(self.params)
        self._bind_state()
        F.bump_param_epoch()
        self.group = process_group
        self.world = 1 if external_grad_sync else (dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1)
        # Slices of the flat buffer, cut by BYTES.  Parameters are stored in module order (conv_in, down, mid, up, conv_out) and the
        # backward produces gradients roughly in reverse, so the slice holding the FIRST parameters completes last and its exchange is
        # the one that cannot hide under the backward: slice sizes grow geometrically (1 : 2 : 4 : ...), the exposed one is the smallest
        # (n_slices = 4 on the 3.46 GB SD-v2 gradient: 0.23 / 0.46 / 0.92 / 1.85 GB).  Large messages keep all seven xGMI links busy.
        n_slices = max(1, min(n_slices, len(self.params)))
        total_w = float(2 ** n_slices - 1)
        targets, acc_w = [], 0.0
        for s_ in range(n_slices - 1):
            acc_w += 2 ** s_
            targets.append(n * acc_w / total_w)
        cuts, ti = [0], 0
        for i in range(1, len(self.params)):
            if ti < len(targets) and self.offsets[i] >= targets[ti] and i > cuts[-1]:
                cuts.append(i)
                ti += 1
                while ti < len(targets) and self.offsets[i] >= targets[ti]:
                    ti += 1
        cuts.append(len(self.params))
        self.slices = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            start = self.offsets[lo]
            end = self.offsets[hi] if hi < len(self.params) else n
            self.slices.append(dict(lo=lo, hi=hi, start=start, end=end, ready=0, work=None, done=False))
        self._index_of = {id(p): i for i, p in enumerate(self.params)}
        self._slice_of = {}
        for si, sl in enumerate(self.slices):
            for i in range(sl["lo"], sl["hi"]):
                self._slice_of[id(self.params[i])] = si
        self.sync_grads = True          # set False on non-final gradient-accumulation micro-steps
        self.profile_exchange = False   # bench.py --gpus N: time what step() waits for, per slice (exchange_exposed_ms)
        self._exposed = []
        self._hooks = []
        if self.world > 1:
            for p in self.params:
                self._hooks.append(p.register_post_accumulate_grad_hook(self._on_grad))

    def _slot(self, buf, i):
        """parameter i's view of a flat buffer (parameters, gradients, both moments): its shape, OHWI-ordered for convolution weights"""
        p, o = self.params[i], self.offsets[i]
        flat = buf[o:o + p.numel()]
        if self._ohwi[i]:
            Co, Ci, kh, kw = p.shape
            return flat.view(Co, kh, kw, Ci).permute(0, 3, 1, 2)
        return flat.view(p.shape)

    def _claim(self, idx, params):
        """autograd.grad_sink: hand the gradient slots `idx` (of `params`) to a backward kernel as its output — once per optimizer step and parameter.
        Several slots must lie back to back (q | k | v, LayerNorm weight | bias).  -> (flat fp32 view over the slots, [one view per parameter]) or None"""
        if not self.direct_grads:
            return None
        for k, i in enumerate(idx):
            if self._claimed[i] or self.params[i] is not params[k]:
                return None
            if k > 0 and self.offsets[i] != self.offsets[idx[k - 1]] + self.params[idx[k - 1]].numel():
                return None
        for i in idx:
            self._claimed[i] = True
        lo, hi = self.offsets[idx[0]], self.offsets[idx[-1]] + self.params[idx[-1]].numel()
        return self.flat_grad[lo:hi], [self._slot(self.flat_grad, i) for i in idx]

    # ---- torch.optim.Optimizer surface -------------------------------------------------------------------------------------------
    def _bind_state(self):
        """state[p]: views of the flat moment buffers; "step" is a view of the device-side applied-step counter shared by all parameters"""
        step = self._steps[0]
        for i, p in enumerate(self.params):
            self.state[p] = {"step": step, "exp_avg": self._slot(self.exp_avg, i), "exp_avg_sq": self._slot(self.exp_avg_sq, i)}

    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, v):
        self.param_groups[0]["lr"] = v

    @property
    def step_count(self):
        """applied steps (host value; synchronises)"""
        return int(self._steps[0].item())

    def skipped_steps(self):
        """optimizer steps dropped because the gradient norm was not finite (host value; synchronises)"""
        return int(self._steps[1].item())

    def state_dict(self):
        sd = super().state_dict()
        # torch's format wants per-parameter tensors that survive on their own.  super().state_dict() hands out the SAME per-parameter
        # dicts self.state holds, so build new ones: rebinding entries in place would cut state[p] loose from the flat moment buffers
        # and every later checkpoint would be stale.
        sd["state"] = {k: {"step": st["step"].detach().to(torch.float32).clone(), "exp_avg": st["exp_avg"].detach().clone(),
                           "exp_avg_sq": st["exp_avg_sq"].detach().clone()} for k, st in sd["state"].items()}
        sd["flat_adamw"] = {"skipped_steps": self.skipped_steps(), "max_grad_norm": self.max_grad_norm}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        extra = state_dict.get("flat_adamw", {})
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "flat_adamw"})   # group hyper-parameters (lr, betas, ...) + per-parameter copies
        steps = set()
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            st = self.state.get(p)
            n = p.numel()
            if not st:                            # parameter without saved state (fresh): zero moments
                self.exp_avg[o:o + n].zero_()
                self.exp_avg_sq[o:o + n].zero_()
                continue
            self._slot(self.exp_avg, i).copy_(st["exp_avg"])
            self._slot(self.exp_avg_sq, i).copy_(st["exp_avg_sq"])
            steps.add(int(torch.as_tensor(st["step"]).item()))
        if len(steps) > 1:
            raise ValueError("FlatAdamW.load_state_dict: parameters carry different step counts %s; one flat buffer has one bias correction" % sorted(steps))
        self._steps[0] = steps.pop() if steps else 0
        self._steps[1] = int(extra.get("skipped_steps", 0))
        self._bind_state()

    # autograd hook: a parameter's gradient is final for this backward
    def _on_grad(self, p):
        if not self.sync_grads:
            return
        self._adopt_one(p, self.offsets[self._index_of[id(p)]])      # a re-bound .grad goes back into its slot BEFORE the slice is exchanged
        sl = self.slices[self._slice_of[id(p)]]
        sl["ready"] += 1
        if sl["ready"] == sl["hi"] - sl["lo"]:
            sl["work"] = dist.all_reduce(self.flat_grad[sl["start"]:sl["end"]], op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    def _finish_exchange(self):
        """wait for the slices the hooks launched, exchange the ones no hook completed (parameters without a gradient this step).  Idempotent
        within an optimizer step: a slice is summed over the ranks exactly once until `step()` / `zero_grad()` re-arm it."""
        if self.world == 1:
            return
        for sl in self.slices:
            if sl["work"] is None and not sl["done"]:
                sl["work"] = dist.all_reduce(self.flat_grad[sl["start"]:sl["end"]], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
        prof = self.profile_exchange and self.flat_grad.is_cuda
        for si, sl in enumerate(self.slices):
            if sl["work"] is not None:
                if prof:     # how long the compute stream stands still for this slice: events on it either side of the wait
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    sl["work"].wait()
                    e1.record()
                    self._exposed.append((si, e0, e1))
                else:
                    sl["work"].wait()
            sl["work"], sl["ready"], sl["done"] = None, 0, True

    def exchange_exposed_ms(self):
        """profile_exchange = True: per slice, the mean time (ms) the compute stream waited for that slice's all-reduce in `step()` since the last
        call — the part of the exchange the backward did not hide.  Synchronises."""
        if not self._exposed:
            return []
        torch.cuda.synchronize(self.flat_grad.device)
        acc = [[0.0, 0] for _ in self.slices]
        for si, e0, e1 in self._exposed:
            acc[si][0] += e0.elapsed_time(e1)
            acc[si][1] += 1
        self._exposed = []
        return [{"slice": i, "mbytes": (sl["end"] - sl["start"]) * 4 / 1e6, "exposed_ms": a[0] / max(a[1], 1)} for i, (sl, a) in enumerate(zip(self.slices, acc))]

    def _rearm_exchange(self):
        for sl in self.slices:
            sl["done"] = False

    def _adopt_one(self, p, o):
        g = p.grad
        slot = self._slot(self.flat_grad, self._index_of[id(p)])
        if g is not None and g.data_ptr() == slot.data_ptr() and g.stride() == slot.stride():
            return
        if g is None:
            slot.zero_()
        else:
            slot.copy_(g)
        p.grad = slot

    def _adopt_grads(self):
        """A caller may have re-bound .grad (zero_grad(set_to_none=True) of a generic training loop, then autograd created fresh tensors;
        a DDP wrap handing out its bucket views): bring every gradient back into its slot of the flat buffer.  No-op in the normal case.
        Runs BEFORE the exchange (the hooks adopt the parameter they fire for; `step()` adopts the rest, i.e. parameters that got no
        gradient, whose slice no hook completed and which is therefore exchanged afterwards by `_finish_exchange`)."""
        for p, o in zip(self.params, self.offsets):
            self._adopt_one(p, o)

    @torch.no_grad()
    def step(self, closure=None, lr_scale=1.0, grad_scale=1.0):
        """all-reduce(mean) -> clip_grad_norm_(max_grad_norm) -> AdamW, no host synchronisation.  lr = param_groups[0]["lr"] * lr_scale."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with ops.on_device_of(self.flat_param):
            self._adopt_grads()
            self._finish_exchange()
            g = self.param_groups[0]
            sumsq = ops.sumsq(self.flat_grad, out=self._sumsq, ws=self._sumsq_ws)     # always: the non-finite guard needs it even without clipping
            ops.adamw_step_guarded_(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, float(g["lr"]) * lr_scale, g["betas"][0], g["betas"][1],
                                    g["eps"], g["weight_decay"], self._steps, self._coef, sumsq, grad_scale=grad_scale / self.world,
                                    max_norm=float(self.max_grad_norm or 0.0))
        self._after_step()
        return loss

    def _after_step(self):
        """the host half of `step()`: what the host must know once the device has stepped (also after a replayed graph did, CapturedTrainStep)"""
        self._rearm_exchange()
        self._claimed = [False] * len(self.params)       # a loop that clears gradients with model.zero_grad() instead of ours still gets the sink next step
        F.bump_param_epoch()

    hyper_words = 2      # the length of the device tensor `set_hyper` fills and `step_at` reads

    def _capture_key(self):
        """what a captured `step_at` bakes in by value (CapturedTrainStep's key); the learning rate is not part of it"""
        g = self.param_groups[0]
        return (tuple(g["betas"]), g["eps"], g["weight_decay"], float(self.max_grad_norm or 0.0), self.direct_grads)

    def set_hyper(self, hyper, lr_scale=1.0, grad_scale=1.0):
        """hyper (fp32 device tensor [2]) <- {lr * lr_scale, grad_scale / world}, each formed in double and rounded ONCE to fp32 as the scalar entry point's
        `c_float` argument is, written by one small fill launch each: nothing is copied from the host or read back"""
        import ctypes
        hyper[0:1].fill_(ctypes.c_float(float(self.param_groups[0]["lr"]) * lr_scale).value)
        hyper[1:2].fill_(ctypes.c_float(grad_scale / self.world).value)
        return hyper

    @torch.no_grad()
    def step_at(self, hyper):
        """The DEVICE half of `step()` for one process, with lr and grad_scale read on the device from `hyper` (`set_hyper`): adopt, `sumsq`, and
        `e2eft_adamw_step_guarded_at` — bit for bit the update of `step()` for the same fp32 values.  Capture-safe; the caller does the host half
        (`_after_step`) once per executed step, i.e. also after every replay."""
        if self.world != 1:
            raise NotImplementedError("FlatAdamW.step_at: the gradient exchange is not part of it (world size %d)" % self.world)
        with ops.on_device_of(self.flat_param):
            self._adopt_grads()
            g = self.param_groups[0]
            sumsq = ops.sumsq(self.flat_grad, out=self._sumsq, ws=self._sumsq_ws)
            ops.adamw_step_guarded_at_(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, hyper, g["betas"][0], g["betas"][1], g["eps"],
                                       g["weight_decay"], self._steps, self._coef, sumsq, max_norm=float(self.max_grad_norm or 0.0))

    def grad_norm(self):
        """global L2 norm of the (averaged) gradient — host value, synchronises.  With world > 1 and `sync_grads` this completes the exchange (each slice
        is summed once per optimizer step, so a following `step()` does not exchange again).  On a gradient-accumulation micro-step (`sync_grads` False) nothing
        is exchanged — summing a partial accumulation across ranks early and then adding local micro-gradients on top would corrupt the step —
        and the value is the norm of THIS rank's local gradient so far."""
        with ops.on_device_of(self.flat_param):
            self._adopt_grads()
            if not self.sync_grads:
                return math.sqrt(float(ops.sumsq(self.flat_grad, out=self._sumsq, ws=self._sumsq_ws).item()))
            self._finish_exchange()
            return math.sqrt(float(ops.sumsq(self.flat_grad, out=self._sumsq, ws=self._sumsq_ws).item())) / self.world

    @torch.no_grad()
    def zero_grad(self, set_to_none=None):
        """direct_grads (the default; or set_to_none=True): every `.grad` becomes None and the flat buffer is NOT cleared — the next backward's kernels write
        the gradients into their slots (see the class docstring), `step()` zeroes the slots that got none.  Otherwise (direct_grads=False, or set_to_none=False
        asked explicitly): ONE memset of the flat buffer, `.grad` stays bound to its slot and autograd accumulates into it."""
        for sl in self.slices:                           # a backward without a step() (skipped iteration): drain its exchange first,
            if sl["work"] is not None:                   # the buffer must not be rewritten under an in-flight all-reduce
                sl["work"].wait()
            sl["work"], sl["ready"] = None, 0
        self._rearm_exchange()
        self._claimed = [False] * len(self.params)
        if self.direct_grads if set_to_none is None else set_to_none:
            for p in self.params:
                p.grad = None
            return
        self.flat_grad.zero_()
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):      # autograd may have re-bound .grad (e.g. set_to_none by a caller)
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + 4 * o:
                p.grad = self._slot(self.flat_grad, i)


class GroupedFlatAdamW(FlatAdamW):
    """`FlatAdamW` over parameter groups: `GroupedFlatAdamW([{"params": ..., "lr": ...}, {"params": ..., "weight_decay": 0.0}, ...], lr=, betas=, eps=,
    weight_decay=)` as `torch.optim.AdamW` takes it — GeoWizard's trainer (GeoWizard/geowizard/training/train_depth_normal.py:428-444, see
    `geowizard_param_groups`), or no weight decay on biases and norm scales.  Up to 8 groups (E2EFT_ADAMW_MAX_GROUPS), each with its own `lr`, `betas`, `eps` and
    `weight_decay`; what a group leaves out comes from the keyword arguments.

    The flat buffer is laid out group after group, each group's parameters in its own order (torch enumerates them the same way: the indices in
    `state_dict()["param_groups"][i]["params"]` agree with a `torch.optim.AdamW` built from the same list, and checkpoints load in both directions), so group i is
    ONE range `group_ranges[i]` of the buffer.  Parameters that do not require a gradient are dropped; a group left empty stays in `param_groups` (scheduler lambdas
    and checkpoints keep lining up) and owns no elements.  Clip, guard and step counter are the whole buffer's: one `sumsq`, one `e2eft_adamw_step_groups` — the
    same two launches as `FlatAdamW.step()`, whatever the number of groups.

    `param_groups` is live: `LambdaLR(optimizer, IterExponential(...))` and `get_scheduler("constant", ...)` scale every group from its own base rate;
    `step(lr_scale=)` multiplies all of them; the `lr` property reads and writes group 0 only.  Everything that hangs on the flat layout — the 16-bit twin, the
    gradient sink (a q | k | v split across groups is not adjacent and takes the ordinary path), the exchange slices, `grad_norm()`, `EMAModel` — is FlatAdamW's."""

    def __init__(self, params, lr=3e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=1.0, n_slices=4, process_group=None,
                 external_grad_sync=False, direct_grads=True):
        from ._lib import ADAMW_MAX_GROUPS
        params = list(params)
        if not (params and isinstance(params[0], dict)):
            params = [{"params": params}]
        if len(params) > ADAMW_MAX_GROUPS:
            raise ValueError("GroupedFlatAdamW: %d parameter groups, the update kernel takes at most %d (E2EFT_ADAMW_MAX_GROUPS)" % (len(params), ADAMW_MAX_GROUPS))
        groups = []
        for g in params:
            g = dict(g)
            g["params"] = [p for p in ([g["params"]] if isinstance(g["params"], torch.Tensor) else g["params"]) if p.requires_grad]
            if "betas" in g:
                g["betas"] = tuple(g["betas"])
            groups.append(g)
        plist = [p for g in groups for p in g["params"]]
        self._init_flat(plist, groups, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay), max_grad_norm, n_slices, process_group,
                        external_grad_sync, direct_grads)
        self.group_ranges, i = [], 0
        for g in self.param_groups:           # [begin, end) of each group in the flat buffers: its parameters' slots, alignment padding included
            k = i + len(g["params"])
            begin = self.offsets[i] if i < len(self.params) else self.numel
            self.group_ranges.append((begin, self.offsets[k] if k < len(self.params) else self.numel) if k > i else (begin, begin))
            i = k
        with ops.on_device_of(self.flat_param):
            self._coef = torch.zeros(2 + 2 * len(self.param_groups), dtype=torch.float32, device=self.flat_param.device)

    @property
    def hyper_words(self):
        return 1 + len(self.param_groups)

    def _table(self, lr_scale=1.0):
        """the by-value group table of one update, read from the live `param_groups`"""
        return [(b, e, float(g["lr"]) * lr_scale, g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])
                for (b, e), g in zip(self.group_ranges, self.param_groups)]

    def _capture_key(self):
        return (tuple((b, e, tuple(g["betas"]), g["eps"], g["weight_decay"]) for (b, e), g in zip(self.group_ranges, self.param_groups)),
                float(self.max_grad_norm or 0.0), self.direct_grads)

    @torch.no_grad()
    def step(self, closure=None, lr_scale=1.0, grad_scale=1.0):
        """`FlatAdamW.step` with every group's own hyper-parameters: lr of group i = param_groups[i]["lr"] * lr_scale"""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with ops.on_device_of(self.flat_param):
            self._adopt_grads()
            self._finish_exchange()
            sumsq = ops.sumsq(self.flat_grad, out=self._sumsq, ws=self._sumsq_ws)
            ops.adamw_step_groups_(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self._table(lr_scale), self._steps, self._coef, sumsq,
                                   grad_scale=grad_scale / self.world, max_norm=float(self.max_grad_norm or 0.0))
        self._after_step()
        return loss

    def set_hyper(self, hyper, lr_scale=1.0, grad_scale=1.0):
        """hyper (fp32 device tensor [1 + n_groups]) <- {grad_scale / world, lr[0] * lr_scale, ...}, each formed in double and rounded ONCE to fp32 as the by-value
        entry point's `float` fields are, one small fill launch per word"""
        import ctypes
        hyper[0:1].fill_(ctypes.c_float(grad_scale / self.world).value)
        for i, g in enumerate(self.param_groups):
            hyper[1 + i:2 + i].fill_(ctypes.c_float(float(g["lr"]) * lr_scale).value)
        return hyper

    @torch.no_grad()
    def step_at(self, hyper):
        """The device half of `step()` with grad_scale and the groups' learning rates read on the device from `hyper` (`set_hyper`): adopt, `sumsq`,
        `e2eft_adamw_step_groups_at`.  Capture-safe; see `FlatAdamW.step_at`."""
        if self.world != 1:
            raise NotImplementedError("GroupedFlatAdamW.step_at: the gradient exchange is not part of it (world size %d)" % self.world)
        with ops.on_device_of(self.flat_param):
            self._adopt_grads()
            sumsq = ops.sumsq(self.flat_grad, out=self._sumsq, ws=self._sumsq_ws)
            ops.adamw_step_groups_at_(self.flat_param, self.flat_grad, self.exp_avg, self.exp_avg_sq, self._table(), hyper, self._steps, self._coef, sumsq,
                                      max_norm=float(self.max_grad_norm or 0.0))


def geowizard_param_groups(unet, learning_rate, class_embedding_lr_mult=10.0):
    """The two parameter groups of GeoWizard's trainer (GeoWizard/geowizard/training/train_depth_normal.py:428-440): every parameter whose name contains
    'class_embedding' at `learning_rate * class_embedding_lr_mult` (`--class_embedding_lr_mult`, default 10: the embedding is freshly initialised), everything else
    at `learning_rate`.  A UNet without a class embedding gives an empty second group, as the reference's loop does.  Pass the list to `GroupedFlatAdamW` (or
    `torch.optim.AdamW`) with `betas=`, `weight_decay=`, `eps=` as lines 441-443 do.
    With `--scale_lr` (lines 411-414) pass learning_rate = learning_rate * gradient_accumulation_steps * train_batch_size * num_processes."""
    params, params_class_embedding = [], []
    for name, param in unet.named_parameters():
        (params_class_embedding if "class_embedding" in name else params).append(param)
    return [{"params": params, "lr": learning_rate}, {"params": params_class_embedding, "lr": learning_rate * class_embedding_lr_mult}]


class EMAModel:
    """`diffusers.training_utils.EMAModel` as GeoWizard's training script uses it (GeoWizard/geowizard/training/train_depth_normal.py:352-353 construct, :785-786
    `step` after every optimizer step, :843-850 `store` / `copy_to` / `restore` around validation, :380-381,388-391 `save_pretrained` / `from_pretrained` /
    `load_state_dict` in the accelerate hooks).  diffusers (0.30.2, third-party) is not in the tree: the constructor arguments, `get_decay`, `step`'s update
    `shadow -= (1 - decay) * (shadow - param)` and the `state_dict` keys are restated from its published definition (tests pin the arithmetic to that
    formula evaluated by torch).

    MI355X-first: when the parameters live in a FlatAdamW buffer (construct the optimizer first) the shadow is ONE flat fp32 buffer with the same layout and
    `step()` is ONE `e2eft_ema_step` launch over it (12 B per parameter, HBM-bound: 10.4 GB -> ~2 ms for the SD-v2 UNet, against 686 x 3 elementwise torch launches);
    `copy_to` / `store` / `restore` are flat device copies (the reference parks the stored copy on the host: 288 GB of HBM make that unnecessary) and bump the
    parameter epoch so that 16-bit weight twins and packed weights are rebuilt.  `shadow_params` stays a list of per-parameter tensors (views of the flat
    shadow).  Parameters outside a flat buffer take the per-tensor form of the same update (torch ops: host-side plumbing, as diffusers does it)."""

    def __init__(self, parameters, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3, foreach=False,
                 model_cls=None, model_config=None, **kwargs):
        parameters = list(parameters)
        self.decay, self.min_decay, self.update_after_step = decay, min_decay, update_after_step
        self.use_ema_warmup, self.inv_gamma, self.power = use_ema_warmup, inv_gamma, power
        self.optimization_step = 0
        self.cur_decay_value = None
        self.temp_stored_params = None
        self.model_cls, self.model_config = model_cls, model_config
        self._flat = self._flat_source(parameters)
        if self._flat is not None:
            owner, flat = self._flat
            with ops.on_device_of(flat):
                self._shadow_flat = flat.detach().clone()
            self.shadow_params = [owner._slot(self._shadow_flat, i) for i in range(len(owner.params))]
        else:
            self._shadow_flat = None
            self.shadow_params = [p.clone().detach() for p in parameters]

    @staticmethod
    def _flat_source(parameters):
        """(FlatAdamW, its flat parameter buffer) when `parameters` are exactly that optimizer's parameters, in its order; else None"""
        tags = [getattr(p, "_e2eft_gslot", None) for p in parameters]
        if not parameters or any(t is None for t in tags):
            return None
        owner = tags[0][0]()
        if owner is None or len(owner.params) != len(parameters) or any(a is not b for a, b in zip(owner.params, parameters)):
            return None
        if any(p.data_ptr() != owner.flat_param.data_ptr() + 4 * o for p, o in zip(parameters, owner.offsets)):
            return None
        return owner, owner.flat_param

    def get_decay(self, optimization_step):
        step = max(0, optimization_step - self.update_after_step - 1)
        if step <= 0:
            return 0.0
        cur = 1 - (1 + step / self.inv_gamma) ** -self.power if self.use_ema_warmup else (1 + step) / (10 + step)
        return max(min(cur, self.decay), self.min_decay)

    @torch.no_grad()
    def step(self, parameters):
        parameters = list(parameters)
        self.optimization_step += 1
        decay = self.get_decay(self.optimization_step)
        self.cur_decay_value = decay
        omd = 1 - decay
        src = self._flat_source(parameters) if self._shadow_flat is not None else None
        # the one-launch form updates EVERY slot; diffusers copies a parameter that does not require a gradient instead of averaging it (below):
        # the flat kernel therefore runs only when every parameter of the buffer is trainable
        if src is not None and src[1].numel() == self._shadow_flat.numel() and all(p.requires_grad for p in parameters):
            with ops.on_device_of(src[1]):
                ops.ema_step_(self._shadow_flat, src[1], omd)
            return
        for s_param, param in zip(self.shadow_params, parameters):
            if param.requires_grad:
                s_param.sub_(omd * (s_param - param))
            else:
                s_param.copy_(param)

    def _one_launch_source(self, parameters, what):
        """the flat parameter buffer the one-launch form reads, or the reason why this EMA has no such form"""
        parameters = list(parameters)
        src = self._flat_source(parameters) if self._shadow_flat is not None else None
        if src is None or src[1].numel() != self._shadow_flat.numel():
            raise NotImplementedError("EMAModel.%s: the capture-safe EMA is the flat one-launch form: the shadow must lie over a FlatAdamW buffer and `parameters` "
                                      "must be that optimizer's parameters in its order (construct the optimizer first, then EMAModel(unet.parameters()))" % what)
        if not all(p.requires_grad for p in parameters):
            raise NotImplementedError("EMAModel.%s: a parameter that does not require a gradient is copied, not averaged; the one-launch form averages every "
                                      "slot, so it runs only when every parameter of the buffer is trainable" % what)
        return src[1]

    def set_decay_word(self, word):
        """The HOST half of `step`: `optimization_step += 1`, `get_decay`, `cur_decay_value`, and word (one-element fp32 device tensor) <- (float)(1 - decay) — the
        value `ops.ema_step_` receives from `step` — by one small fill launch: nothing is copied from the host or read back.  Call it once per optimizer step,
        before the launch (or the replay) of `step_at`."""
        import ctypes
        if self._shadow_flat is None:
            raise NotImplementedError("EMAModel.set_decay_word: the capture-safe EMA is the flat one-launch form: the shadow must lie over a FlatAdamW buffer")
        self._one_launch_source(self._flat[0].params, "set_decay_word")      # (the optimizer the shadow was laid over: still flat, every parameter trainable)
        self.optimization_step += 1
        decay = self.get_decay(self.optimization_step)
        self.cur_decay_value = decay
        word.fill_(ctypes.c_float(1 - decay).value)
        return word

    @torch.no_grad()
    def step_at(self, parameters, word):
        """The DEVICE half of `step`: ONE `e2eft_ema_step_at` launch over the flat shadow with 1 - decay read on the device from `word` (`set_decay_word`) — bit
        for bit the update of `step` for the same value.  Capture-safe; only the flat one-launch form exists (refused otherwise, with the reason)."""
        flat = self._one_launch_source(parameters, "step_at")
        with ops.on_device_of(flat):
            ops.ema_step_at_(self._shadow_flat, flat, word)

    @torch.no_grad()
    def copy_to(self, parameters):
        parameters = list(parameters)
        src = self._flat_source(parameters) if self._shadow_flat is not None else None
        if src is not None and src[1].numel() == self._shadow_flat.numel():
            src[1].copy_(self._shadow_flat)
        else:
            for s_param, param in zip(self.shadow_params, parameters):
                param.data.copy_(s_param.to(param.device).data)
        F.bump_param_epoch()          # (`.data.copy_` moves no version counter: derived 16-bit / packed weights are keyed on the epoch)

    @torch.no_grad()
    def store(self, parameters):
        parameters = list(parameters)
        src = self._flat_source(parameters) if self._shadow_flat is not None else None
        self.temp_stored_params = src[1].detach().clone() if src is not None else [p.detach().clone() for p in parameters]

    @torch.no_grad()
    def restore(self, parameters):
        if self.temp_stored_params is None:
            raise RuntimeError("This ExponentialMovingAverage has no `store()`ed weights to `restore()`")
        parameters = list(parameters)
        if isinstance(self.temp_stored_params, torch.Tensor):
            src = self._flat_source(parameters)
            if src is not None and src[1].numel() == self.temp_stored_params.numel():
                src[1].copy_(self.temp_stored_params)
            else:   # `parameters` are not (any more) the optimizer's list in its order: per-slot copies out of the stored flat buffer, in the stored order
                owner = self._flat[0]
                if len(parameters) != len(owner.params):
                    raise ValueError("restore(): %d parameters were stored, %d given" % (len(owner.params), len(parameters)))
                for i, param in enumerate(parameters):
                    param.data.copy_(owner._slot(self.temp_stored_params, i))
        else:
            for c_param, param in zip(self.temp_stored_params, parameters):
                param.data.copy_(c_param.data)
        self.temp_stored_params = None
        F.bump_param_epoch()

    def to(self, device=None, dtype=None):
        if self._shadow_flat is not None:
            if device is not None and torch.device(device) != self._shadow_flat.device or dtype not in (None, torch.float32):
                raise ValueError("EMAModel over a FlatAdamW buffer lives where the buffer lives (fp32 on %s)" % self._shadow_flat.device)
            return
        self.shadow_params = [p.to(device=device, dtype=dtype) if p.is_floating_point() else p.to(device=device) for p in self.shadow_params]

    def state_dict(self):
        return {"decay": self.decay, "min_decay": self.min_decay, "optimization_step": self.optimization_step, "update_after_step": self.update_after_step,
                "use_ema_warmup": self.use_ema_warmup, "inv_gamma": self.inv_gamma, "power": self.power, "shadow_params": self.shadow_params}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        for k in ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power"):
            setattr(self, k, state_dict.get(k, getattr(self, k)))
        if not 0.0 <= self.decay <= 1.0:
            raise ValueError("Decay must be between 0 and 1")
        sp = state_dict.get("shadow_params", None)
        if sp is not None:
            if len(sp) != len(self.shadow_params) or not all(isinstance(t, torch.Tensor) for t in sp):
                raise ValueError("shadow_params must be a list of %d tensors" % len(self.shadow_params))
            for mine, theirs in zip(self.shadow_params, sp):
                mine.copy_(theirs)

    def save_pretrained(self, path):
        """the EMA weights as a model checkpoint whose config carries the EMA hyper-parameters (diffusers' layout: `unet_ema/`)"""
        if self.model_cls is None or self.model_config is None:
            raise ValueError("`save_pretrained` can only be used if `model_cls` and `model_config` were defined at __init__.")
        model = self.model_cls(**{k: v for k, v in dict(self.model_config).items() if not k.startswith("_")})
        sd = self.state_dict()
        sd.pop("shadow_params")
        model.register_to_config(**sd)
        with torch.no_grad():
            for s_param, param in zip(self.shadow_params, model.parameters()):
                param.copy_(s_param.to(param.device))
        model.save_pretrained(path)

    @classmethod
    def from_pretrained(cls, path, model_cls):
        """diffusers: `model_cls.load_config(path, return_unused_kwargs=True)` splits the EMA hyper-parameters off the model config; here the model loader
        ignores keys it does not know, and the EMA keys are read from the same config.json"""
        import json
        import os
        with open(os.path.join(path, model_cls.config_name)) as f:
            raw = json.load(f)
        ema_kwargs = {k: raw[k] for k in ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power") if k in raw}
        model = model_cls.from_pretrained(path)
        ema = cls(model.parameters(), model_cls=model_cls, model_config=model.config)
        ema.load_state_dict(ema_kwargs)
        return ema


def lr_lambda_for_world(lr_total_iter_length, lr_exp_warmup_steps, num_processes=None, final_ratio=0.01):
    """the `lr_func` of training/train.py:356: `accelerate` steps a prepared scheduler `num_processes` times per optimizer step, so the reference stretches BOTH
    lengths by the number of processes.  With `LambdaLR(FlatAdamW, ...)` stepped once per optimizer step (no accelerate wrapper) pass num_processes=1; under
    `accelerator.prepare(lr_scheduler)` pass the world size (default: torch.distributed's), exactly as the reference does."""
    if num_processes is None:
        num_processes = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
    return IterExponential(total_iter_length=lr_total_iter_length * num_processes, final_ratio=final_ratio, warmup_steps=lr_exp_warmup_steps * num_processes)


def train_step(unet, vae, optimizer, batches, empty_encoding, modality="depth", lr_scale=1.0, gather_loss=False, train_batch_size=1):
    """One optimizer step over `batches` (a list of micro-batches = gradient accumulation, train.py:470,559-566): returns the
    mean micro-loss as a device tensor.  gather_loss=True: every micro-step's loss is averaged over the ranks as train.py:559 does for logging
    (`dist.gather_mean`: one small all-gather per micro-step, no host synchronisation).  train_batch_size: the CONFIGURED per-rank batch size the
    reference repeats the loss by (`args.train_batch_size`, a constant — never the size of the batch at hand: a ragged last batch would make the ranks'
    all-gather sizes differ; the repeat does not change the mean)."""
    from . import dist as D
    n = len(batches)
    total = None
    for i, batch in enumerate(batches):
        optimizer.sync_grads = i == n - 1
        loss = e2e_ft_loss(unet, vae, batch, empty_encoding, modality)
        (loss / n).backward()
        if gather_loss:
            loss = D.gather_mean(loss, train_batch_size)
        total = loss.detach() if total is None else total + loss.detach()
    optimizer.step(lr_scale=lr_scale)
    optimizer.zero_grad()
    return total / n


class CapturedTrainStep:
    """`train_step` replayed from hipGraphs: `step = CapturedTrainStep(unet, vae, optimizer, empty_encoding, modality, ...)`, then
    `step(batches, lr_scale=1.0)` is one optimizer step over `len(batches) == accumulation` micro-batches followed by `zero_grad`, and returns the mean micro-loss
    as a device tensor — `train_step`'s contract, and its results bit for bit.  `CapturedTrainStep.geowizard(unet, vae, optimizer, domain, depth_scale,
    normal_scale, ...)` is the same object around `geowizard_e2e_ft_loss`; it is called as `step(batches, lr_scale, imgs_embed=[one [b,1,X] embedding per
    micro-batch])`.

    Per key — micro-batch shapes and dtypes, modality / loss, noise_type (and the generator's seed, which travels by value), activation recompute, compute dtype,
    accumulation, the optimizer's by-value hyper-parameters — the FIRST call runs eagerly and is a real step (it fills what the library sizes lazily), the
    SECOND captures and then replays, later calls only replay.  An entry is up to three graphs over one memory pool:
      first   micro-step 0: the parameter epoch is bumped before the capture, so every weight derived from the parameters (the 16-bit twin's cast, packed /
              concatenated / phase weights) is REBUILT inside it, and the gradients are written into the flat buffer;
      later   micro-steps 1 .. accumulation-1 (absent for accumulation == 1): derived weights reused, gradients accumulated in place;
      update  `FlatAdamW.step_at`: adopt, `sumsq`, `e2eft_adamw_step_guarded_at`, which reads lr and grad_scale from two device words the host fills before the
              replay — a scheduler-driven lr and a changing lr_scale need no recapture.  A `GroupedFlatAdamW` is stepped the same way
              (`e2eft_adamw_step_groups_at`, `optimizer.hyper_words` = 1 + n_groups device words; every group's range, betas, eps and weight decay are in the key).
    The micro-batch is copied into static buffers before each replay (host or device tensors).  After every step, replayed or not, the host does what
    `FlatAdamW.step()` + `zero_grad()` leave behind: slices re-armed, claims cleared, `.grad` None, the parameter epoch bumped — so an eager forward of the same
    UNet between steps rebuilds its derived weights from the new parameters, and `state_dict()` / `skipped_steps()` / `step_count` read the device words the
    graph advanced.  Gradients: the optimizer's own mode (direct_grads: the captured backward kernels write the flat buffer's slots, exactly as eagerly — what the
    host decides while capturing is what an eager step decides, and the replay repeats its launches).

    noise_type "zeros" / None are captured as they are; "gaussian" needs a `noise.DeviceNoise` and draws through `noise.randn_at`, the draw set before each
    micro-step's replay (`noise.set_draw`): every micro-step sees what the eager sequence on that generator would have drawn.

    Refused: "pyramid" / "geowizard_pyramid" (their level sizes are host draws, so the launches differ from call to call); a world size above 1 or an optimizer
    with exchange hooks (RCCL inside a capture is not built); `gather_loss`; the diffusion objective (its timesteps are drawn per step); an EMA inside the step
    (call `EMAModel.step` after it, eagerly).  A changed frozen VAE, or `unet.to(...)`, needs a new object: graphs bake addresses."""

    MAX_ENTRIES = 4

    def __init__(self, unet, vae, optimizer, empty_encoding=None, modality="depth", noise_type="zeros", generator=None, accumulation=1, gather_loss=False,
                 ema=None, loss="e2e_ft", domain="indoor", depth_scale=0.5, normal_scale=1.0):
        from . import noise as N
        if loss == "diffusion":
            raise NotImplementedError("CapturedTrainStep: the diffusion objective draws its timesteps per step on the host's generator; it is not captured")
        if loss not in ("e2e_ft", "geowizard"):
            raise ValueError("CapturedTrainStep: loss must be 'e2e_ft' or 'geowizard', got %r" % (loss,))
        if noise_type in ("pyramid", "geowizard_pyramid"):
            raise ValueError("CapturedTrainStep: noise_type=%r is not captured: its level sizes are fresh host draws per call, so the launches of one step are "
                             "not the launches of the next; use train_step" % noise_type)
        if noise_type not in ("zeros", "gaussian") + ((None,) if loss == "e2e_ft" else ()):
            raise ValueError("Unknown noise type %s" % noise_type)
        if noise_type == "gaussian" and (not isinstance(generator, N.DeviceNoise) or isinstance(generator, N.DrawAt)):
            raise TypeError("CapturedTrainStep: noise_type='gaussian' draws on the device: pass generator=noise.DeviceNoise(seed)")
        if gather_loss:
            raise NotImplementedError("CapturedTrainStep: gather_loss is a collective per micro-step; RCCL inside a capture is not built")
        if ema is not None:
            raise NotImplementedError("CapturedTrainStep: the EMA stays an eager call after the step (EMAModel.step)")
        self._init_common(unet, vae, optimizer, empty_encoding, modality, noise_type, generator, accumulation, loss, domain, depth_scale, normal_scale)

    def _init_common(self, unet, vae, optimizer, empty_encoding, modality, noise_type, generator, accumulation, loss, domain, depth_scale, normal_scale):
        """what every captured step checks and holds, whatever loss and noise it was built for (the mode-specific refusals come before it)"""
        if not isinstance(optimizer, FlatAdamW):
            raise TypeError("CapturedTrainStep steps a FlatAdamW (the update it captures is FlatAdamW.step_at)")
        if getattr(optimizer, "world", 1) != 1 or optimizer._hooks:
            raise NotImplementedError("CapturedTrainStep: world size %s / gradient-exchange hooks: RCCL inside a capture is not built; use train_step"
                                      % getattr(optimizer, "world", 1))
        if loss == "e2e_ft" and empty_encoding is None:
            raise ValueError("CapturedTrainStep: empty_encoding is required")
        if int(accumulation) < 1:
            raise ValueError("CapturedTrainStep: accumulation must be >= 1")
        self.unet, self.vae, self.optimizer = unet, vae, optimizer
        self.empty_encoding, self.modality, self.noise_type, self.generator = empty_encoding, modality, noise_type, generator
        self.accumulation, self.loss = int(accumulation), loss
        self.domain, self.depth_scale, self.normal_scale = domain, depth_scale, normal_scale
        self._entries = {}
        with ops.on_device_of(optimizer.flat_param):
            self._hyper = torch.zeros(optimizer.hyper_words, dtype=torch.float32, device=optimizer.flat_param.device)

    @classmethod
    def geowizard(cls, unet, vae, optimizer, domain="indoor", depth_scale=0.5, normal_scale=1.0, noise_type="zeros", generator=None, accumulation=1, **kw):
        """the same step around `geowizard_e2e_ft_loss`; call it as `step(batches, lr_scale, imgs_embed=[...])`"""
        return cls(unet, vae, optimizer, None, None, noise_type, generator, accumulation, loss="geowizard", domain=domain, depth_scale=depth_scale,
                   normal_scale=normal_scale, **kw)

    # ---- one entry: static buffers + graphs.  Data only — no bound method, no closure over self (a cycle would hand the graphs to the cyclic collector, and a
    # graph destroyed inside a later capture aborts the process; pipeline._dn_entry) -------------------------------------------------------------------------
    def _fields(self):
        if self.loss == "geowizard":
            return ("rgb", "val_mask", "metric", "normals")
        return ("rgb", "val_mask", "metric" if self.modality == "depth" else "normals")

    def _mode_key(self):
        """the part of the key that does not depend on the micro-batch (read once per call: the recompute flag walks the modules)"""
        core = getattr(self.unet, "module", self.unet)
        recompute = core.training and any(getattr(m, "gradient_checkpointing", False) for net in (core, self.vae) for m in net.modules())
        return (self.loss, self.modality, self.domain, self.depth_scale, self.normal_scale, self.noise_type,
                self.generator.seed if self.noise_type == "gaussian" else None, bool(recompute), getattr(core, "compute_dtype", core.dtype),
                self.accumulation) + self.optimizer._capture_key()

    def _batch_key(self, batch, embed):
        return (tuple((k, tuple(batch[k].shape), batch[k].dtype) for k in self._fields()), None if embed is None else (tuple(embed.shape), embed.dtype))

    def _new_entry(self, batch, embed):
        from . import noise as N
        core = getattr(self.unet, "module", self.unet)
        dev, dt = core.device, getattr(core, "compute_dtype", core.dtype)
        ent = {"batch": {k: torch.empty(batch[k].shape, dtype=batch[k].dtype, device=dev) for k in self._fields()},
               "embed": None if embed is None else torch.empty(embed.shape, dtype=embed.dtype, device=dev),
               "ctx": None if self.empty_encoding is None else self.empty_encoding.detach().to(device=dev, dtype=dt),
               "total": torch.zeros((), dtype=torch.float32, device=dev), "draw": torch.zeros(1, dtype=torch.int64, device=dev), "graphs": None, "alive": None}
        ent["gen"] = N.DrawAt(self.generator.seed, ent["draw"]) if self.noise_type == "gaussian" else None
        return ent

    def _takes_embed(self):
        """the GeoWizard UNet: one image embedding per micro-batch, and the class embedding read in place"""
        return self.loss == "geowizard"

    def _loss(self, ent):
        if self.loss == "geowizard":
            return geowizard_e2e_ft_loss(self.unet, self.vae, ent["batch"], ent["embed"], self.domain, self.depth_scale, self.normal_scale,
                                         noise_type=self.noise_type, generator=ent["gen"])
        return e2e_ft_loss(self.unet, self.vae, ent["batch"], ent["ctx"], self.modality, noise_type=self.noise_type, generator=ent["gen"])

    def _feed(self, ent):
        """before a micro-step runs or is replayed: the device words its draws read, from the caller's generator (the source of truth)"""
        from . import noise as N
        if ent["gen"] is not None:
            N.set_draw(ent["draw"], self.generator)

    def _alive(self, ent):
        """what the captured forward reads in place: it must exist before the capture and outlive it"""
        if self._takes_embed():
            core = getattr(self.unet, "module", self.unet)
            return geowizard_class_embedding(ent["batch"]["rgb"].shape[0], self.domain, getattr(core, "compute_dtype", core.dtype), core.device)
        return None

    def _update(self):
        """the update graph's content (and the eager first call's update): only device work on the current stream"""
        self.optimizer.step_at(self._hyper)

    def _micro(self, ent, first):
        """one micro-step on the entry's static buffers: `train_step`'s loop body.  Only device work on the current stream."""
        loss = self._loss(ent)
        (loss / self.accumulation).backward()
        if first:
            ent["total"].copy_(loss.detach())
        else:
            ent["total"].add_(loss.detach())

    def _capture(self, ent):
        from . import modules as M
        opt = self.optimizer
        ent["alive"] = self._alive(ent)
        F.bump_param_epoch()              # every derived weight misses its cache: its builder's launches become part of the first graph
        torch.cuda.synchronize()
        pool = torch.cuda.graph_pool_handle()
        graphs = {"first": torch.cuda.CUDAGraph(), "later": torch.cuda.CUDAGraph() if self.accumulation > 1 else None, "update": torch.cuda.CUDAGraph()}
        keep, M.PRESERVE_RNG_STATE = M.PRESERVE_RNG_STATE, False
        try:
            with torch.cuda.graph(graphs["first"], pool=pool):
                self._micro(ent, True)
            if graphs["later"] is not None:
                with torch.cuda.graph(graphs["later"], pool=pool):
                    self._micro(ent, False)
            with torch.cuda.graph(graphs["update"], pool=pool):
                self._update()
        finally:
            M.PRESERVE_RNG_STATE = keep
            # nothing captured has run: the host goes back to the state before a step (gradients of the capture are addresses inside the graphs now)
            opt._after_step()
            opt.zero_grad()
        ent["graphs"] = graphs

    def _set_step_words(self, lr_scale):
        """once per optimizer step, before any launch of it: the device words the update reads"""
        self.optimizer.set_hyper(self._hyper, lr_scale)

    def __call__(self, batches, lr_scale=1.0, imgs_embed=None):
        n = self.accumulation
        if len(batches) != n:
            raise ValueError("CapturedTrainStep: %d micro-batches given, accumulation is %d (the graphs of an entry are one optimizer step)" % (len(batches), n))
        if self._takes_embed():
            if imgs_embed is None or len(imgs_embed) != n:
                raise ValueError("CapturedTrainStep.geowizard: imgs_embed must hold one embedding per micro-batch (%d)" % n)
        elif imgs_embed is not None:
            raise ValueError("CapturedTrainStep: imgs_embed belongs to the GeoWizard step")
        opt = self.optimizer
        if opt.world != 1 or opt._hooks:
            raise NotImplementedError("CapturedTrainStep: world size %s / gradient-exchange hooks: RCCL inside a capture is not built" % opt.world)
        embeds = imgs_embed if imgs_embed is not None else [None] * n
        keys = [self._batch_key(b, e) for b, e in zip(batches, embeds)]
        if any(k != keys[0] for k in keys[1:]):
            raise ValueError("CapturedTrainStep: the micro-batches of one step must share shapes and dtypes")
        key = keys[0] + self._mode_key()
        with ops.on_device_of(opt.flat_param):
            ent = self._entries.get(key)
            if ent is None:
                while len(self._entries) >= self.MAX_ENTRIES:          # (released here, outside any capture)
                    del self._entries[next(iter(self._entries))]
                ent = self._entries[key] = self._new_entry(batches[0], embeds[0])
            elif ent["graphs"] is None:
                self._capture(ent)
            graphs = ent["graphs"]
            self._set_step_words(lr_scale)
            opt.sync_grads = True
            for i, (batch, embed) in enumerate(zip(batches, embeds)):
                for k, t in ent["batch"].items():
                    t.copy_(batch[k])
                if embed is not None:
                    ent["embed"].copy_(embed)
                self._feed(ent)
                if graphs is None:
                    self._micro(ent, i == 0)
                else:
                    graphs["first" if i == 0 else "later"].replay()
            if graphs is None:
                self._update()
            else:
                graphs["update"].replay()
            opt._after_step()
            opt._opt_called = True          # (what torch's lr schedulers look at before they warn about a scheduler stepped ahead of its optimizer)
            opt.zero_grad()
            return ent["total"] / n


class CapturedTrainStepAt(CapturedTrainStep):
    """`CapturedTrainStep` for what the base class refuses because it changes from step to step on the host: every such value moves from a
    launch argument into device words that belong to the graphs, and the host fills those words before the replay — what §3.26 did for `lr` and the Gaussian draw.

      noise_type="pyramid" (E2E-FT loss) / "geowizard_pyramid" (both GeoWizard losses; the name "pyramid" stays refused there, GEOWIZARD_PYRAMID_MESSAGE):
          the level sizes are drawn on the host per micro-step, in micro-step order, by `noise.pyramid_level_sizes` / `noise.geowizard_pyramid_level_sizes` from
          Python's `random` / numpy's global stream — both end where the eager loop leaves them — and written with `noise.set_pyramid_table` before that
          micro-step's replay; the captured kernels are `e2eft_pyramid_noise_at` / `e2eft_pyramid_noise_weighted_at`.
      loss="diffusion" (`CapturedTrainStepAt.diffusion(unet, vae, optimizer, domain, noise_scheduler, prediction_type, noise_type, generator=, accumulation=,
          ema=)`, called as `step(batches, lr_scale, imgs_embed=[...])` with the fields rgb / depth / normals / val_mask): `geowizard_diffusion_loss` with
          `timesteps=` the generator — the timesteps come from the caller's `noise.DeviceNoise` (`e2eft_randint_fill_at`), drawn before the noise, so a generator
          is needed even with noise_type="zeros".  The timesteps are not torch's: the eager loop this step reproduces passes `timesteps=generator` too.
      ema=EMAModel: `EMAModel.step_at` is the LAST node of the update graph (it also runs after a step the guard skipped, as the eager call and diffusers do) and
          the decay word is filled next to `set_hyper` (`EMAModel.set_decay_word`).  Only the flat one-launch EMA over this optimizer's buffer.

    One micro-step may make two draws (timesteps, then noise): its `noise.DrawAt` carries one device word per draw and, for the pyramids, the table; each reads the
    value `generator.next_draw()` returns at that point of the eager order.  The key gains the loss, the prediction type, `num_train_timesteps`, the discount, the
    generator's seed and the identity of the EMA's shadow; the entry keeps alive what the graphs read in place (the scheduler's `alphas_cumprod` table on the
    device, the class embedding; the timestep tensor is an allocation of the graphs' own pool).  Everything else — eager first call, capturing second,
    `GroupedFlatAdamW`, activation recompute, static input buffers — is inherited.

    Still refused, before any capture: world size > 1 / exchange hooks, `gather_loss`, an EMA that is not the flat one-launch form over this optimizer."""

    DISCOUNT = 0.9            # what `e2e_ft_loss` / the GeoWizard losses draw their pyramids with (the default of noise.*pyramid_noise_into)

    def __init__(self, unet, vae, optimizer, empty_encoding=None, modality="depth", noise_type="zeros", generator=None, accumulation=1, gather_loss=False,
                 ema=None, loss="e2e_ft", domain="indoor", depth_scale=0.5, normal_scale=1.0, noise_scheduler=None, prediction_type=None):
        from . import noise as N
        if loss not in ("e2e_ft", "geowizard", "diffusion"):
            raise ValueError("CapturedTrainStepAt: loss must be 'e2e_ft', 'geowizard' or 'diffusion', got %r" % (loss,))
        if loss != "e2e_ft" and noise_type == "pyramid":
            raise ValueError(GEOWIZARD_PYRAMID_MESSAGE)
        if noise_type not in (("zeros", "gaussian", "pyramid", None) if loss == "e2e_ft" else ("zeros", "gaussian", "geowizard_pyramid")):
            raise ValueError("Unknown noise type %s" % noise_type)
        draws = loss == "diffusion" or noise_type in ("gaussian", "pyramid", "geowizard_pyramid")
        if draws and (not isinstance(generator, N.DeviceNoise) or isinstance(generator, N.DrawAt)):
            raise TypeError("CapturedTrainStepAt: %s draws on the device: pass generator=noise.DeviceNoise(seed)"
                            % ("the diffusion objective (its timesteps)" if loss == "diffusion" else "noise_type=%r" % noise_type))
        if gather_loss:
            raise NotImplementedError("CapturedTrainStepAt: gather_loss is a collective per micro-step; RCCL inside a capture is not built")
        self._init_common(unet, vae, optimizer, empty_encoding, modality, noise_type, generator, accumulation, loss, domain, depth_scale, normal_scale)
        self.ema, self.noise_scheduler, self.prediction_type = ema, noise_scheduler, prediction_type
        if loss == "diffusion":
            if noise_scheduler is None:
                from .scheduler import DDPMScheduler
                self.noise_scheduler = DDPMScheduler()            # ONE scheduler for every step: its device table is uploaded once, outside any capture
            self.prediction_type = prediction_type if prediction_type is not None else self.noise_scheduler.config.prediction_type
            if self.prediction_type not in ("epsilon", "v_prediction"):
                raise ValueError("Unknown prediction type %s" % self.prediction_type)
        if ema is not None:
            if not isinstance(ema, EMAModel):
                raise TypeError("CapturedTrainStepAt: ema must be a training.EMAModel")
            ema._one_launch_source(optimizer.params, "step_at")            # (raises with the reason)
            if ema._flat[0] is not optimizer:
                raise NotImplementedError("CapturedTrainStepAt: the EMA's shadow must lie over THIS optimizer's flat buffer")
            with ops.on_device_of(optimizer.flat_param):
                self._ema_word = torch.zeros(1, dtype=torch.float32, device=optimizer.flat_param.device)

    @classmethod
    def diffusion(cls, unet, vae, optimizer, domain="indoor", noise_scheduler=None, prediction_type=None, noise_type="gaussian", generator=None, accumulation=1,
                  ema=None, **kw):
        """the same step around `geowizard_diffusion_loss` (GeoWizard's default objective); call it as `step(batches, lr_scale, imgs_embed=[...])`"""
        return cls(unet, vae, optimizer, None, None, noise_type, generator, accumulation, ema=ema, loss="diffusion", domain=domain, noise_scheduler=noise_scheduler,
                   prediction_type=prediction_type, **kw)

    def _pyramid(self):
        return self.noise_type in ("pyramid", "geowizard_pyramid")

    def _takes_embed(self):
        return self.loss in ("geowizard", "diffusion")

    def _fields(self):
        if self.loss == "diffusion":
            return ("rgb", "depth", "normals", "val_mask")
        return super()._fields()

    def _mode_key(self):
        T = self.noise_scheduler.config.num_train_timesteps if self.loss == "diffusion" else None
        return super()._mode_key() + (None if self.generator is None else self.generator.seed, self.prediction_type, T, self.DISCOUNT if self._pyramid() else None,
                                      None if self.ema is None else self.ema._shadow_flat.data_ptr())

    def _new_entry(self, batch, embed):
        from . import noise as N
        ent = super()._new_entry(batch, embed)
        dev = ent["total"].device
        words = int(self.loss == "diffusion") + int(self.noise_type == "gaussian")
        ent["draw"] = torch.zeros(2, dtype=torch.int64, device=dev)                          # one word per draw site of a micro-step: [timesteps, Gaussian noise]
        ent["table"] = torch.zeros(ops.PYRAMID_TABLE_WORDS, dtype=torch.int64, device=dev) if self._pyramid() else None      # (its word 0 is the pyramid's draw)
        f = 2 ** (len(self.vae.config.block_out_channels) - 1)
        ent["hw"] = (batch["rgb"].shape[-2] // f, batch["rgb"].shape[-1] // f)               # the latent grid the level sizes are drawn for
        ent["gen"] = (N.DrawAt(self.generator.seed, ent["draw"][1:2], ent["table"], ent["hw"], randint_dev=ent["draw"][0:1])
                      if (words or self._pyramid()) else None)
        return ent

    def _loss(self, ent):
        if self.loss == "diffusion":
            return geowizard_diffusion_loss(self.unet, self.vae, ent["batch"], ent["embed"], self.domain, self.noise_scheduler, self.noise_type, ent["gen"],
                                            timesteps=ent["gen"], prediction_type=self.prediction_type)
        return super()._loss(ent)

    def _feed(self, ent):
        """the words of this micro-step's draws, in the eager order: timesteps, then noise; the level sizes are the host draw the eager loss would make here"""
        from . import noise as N
        if self.loss == "diffusion":
            N.set_draw(ent["gen"].randint_dev, self.generator)
        if self.noise_type == "gaussian":
            N.set_draw(ent["gen"].draw_dev, self.generator)
        elif self._pyramid():
            rows, cols = ent["hw"]
            sizes = N.pyramid_level_sizes(rows, cols) if self.noise_type == "pyramid" else N.geowizard_pyramid_level_sizes(rows, cols)
            N.set_pyramid_table(ent["table"], self.generator, sizes, rows, cols)

    def _alive(self, ent):
        alive = super()._alive(ent)
        if self.loss == "diffusion":
            return (alive, self.noise_scheduler, self.noise_scheduler.alphas_cumprod_on(ent["total"].device))
        return alive

    def _set_step_words(self, lr_scale):
        super()._set_step_words(lr_scale)
        if self.ema is not None:
            self.ema.set_decay_word(self._ema_word)

    def _update(self):
        super()._update()
        if self.ema is not None:
            self.ema.step_at(self.optimizer.params, self._ema_word)


def synthetic_batch(batch, height, width, device, seed=0, dtype=torch.float32):
    """"Hypersim-val synthetic" micro-batch: uniform-noise rgb in [-1,1]; metric depth = tilted plane + 3 boxes in
    [0.5, 20] m, normalised to [-1,1] by its 2 % / 98 % quantiles (load.py:255-267); normals of that surface; 5 % invalid pixels."""
    g = torch.Generator(device=device).manual_seed(seed)
    rgb = (torch.randint(0, 256, (batch, 3, height, width), generator=g, device=device, dtype=torch.int32).float() / 255.0 * 2.0 - 1.0)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, height, device=device), torch.linspace(-1, 1, width, device=device), indexing="ij")
    depth = torch.empty((batch, 1, height, width), device=device)
    for b in range(batch):
        c = torch.rand(3, generator=g, device=device)
        d = 6.0 + 4.0 * (c[0] - 0.5) * xx + 4.0 * (c[1] - 0.5) * yy + 8.0 * c[2]
        for _ in range(3):
            r = torch.rand(5, generator=g, device=device)
            x0, y0 = r[0] * 1.4 - 1.0, r[1] * 1.4 - 1.0
            box = (xx > x0) & (xx < x0 + 0.2 + 0.5 * r[2]) & (yy > y0) & (yy < y0 + 0.2 + 0.5 * r[3])
            d = torch.where(box, 0.5 + 5.0 * r[4] + 0.0 * d, d)
        depth[b, 0] = d.clamp(0.5, 20.0)
    flat = depth.view(batch, -1)
    lo = torch.quantile(flat, 0.02, dim=1).view(batch, 1, 1, 1)
    hi = torch.quantile(flat, 0.98, dim=1).view(batch, 1, 1, 1)
    metric = (((depth - lo) / (hi - lo).clamp_min(1e-6) - 0.5) * 2.0).clamp(-1, 1)
    dzdx = torch.gradient(depth[:, 0], dim=2)[0]
    dzdy = torch.gradient(depth[:, 0], dim=1)[0]
    normals = torch.nn.functional.normalize(torch.stack([-dzdx * width / 2, -dzdy * height / 2, torch.ones_like(dzdx)], dim=1), dim=1)
    mask = torch.rand((batch, 1, height, width), generator=g, device=device) > 0.05
    return {"rgb": rgb.to(dtype), "metric": metric, "normals": normals, "val_mask": mask}
