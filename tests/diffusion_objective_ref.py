"""Plain-torch CPU restatement of the GeoWizard trainer's DIFFUSION objective: GeoWizard/geowizard/training/train_depth_normal.py:598-717 without `--e2e_ft`,
written anew from the trainer's text over the oracle's UNet / VAE (oracle.unet_ref.unet_forward, oracle.pipeline_ref.encode_rgb_ref) and schedule
(pipeline_ref.alphas_cumprod).  TEST INFRASTRUCTURE ONLY: the fixture script tests/golden/make_diffusion_objective_golden.py and the CPU / GPU tests share it.

diffusers is not importable here, so its two scheduler methods are restated from their definitions (scheduling_ddpm.py `add_noise` / `get_velocity`): the
alphas_cumprod table is cast to the sample's dtype FIRST, the coefficients `abar[t] ** 0.5` and `(1 - abar[t]) ** 0.5` are flattened and broadcast over the
trailing dimensions, and
    add_noise    = abar[t] ** 0.5 * x0    + (1 - abar[t]) ** 0.5 * noise
    get_velocity = abar[t] ** 0.5 * noise - (1 - abar[t]) ** 0.5 * sample
Every step is one correctly rounded IEEE operation in the sample's dtype, which is what the kernels must reproduce; the root is taken by `root()` below because
torch's own fp32 root on the CPU is not correctly rounded on every host.

Also here: the seeded inputs of the fixture (the validity mask, the noise, the timesteps) and `geowizard_e2e_ft_noise_forward_ref`, which is
oracle.pipeline_ref.geowizard_train_forward_ref rewritten for x_t = noise (:668)."""
import torch

from oracle import pipeline_ref, unet_ref
from oracle.losses_ref import ssi_loss_ref, angular_loss_ref

TIMESTEPS = (0, 731)          # per image; the rows carry [0, 731, 0, 731] (`.repeat(2)`, :651)
NOISE_SEED = 77
MASK_SEED = 5
SELECTED_CELLS = (49, 55)     # of 64 per image under objective_mask()
TARGET_STRIDE = 7             # the golden file keeps target.reshape(-1)[::TARGET_STRIDE]


def root(x):
    """`x ** 0.5` as the CORRECTLY ROUNDED root in x's dtype, on every host: taken in float64 and rounded once (53 bits are more than twice 24 plus two, so the
    second rounding cannot move an fp32 result).  torch's own fp32 `** 0.5` (= `sqrt`) on the CPU goes through a vector math library that is NOT correctly
    rounded and differs between hosts: one ulp off at 5 of the schedule's 1000 entries where the fixture was made, at many more (t = 8, 9, 12, ... and t = 500)
    where the GPU tests first ran — so "torch's eager result" is not one set of bits, and the restatement pins the IEEE one
    (tests/test_diffusion_objective_cpu.py prints the count for the host it runs on)."""
    return (x.double() ** 0.5).to(x.dtype)


def _coefficients(abar, sample, timesteps):
    abar = abar.to(dtype=sample.dtype)
    sa = root(abar[timesteps]).flatten()
    sb = root(1 - abar[timesteps]).flatten()
    while sa.dim() < sample.dim():
        sa = sa.unsqueeze(-1)
        sb = sb.unsqueeze(-1)
    return sa, sb


def add_noise_ref(abar, original_samples, noise, timesteps):
    """`noise_scheduler.add_noise` (:671)"""
    sa, sb = _coefficients(abar, original_samples, timesteps)
    return sa * original_samples + sb * noise


def get_velocity_ref(abar, sample, noise, timesteps):
    """`noise_scheduler.get_velocity` (:680)"""
    sa, sb = _coefficients(abar, sample, timesteps)
    return sa * noise - sb * sample


def latent_mask_ref(val_mask):
    """:606-608, before the repeat of :609: val_mask bool [B,1,H,W] -> bool [B,1,H/8,W/8]"""
    invalid_mask = ~val_mask
    return ~torch.max_pool2d(invalid_mask.float(), 8, 8).bool()


def target_ref(abar, geo_latents, noise, timesteps, prediction_type):
    """:677-682"""
    if prediction_type == "epsilon":
        return noise
    if prediction_type == "v_prediction":
        return get_velocity_ref(abar, geo_latents, noise, timesteps)
    raise ValueError("Unknown prediction type %s" % prediction_type)


def masked_mse_ref(noise_pred, target, latent_mask):
    """:609,713-717: latent_mask bool [B,1,h,w] -> (loss, n_selected)"""
    lm = latent_mask.repeat((noise_pred.shape[0] // latent_mask.shape[0], noise_pred.shape[1], 1, 1))
    loss = torch.zeros((), dtype=torch.float32)
    if lm.any():
        loss = torch.nn.functional.mse_loss(noise_pred[lm].float(), target[lm].float(), reduction="mean")
    return loss, int(lm.sum())


def objective_mask():
    """2 x 1 x 64 x 64, all valid except — image 0: rows 0:24 of columns 40:64 (nine whole cells) and six seeded single pixels; image 1: pixel (37, 5) and
    rows 8:16 (a whole row of cells).  The trainer's mask then selects 49 and 55 of the 64 cells (SELECTED_CELLS)."""
    m = torch.ones(2, 1, 64, 64, dtype=torch.bool)
    m[0, 0, 0:24, 40:64] = False
    g = torch.Generator().manual_seed(MASK_SEED)
    ys = torch.randint(0, 64, (6,), generator=g)
    xs = torch.randint(0, 64, (6,), generator=g)
    m[0, 0, ys, xs] = False
    m[1, 0, 37, 5] = False
    m[1, 0, 8:16, :] = False
    return m


def objective_inputs():
    """-> (batch, emb, timesteps [b], noise [2b,4,8,8]): golden_cases.geo_train_inputs() with a 3-channel `depth` made from `metric` and objective_mask()"""
    import golden_cases as gc
    batch, emb = gc.geo_train_inputs()
    batch = dict(batch)
    batch["depth"] = batch["metric"].repeat(1, 3, 1, 1)
    batch["val_mask"] = objective_mask()
    b = batch["rgb"].shape[0]
    noise = torch.randn(2 * b, 4, 8, 8, generator=torch.Generator().manual_seed(NOISE_SEED))
    return batch, emb, torch.tensor(TIMESTEPS, dtype=torch.long), noise


def geowizard_diffusion_forward_ref(unet_sd, unet_cfg, vae_sd, vae_cfg, batch, img_embed, timesteps, noise, prediction_type="v_prediction", domain="indoor",
                                    dtype=torch.float32):
    """Forward half of train_depth_normal.py:598-717 without --e2e_ft, with the timesteps (:651, one per image) and the noise (:656-663) given.
    dtype: the trainer's weight_dtype (state dicts and inputs are cast to it).  Returns (loss, n_selected, target, noisy_geo_latents)."""
    if dtype != torch.float32:
        unet_sd = {k: v.to(dtype) for k, v in unet_sd.items()}
        vae_sd = {k: v.to(dtype) for k, v in vae_sd.items()}
    rgb = batch["rgb"].to(dtype)                                                         # :602
    depth = batch["depth"].to(dtype)                                                     # :604
    latent_mask = latent_mask_ref(batch["val_mask"].bool())                              # :606-608
    normals = batch["normals"].to(dtype) * -1                                            # :611
    with torch.no_grad():                                                                # :624,634-638
        batch_latents = pipeline_ref.encode_rgb_ref(vae_sd, vae_cfg, torch.cat((rgb, depth, normals), dim=0))
        rgb_latents, depth_latents, normal_latents = torch.chunk(batch_latents, 3, dim=0)
    geo_latents = torch.cat((depth_latents, normal_latents), dim=0)                      # :639
    bsz = rgb_latents.shape[0]
    timesteps = timesteps.reshape(bsz).repeat(2).long()                                  # :651-652
    noise = noise.to(dtype)
    abar = pipeline_ref.alphas_cumprod()
    noisy_geo_latents = add_noise_ref(abar, geo_latents, noise, timesteps)               # :671
    target = target_ref(abar, geo_latents, noise, timesteps, prediction_type)            # :677-682
    ctx = img_embed.to(dtype).repeat(2, 1, 1)                                            # :684
    cls = pipeline_ref.geowizard_class_embedding(bsz, domain, dtype)                     # :686-701
    unet_input = torch.cat((rgb_latents.repeat(2, 1, 1, 1), noisy_geo_latents), dim=1)   # :704
    noise_pred = unet_ref.unet_forward(unet_sd, unet_cfg, unet_input, timesteps, ctx, class_labels=cls)      # :706-709
    loss, n_selected = masked_mse_ref(noise_pred, target, latent_mask)                   # :609,713-717
    return loss, n_selected, target, noisy_geo_latents


def geowizard_e2e_ft_noise_forward_ref(unet_sd, unet_cfg, vae_sd, vae_cfg, batch, img_embed, noise, domain="indoor"):
    """oracle.pipeline_ref.geowizard_train_forward_ref (train_depth_normal.py:597-768 with --e2e_ft) for x_t = noise (:668) instead of zeros:
    v-prediction x0 = sqrt(abar) * x_t - sqrt(1 - abar) * v at t = 999 (:723-726).  Returns (loss, ssi, angular)."""
    rgb_latents = pipeline_ref.encode_rgb_ref(vae_sd, vae_cfg, batch["rgb"])
    B = rgb_latents.shape[0]
    t = 999
    ctx = img_embed.repeat(2, 1, 1)
    cls = pipeline_ref.geowizard_class_embedding(B, domain, rgb_latents.dtype)
    v = unet_ref.unet_forward(unet_sd, unet_cfg, torch.cat([rgb_latents.repeat(2, 1, 1, 1), noise], dim=1), torch.full((2 * B,), t), ctx, class_labels=cls)
    x0 = pipeline_ref.v_to_x0(v, noise, t)
    est = pipeline_ref.decode_ref(vae_sd, vae_cfg, x0)
    d_est, n_est = torch.chunk(est, 2, dim=0)
    d_est = torch.clamp(d_est.mean(dim=1, keepdim=True), -1, 1)
    n_est = torch.clamp(n_est / (torch.norm(n_est, p=2, dim=1, keepdim=True) + 1e-5), -1, 1)
    mask = batch["val_mask"].bool()
    ssi = ssi_loss_ref(d_est, batch["metric"], mask)
    ang = angular_loss_ref(n_est, batch["normals"] * -1, mask)
    return 0.5 * ssi + 1.0 * ang, ssi, ang
