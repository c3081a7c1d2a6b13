// diffusion.hip — the diffusion objective of the GeoWizard trainer (GeoWizard/geowizard/training/train_depth_normal.py without --e2e_ft):
//   :606-609  latent validity mask      latent_mask = ~max_pool2d((~val_mask).float(), 8, 8).bool()
//   :671      noise_scheduler.add_noise x_t    = sqrt(abar_t) * x0    + sqrt(1 - abar_t) * noise
//   :677-682  target by prediction type epsilon: noise;  v_prediction (get_velocity, :680): sqrt(abar_t) * noise - sqrt(1 - abar_t) * x0
//   :713-717  F.mse_loss(noise_pred[latent_mask].float(), target[latent_mask].float(), reduction="mean") and its gradient
// gfx950, wave64.  These tensors are a few thousand elements (4 x 4 x 60 x 80 at the recipe's shape): the kernels are launch-bound, so the file's job is
// few launches (one per entry point, two for the loss: partials + combine) and no host synchronisation — t, abar, n_selected and grad_out are read on the
// device, nothing is allocated, every call is capture-safe.
//
// Rounding (the CONTRACT of include/e2eft.h; tests/diffusion_objective_ref.py restates it): every product, sum, difference and square root of the mixing
// formulas is one correctly rounded fp32 operation, as in torch's eager `a * x + b * n`.  The file is compiled with -ffp-contract=off (build.py) and repeats
// that as a pragma: __fmul_rn / __fadd_rn / __fsub_rn are plain `*` / `+` / `-` in HIP's headers and would otherwise contract into an FMA; __fsqrt_rn is the
// NATIVE (1 ulp) root there, so the root is sqrt_rn below (through fp64).
// Sums: fp64 in a fixed order through reduce.h, no floating-point atomics.
#include "common.h"

#pragma clang fp contract(off)

namespace e2eft {

constexpr int MSE_NBLK = 256;      // most partial blocks of the masked MSE (the workspace is sized for the blocks a problem launches)

struct Coef {
    float sa, sb;
};
// Correctly rounded fp32 square root through fp64: the fp64 root carries 53 bits and no fp32 root lies within 2^-25 relative of a rounding midpoint, so the
// second rounding cannot move the result — whatever the accuracy of the fp32 root instruction and of the fix-up sqrtf expands to.  Two roots per thread cost
// nothing in a launch-bound kernel.
__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }

// row coefficients; t clamped into the table (a valid t is the caller's contract, e2eft.h)
__device__ __forceinline__ Coef row_coef(const int64_t* __restrict__ t, const float* __restrict__ abar, int row, int n_t) {
    long ti = (long)t[row];
    ti = ti < 0 ? 0 : (ti >= n_t ? n_t - 1 : ti);
    const float a = abar[ti];
    return {sqrt_rn(a), sqrt_rn(__fsub_rn(1.0f, a))};
}
__device__ __forceinline__ float mix_add_noise(Coef k, float x0, float n) { return __fadd_rn(__fmul_rn(k.sa, x0), __fmul_rn(k.sb, n)); }
__device__ __forceinline__ float mix_velocity(Coef k, float x0, float n) { return __fsub_rn(__fmul_rn(k.sa, n), __fmul_rn(k.sb, x0)); }

// c == 4 operands whose pixels are aligned to 4 elements move as ONE pixel per access; everything else element by element
template <typename T> __device__ __forceinline__ void load_px(const T* p, int c, bool vec, float v[4], int ch0) {
    if (vec) {
        if constexpr (sizeof(T) == 4) {
            const floatx4 r = *reinterpret_cast<const floatx4*>(p);
            v[0] = r[0], v[1] = r[1], v[2] = r[2], v[3] = r[3];
        } else {
            union {
                u32x2 raw;
                T e[4];
            } r;
            r.raw = *reinterpret_cast<const u32x2*>(p);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = to_f(r.e[k]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ch0 + k < c ? to_f(p[ch0 + k]) : 0.f;
    }
}
template <typename T> __device__ __forceinline__ void store_px(T* p, int c, bool vec, const float v[4], int ch0) {
    if (vec) {
        if constexpr (sizeof(T) == 4) {
            floatx4 r = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<floatx4*>(p) = r;
        } else {
            union {
                u32x2 raw;
                T e[4];
            } r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r.e[k] = from_f<T>(v[k]);
            *reinterpret_cast<u32x2*>(p) = r.raw;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (ch0 + k < c) p[ch0 + k] = from_f<T>(v[k]);
    }
}

struct DiffShape {
    int rows, hw, c, batch, n_t;
    int ldx0, ldn, ldy;
    int cq;              // channel quads per pixel: (c + 3) / 4
    long items;          // rows * hw * cq — one thread per (pixel, channel quad)
};

// ---- a. latent validity mask: one thread per 8 x 8 cell ------------------------------------------------------------------------------------------------
// A row of a cell is 8 consecutive bytes; width % 8 == 0, so it is 8-byte aligned whenever val_mask is (WORDS), and the threads of a wave read
// consecutive words.  A word holds a zero byte  <=>  (w - 0x01..01) & ~w & 0x80..80 != 0.
template <bool WORDS>
__global__ __launch_bounds__(256) void latent_mask_kernel(long cells, int hl, int wl, const uint8_t* __restrict__ vm, uint8_t* __restrict__ lm) {
    const long it = (long)blockIdx.x * 256 + threadIdx.x;
    if (it >= cells) return;
    const long bi = it / wl;                    // b * hl + i
    const int j = (int)(it - bi * wl);
    const long b = bi / hl;
    const int i = (int)(bi - b * hl);
    const int width = wl * 8;
    const uint8_t* p = vm + ((b * hl * 8 + (long)i * 8) * width + (long)j * 8);
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if constexpr (WORDS) {
            const uint64_t w = *reinterpret_cast<const uint64_t*>(p + (long)r * width);
            ok = ok && (((w - 0x0101010101010101ull) & ~w & 0x8080808080808080ull) == 0ull);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) ok = ok && p[(long)r * width + q] != 0;
        }
    }
    lm[it] = ok ? 1 : 0;
}

// ---- b. forward diffusion / velocity into a strided destination ----------------------------------------------------------------------------------------
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void diffusion_mix_kernel(DiffShape s, int kind, bool vec_in, bool vec_out, const int64_t* __restrict__ t,
                                                            const float* __restrict__ abar, const TI* __restrict__ x0, const TI* __restrict__ noise,
                                                            TO* __restrict__ y) {
    const long it = (long)blockIdx.x * 256 + threadIdx.x;
    if (it >= s.items) return;
    const long gp = it / s.cq;                  // row * hw + pixel
    const int ch0 = (int)(it - gp * s.cq) * 4;
    const Coef k = row_coef(t, abar, (int)(gp / s.hw), s.n_t);
    float a[4], n[4], o[4];
    load_px(x0 + gp * s.ldx0, s.c, vec_in, a, ch0);
    load_px(noise + gp * s.ldn, s.c, vec_in, n, ch0);
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = kind == E2EFT_DIFFUSION_VELOCITY ? mix_velocity(k, a[q], n[q]) : mix_add_noise(k, a[q], n[q]);
    store_px(y + gp * s.ldy, s.c, vec_out, o, ch0);
}

// ---- c. masked MSE, forward ----------------------------------------------------------------------------------------------------------------------------
// pass 1: per block (sum of squared differences, selected count), fp64; the optional target tensor is written for EVERY element (selected or not)
template <typename TI, typename TP>
__global__ __launch_bounds__(256) void masked_mse_partial_kernel(DiffShape s, int prediction, bool vec_in, bool vec_p, const int64_t* __restrict__ t,
                                                                 const float* __restrict__ abar, const TP* __restrict__ pred, const TI* __restrict__ x0,
                                                                 const TI* __restrict__ noise, const uint8_t* __restrict__ lm, float* __restrict__ tgt,
                                                                 double* __restrict__ part /* [gridDim.x][2] */) {
    double v[2] = {0.0, 0.0};
    const bool vp = prediction == E2EFT_PREDICTION_V;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < s.items; it += (long)gridDim.x * 256) {
        const long gp = it / s.cq;
        const int ch0 = (int)(it - gp * s.cq) * 4;
        const int row = (int)(gp / s.hw);
        const int pix = (int)(gp - (long)row * s.hw);
        const bool sel = lm[(long)(row % s.batch) * s.hw + pix] != 0;
        if (!sel && !tgt) continue;
        float a[4] = {0.f, 0.f, 0.f, 0.f}, n[4], p[4];
        load_px(noise + gp * s.ldn, s.c, vec_in, n, ch0);
        if (vp) {
            const Coef k = row_coef(t, abar, row, s.n_t);
            load_px(x0 + gp * s.ldx0, s.c, vec_in, a, ch0);
#pragma unroll
            for (int q = 0; q < 4; ++q) n[q] = mix_velocity(k, a[q], n[q]);
        }
        if (tgt) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (ch0 + q < s.c) tgt[gp * s.c + ch0 + q] = n[q];
        }
        if (sel) {
            load_px(pred + gp * s.ldy, s.c, vec_p, p, ch0);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (ch0 + q < s.c) {
                    const double d = (double)__fsub_rn(p[q], n[q]);
                    v[0] += d * d;
                    v[1] += 1.0;
                }
        }
    }
    block_sums<2>(v, part + (long)blockIdx.x * 2);
}

// pass 2, one block: thread k adds partials k, k + 256, ... in order, block_sums the rest; loss = sum / count rounded once, 0 for an empty selection
__global__ __launch_bounds__(256) void masked_mse_combine_kernel(int nparts, const double* __restrict__ part, float* __restrict__ loss,
                                                                 int64_t* __restrict__ n_selected) {
    __shared__ double tot[2];
    double v[2] = {0.0, 0.0};
    for (int k = threadIdx.x; k < nparts; k += 256) {
        v[0] += part[(long)k * 2];
        v[1] += part[(long)k * 2 + 1];
    }
    block_sums<2>(v, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        n_selected[0] = (int64_t)tot[1];
        loss[0] = tot[1] > 0.0 ? (float)(tot[0] / tot[1]) : 0.f;
    }
}

// ---- d. masked MSE, backward ---------------------------------------------------------------------------------------------------------------------------
// scale = grad_out * 2 / n_selected in fp64, rounded once; dpred = (pred - target) * scale on the selected elements, +0 elsewhere and for n_selected == 0
template <typename TI, typename TP>
__global__ __launch_bounds__(256) void masked_mse_bwd_kernel(DiffShape s, int prediction, bool vec_in, bool vec_p, bool vec_d, int lddp,
                                                             const int64_t* __restrict__ t, const float* __restrict__ abar, const TP* __restrict__ pred,
                                                             const TI* __restrict__ x0, const TI* __restrict__ noise, const uint8_t* __restrict__ lm,
                                                             const int64_t* __restrict__ n_selected, const float* __restrict__ grad_out,
                                                             TP* __restrict__ dpred) {
    const long it = (long)blockIdx.x * 256 + threadIdx.x;
    if (it >= s.items) return;
    const long gp = it / s.cq;
    const int ch0 = (int)(it - gp * s.cq) * 4;
    const int row = (int)(gp / s.hw);
    const int pix = (int)(gp - (long)row * s.hw);
    const int64_t nsel = n_selected[0];
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (nsel > 0 && lm[(long)(row % s.batch) * s.hw + pix] != 0) {
        const float scale = (float)(2.0 * (double)grad_out[0] / (double)nsel);
        float a[4], n[4], p[4];
        load_px(noise + gp * s.ldn, s.c, vec_in, n, ch0);
        if (prediction == E2EFT_PREDICTION_V) {
            const Coef k = row_coef(t, abar, row, s.n_t);
            load_px(x0 + gp * s.ldx0, s.c, vec_in, a, ch0);
#pragma unroll
            for (int q = 0; q < 4; ++q) n[q] = mix_velocity(k, a[q], n[q]);
        }
        load_px(pred + gp * s.ldy, s.c, vec_p, p, ch0);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = __fmul_rn(__fsub_rn(p[q], n[q]), scale);
    }
    store_px(dpred + gp * lddp, s.c, vec_d, o, ch0);
}

// an operand moves pixel-wise when c == 4 and its base and pixel stride keep every pixel aligned to 4 elements
static bool px_vec(int c, const void* p, int ld, size_t elem) { return c == 4 && ld % 4 == 0 && ((uintptr_t)p % (4 * elem)) == 0; }

static int diff_shape(const e2eft_diffusion_desc* d, const char* who, bool need_batch, DiffShape& s) {
    E2EFT_REQUIRE(d, "%s: null descriptor", who);
    E2EFT_REQUIRE(d->dtype >= 0 && d->dtype <= 2 && d->dtype_out >= 0 && d->dtype_out <= 2, "%s: bad dtype (%d, %d)", who, d->dtype, d->dtype_out);
    E2EFT_REQUIRE(d->rows > 0 && d->hw > 0 && d->c > 0, "%s: shape", who);
    E2EFT_REQUIRE((long)d->rows * d->hw * d->c < (1L << 31), "%s: more than 2^31 - 1 elements", who);
    E2EFT_REQUIRE(d->ldx0 >= d->c && d->ldn >= d->c && d->ldy >= d->c, "%s: a pixel stride (ldx0 %d, ldn %d, ldy %d) is smaller than c = %d", who, d->ldx0,
                  d->ldn, d->ldy, d->c);
    E2EFT_REQUIRE(d->n_timesteps >= 1, "%s: n_timesteps", who);
    if (need_batch) {
        E2EFT_REQUIRE(d->batch > 0, "%s: batch", who);
        E2EFT_REQUIRE(d->prediction == E2EFT_PREDICTION_EPSILON || d->prediction == E2EFT_PREDICTION_V,
                      "%s: Unknown prediction type %d (epsilon = 0 and v_prediction = 1 are the trainer's two)", who, d->prediction);
    }
    s.rows = d->rows, s.hw = d->hw, s.c = d->c, s.batch = need_batch ? d->batch : 1, s.n_t = d->n_timesteps;
    s.ldx0 = d->ldx0, s.ldn = d->ldn, s.ldy = d->ldy;
    s.cq = (d->c + 3) / 4;
    s.items = (long)d->rows * d->hw * s.cq;
    return 0;
}

static int mse_blocks(long rows, long hw, long c) {
    const long nb = (rows * hw * ((c + 3) / 4) + 255) / 256;
    return (int)(nb > MSE_NBLK ? MSE_NBLK : nb);
}

// two dtypes -> the kernel's two template types
#define E2EFT_DISPATCH_2(dt_a, TA, dt_b, TB, ...) E2EFT_DISPATCH_DTYPE(dt_a, TA, E2EFT_DISPATCH_DTYPE(dt_b, TB, __VA_ARGS__))

}  // namespace e2eft

using namespace e2eft;

extern "C" int e2eft_latent_valid_mask(int32_t batch, int32_t height, int32_t width, const uint8_t* val_mask, uint8_t* latent_mask, void* stream) {
    E2EFT_REQUIRE(val_mask && latent_mask, "latent_valid_mask: null pointer");
    E2EFT_REQUIRE(batch > 0 && height > 0 && width > 0, "latent_valid_mask: shape");
    E2EFT_REQUIRE(height % 8 == 0 && width % 8 == 0, "latent_valid_mask: height %d and width %d must be multiples of 8 (the VAE's downsampling)", height, width);
    E2EFT_REQUIRE((long)batch * height * width < (1L << 31), "latent_valid_mask: more than 2^31 - 1 pixels");
    const int hl = height / 8, wl = width / 8;
    const long cells = (long)batch * hl * wl;
    const unsigned nb = (unsigned)((cells + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (((uintptr_t)val_mask & 7) == 0) hipLaunchKernelGGL((latent_mask_kernel<true>), dim3(nb), dim3(256), 0, s, cells, hl, wl, val_mask, latent_mask);
    else hipLaunchKernelGGL((latent_mask_kernel<false>), dim3(nb), dim3(256), 0, s, cells, hl, wl, val_mask, latent_mask);
    return check_launch("latent_valid_mask");
}

extern "C" int e2eft_diffusion_mix(const e2eft_diffusion_desc* d, int32_t kind, const int64_t* t, const float* abar, const void* x0, const void* noise,
                                   void* y, void* stream) {
    DiffShape sh;
    if (int rc = diff_shape(d, "diffusion_mix", false, sh)) return rc;
    E2EFT_REQUIRE(kind == E2EFT_DIFFUSION_ADD_NOISE || kind == E2EFT_DIFFUSION_VELOCITY, "diffusion_mix: unknown kind %d", kind);
    E2EFT_REQUIRE(t && abar && x0 && noise && y, "diffusion_mix: null pointer");
    const size_t ei = dtype_size(d->dtype), eo = dtype_size(d->dtype_out);
    const bool vec_in = px_vec(d->c, x0, d->ldx0, ei) && px_vec(d->c, noise, d->ldn, ei), vec_out = px_vec(d->c, y, d->ldy, eo);
    const unsigned nb = (unsigned)((sh.items + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    E2EFT_DISPATCH_2(d->dtype, TI, d->dtype_out, TO,
                     hipLaunchKernelGGL((diffusion_mix_kernel<TI, TO>), dim3(nb), dim3(256), 0, s, sh, (int)kind, vec_in, vec_out, t, abar, (const TI*)x0,
                                        (const TI*)noise, (TO*)y));
    return check_launch("diffusion_mix");
}

// workspace: the partial (sum, count) pairs of the blocks the problem launches
extern "C" size_t e2eft_masked_mse_workspace_bytes(int32_t rows, int32_t hw, int32_t c) {
    if (rows <= 0 || hw <= 0 || c <= 0 || (long)rows * hw * c >= (1L << 31)) return 0;
    return (size_t)mse_blocks(rows, hw, c) * 2 * sizeof(double);
}

extern "C" int e2eft_masked_mse_fwd(const e2eft_diffusion_desc* d, const int64_t* t, const float* abar, const void* pred, const void* x0, const void* noise,
                                    const uint8_t* latent_mask, float* loss, int64_t* n_selected, float* out_target, void* workspace, size_t ws_bytes,
                                    void* stream) {
    DiffShape sh;
    if (int rc = diff_shape(d, "masked_mse_fwd", true, sh)) return rc;
    E2EFT_REQUIRE(t && abar && pred && x0 && noise && latent_mask && loss && n_selected && workspace, "masked_mse_fwd: null pointer");
    const size_t need = e2eft_masked_mse_workspace_bytes(d->rows, d->hw, d->c);
    if (ws_bytes < need) return fail(E2EFT_ERR_WORKSPACE, "masked_mse_fwd: workspace %zu < %zu", ws_bytes, need);
    E2EFT_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)n_selected & 7) == 0, "masked_mse_fwd: workspace and n_selected must be 8-byte aligned");
    const size_t ei = dtype_size(d->dtype), ep = dtype_size(d->dtype_out);
    const bool vec_in = px_vec(d->c, x0, d->ldx0, ei) && px_vec(d->c, noise, d->ldn, ei), vec_p = px_vec(d->c, pred, d->ldy, ep);
    const int nb = mse_blocks(d->rows, d->hw, d->c);
    double* part = (double*)workspace;
    hipStream_t s = (hipStream_t)stream;
    E2EFT_DISPATCH_2(d->dtype, TI, d->dtype_out, TP,
                     hipLaunchKernelGGL((masked_mse_partial_kernel<TI, TP>), dim3(nb), dim3(256), 0, s, sh, (int)d->prediction, vec_in, vec_p, t, abar,
                                        (const TP*)pred, (const TI*)x0, (const TI*)noise, latent_mask, out_target, part));
    hipLaunchKernelGGL(masked_mse_combine_kernel, dim3(1), dim3(256), 0, s, nb, (const double*)part, loss, n_selected);
    return check_launch("masked_mse_fwd");
}

extern "C" int e2eft_masked_mse_bwd(const e2eft_diffusion_desc* d, const int64_t* t, const float* abar, const void* pred, const void* x0, const void* noise,
                                    const uint8_t* latent_mask, const int64_t* n_selected, const float* grad_out, void* dpred, int32_t lddp, void* stream) {
    DiffShape sh;
    if (int rc = diff_shape(d, "masked_mse_bwd", true, sh)) return rc;
    E2EFT_REQUIRE(t && abar && pred && x0 && noise && latent_mask && n_selected && grad_out && dpred, "masked_mse_bwd: null pointer");
    E2EFT_REQUIRE(lddp >= d->c, "masked_mse_bwd: lddp %d is smaller than c = %d", lddp, d->c);
    E2EFT_REQUIRE(((uintptr_t)n_selected & 7) == 0, "masked_mse_bwd: n_selected must be 8-byte aligned");
    const size_t ei = dtype_size(d->dtype), ep = dtype_size(d->dtype_out);
    const bool vec_in = px_vec(d->c, x0, d->ldx0, ei) && px_vec(d->c, noise, d->ldn, ei), vec_p = px_vec(d->c, pred, d->ldy, ep),
               vec_d = px_vec(d->c, dpred, lddp, ep);
    const unsigned nb = (unsigned)((sh.items + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    E2EFT_DISPATCH_2(d->dtype, TI, d->dtype_out, TP,
                     hipLaunchKernelGGL((masked_mse_bwd_kernel<TI, TP>), dim3(nb), dim3(256), 0, s, sh, (int)d->prediction, vec_in, vec_p, vec_d, (int)lddp, t,
                                        abar, (const TP*)pred, (const TI*)x0, (const TI*)noise, latent_mask, n_selected, grad_out, (TP*)dpred));
    return check_launch("masked_mse_bwd");
}
