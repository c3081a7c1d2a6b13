// denoise.hip — the DDIM update of multi-step inference (marigold_pipeline.py:457-468, geowizard_pipeline.py:319-336), in place on the latent channels of the
// UNet input.
//
// With eta = 0 and no clipping a DDIM step is linear in (x_t, model_output) for every prediction type, and so is the predicted x0 of the last step
// (scheduler.DDIMScheduler.step_coefficients builds the table):
//     x[p, ch] = fmaf(c_x, x[p, ch], c_v * v[p, ch])        fp32, rounded once to the storage dtype
// — the arithmetic of latent_x0_kernel (noise.hip), so equal fp32 coefficients give equal bits.  (c_x, c_v) are read from DEVICE memory: a captured graph that
// contains this launch serves every step of every schedule, the host copies row i of the table into `coef` before replay i.
//
// Every thread reads the elements it owns before it writes them and no thread reads another thread's output: in place is safe whatever the launch geometry.
#include <type_traits>
#include "common.h"

namespace e2eft {

// PIX: c == 4 and both views aligned to a whole pixel — one 16-byte (fp32) / 8-byte (16-bit) load of x, one of v, one store per pixel.
// otherwise one element per item.
template <typename T, bool PIX>
__global__ __launch_bounds__(256) void ddim_step_kernel(long pixels, int c, int ldx, int ldv, const float* __restrict__ coef, T* x, const T* __restrict__ v) {
    const float cx = coef[0], cv = coef[1];
    if constexpr (PIX) {
        typedef typename std::conditional<sizeof(T) == 4, u32x4, u32x2>::type Raw;
        union Px {
            Raw raw;
            T e[4];
        };
        for (long pix = (long)blockIdx.x * 256 + threadIdx.x; pix < pixels; pix += (long)gridDim.x * 256) {
            Px a, b, r;
            a.raw = *reinterpret_cast<const Raw*>(x + pix * ldx);
            b.raw = *reinterpret_cast<const Raw*>(v + pix * ldv);
#pragma unroll
            for (int e = 0; e < 4; ++e) r.e[e] = from_f<T>(fmaf(cx, to_f(a.e[e]), cv * to_f(b.e[e])));
            *reinterpret_cast<Raw*>(x + pix * ldx) = r.raw;
        }
    } else {
        const long total = pixels * c;
        for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
            const long pix = it / c;
            const int ch = (int)(it - pix * c);
            T* px = x + pix * ldx + ch;
            *px = from_f<T>(fmaf(cx, to_f(*px), cv * to_f(v[pix * ldv + ch])));
        }
    }
}

}  // namespace e2eft

using namespace e2eft;

extern "C" int e2eft_ddim_step(int32_t dtype, int64_t pixels, int32_t c, int32_t ldx, int32_t ldv, const float* coef, void* x, const void* v, void* stream) {
    E2EFT_REQUIRE(coef && x && v, "ddim_step: null pointer");
    E2EFT_REQUIRE(dtype >= 0 && dtype <= 2, "ddim_step: bad dtype");
    E2EFT_REQUIRE(pixels > 0 && c > 0 && ldx >= c && ldv >= c, "ddim_step: shape");
    E2EFT_REQUIRE((long)pixels * c < (1L << 40), "ddim_step: more than 2^40 - 1 elements");
    const size_t pixel_bytes = 4 * dtype_size(dtype);
    const bool pix = c == 4 && ldx % 4 == 0 && ldv % 4 == 0 && ((uintptr_t)x % pixel_bytes) == 0 && ((uintptr_t)v % pixel_bytes) == 0;
    const long items = pix ? (long)pixels : (long)pixels * c;
    long nb = (items + 255) / 256;
    nb = nb > 16384 ? 16384 : nb;
    hipStream_t s = (hipStream_t)stream;
    E2EFT_DISPATCH_DTYPE(dtype, T, {
        if (pix) hipLaunchKernelGGL((ddim_step_kernel<T, true>), dim3((unsigned)nb), dim3(256), 0, s, (long)pixels, c, ldx, ldv, coef, (T*)x, (const T*)v);
        else hipLaunchKernelGGL((ddim_step_kernel<T, false>), dim3((unsigned)nb), dim3(256), 0, s, (long)pixels, c, ldx, ldv, coef, (T*)x, (const T*)v);
    });
    return check_launch("ddim_step");
}
