// f32split.hip — fp32 convolutions on the f16 matrix pipe (round 6).
//
// The reference trains and evaluates in fp32 (`--mixed_precision "no"`, training/scripts/train_marigold_e2e_ft_depth.sh:15); on gfx950 the fp32 matrix instruction
// (v_mfma_f32_32x32x2_f32) peaks at 157 TF/s, a sixteenth of the f16 pipe, and the 3x3 VAE convolutions are three quarters of a strict-fp32 training step.
// An fp32 value x with |x| * s < 2^15 (s a power of two) splits EXACTLY into two f16 terms up to 2^-22 |x|:
//     x0 = f16(x s),   x1 = f16(x s - x0)          (x s - x0 is representable in fp32: Sterbenz; both roundings to nearest even)
// and a product of two such values is  x0 w0 + x0 w1 + x1 w0  up to 3 * 2^-22 |x w| (the dropped x1 w1 term is 2^-22) — each term is an exact f16 x f16 product
// accumulated in fp32 by v_mfma_f32_32x32x16_f16.  That error is below what the fp32 accumulation of a K = 1152 ... 4608 reduction adds on EITHER pipe
// (~sqrt(K) 2^-24), and it is measured, not argued: tests/test_f32split_gpu.py compares both routes with a float64 convolution (bar: 1.5 x the fp32 instruction's
// error; measured 0.4 - 1.16 x).  Range: the scale comes from the tensor's own maximum (one reduction pass, on the device: no host synchronisation), so nothing
// overflows; values more than 2^17 below the maximum lose RELATIVE precision (their x1 is an f16 subnormal) and keep an ABSOLUTE error of 2^-39 of the maximum;
// below 2^-39 of it they vanish.  Forward and data-gradient products reduce over the channels and live with that: per output element
//     err <= 2^-37 amax(X) sum|w| + 2^-20 sum|x w| + the accumulation error        (tests/test_f32split_range_gpu.py)
// so an output that is small beside an outlier elsewhere in the tensor is only that accurate.  A WEIGHT GRADIENT separates per channel and gets one scale per
// channel of each operand (e2eft_f32_split2_cols / e2eft_f32_split_wgrad_finish below): every entry keeps the 2^-22 split relative to its own two columns.
//   e2eft_f32_split2            x fp32 [pixels][c]  ->  planes f16 [pixels][x0 (c) | x1 (c)],  scale[1] = s, scale[2] = 1 / s
//   e2eft_conv2d_fwd_f32split   the 3x3 / stride-1 / pad-1 convolution of such planes with weights split the same way on the host (once per weight):
//                               igemm6_kernel<f16, ..., F32O> — K runs over the blocks (x0, w0), (x0, w1), (x1, w0); fp32 bias / residual / output / statistics.
// Three f16 MFMAs per fp32 product against sixteen times the rate: 2.9 ms instead of 11.8 ms for 128 -> 128 at 16 x 576^2, plus the two split passes (12 B / element).
#include "igemm.h"

namespace e2eft {

// |x| maximum of an fp32 [pixels][ldx] tensor's first c columns (c % 4 == 0): non-negative floats order like their bit patterns
__global__ __launch_bounds__(256) void absmax_f32_kernel(long pixels, int c, int ldx, const float* __restrict__ x, unsigned* __restrict__ amax_bits) {
    const int c4 = c >> 2;
    const long total = pixels * c4;
    float m = 0.f;
    const long stride = (long)gridDim.x * 256;
    auto at = [&](const long it) -> floatx4 {
        const long pix = it / c4;
        const int ch = (int)(it - pix * c4) * 4;
        return *reinterpret_cast<const floatx4*>(x + pix * ldx + ch);
    };
    auto fold = [&](const floatx4& v) { m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3]))); };   // (fmaxf drops NaNs: a NaN input shows in the output through x0 anyway)
    long it = (long)blockIdx.x * 256 + threadIdx.x;
    for (; it + 3 * stride < total; it += 4 * stride) {      // four independent 16-byte loads in flight per thread (1024 workgroups have to cover the HBM latency)
        const floatx4 v0 = at(it), v1 = at(it + stride), v2 = at(it + 2 * stride), v3 = at(it + 3 * stride);
        fold(v0); fold(v1); fold(v2); fold(v3);
    }
    for (; it < total; it += stride) fold(at(it));
    m = wave_max(m);
    // ONE atomic per workgroup, at most 1024 workgroups: 16 k same-address atomics (one per wave of 4096 workgroups) cost 0.25 ms — more than the pass itself on a 100 MB tensor
    __shared__ float wmax[4];
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        if (m > 0.f) atomicMax(amax_bits, __float_as_uint(m));
    }
}

// the maxima start from zero.  A kernel, not hipMemsetAsync: in a training step these entry points also run on autograd's backward thread, and under a stream capture
// begun on another thread (training.CapturedTrainStep) the replayed graph behaved as if it held their kernels but not their memsets — the maxima of one replay leaked
// into the next
__global__ __launch_bounds__(256) void clear_words_kernel(int n, unsigned* __restrict__ p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}

// power-of-two scale that brings amax into [2^14, 2^15): (s, 1 / s); 1 for an all-zero or non-finite tensor
__device__ __forceinline__ void split_scale(const unsigned amax_bits, float& s, float& inv) {
    const int ex = (int)((amax_bits >> 23) & 0xffu);        // biased exponent: amax in [2^(ex - 127), 2^(ex - 126))
    int k = 0;
    if (amax_bits != 0u && ex != 0xff) k = 14 - (ex == 0 ? -126 : ex - 127);
    k = k > 100 ? 100 : k < -100 ? -100 : k;
    s = __uint_as_float((unsigned)(127 + k) << 23);
    inv = __uint_as_float((unsigned)(127 - k) << 23);
}

// one thread: eight channels of one pixel -> one 16-byte unit of each plane
// (coff, ctot: this source's first column inside a plane and the plane's width — two sources side by side are the split of their channel concatenation)
// third != 0: the first plane is written a second time behind the second one — the [w0 | w1 | w0] rows of a split WEIGHT (e2eft_f32_split_weight)
__global__ __launch_bounds__(256) void split2_f16_kernel(long pixels, int c, int ldx, int ldp, int coff, int ctot, int third, const float* __restrict__ x, f16* __restrict__ planes,
                                                         const unsigned* __restrict__ amax_bits, float* __restrict__ scale_out) {
    float s, inv;
    split_scale(*amax_bits, s, inv);
    if (blockIdx.x == 0 && threadIdx.x == 0) { scale_out[1] = s; scale_out[2] = inv; }
    const int c8 = c >> 3;
    const long total = pixels * c8;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const long pix = it / c8;
        const int ch = (int)(it - pix * c8) * 8;
        const floatx4 a = *reinterpret_cast<const floatx4*>(x + pix * ldx + ch);
        const floatx4 b = *reinterpret_cast<const floatx4*>(x + pix * ldx + ch + 4);
        const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        Vec16<f16> p0, p1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float t = v[e] * s;
            const f16 h0 = (f16)t;                      // round to nearest even
            p0.e[e] = h0;
            p1.e[e] = (f16)(t - (float)h0);             // exact difference, rounded once
        }
        st16(planes + pix * ldp + coff + ch, p0);
        st16(planes + pix * ldp + ctot + coff + ch, p1);
        if (third) st16(planes + pix * ldp + 2 * ctot + coff + ch, p0);
    }
}

// ---- per-channel scales: the operands of a weight gradient.  dW[co][tap][ci] = sum_pixels dY[.][co] X[.][ci] separates per output channel and per input channel, so
// each column of dY and of X gets its OWN power-of-two scale and the result is scaled back by the outer product of the inverses: every column keeps the full 2^-22
// split whatever the other columns (or one outlier elsewhere in the tensor) hold.
// |x| maxima per column of an fp32 [pixels][ldx] tensor's first c columns (c % 4 == 0) into amax_bits[0, c).  gridDim.x * 256 is a multiple of c / 4 (the host rounds
// it), so a thread keeps ONE group of four columns through its stride loop; threads of a workgroup that share a group meet in LDS, then one atomic per column and
// workgroup, as contiguous 256-byte wave instructions
__global__ __launch_bounds__(256) void col_absmax_f32_kernel(long pixels, int c, int ldx, const float* __restrict__ x, unsigned* __restrict__ amax_bits) {
    __shared__ unsigned smax[1024];
    const int c4 = c >> 2;
    const int nslot = c4 < 256 ? c4 : 256;                   // distinct column groups in this workgroup
    for (int i = threadIdx.x; i < 4 * nslot; i += 256) smax[i] = 0u;
    __syncthreads();
    const long first = (long)blockIdx.x * 256 + threadIdx.x;
    const int cg = (int)(first % c4);
    const long pstep = (long)gridDim.x * 256 / c4;
    const float* xc = x + cg * 4;
    floatx4 m = {0.f, 0.f, 0.f, 0.f};
    auto fold = [&](const floatx4& v) {                      // (fmaxf drops NaNs, as in absmax_f32_kernel)
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = fmaxf(m[j], fabsf(v[j]));
    };
    long pix = first / c4;
    for (; pix + 3 * pstep < pixels; pix += 4 * pstep) {     // four independent 16-byte loads in flight per thread
        const floatx4 v0 = *reinterpret_cast<const floatx4*>(xc + pix * ldx), v1 = *reinterpret_cast<const floatx4*>(xc + (pix + pstep) * ldx);
        const floatx4 v2 = *reinterpret_cast<const floatx4*>(xc + (pix + 2 * pstep) * ldx), v3 = *reinterpret_cast<const floatx4*>(xc + (pix + 3 * pstep) * ldx);
        fold(v0); fold(v1); fold(v2); fold(v3);
    }
    for (; pix < pixels; pix += pstep) fold(*reinterpret_cast<const floatx4*>(xc + pix * ldx));
    const int slot = (int)threadIdx.x % nslot;               // threads of one group: threadIdx.x equal modulo c4 (only when c4 < 256)
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (m[j] > 0.f) atomicMax(&smax[4 * slot + j], __float_as_uint(m[j]));
    __syncthreads();
    const long col0 = ((long)blockIdx.x * 256 % c4) * 4;     // slot 0's first column
    for (int i = threadIdx.x; i < 4 * nslot; i += 256)
        if (smax[i] != 0u) atomicMax(amax_bits + (int)((col0 + i) % c), smax[i]);
}

// split2_f16_kernel under per-column scales: column ch of this source is scaled by split_scale(amax_bits[coff + ch]); the first workgroup leaves the inverse
// scales in inv_out[coff + ch].  gridDim.x * 256 is a multiple of c / 8: a thread's eight scales stay in registers
__global__ __launch_bounds__(256) void split2_f16_cols_kernel(long pixels, int c, int ldx, int ldp, int coff, int ctot, const float* __restrict__ x, f16* __restrict__ planes,
                                                              const unsigned* __restrict__ amax_bits, float* __restrict__ inv_out) {
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < c; i += 256) {
            float s, inv;
            split_scale(amax_bits[coff + i], s, inv);
            inv_out[coff + i] = inv;
        }
    const int c8 = c >> 3;
    const long first = (long)blockIdx.x * 256 + threadIdx.x;
    const int ch = (int)(first % c8) * 8;
    const long pstep = (long)gridDim.x * 256 / c8;
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float inv;
        split_scale(amax_bits[coff + ch + e], s[e], inv);
    }
    for (long pix = first / c8; pix < pixels; pix += pstep) {
        const floatx4 a = *reinterpret_cast<const floatx4*>(x + pix * ldx + ch);
        const floatx4 b = *reinterpret_cast<const floatx4*>(x + pix * ldx + ch + 4);
        const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        Vec16<f16> p0, p1;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float t = v[e] * s[e];
            const f16 h0 = (f16)t;                      // round to nearest even
            p0.e[e] = h0;
            p1.e[e] = (f16)(t - (float)h0);             // exact difference, rounded once
        }
        st16(planes + pix * ldp + coff + ch, p0);
        st16(planes + pix * ldp + ctot + coff + ch, p1);
    }
}

// out[co][tap][ci] = (t0 + t1 + t2) * inv_dy[co] * inv_x[ci]: the three partial gradients of the split operands, scaled back — exactly, all scales being powers of two.
// The two exponents are added as integers and applied in two halves of the same sign, so every intermediate lies between the sum and the result: nothing overflows
// or is flushed on the way where the result itself is a normal fp32 value (|exponent| <= 100 each: split_scale).  out may be t0.
__global__ __launch_bounds__(256) void wgrad_unscale_kernel(long rows, int n, int cin, const float* t0, const float* t1, const float* t2,
                                                            const float* __restrict__ inv_dy, const float* __restrict__ inv_x, float* out) {
    const int n4 = n >> 2;
    const long total = rows * n4;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const long co = it / n4;
        const int ci = (int)((it - co * n4) * 4 % cin);
        const floatx4 a = *reinterpret_cast<const floatx4*>(t0 + it * 4), b = *reinterpret_cast<const floatx4*>(t1 + it * 4), d = *reinterpret_cast<const floatx4*>(t2 + it * 4);
        const floatx4 ix = *reinterpret_cast<const floatx4*>(inv_x + ci);
        const int ea = (int)((__float_as_uint(inv_dy[co]) >> 23) & 0xffu) - 127;
        floatx4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = ea + (int)((__float_as_uint(ix[j]) >> 23) & 0xffu) - 127;
            const int h = k >> 1;
            r[j] = ((a[j] + b[j]) + d[j]) * __uint_as_float((unsigned)(127 + h) << 23) * __uint_as_float((unsigned)(127 + k - h) << 23);
        }
        *reinterpret_cast<floatx4*>(out + it * 4) = r;
    }
}

// the implicit-GEMM parameter block of an fp32 convolution whose input arrives as split planes: any filter / stride / padding of e2eft_conv2d_fwd without a second
// source and without a fused upsample; K = taps * 3 * c1
static bool f32split_params(const E2eftConvDesc* d, IgemmParams& p) {
    if (!d || d->dtype != E2EFT_F32 || d->c2 != 0 || !option(E2EFT_OPT_F32_SPLIT)) return false;
    if (d->batch <= 0 || d->hin <= 0 || d->win <= 0 || d->cout <= 0 || d->c1 <= 0 || d->hout <= 0 || d->wout <= 0) return false;
    if (d->kh <= 0 || d->kw <= 0 || d->stride <= 0 || d->hl != d->hin || d->wl != d->win) return false;
    if ((d->hout - 1) * d->stride - d->pad_t >= d->hl || (d->wout - 1) * d->stride - d->pad_l >= d->wl) return false;
    const int taps = d->kh * d->kw;
    if (d->c1 % 64 != 0 || d->ldx1 < 2 * d->c1 || d->ldx1 % 8 != 0 || d->ldw < taps * 3 * d->c1 || d->ldw % 8 != 0 || (long)d->batch * d->hout * d->wout >= 2147483647L) return false;
    p = conv_params(d);
    p.c1 = p.cin = 3 * d->c1; p.split_c = d->c1; p.K = taps * 3 * d->c1;   // the split form
    if (d->ldr <= 0) p.ldr = d->ldo;
    return true;
}

}  // namespace e2eft

using namespace e2eft;

static void clear_words(float* p, int n, hipStream_t s) {
    hipLaunchKernelGGL(clear_words_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, reinterpret_cast<unsigned*>(p));
}

extern "C" int e2eft_f32_split2(const float* x, int64_t pixels, int32_t c, int32_t ldx, void* planes, int32_t ldp, float* scale, void* stream) {
    E2EFT_REQUIRE(x && planes && scale && pixels > 0, "f32_split2: null pointer / empty tensor");
    E2EFT_REQUIRE(c > 0 && c % 8 == 0 && ldx >= c && ldx % 4 == 0 && ldp >= 2 * c && ldp % 8 == 0, "f32_split2: c=%d ldx=%d ldp=%d (c %% 8, ldx %% 4, ldp %% 8, ldp >= 2 c)", c, ldx, ldp);
    E2EFT_REQUIRE(al16(x) && al16(planes) && ((uintptr_t)scale & 3) == 0, "f32_split2: alignment");
    hipStream_t s = (hipStream_t)stream;
    clear_words(scale, 1, s);
    const long units = pixels * (c / 8);
    long nb = (units + 255) / 256;
    const long nbm = nb > 1024 ? 1024 : nb;          // the reduction: few atomics
    hipLaunchKernelGGL(absmax_f32_kernel, dim3((unsigned)nbm), dim3(256), 0, s, (long)pixels, c, ldx, x, reinterpret_cast<unsigned*>(scale));
    if (nb > 65536) nb = 65536;
    hipLaunchKernelGGL(split2_f16_kernel, dim3((unsigned)nb), dim3(256), 0, s, (long)pixels, c, ldx, ldp, 0, c, 0, x, (f16*)planes, reinterpret_cast<const unsigned*>(scale), scale);
    tag_kernel("split2_f16_kernel");
    return check_launch("f32_split2");
}

// a packed fp32 weight [rows = cout * taps][c] -> the operand e2eft_conv2d_fwd_f32split / e2eft_gemm_f32split multiply with: f16 [rows][w0 (c) | w1 (c) | w0 (c)] with
// w s_w = w0 + w1, scale[1] = s_w, scale[2] = 1 / s_w (the consumers' w_inv_scale = scale + 2).  Two launches on the device: trainable weights are split once per
// optimizer step and parameter, several hundred times per step — as a dozen tensor-library calls each that was the largest host-side cost of the fp32 step.
extern "C" int e2eft_f32_split_weight(const float* w, int64_t rows, int32_t c, void* w_split, float* scale, void* stream) {
    E2EFT_REQUIRE(w && w_split && scale && rows > 0, "f32_split_weight: null pointer / empty weight");
    E2EFT_REQUIRE(c > 0 && c % 8 == 0, "f32_split_weight: c=%d must be a multiple of 8", c);
    E2EFT_REQUIRE(al16(w) && al16(w_split) && ((uintptr_t)scale & 3) == 0, "f32_split_weight: alignment");
    hipStream_t s = (hipStream_t)stream;
    clear_words(scale, 1, s);
    const long units = rows * (c / 8);
    long nb = (units + 255) / 256;
    const long nbm = nb > 1024 ? 1024 : nb;
    hipLaunchKernelGGL(absmax_f32_kernel, dim3((unsigned)nbm), dim3(256), 0, s, (long)rows, c, c, w, reinterpret_cast<unsigned*>(scale));
    if (nb > 65536) nb = 65536;
    hipLaunchKernelGGL(split2_f16_kernel, dim3((unsigned)nb), dim3(256), 0, s, (long)rows, c, c, 3 * c, 0, c, 1, w, (f16*)w_split, reinterpret_cast<const unsigned*>(scale), scale);
    return check_launch("f32_split_weight");
}

// the channel concatenation [x1 (c1) | x2 (c2)] of two fp32 tensors as ONE pair of planes under ONE scale (the two-source convolutions of the UNet's up blocks:
// unet_2d_blocks.py:2328,2456 `torch.cat([hidden_states, res_hidden_states], dim=1)`): planes [pixels][x1_0 | x2_0 | x1_1 | x2_1], ldp >= 2 (c1 + c2)
extern "C" int e2eft_f32_split2_cat(const float* x1, int32_t c1, int32_t ldx1, const float* x2, int32_t c2, int32_t ldx2, int64_t pixels, void* planes, int32_t ldp,
                                    float* scale, void* stream) {
    E2EFT_REQUIRE(x1 && x2 && planes && scale && pixels > 0, "f32_split2_cat: null pointer / empty tensor");
    E2EFT_REQUIRE(c1 > 0 && c1 % 8 == 0 && c2 > 0 && c2 % 8 == 0 && ldx1 >= c1 && ldx1 % 4 == 0 && ldx2 >= c2 && ldx2 % 4 == 0 && ldp >= 2 * (c1 + c2) && ldp % 8 == 0,
                  "f32_split2_cat: c1=%d c2=%d ldx1=%d ldx2=%d ldp=%d", c1, c2, ldx1, ldx2, ldp);
    E2EFT_REQUIRE(al16(x1) && al16(x2) && al16(planes) && ((uintptr_t)scale & 3) == 0, "f32_split2_cat: alignment");
    hipStream_t s = (hipStream_t)stream;
    clear_words(scale, 1, s);
    const float* xs[2] = {x1, x2};
    const int cs[2] = {c1, c2}, lds[2] = {ldx1, ldx2};
    for (int i = 0; i < 2; ++i) {      // one maximum over both sources
        long nb = (pixels * (cs[i] / 8) + 255) / 256;
        if (nb > 1024) nb = 1024;
        hipLaunchKernelGGL(absmax_f32_kernel, dim3((unsigned)nb), dim3(256), 0, s, (long)pixels, cs[i], lds[i], xs[i], reinterpret_cast<unsigned*>(scale));
    }
    for (int i = 0; i < 2; ++i) {
        long nb = (pixels * (cs[i] / 8) + 255) / 256;
        if (nb > 65536) nb = 65536;
        hipLaunchKernelGGL(split2_f16_kernel, dim3((unsigned)nb), dim3(256), 0, s, (long)pixels, cs[i], lds[i], ldp, i ? c1 : 0, c1 + c2, 0, xs[i], (f16*)planes,
                           reinterpret_cast<const unsigned*>(scale), scale);
    }
    tag_kernel("split2_f16_kernel");
    return check_launch("f32_split2_cat");
}

// the planes of [x1 (c1) | x2 (c2)] (x2 null, c2 = 0: one source) under per-COLUMN power-of-two scales, for the operands of a weight gradient:
// planes [pixels][x1_0 | x2_0 | x1_1 | x2_1] as e2eft_f32_split2_cat's; colscale: 2 (c1 + c2) device floats — [0, c1 + c2) workspace (the maxima),
// [c1 + c2, 2 (c1 + c2)) the inverse scales 1 / s[column] on return.  Two launches per source, no host read.
extern "C" int e2eft_f32_split2_cols(const float* x1, int32_t c1, int32_t ldx1, const float* x2, int32_t c2, int32_t ldx2, int64_t pixels, void* planes, int32_t ldp,
                                     float* colscale, void* stream) {
    E2EFT_REQUIRE(x1 && planes && colscale && pixels > 0 && (x2 != nullptr) == (c2 != 0), "f32_split2_cols: null pointer / empty tensor");
    E2EFT_REQUIRE(c1 > 0 && c1 % 8 == 0 && c2 >= 0 && c2 % 8 == 0 && ldx1 >= c1 && ldx1 % 4 == 0 && (!x2 || (ldx2 >= c2 && ldx2 % 4 == 0)) && ldp >= 2 * (c1 + c2) && ldp % 8 == 0,
                  "f32_split2_cols: c1=%d c2=%d ldx1=%d ldx2=%d ldp=%d", c1, c2, ldx1, ldx2, ldp);
    E2EFT_REQUIRE(al16(x1) && al16(x2) && al16(planes) && ((uintptr_t)colscale & 3) == 0, "f32_split2_cols: alignment");
    hipStream_t s = (hipStream_t)stream;
    const int ctot = c1 + c2;
    clear_words(colscale, ctot, s);
    const float* xs[2] = {x1, x2};
    const int cs[2] = {c1, c2}, lds[2] = {ldx1, ldx2}, offs[2] = {0, c1};
    // workgroups for `units` work items of `per` columns groups per pixel: at most `cap`, a multiple of what makes gridDim.x * 256 a multiple of `per`
    auto grid = [](long units, int per, long cap) -> unsigned {
        int g = per, r = 256;
        while (r) { const int t = g % r; g = r; r = t; }      // gcd(per, 256)
        const long mult = per / g;
        long nb = (units + 255) / 256;
        nb = nb > cap ? cap : nb < 1 ? 1 : nb;
        return (unsigned)((nb + mult - 1) / mult * mult);
    };
    unsigned* bits = reinterpret_cast<unsigned*>(colscale);
    for (int i = 0; i < 2 && cs[i]; ++i)
        hipLaunchKernelGGL(col_absmax_f32_kernel, dim3(grid(pixels * (cs[i] / 4) / 4, cs[i] / 4, 1024)), dim3(256), 0, s, (long)pixels, cs[i], lds[i], xs[i], bits + offs[i]);
    for (int i = 0; i < 2 && cs[i]; ++i)
        hipLaunchKernelGGL(split2_f16_cols_kernel, dim3(grid(pixels * (cs[i] / 8), cs[i] / 8, 65536)), dim3(256), 0, s, (long)pixels, cs[i], lds[i], ldp, offs[i], ctot, xs[i],
                           (f16*)planes, bits, colscale + ctot);
    return check_launch("f32_split2_cols");
}

// the weight gradient of two such operands: out [cout][n = taps * cin] = (t0 + t1 + t2) / (s_dy[co] s_x[ci]) for the 16-bit kernel's three results on the planes
// (d0, x0), (d0, x1), (d1, x0) — dense fp32 [cout][n] each, 16-byte aligned; inv_dy [cout], inv_x [cin]: the inverse scales e2eft_f32_split2_cols left.  out may be t0.
extern "C" int e2eft_f32_split_wgrad_finish(const float* t0, const float* t1, const float* t2, int64_t cout, int32_t taps, int32_t cin, const float* inv_dy, const float* inv_x,
                                            float* out, void* stream) {
    E2EFT_REQUIRE(t0 && t1 && t2 && inv_dy && inv_x && out && cout > 0 && taps > 0, "f32_split_wgrad_finish: null pointer / empty gradient");
    E2EFT_REQUIRE(cin > 0 && cin % 4 == 0 && (long)taps * cin < 2147483647L, "f32_split_wgrad_finish: cin=%d must be a multiple of 4", cin);
    E2EFT_REQUIRE(al16(t0) && al16(t1) && al16(t2) && al16(out) && al16(inv_x), "f32_split_wgrad_finish: pointers must be 16-byte aligned");
    const int n = taps * cin;
    long nb = (cout * (n / 4) + 255) / 256;
    if (nb > 65536) nb = 65536;
    hipLaunchKernelGGL(wgrad_unscale_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (long)cout, n, cin, t0, t1, t2, inv_dy, inv_x, out);
    return check_launch("f32_split_wgrad_finish");
}

// pure host arithmetic: would e2eft_conv2d_fwd_f32split take this launch (with 16-byte aligned pointers)?  desc: dtype E2EFT_F32, c1 = channels of the fp32
// tensor, ldx1 = pixel stride of the PLANES in f16 elements (>= 2 c1), ldw = weight row length in f16 elements (>= kh kw 3 c1), ldo / ldr in fp32 elements
extern "C" int e2eft_conv2d_fwd_f32split_supported(const E2eftConvDesc* d) {
    IgemmParams p;
    return f32split_params(d, p) && persistent_family_eligible(E2EFT_F16, 1, p, 1) ? 1 : 0;
}

extern "C" int e2eft_conv2d_fwd_f32split(const E2eftConvDesc* d, const void* planes, const float* scale, const void* w_split, const float* w_inv_scale, const float* bias,
                                         const float* residual, float* out, float* gn_partial, size_t gn_partial_bytes, int32_t* slab_rows, void* stream) {
    if (slab_rows) *slab_rows = 0;
    E2EFT_REQUIRE(d && planes && w_split && out, "conv2d_fwd_f32split: null pointer");
    IgemmParams p;
    if (!f32split_params(d, p)) return fail(E2EFT_ERR_UNSUPPORTED, "conv2d_fwd_f32split: not an fp32 convolution of 64-channel multiples from split planes (ask e2eft_conv2d_fwd_f32split_supported)");
    E2EFT_REQUIRE(al16(planes) && al16(w_split) && al16(out), "conv2d_fwd_f32split: pointers must be 16-byte aligned");
    p.x1 = planes; p.w = w_split; p.bias = bias; p.residual = residual; p.out = out;
    p.alpha_dev = scale ? scale + 2 : nullptr;
    p.alpha_dev2 = w_inv_scale;
    if (gn_partial && slab_rows) {
        if (const int rcw = check_gn_partial("conv2d_fwd_f32split", gn_partial_bytes, d->batch, p.rows_per_img, d->cout)) return rcw;
        p.gn_partial = gn_partial;
    }
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_persistent_family(E2EFT_F16, 1, p, 1, s);                   // 3x3 / stride 1 / pad 1 on a 32 x 8 grid: the halo-patch kernel; else whole 256-row tiles on igemm5
    if (rc < 0 && p.gn_partial) {                                               // statistics need whole tiles inside one image: without them (the consumer runs its own pass)
        p.gn_partial = nullptr;
        rc = launch_igemm_persistent(E2EFT_F16, 1, p, 1, s);
    }
    if (rc < 0) return fail(E2EFT_ERR_UNSUPPORTED, "conv2d_fwd_f32split: this launch is not eligible for the persistent kernels");
    if (rc == 0 && slab_rows && p.gn_partial) *slab_rows = p.rows_per_img / p.gn_nslabs;
    return rc;
}

// ---- nn.Linear in fp32 from split planes: out[m][n] = alpha / (s s_w) * sum_k a[m][k] w[n][k] + bias[n] + residual[m][n] on igemm5's GEMM mode.  `d`: dtype E2EFT_F32, k = the
// fp32 operand's columns (% 64 == 0), lda = row stride of the PLANES in f16 elements (>= 2 k), ldw = row length of w_split [n][w0 (k) | w1 (k) | w0 (k)] (>= 3 k), ldo / ldr
// in fp32 elements, one problem (nzo = nzi = 1), bias along n.  m > 256 (a ragged last 256-row tile is masked): ask e2eft_gemm_f32split_supported first.
static bool f32split_gemm_params(const E2eftGemmDesc* d, IgemmParams& p) {
    if (!d || d->dtype != E2EFT_F32 || !option(E2EFT_OPT_F32_SPLIT) || d->nzo != 1 || d->nzi != 1 || d->bias_along_m) return false;
    if (d->m <= 0 || d->n <= 0 || d->k <= 0 || d->k % 64 != 0 || d->lda < 2 * d->k || d->lda % 8 != 0 || d->ldw < 3 * d->k || d->ldw % 8 != 0 || d->ldo < d->n) return false;
    p = IgemmParams{};
    p.M = d->m; p.N = d->n; p.K = 3 * d->k;
    p.ldx1 = d->lda; p.c1 = 3 * d->k; p.cin = 3 * d->k; p.split_c = d->k;
    p.ldw = d->ldw; p.ldr = d->ldr > 0 ? d->ldr : d->ldo; p.ldo = d->ldo;
    p.rows_per_img = 1;
    p.alpha = d->alpha;
    p.nzi = 1;
    return true;
}

extern "C" int e2eft_gemm_f32split_supported(const E2eftGemmDesc* d) {
    IgemmParams p;
    return f32split_gemm_params(d, p) && persistent_family_eligible(E2EFT_F16, 0, p, 1) ? 1 : 0;   // (GEMM mode: igemm5)
}

extern "C" int e2eft_gemm_f32split(const E2eftGemmDesc* d, const void* planes, const float* scale, const void* w_split, const float* w_inv_scale, const float* bias,
                                   const float* residual, float* out, void* stream) {
    E2EFT_REQUIRE(d && planes && w_split && out, "gemm_f32split: null pointer");
    IgemmParams p;
    if (!f32split_gemm_params(d, p)) return fail(E2EFT_ERR_UNSUPPORTED, "gemm_f32split: not an fp32 GEMM of 64-column multiples from split planes (ask e2eft_gemm_f32split_supported)");
    E2EFT_REQUIRE(al16(planes) && al16(w_split) && al16(out), "gemm_f32split: pointers must be 16-byte aligned");
    p.x1 = planes; p.w = w_split; p.bias = bias; p.residual = residual; p.out = out;
    p.alpha_dev = scale ? scale + 2 : nullptr;
    p.alpha_dev2 = w_inv_scale;
    const int rc = launch_igemm_persistent(E2EFT_F16, 0, p, 1, (hipStream_t)stream);
    if (rc < 0) return fail(E2EFT_ERR_UNSUPPORTED, "gemm_f32split: this launch is not eligible for the persistent kernel");
    return rc;
}

// ---- nearest-2x upsample + 3x3 / stride-1 / pad-1 convolution in fp32 as four 2x2 phase convolutions of the split planes (e2eft_upconv2x_fwd's algebra, igemm.hip).
// `d` as e2eft_upconv2x_fwd's (dtype E2EFT_F32, hl = 2 hin, ...) with ldx1 = the planes' pixel stride in f16 elements; w_phase_split: f16 [4][cout][2][2][w0 | w1 | w0]
// (the fp32 phase weights of autograd.phase_conv_weight split as ONE tensor: one scale).  The halo-patch kernel's 2x2-tap variant where the grid allows, else igemm5.
static bool f32split_upconv_ok(const E2eftConvDesc* d) {
    if (!d || d->dtype != E2EFT_F32 || d->c2 != 0 || !option(E2EFT_OPT_F32_SPLIT) || !option(E2EFT_OPT_UPCONV_PHASES)) return false;
    if (d->kh != 3 || d->kw != 3 || d->stride != 1 || d->pad_t != 1 || d->pad_l != 1 || d->hl != 2 * d->hin || d->wl != 2 * d->win || d->hout != d->hl || d->wout != d->wl) return false;
    if (d->batch <= 0 || d->hin <= 0 || d->win <= 0 || d->c1 <= 0 || d->c1 % 64 != 0 || d->cout % 8 != 0 || d->ldo % 8 != 0 || d->alpha != 1.0f) return false;
    return !(d->ldx1 < 2 * d->c1 || d->ldx1 % 8 != 0 || d->win % 16 != 0 || ((long)d->hin * d->win) % 256 != 0 || (long)d->batch * d->hin * d->win >= 2147483647L);
}

extern "C" int e2eft_upconv2x_fwd_f32split_supported(const E2eftConvDesc* d) {
    return f32split_upconv_ok(d) && persistent_family_eligible(E2EFT_F16, 1, upconv2x_phase_params(d, 0, 3), 1) ? 1 : 0;
}

extern "C" int e2eft_upconv2x_fwd_f32split(const E2eftConvDesc* d, const void* planes, const float* scale, const void* w_phase_split, const float* w_inv_scale,
                                           const float* bias, float* out, float* gn_partial, size_t gn_partial_bytes, int32_t* slab_rows, void* stream) {
    if (slab_rows) *slab_rows = 0;
    E2EFT_REQUIRE(d && planes && w_phase_split && out, "upconv2x_f32split: null pointer");
    if (!e2eft_upconv2x_fwd_f32split_supported(d)) return fail(E2EFT_ERR_UNSUPPORTED, "upconv2x_f32split: this launch is not eligible (ask e2eft_upconv2x_fwd_f32split_supported)");
    E2EFT_REQUIRE(al16(planes) && al16(w_phase_split) && al16(out) && (!bias || al16(bias)), "upconv2x_f32split: pointers must be 16-byte aligned");
    IgemmParams io = {};
    io.x1 = planes; io.w = w_phase_split; io.bias = bias; io.out = out;
    io.alpha_dev = scale ? scale + 2 : nullptr;
    io.alpha_dev2 = w_inv_scale;
    if (gn_partial && slab_rows) {
        if (const int rcw = check_gn_partial("upconv2x_f32split", gn_partial_bytes, d->batch, 4L * d->hin * d->win, d->cout)) return rcw;
        io.gn_partial = gn_partial;
    }
    return run_upconv2x_phases(d, E2EFT_F16, 3, io, true, slab_rows, "upconv2x_f32split", (hipStream_t)stream);
}
