// normaleval.hip — surface-normal evaluation on the device: the arithmetic of DSINE's benchmark mode.
//   per-pixel error  /root/reference/DSINE/utils/utils.py:150-158 (compute_normal_error): acos(clamp(cosine_similarity(pred, gt, dim=1), -1, 1))
//                    * 180 / pi, fp32, in torch's order (each vector divided by max(|v|, 1e-8), then the dot product)
//   accumulation     DSINE/projects/dsine/test.py:104-113: the errors of the valid pixels of every image, in (b, y, x) order, appended to one list
//   metrics          DSINE/utils/utils.py:161-178 (compute_normal_metrics): mean, median, rmse and the shares below 5 / 7.5 / 11.25 / 22.5 / 30 deg
// Update (HBM-bound): one pass over (pred, gt, mask) with arbitrary element strides writes the errors into a dense fp32 buffer (a masked-out pixel
// gets +inf, which sorts above every valid value as an unsigned bit pattern) and reduces the update's totals over fixed per-block partials in a
// fixed order (no atomics: bit-reproducible), then adds them to the running totals on the device.
// Finalize: the exact median by the radix select of select.h with the fp32 bit patterns as keys (the errors are >= 0), the second middle element
// of an even count as its successor, and the fp64 record.  Nothing is read back to the host: the launch sequence is fixed and capturable in a
// graph; the kernels read the counts they need from device memory.
#include "common.h"
#include "select.h"

namespace e2eft {

constexpr int NE_UBLK = 2048;         // update: partial blocks (at most: 8 blocks of 4 waves per CU)
constexpr int NE_UTHREADS = 256;
constexpr int NE_NTOT = 9;            // totals: int64 n, nan, count[5]; double sum, sumsq
constexpr int NE_HBLK = 512;          // finalize: histogram / min partial blocks
constexpr int NE_HTHREADS = 512;
constexpr uint32_t NE_INF_BITS = 0x7f800000u;

struct NeLayout {
    int64_t* upart;       // [NE_UBLK][NE_NTOT] update partials (counts as int64, sums as double bit patterns)
    SelState* state;      // the median's selection
    uint32_t* hist;       // [SEL_BINS]
    uint32_t* mpart;      // [NE_HBLK] successor partials
};

static size_t ne_bytes() { return (size_t)NE_UBLK * NE_NTOT * 8 + sizeof(SelState) + (size_t)SEL_BINS * 4 + (size_t)NE_HBLK * 4; }

static NeLayout ne_layout(void* ws) {
    NeLayout l;
    char* p = (char*)ws;
    l.upart = (int64_t*)p;
    p += (size_t)NE_UBLK * NE_NTOT * 8;
    l.state = (SelState*)p;
    p += sizeof(SelState);
    l.hist = (uint32_t*)p;
    p += (size_t)SEL_BINS * 4;
    l.mpart = (uint32_t*)p;
    return l;
}

// torch.cosine_similarity (ATen: x / max(|x|, eps) per vector, then the product summed over the channel) -> clamp -> acos -> degrees, in fp32
__device__ __forceinline__ float ne_angle(float p0, float p1, float p2, float g0, float g1, float g2) {
    const float np_ = fmaxf(__fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(p0, p0), __fmul_rn(p1, p1)), __fmul_rn(p2, p2))), 1e-8f);
    const float ng = fmaxf(__fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(g0, g0), __fmul_rn(g1, g1)), __fmul_rn(g2, g2))), 1e-8f);
    const float a0 = __fdiv_rn(p0, np_), a1 = __fdiv_rn(p1, np_), a2 = __fdiv_rn(p2, np_);
    const float b0 = __fdiv_rn(g0, ng), b1 = __fdiv_rn(g1, ng), b2 = __fdiv_rn(g2, ng);
    float c = __fadd_rn(__fadd_rn(__fmul_rn(a0, b0), __fmul_rn(a1, b1)), __fmul_rn(a2, b2));
    if (c == c) c = fminf(fmaxf(c, -1.0f), 1.0f);             // torch.clamp propagates NaN; fminf / fmaxf alone would drop it
    const float t = __fmul_rn(acosf(c), 180.0f);
    return __fdiv_rn(t, 3.14159274101257324f);               // float(np.pi)
}

// update pass: pixel i of the update (row-major over b, y, x) -> err[i]; per-block totals into part[blockIdx.x]
__global__ __launch_bounds__(NE_UTHREADS) void ne_update_kernel(e2eft_normal_eval_desc d, const float* __restrict__ pred, const float* __restrict__ gt,
                                                                const uint8_t* __restrict__ mask, float* __restrict__ err, int64_t* __restrict__ part) {
    const int64_t hw = (int64_t)d.height * d.width, total = hw * d.batch;
    double s = 0.0, ss = 0.0;
    uint32_t cnt[7] = {0, 0, 0, 0, 0, 0, 0};                 // n, nan, < 5, < 7.5, < 11.25, < 22.5, < 30
    auto pixel = [&](int64_t i, int64_t b, int32_t y, int32_t x) {
        if (mask && !mask[b * d.mask_stride[0] + y * d.mask_stride[1] + x * d.mask_stride[2]]) {
            err[i] = __int_as_float(NE_INF_BITS);
            return;
        }
        const float* pp = pred + b * d.pred_stride[0] + y * d.pred_stride[2] + x * d.pred_stride[3];
        const float* gp = gt + b * d.gt_stride[0] + y * d.gt_stride[2] + x * d.gt_stride[3];
        const int64_t pc = d.pred_stride[1], gc = d.gt_stride[1];
        const float t = ne_angle(pp[0], pp[pc], pp[2 * pc], gp[0], gp[gc], gp[2 * gc]);
        err[i] = t;
        cnt[0] += 1;
        if (t != t) {
            cnt[1] += 1;
        } else {
            s += (double)t;
            ss += (double)t * (double)t;
        }
        cnt[2] += t < 5.0f;
        cnt[3] += t < 7.5f;
        cnt[4] += t < 11.25f;
        cnt[5] += t < 22.5f;
        cnt[6] += t < 30.0f;
    };
    if (total < 0x7fffffffLL) {                              // 32-bit index arithmetic (every realistic update)
        const uint32_t uhw = (uint32_t)hw, uw = (uint32_t)d.width;
        for (uint32_t i = blockIdx.x * NE_UTHREADS + threadIdx.x; i < (uint32_t)total; i += gridDim.x * NE_UTHREADS) {
            const uint32_t b = i / uhw, r = i - b * uhw, y = r / uw;
            pixel(i, b, (int32_t)y, (int32_t)(r - y * uw));
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * NE_UTHREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * NE_UTHREADS) {
            const int64_t b = i / hw, r = i - b * hw;
            const int32_t y = (int32_t)(r / d.width);
            pixel(i, b, y, (int32_t)(r - (int64_t)y * d.width));
        }
    }
    __shared__ uint32_t redc[NE_UTHREADS / 64][7];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        cnt[k] = wave_sum(cnt[k]);
        if (lane == 0) redc[wave][k] = cnt[k];
    }
    int64_t* o = part + (int64_t)blockIdx.x * NE_NTOT;
    double sv[2] = {s, ss};
    block_sums<2, NE_UTHREADS / 64>(sv, reinterpret_cast<double*>(o + 7));      // (its barrier covers redc too)
    if (threadIdx.x < 7) {
        int64_t v = 0;
        for (int w = 0; w < NE_UTHREADS / 64; ++w) v += redc[w][threadIdx.x];
        o[threadIdx.x] = v;
    }
}

// the update's totals over its nblk partials in a fixed order (thread t takes partials t, t + 256, ...; then a fixed butterfly per wave and the four
// waves in order), added to the running totals
__global__ __launch_bounds__(256) void ne_update_reduce_kernel(int nblk, const int64_t* __restrict__ part, int64_t* __restrict__ totals) {
    __shared__ int64_t redc[4][7];
    __shared__ double reds[4][2];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int64_t c[7] = {0, 0, 0, 0, 0, 0, 0};
    double s = 0.0, ss = 0.0;
    for (int j = t; j < nblk; j += 256) {
        const int64_t* p = part + (int64_t)j * NE_NTOT;
#pragma unroll
        for (int k = 0; k < 7; ++k) c[k] += p[k];
        s += __longlong_as_double(p[7]);
        ss += __longlong_as_double(p[8]);
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) c[k] = wave_sum(c[k]);
    s = wave_sum(s);
    ss = wave_sum(ss);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) redc[wave][k] = c[k];
        reds[wave][0] = s;
        reds[wave][1] = ss;
    }
    __syncthreads();
    if (t < 7) {
        totals[t] += redc[0][t] + redc[1][t] + redc[2][t] + redc[3][t];
    } else if (t < 9) {
        const int k = t - 7;
        const double v = reds[0][k] + reds[1][k] + reds[2][k] + reds[3][k];      // the waves left to right, as block_sums
        totals[t] = __double_as_longlong(__longlong_as_double(totals[t]) + v);
    }
}

// the median's rank rule: rank (n - 1) / 2 of the n valid values, and its successor when n is even
struct NeMedianRank {
    __device__ SelRank operator()(int64_t n, int) const { return SelRank{(n - 1) / 2, (n & 1) == 0, 0.0}; }
};

// select setup: nothing to select when n == 0 or a NaN is among the valid values (the record is NaN).  grid SEL_BINS / 256 x 256
__global__ void ne_init_kernel(const int64_t* __restrict__ totals, SelState* __restrict__ state, uint32_t* __restrict__ hist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    hist[i] = 0;
    if (i == 0) select_init(state, totals[0] > 0 && totals[1] == 0);
}

// digit p of the values u < +inf
__global__ __launch_bounds__(NE_HTHREADS) void ne_hist_kernel(int p, int64_t m, const uint32_t* __restrict__ bits, const SelState* __restrict__ state,
                                                              uint32_t* __restrict__ hist) {
    DigitHist<uint32_t, 1> h(p, state);
    if (!h.any) return;
    h.zero();
    auto take = [&](uint32_t u) {
        if (u < NE_INF_BITS) h.add(u);
    };
    const int64_t m4 = m >> 2;
    const u32x4* b4 = reinterpret_cast<const u32x4*>(bits);
    for (int64_t i = (int64_t)blockIdx.x * NE_HTHREADS + threadIdx.x; i < m4; i += (int64_t)gridDim.x * NE_HTHREADS) {
        const u32x4 v = b4[i];
        take(v.x);
        take(v.y);
        take(v.z);
        take(v.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (m & 3)) take(bits[m4 * 4 + threadIdx.x]);
    h.flush(hist);
}

// b when it lies outside a's last histogram: the smallest value above a (and below +inf)
__global__ __launch_bounds__(NE_HTHREADS) void ne_min_kernel(int64_t m, const uint32_t* __restrict__ bits, const SelState* __restrict__ state,
                                                             uint32_t* __restrict__ mpart) {
    SuccMin<uint32_t, 1> mn(state);
    if (!mn.any()) return;
    for (int64_t i = (int64_t)blockIdx.x * NE_HTHREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * NE_HTHREADS) {
        const uint32_t u = bits[i];
        if (u < NE_INF_BITS) mn.take(u);
    }
    mn.store(mpart + blockIdx.x, 0);
}

// the record [mean, median, rmse, a1..a5, n] (utils.py:167-177; NaN as numpy: a NaN error makes mean, median, rmse NaN, the a_i count it in n)
__global__ __launch_bounds__(64) void ne_finish_kernel(int nblk, const int64_t* __restrict__ totals, const SelState* __restrict__ state,
                                                       const uint32_t* __restrict__ mpart, double* __restrict__ out) {
    const uint32_t bkey = select_successor(*state, mpart, nblk);
    if (threadIdx.x != 0) return;
    const int64_t n = totals[0], nan = totals[1];
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const double dn = (double)n;
    double mean = qnan, median = qnan, rmse = qnan;
    if (n > 0 && nan == 0) {
        mean = __longlong_as_double(totals[7]) / dn;
        rmse = sqrt(__longlong_as_double(totals[8]) / dn);
        const float a = __uint_as_float((uint32_t)state->prefix);
        if (state->succ_needed) {
            const float b = __uint_as_float(bkey);
            median = (double)(__fmul_rn(__fadd_rn(a, b), 0.5f));     // np.median of float32: the float32 mean of the two middle values
        } else {
            median = (double)a;
        }
    }
    out[0] = mean;
    out[1] = median;
    out[2] = rmse;
    for (int k = 0; k < 5; ++k) out[3 + k] = n > 0 ? 100.0 * ((double)totals[2 + k] / dn) : qnan;
    out[8] = dn;
}

}  // namespace e2eft

using namespace e2eft;

extern "C" size_t e2eft_normal_eval_workspace_bytes(void) { return ne_bytes(); }

extern "C" int e2eft_normal_eval_update(const e2eft_normal_eval_desc* desc, const float* pred, const float* gt, const uint8_t* mask, float* err,
                                        int64_t err_offset, int64_t err_capacity, int64_t* totals, void* workspace, size_t ws_bytes, void* stream) {
    E2EFT_REQUIRE(desc && pred && gt && err && totals && workspace, "normal_eval_update: null pointer");
    const e2eft_normal_eval_desc d = *desc;
    E2EFT_REQUIRE(d.batch > 0 && d.height > 0 && d.width > 0, "normal_eval_update: shape %d x %d x %d", d.batch, d.height, d.width);
    const int64_t total = (int64_t)d.batch * d.height * d.width;
    E2EFT_REQUIRE(err_offset >= 0 && err_capacity >= 0 && err_offset <= err_capacity && total <= err_capacity - err_offset,
                  "normal_eval_update: %lld errors at offset %lld exceed the capacity %lld", (long long)total, (long long)err_offset, (long long)err_capacity);
    for (int k = 0; k < 4; ++k)
        E2EFT_REQUIRE(d.pred_stride[k] >= 0 && d.gt_stride[k] >= 0, "normal_eval_update: negative stride");
    for (int k = 0; k < 3; ++k) E2EFT_REQUIRE(d.mask_stride[k] >= 0, "normal_eval_update: negative mask stride");
    const size_t need = ne_bytes();
    if (ws_bytes < need) return fail(E2EFT_ERR_WORKSPACE, "normal_eval_update: workspace %zu < %zu", ws_bytes, need);
    E2EFT_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)totals & 7) == 0, "normal_eval_update: workspace must be 16-byte, totals 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const NeLayout l = ne_layout(workspace);
    const int nblk = (int)(total / NE_UTHREADS + 1 < NE_UBLK ? total / NE_UTHREADS + 1 : NE_UBLK);
    hipLaunchKernelGGL(ne_update_kernel, dim3(nblk), dim3(NE_UTHREADS), 0, s, d, pred, gt, mask, err + err_offset, l.upart);
    hipLaunchKernelGGL(ne_update_reduce_kernel, dim3(1), dim3(256), 0, s, nblk, (const int64_t*)l.upart, totals);
    return check_launch("normal_eval_update");
}

extern "C" int e2eft_normal_eval_finalize(const float* err, int64_t count, const int64_t* totals, double* out, void* workspace, size_t ws_bytes,
                                          void* stream) {
    E2EFT_REQUIRE(totals && out && workspace, "normal_eval_finalize: null pointer");
    E2EFT_REQUIRE(count >= 0 && count < 0xffffffffLL, "normal_eval_finalize: count %lld out of range (< 2^32)", (long long)count);
    E2EFT_REQUIRE(err || count == 0, "normal_eval_finalize: null error buffer");
    E2EFT_REQUIRE(((uintptr_t)err & 15) == 0, "normal_eval_finalize: error buffer must be 16-byte aligned");
    const size_t need = ne_bytes();
    if (ws_bytes < need) return fail(E2EFT_ERR_WORKSPACE, "normal_eval_finalize: workspace %zu < %zu", ws_bytes, need);
    E2EFT_REQUIRE(((uintptr_t)workspace & 15) == 0, "normal_eval_finalize: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const NeLayout l = ne_layout(workspace);
    const uint32_t* bits = (const uint32_t*)err;
    hipLaunchKernelGGL(ne_init_kernel, dim3(SEL_BINS / 256), dim3(256), 0, s, totals, l.state, l.hist);
    for (int p = 0; p < select_digits(32); ++p) {
        hipLaunchKernelGGL(ne_hist_kernel, dim3(NE_HBLK), dim3(NE_HTHREADS), 0, s, p, count, bits, (const SelState*)l.state, l.hist);
        hipLaunchKernelGGL((select_scan_kernel<uint32_t, NeMedianRank>), dim3(1), dim3(SEL_BINS / 2), 0, s, p, l.hist, l.state, NeMedianRank{});
    }
    hipLaunchKernelGGL(ne_min_kernel, dim3(NE_HBLK), dim3(NE_HTHREADS), 0, s, count, bits, (const SelState*)l.state, l.mpart);
    hipLaunchKernelGGL(ne_finish_kernel, dim3(1), dim3(64), 0, s, NE_HBLK, totals, (const SelState*)l.state, (const uint32_t*)l.mpart, out);
    return check_launch("normal_eval_finalize");
}
