// hypersimprep.hip — raw Hypersim frames to training inputs on the device: the offline step the reference runs once over the dataset
// (Marigold/script/dataset_preprocess/hypersim/preprocess_hypersim.py:83-138 over hypersim_util.py:9-69), for a batch of frames.
//   tone map     brightness = (0.3 r + 0.59 g) + 0.11 b in fp64 over the pixels whose render_entity_id != -1; its 90th percentile with numpy's
//                default "linear" rule: virtual index 0.9 (n - 1), the two neighbouring EXACT order statistics, numpy's two-branch lerp;
//                scale = 1 (no valid pixel) / 0 (percentile < 1e-4) / numerator / percentile; out = clip(pow(max(scale rgb, 0), 1 / 2.2), 0, 1);
//                rgb_u8 = trunc(out * 255).
//   planar depth distance / double(norm32) * focal with norm32 = sqrtf((x x + y y) + z z) of the float32 pixel grid x = j - W / 2 + 1 / 2,
//                y = i - H / 2 + 1 / 2, z = float(focal); invalid pixels 0; * 1000, truncated to uint16 (the file), or float(u16 / 1000.0) — what the
//                training loader makes of the file.
//   record       invalid ratio, mean / std / min / max of the uint8 image and of u16 / 1000, the count of ids equal to 0 (the reference asserts
//                there are none), a flag for a NaN among the valid brightness values, n, the percentile and the scale.
// The percentile is an exact selection, not a sort: the radix select of select.h over order_key(brightness), 64-bit keys in six digits, for every
// frame of the batch in the same launches.  The keys are never stored: each pass recomputes the brightness from colour and id (10 B per pixel for
// fp16 colour, less than writing and re-reading an 8 B key would cost over six passes, and no workspace that grows with the image).
// hp_hist_kernel is the digit pass (the first one also counts the zero ids and the NaNs), hp_min_kernel the successor pass (skipped by frames that
// do not need it).  hp_scale_kernel turns a, b and the weight into the frame's scale; hp_apply_kernel writes the images and integer partial
// sums; hp_record_kernel writes the fp64 record.  All on the caller's stream, no host read-back: capturable in a graph.
// Built with -ffp-contract=off: no FMA may fuse a product the reference rounds.
#include "common.h"
#include "select.h"

namespace e2eft {

constexpr int HP_THREADS = 256, HP_TARGET_BLOCKS = 2048, HP_NSTAT = 10, HP_NREC = E2EFT_HYPERSIM_RECORD;
// state[frame]: the percentile's selection; n = the frame's valid pixels
// stats[frame]: 0 ids equal to 0, 1 NaN brightness among valid, 2 sum u8, 3 sum u8^2, 4 min u8, 5 max u8, 6 sum u16, 7 sum u16^2, 8 min u16, 9 max u16

struct HpLayout {
    SelState* state;
    unsigned long long* stats;
    uint32_t* hist;
    uint64_t* mpart;
    double* scale;
    size_t bytes;
};

static inline int hp_blocks_per_frame(int batch, int64_t n) {
    int64_t by_size = (n + HP_THREADS - 1) / HP_THREADS, by_target = HP_TARGET_BLOCKS / batch;
    if (by_target < 1) by_target = 1;
    return (int)(by_size < by_target ? by_size : by_target);
}

static inline HpLayout hp_layout(void* ws, int batch, int nblk) {
    HpLayout l;
    char* p = (char*)ws;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char* r = p + o;
        o += (bytes + 15) & ~(size_t)15;
        return r;
    };
    l.state = (SelState*)take(sizeof(SelState) * batch);
    l.stats = (unsigned long long*)take(sizeof(unsigned long long) * HP_NSTAT * batch);
    l.hist = (uint32_t*)take(sizeof(uint32_t) * SEL_BINS * batch);
    l.mpart = (uint64_t*)take(sizeof(uint64_t) * (size_t)nblk * batch);
    l.scale = (double*)take(sizeof(double) * batch);
    l.bytes = o;
    return l;
}

template <typename T> __device__ __forceinline__ double hp_brightness(const T* __restrict__ c) {     // hypersim_util.py:24-26, left to right
    return (0.3 * (double)c[0] + 0.59 * (double)c[1]) + 0.11 * (double)c[2];
}

// numpy's "linear" percentile: virtual index 0.9 (n - 1) in fp64, k = its floor, gamma = the fraction; rank k + 1 is read unless k is the last
struct HpPercentileRank {
    __device__ SelRank operator()(int64_t n, int) const {
        const double v = (double)(n - 1) * 0.9;
        const double fl = floor(v);
        return SelRank{(int64_t)fl, (int64_t)fl + 1 <= n - 1, v - fl};
    }
};

__global__ void hp_init_kernel(int batch, SelState* __restrict__ state, unsigned long long* __restrict__ stats, uint32_t* __restrict__ hist) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)batch * SEL_BINS) hist[i] = 0;
    if (i < batch) select_init(state + i, true);
    if (i < (int64_t)batch * HP_NSTAT) {
        const int k = (int)(i % HP_NSTAT);
        stats[i] = (k == 4 || k == 8) ? ~0ull : 0ull;
    }
}

// digit p of the keys of the valid pixels of frame blockIdx.y.  First pass: the ids equal to 0 and the NaN keys are counted for the record.
template <typename T>
__global__ __launch_bounds__(HP_THREADS) void hp_hist_kernel(int64_t n, int p, const T* __restrict__ color, const int32_t* __restrict__ ids,
                                                             const SelState* __restrict__ state, uint32_t* __restrict__ hist, unsigned long long* __restrict__ stats) {
    __shared__ uint32_t extra[2];
    const int f = blockIdx.y, t = threadIdx.x;
    const bool first = p == 0;
    DigitHist<uint64_t, 1> h(p, state + f);
    if (!h.any) return;                                               // no valid pixel: nothing to select
    if (t < 2) extra[t] = 0;
    h.zero();
    const T* c = color + (int64_t)f * n * 3;
    const int32_t* id = ids + (int64_t)f * n;
    uint32_t zeros = 0, nans = 0;
    for (int64_t i = (int64_t)blockIdx.x * HP_THREADS + t; i < n; i += (int64_t)gridDim.x * HP_THREADS) {
        const int32_t e = id[i];
        zeros += e == 0;
        if (e == -1) continue;
        const double b = hp_brightness(c + i * 3);
        nans += b != b;
        h.add(order_key(b));
    }
    if (first) {
        if (zeros) atomicAdd(&extra[0], zeros);
        if (nans) atomicAdd(&extra[1], nans);
    }
    h.flush(hist + (int64_t)f * SEL_BINS);
    if (first && t < 2 && extra[t]) atomicAdd(&stats[(int64_t)f * HP_NSTAT + t], (unsigned long long)extra[t]);
}

// b where a's run ends at rank k and the last histogram holds nothing above it: the smallest key above a among the valid pixels, per block
template <typename T>
__global__ __launch_bounds__(HP_THREADS) void hp_min_kernel(int64_t n, const T* __restrict__ color, const int32_t* __restrict__ ids, const SelState* __restrict__ state,
                                                            uint64_t* __restrict__ mpart) {
    const int f = blockIdx.y;
    SuccMin<uint64_t, 1> mn(state + f);
    if (!mn.any()) return;
    const T* c = color + (int64_t)f * n * 3;
    const int32_t* id = ids + (int64_t)f * n;
    for (int64_t i = (int64_t)blockIdx.x * HP_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * HP_THREADS) {
        if (id[i] == -1) continue;
        mn.take(order_key(hp_brightness(c + i * 3)));
    }
    mn.store(mpart + (int64_t)f * gridDim.x + blockIdx.x, 0);
}

// one wave per frame: percentile (numpy's _lerp: a + (b - a) t, or b - (b - a) (1 - t) where t >= 0.5; NaN when a valid brightness is NaN) -> scale
__global__ __launch_bounds__(64) void hp_scale_kernel(int nblk, double numerator, const SelState* __restrict__ state, const unsigned long long* __restrict__ stats,
                                                      const uint64_t* __restrict__ mpart, double* __restrict__ scale, double* __restrict__ record) {
    const int f = blockIdx.x;
    const SelState* st = state + f;
    const uint64_t bkey = select_successor(*st, mpart + (int64_t)f * nblk, nblk);
    if (threadIdx.x != 0) return;
    double p = __longlong_as_double(0x7ff8000000000000LL), s = 1.0;
    if (st->n != 0) {
        if (stats[(int64_t)f * HP_NSTAT + 1] == 0) p = quantile_lerp(order_value(st->prefix), order_value(bkey), st->weight);
        s = p < 1e-4 ? 0.0 : numerator / p;
    }
    scale[f] = s;
    record[(int64_t)f * HP_NREC + 12] = p;
    record[(int64_t)f * HP_NREC + 13] = s;
}

__device__ __forceinline__ uint32_t hp_tone_u8(double v, double s) {
    double x = s * v;
    x = x != x ? x : (x > 0.0 ? x : 0.0);                              // np.maximum(x, 0): a NaN stays
    double o = pow(x, 1.0 / 2.2);
    if (o != o) return 0;                                              // NaN -> 0 (numpy's cast is platform-defined there)
    o = o < 0.0 ? 0.0 : (o > 1.0 ? 1.0 : o);
    return (uint32_t)(o * 255.0);
}

// double -> uint16, defined as the reference's x86-64 host is observed to cast (numpy's float64 -> uint16): the low 16 bits of the truncated integer
// while it fits int32 (65536 mm and more wrap, negative values wrap from the top), 0 for a NaN and for anything beyond the int32 range
__device__ __forceinline__ uint32_t hp_cast_u16(double v) {
    if (!(v > -2147483649.0 && v < 2147483648.0)) return 0;
    return (uint32_t)(int32_t)v & 0xffffu;
}

template <typename TC, typename TD, typename TO>
__global__ __launch_bounds__(HP_THREADS) void hp_apply_kernel(int height, int width, double focal, const TC* __restrict__ color, const TD* __restrict__ dist,
                                                              const int32_t* __restrict__ ids, const double* __restrict__ scale, uint8_t* __restrict__ rgb,
                                                              TO* __restrict__ depth, unsigned long long* __restrict__ stats) {
    const int f = blockIdx.y, t = threadIdx.x;
    const int64_t n = (int64_t)height * width;
    const double s = scale[f];
    const float z = (float)focal;
    const TC* c = color + (int64_t)f * n * 3;
    const TD* dd = dist + (int64_t)f * n;
    const int32_t* id = ids + (int64_t)f * n;
    uint8_t* o8 = rgb + (int64_t)f * n * 3;
    TO* od = depth + (int64_t)f * n;
    unsigned long long s8 = 0, q8 = 0, sd = 0, qd = 0;
    uint32_t mn8 = 255, mx8 = 0, mnd = 65535, mxd = 0;
    for (int64_t i = (int64_t)blockIdx.x * HP_THREADS + t; i < n; i += (int64_t)gridDim.x * HP_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t u = hp_tone_u8((double)c[i * 3 + k], s);
            o8[i * 3 + k] = (uint8_t)u;
            s8 += u;
            q8 += u * u;
            mn8 = u < mn8 ? u : mn8;
            mx8 = u > mx8 ? u : mx8;
        }
        uint32_t u = 0;
        if (id[i] != -1) {
            const int y = (int)((uint32_t)i / (uint32_t)width), x = (int)((uint32_t)i - (uint32_t)y * (uint32_t)width);      // n < 2^31
            const float px = (float)((double)x - 0.5 * (double)width + 0.5), py = (float)((double)y - 0.5 * (double)height + 0.5);
            // the correctly rounded float32 root through fp64 (53 >= 2 * 24 + 2 bits: the second rounding cannot change it); __fsqrt_rn is the
            // native 1-ulp instruction in this toolchain
            const float nrm = (float)sqrt((double)__fadd_rn(__fadd_rn(__fmul_rn(px, px), __fmul_rn(py, py)), __fmul_rn(z, z)));
            u = hp_cast_u16(((double)dd[i] / (double)nrm * focal) * 1000.0);
        }
        if (sizeof(TO) == 2) od[i] = (TO)u;
        else od[i] = (TO)(float)((double)u / 1000.0);                  // the loader's (u16 / 1000).astype(float32)
        sd += u;
        qd += (unsigned long long)u * u;
        mnd = u < mnd ? u : mnd;
        mxd = u > mxd ? u : mxd;
    }
    unsigned long long v[8] = {s8, q8, mn8, mx8, sd, qd, mnd, mxd};
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (k & 3) == 2 ? wave_min(v[k]) : (k & 3) == 3 ? wave_max(v[k]) : wave_sum(v[k]);
    if ((t & 63) == 0) {
        unsigned long long* st = stats + (int64_t)f * HP_NSTAT + 2;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool isMin = (k & 3) == 2, isMax = (k & 3) == 3;
            if (isMin) atomicMin(&st[k], v[k]);
            else if (isMax) atomicMax(&st[k], v[k]);
            else atomicAdd(&st[k], v[k]);
        }
    }
}

// sqrt of the population variance of `cnt` integers with sum s and sum of squares q: (cnt q - s^2) / cnt^2 with the numerator exact in 128 bits
__device__ __forceinline__ double hp_std(unsigned long long cnt, unsigned long long s, unsigned long long q) {
    const unsigned __int128 num = (unsigned __int128)cnt * q - (unsigned __int128)s * s;
    const double d = (double)(uint64_t)(num >> 64) * 18446744073709551616.0 + (double)(uint64_t)num;
    return sqrt(d) / (double)cnt;
}

__global__ void hp_record_kernel(int batch, int64_t n, const SelState* __restrict__ state, const unsigned long long* __restrict__ stats, double* __restrict__ record) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= batch) return;
    const unsigned long long* s = stats + (int64_t)f * HP_NSTAT;
    double* r = record + (int64_t)f * HP_NREC;
    const int64_t nv = state[f].n;
    r[0] = (double)(n - nv) / (double)n;
    r[1] = (double)s[2] / (double)(3 * n);
    r[2] = hp_std(3ull * n, s[2], s[3]);
    r[3] = (double)s[4];
    r[4] = (double)s[5];
    r[5] = (double)s[6] / 1000.0 / (double)n;
    r[6] = hp_std(n, s[6], s[7]) / 1000.0;
    r[7] = (double)s[8] / 1000.0;
    r[8] = (double)s[9] / 1000.0;
    r[9] = (double)s[0];
    r[10] = s[1] ? 1.0 : 0.0;
    r[11] = (double)nv;
    r[14] = 0.0;
    r[15] = 0.0;
}

static int hp_check_desc(const e2eft_hypersim_desc* desc, const char* who) {
    E2EFT_REQUIRE(desc, "%s: null descriptor", who);
    E2EFT_REQUIRE(desc->batch > 0 && desc->height > 0 && desc->width > 0, "%s: shape %d x %d x %d", who, desc->batch, desc->height, desc->width);
    E2EFT_REQUIRE(desc->batch <= 65535, "%s: batch %d out of range (<= 65535: one grid row per frame)", who, desc->batch);
    E2EFT_REQUIRE((int64_t)desc->height * desc->width < (1ll << 31), "%s: height * width %lld out of range (< 2^31)", who, (long long)desc->height * desc->width);
    E2EFT_REQUIRE(desc->color_dtype == E2EFT_F32 || desc->color_dtype == E2EFT_F16, "%s: color_dtype %d (E2EFT_F32 or E2EFT_F16)", who, desc->color_dtype);
    E2EFT_REQUIRE(desc->distance_dtype == E2EFT_F32 || desc->distance_dtype == E2EFT_F16, "%s: distance_dtype %d (E2EFT_F32 or E2EFT_F16)", who, desc->distance_dtype);
    E2EFT_REQUIRE(desc->depth_format == E2EFT_HYPERSIM_DEPTH_U16 || desc->depth_format == E2EFT_HYPERSIM_DEPTH_F32, "%s: depth_format %d", who, desc->depth_format);
    E2EFT_REQUIRE(desc->focal > 0.0 && desc->focal < 1e30, "%s: focal %g must be positive and finite", who, desc->focal);
    E2EFT_REQUIRE(desc->scale_numerator > 0.0 && desc->scale_numerator < 1e30, "%s: scale_numerator %g must be positive and finite", who, desc->scale_numerator);
    return E2EFT_OK;
}

template <typename TC, typename TD>
static void hp_launch(const e2eft_hypersim_desc& d, const HpLayout& l, int nblk, const void* color, const void* dist, const int32_t* ids, uint8_t* rgb, void* depth,
                      double* record, hipStream_t s) {
    const int64_t n = (int64_t)d.height * d.width;
    const TC* c = (const TC*)color;
    const dim3 grid(nblk, d.batch);
    const int64_t ninit = (int64_t)d.batch * SEL_BINS;
    hipLaunchKernelGGL(hp_init_kernel, dim3((unsigned)((ninit + 255) / 256)), dim3(256), 0, s, d.batch, l.state, l.stats, l.hist);
    for (int p = 0; p < select_digits(64); ++p) {
        hipLaunchKernelGGL((hp_hist_kernel<TC>), grid, dim3(HP_THREADS), 0, s, n, p, c, ids, (const SelState*)l.state, l.hist, l.stats);
        hipLaunchKernelGGL((select_scan_kernel<uint64_t, HpPercentileRank>), dim3(d.batch), dim3(SEL_BINS / 2), 0, s, p, l.hist, l.state, HpPercentileRank{});
    }
    hipLaunchKernelGGL((hp_min_kernel<TC>), grid, dim3(HP_THREADS), 0, s, n, c, ids, (const SelState*)l.state, l.mpart);
    hipLaunchKernelGGL(hp_scale_kernel, dim3(d.batch), dim3(64), 0, s, nblk, d.scale_numerator, (const SelState*)l.state, (const unsigned long long*)l.stats,
                       (const uint64_t*)l.mpart, l.scale, record);
    if (d.depth_format == E2EFT_HYPERSIM_DEPTH_U16)
        hipLaunchKernelGGL((hp_apply_kernel<TC, TD, uint16_t>), grid, dim3(HP_THREADS), 0, s, d.height, d.width, d.focal, c, (const TD*)dist, ids,
                           (const double*)l.scale, rgb, (uint16_t*)depth, l.stats);
    else
        hipLaunchKernelGGL((hp_apply_kernel<TC, TD, float>), grid, dim3(HP_THREADS), 0, s, d.height, d.width, d.focal, c, (const TD*)dist, ids,
                           (const double*)l.scale, rgb, (float*)depth, l.stats);
    hipLaunchKernelGGL(hp_record_kernel, dim3((d.batch + 63) / 64), dim3(64), 0, s, d.batch, n, (const SelState*)l.state, (const unsigned long long*)l.stats, record);
}

}  // namespace e2eft

using namespace e2eft;

extern "C" size_t e2eft_hypersim_preprocess_workspace_bytes(const e2eft_hypersim_desc* desc) {
    if (hp_check_desc(desc, "hypersim_preprocess_workspace_bytes") != E2EFT_OK) return 0;
    return hp_layout(nullptr, desc->batch, hp_blocks_per_frame(desc->batch, (int64_t)desc->height * desc->width)).bytes;
}

extern "C" int e2eft_hypersim_preprocess(const e2eft_hypersim_desc* desc, const void* color, const void* distance, const int32_t* entity_id, uint8_t* rgb_u8,
                                         void* depth, double* record, void* workspace, size_t ws_bytes, void* stream) {
    const int rc = hp_check_desc(desc, "hypersim_preprocess");
    if (rc != E2EFT_OK) return rc;
    E2EFT_REQUIRE(color && distance && entity_id && rgb_u8 && depth && record && workspace, "hypersim_preprocess: null pointer");
    const e2eft_hypersim_desc d = *desc;
    const int nblk = hp_blocks_per_frame(d.batch, (int64_t)d.height * d.width);
    const size_t need = hp_layout(nullptr, d.batch, nblk).bytes;
    if (ws_bytes < need) return fail(E2EFT_ERR_WORKSPACE, "hypersim_preprocess: workspace %zu < %zu", ws_bytes, need);
    E2EFT_REQUIRE(al16(workspace) && ((uintptr_t)record & 7) == 0, "hypersim_preprocess: workspace must be 16-byte, record 8-byte aligned");
    E2EFT_REQUIRE(((uintptr_t)color & 3) == 0 && ((uintptr_t)distance & 3) == 0 && ((uintptr_t)entity_id & 3) == 0 && ((uintptr_t)depth & 3) == 0,
                  "hypersim_preprocess: color, distance, entity_id and depth must be 4-byte aligned");
    const HpLayout l = hp_layout(workspace, d.batch, nblk);
    hipStream_t s = (hipStream_t)stream;
    const bool c16 = d.color_dtype == E2EFT_F16, d16 = d.distance_dtype == E2EFT_F16;
    if (c16 && d16) hp_launch<f16, f16>(d, l, nblk, color, distance, entity_id, rgb_u8, depth, record, s);
    else if (c16) hp_launch<f16, float>(d, l, nblk, color, distance, entity_id, rgb_u8, depth, record, s);
    else if (d16) hp_launch<float, f16>(d, l, nblk, color, distance, entity_id, rgb_u8, depth, record, s);
    else hp_launch<float, float>(d, l, nblk, color, distance, entity_id, rgb_u8, depth, record, s);
    return check_launch("hypersim_preprocess");
}
