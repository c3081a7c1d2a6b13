// normalprep.hip — the surface-normal benchmarks' per-sample preparation on the device: what DSINE's benchmark mode does to a sample between decoding
// its files and calling the pipeline (DSINE/data/datasets/{nyuv2,scannet,ibims,sintel}/__init__.py, DSINE/data/augmentations/basic.py:68-84,221-239,
// DSINE/projects/dsine/test.py:59-65), for a batch of frames.
//
// e2eft_normal_gt_prepare: a decoded normal raster [B,H,W,3] -> planar normals [B,3,H,W] fp32, mask [B,1,H,W], valid counts [B].
//   uint8 (NYUv2, ScanNet)     mask = r + g + b > 0 (integer sum), normal = (float(u8) / 255.0f) * 2.0f - 1.0f
//   float32 (iBims-1, Sintel)  mask = sqrtf((r r + g g) + b b) > 0.5f (np.linalg.norm's order of additions; a NaN is invalid), the values pass through
//                              bit for bit (they are moved as 32-bit words, never through a floating-point operation)
//   One wave per run of NG_RUN_BYTES = 1008 bytes of one row: 336 uint8 pixels or 84 float32 pixels.  A pixel is 3 elements, so a row starts at any
//   alignment and no pixel is aligned to anything; each lane takes the ALIGNED 16-byte chunk lane of the 64 that cover the run (1008 bytes at any of
//   the 16 offsets fit in 1024) — one 16-byte load where the whole chunk lies inside the row, element loads for the row's ragged first and last
//   chunk (nothing outside the row is ever read).  A run holds whole pixels, so no pixel straddles two waves; two neighbouring runs may both load
//   the chunk that holds their common border.
//   LDS layout: the 64 chunks exactly as loaded, linear (1024 bytes per wave, written with one 16-byte store per lane).  The read side is lane p
//   taking elements off + 3 p + c: for float32 that is a stride of 3 dwords across the lanes, and 3 is coprime to the 32 banks of a 4-byte LDS read,
//   so the 32 lanes of each half-wave fall on 32 different banks — no padding or swizzle can do better than the plain layout.  For uint8 the 32
//   lanes read bytes 3 apart: 96 bytes = at most 25 consecutive dwords, fewer than the 32 banks; lanes that share a dword are served by one access.
//   Stores are then one element per lane along each of the three planes and the mask.
//   n_valid as in evalprep.hip: one integer atomic add per block into a counter cleared on the stream first; exact in any order.
//
// e2eft_dsine_rgb_requantize: the image round trip of test.py:59-65 on the decoded bytes.  The reference normalises the image (x / 255, ImageNet
//   mean / std, all fp32), takes the minimum and maximum of that tensor over all channels, maps (img - min) / (max - min) * 255.0 and truncates to
//   uint8.  Every step is a function of (channel, byte), 768 cases per image, so two passes over the bytes do it exactly:
//   pass 1  each channel's smallest and largest byte: 16 pixels (48 bytes, three 16-byte loads) per lane and step, a wave reduction, the four waves
//           joined through LDS, then one integer atomic for the minimum and one for the maximum per channel and block.  The minimum is kept as the
//           MAXIMUM of 255 - v, so that all six counters start from zero and ONE clear on the stream serves them (the pattern of n_valid above,
//           which replays from a captured graph.  An earlier form set the minima to all ones and the maxima to zero with two memsets; captured
//           in a graph, its second replay produced an empty range.  The cause was not isolated; the single clear is the form that is tested);
//   pass 2  each block rebuilds the 768-entry table in LDS from those six bytes — f(c, v) = (float(v) / 255.0f - mean_c) / std_c is monotone in v, so
//           the tensor's minimum is the least f(c, lo_c) and its maximum the greatest f(c, hi_c); range = float(double(max) - double(min)) (the
//           reference's Python double difference, rounded when it divides the fp32 tensor); out = uint8(trunc(((f - min) / range) * 255.0f)), true
//           fp32 divisions — and maps 16 pixels per lane and step: three 16-byte loads, 48 table reads, three 16-byte stores ([H,W,3]: the same
//           48 bytes; [3,H,W]: 16 bytes along each plane).  A group whose addresses are not 16-byte aligned (a later frame of a batch whose frame
//           size is no multiple of 16, a plane of odd size) or that is cut by the image's end is moved byte by byte; nothing outside is touched.
//   max == min (one single normalised value in the whole image) makes the reference divide by zero; this writes zeros.
#include <algorithm>
#include "common.h"

namespace e2eft {

constexpr int NG_ROWS = 4, NG_THREADS = 64 * NG_ROWS, NG_RUN_BYTES = 1008;

__device__ __forceinline__ float ng_decode_u8(uint8_t v) { return __fdiv_rn((float)v, 255.0f) * 2.0f - 1.0f; }

template <typename T>
__global__ __launch_bounds__(NG_THREADS) void ng_kernel(const int H, const int W, const T* __restrict__ raw, uint32_t* __restrict__ normal, uint8_t* __restrict__ mask,
                                                        int32_t* __restrict__ n_valid) {
    constexpr int E = 16 / sizeof(T);                                  // elements per 16-byte chunk: 16 (uint8) or 4 (float32, moved as uint32)
    constexpr int NP = NG_RUN_BYTES / (3 * (int)sizeof(T));            // pixels per run: 336 or 84
    __shared__ __attribute__((aligned(16))) T sraw[NG_ROWS][64 * E];
    __shared__ int cnt[NG_ROWS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.z, y = blockIdx.y * NG_ROWS + w;
    const bool live = y < H;
    const int p0 = (int)blockIdx.x * NP;                               // first pixel of this run (< W by the grid)
    int off = 0;                                                       // elements of the first chunk that lie before the run's first element
    if (live) {
        const T* row = raw + ((int64_t)b * H + y) * W * 3;
        const T* first = row + 3 * p0;
        off = (int)(((uintptr_t)first & 15) / sizeof(T));
        const int k0 = 3 * p0 - off + lane * E;                        // this lane's chunk, as an element index of the row (negative before the row)
        const T* chunk = row + k0;                                     // 16-byte aligned
        Vec16<T> q;
        if (k0 >= 0 && k0 + E <= 3 * W) {
            q = ld16(chunk);
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) q.e[e] = (k0 + e >= 0 && k0 + e < 3 * W) ? chunk[e] : (T)0;
        }
        st16(&sraw[w][lane * E], q);
    }
    __syncthreads();
    int c = 0;
    if (live) {
        const int64_t hw = (int64_t)H * W, o = (int64_t)b * 3 * hw + (int64_t)y * W, om = (int64_t)b * hw + (int64_t)y * W;
#pragma unroll
        for (int j = 0; j < (NP + 63) / 64; ++j) {
            const int p = lane + 64 * j, x = p0 + p;
            if (p < NP && x < W) {
                const T r = sraw[w][off + 3 * p], g = sraw[w][off + 3 * p + 1], bl = sraw[w][off + 3 * p + 2];
                uint8_t ok;
                if constexpr (sizeof(T) == 1) {
                    ok = ((int)r + (int)g + (int)bl) > 0 ? 1 : 0;
                    normal[o + x] = __float_as_uint(ng_decode_u8(r));
                    normal[o + hw + x] = __float_as_uint(ng_decode_u8(g));
                    normal[o + 2 * hw + x] = __float_as_uint(ng_decode_u8(bl));
                } else {
                    const float fr = __uint_as_float(r), fg = __uint_as_float(g), fb = __uint_as_float(bl);
                    ok = __fsqrt_rn((fr * fr + fg * fg) + fb * fb) > 0.5f ? 1 : 0;
                    normal[o + x] = r;
                    normal[o + hw + x] = g;
                    normal[o + 2 * hw + x] = bl;
                }
                mask[om + x] = ok;
                c += ok;
            }
        }
    }
    c = wave_sum(c);
    if (lane == 0) cnt[w] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int s = ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
        if (s) atomicAdd(&n_valid[b], s);
    }
}

// ---- the image round trip -------------------------------------------------------------------------------------------------------------------------------
constexpr int RQ_THREADS = 256, RQ_GROUP = 16;                         // pixels per lane and step: 48 bytes in, three 16-byte chunks
__device__ __forceinline__ bool rq_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the 48 bytes of pixel group g of an image of n bytes -> v[48]; `fill` where the group runs past the image
__device__ __forceinline__ void rq_load(const uint8_t* __restrict__ img, const int n, const int g, const uint8_t fill, uint8_t (&v)[3 * RQ_GROUP]) {
    const uint8_t* p = img + (int64_t)g * (3 * RQ_GROUP);
    const int left = n - g * (3 * RQ_GROUP);
    if (left >= 3 * RQ_GROUP && rq_al16(p)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const Vec16<uint8_t> q = ld16(p + 16 * k);
#pragma unroll
            for (int e = 0; e < 16; ++e) v[16 * k + e] = q.e[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 3 * RQ_GROUP; ++e) v[e] = e < left ? p[e] : fill;
    }
}

__global__ __launch_bounds__(RQ_THREADS) void rq_range_kernel(const int n, const uint8_t* __restrict__ rgb, uint32_t* __restrict__ nlo, uint32_t* __restrict__ hi) {
    __shared__ uint32_t slo[RQ_THREADS / 64][3], shi[RQ_THREADS / 64][3];
    const int b = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint8_t* img = rgb + (int64_t)b * n;
    const int groups = (n + 3 * RQ_GROUP - 1) / (3 * RQ_GROUP);
    uint32_t l[3] = {255u, 255u, 255u}, h[3] = {0u, 0u, 0u};
    for (int g = (int)blockIdx.x * RQ_THREADS + (int)threadIdx.x; g < groups; g += (int)gridDim.x * RQ_THREADS) {
        uint8_t v[3 * RQ_GROUP];
        rq_load(img, n, g, 0, v);
        const int left = n - g * (3 * RQ_GROUP);
#pragma unroll
        for (int e = 0; e < 3 * RQ_GROUP; ++e) {                       // a group starts on a pixel: byte e belongs to channel e % 3
            h[e % 3] = max(h[e % 3], (uint32_t)v[e]);                  // the fill 0 never raises a maximum
            l[e % 3] = min(l[e % 3], e < left ? (uint32_t)v[e] : 255u);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        l[c] = wave_min(l[c]);
        h[c] = wave_max(h[c]);
        if (lane == 0) slo[w][c] = l[c], shi[w][c] = h[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        atomicMax(&nlo[b * 3 + c], 255u - min(min(slo[0][c], slo[1][c]), min(slo[2][c], slo[3][c])));     // min v = 255 - max (255 - v)
        atomicMax(&hi[b * 3 + c], max(max(shi[0][c], shi[1][c]), max(shi[2][c], shi[3][c])));
    }
}

__device__ __forceinline__ float rq_norm(const int c, const uint32_t v) {
    // transforms.Normalize(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)) on float(v) / 255.0f; the constants are the doubles rounded to fp32
    const float mean = c == 0 ? 0.485f : c == 1 ? 0.456f : 0.406f, std = c == 0 ? 0.229f : c == 1 ? 0.224f : 0.225f;
    return __fdiv_rn(__fdiv_rn((float)v, 255.0f) - mean, std);
}

template <bool CHW>
__global__ __launch_bounds__(RQ_THREADS) void rq_map_kernel(const int n, const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ nlo, const uint32_t* __restrict__ hi,
                                                            uint8_t* __restrict__ out) {
    __shared__ uint8_t table[3][256];
    const int b = blockIdx.y;
    {
        const float mn = fminf(fminf(rq_norm(0, 255u - nlo[b * 3]), rq_norm(1, 255u - nlo[b * 3 + 1])), rq_norm(2, 255u - nlo[b * 3 + 2]));
        const float mx = fmaxf(fmaxf(rq_norm(0, hi[b * 3]), rq_norm(1, hi[b * 3 + 1])), rq_norm(2, hi[b * 3 + 2]));
        const float range = (float)((double)mx - (double)mn);
        const uint32_t v = threadIdx.x;                                // RQ_THREADS == 256: one byte value per thread
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // bytes outside [lo_c, hi_c] do not occur in the image; their entries are never read (the clamp only keeps the conversion defined)
            const float t = __fdiv_rn(rq_norm(c, v) - mn, range) * 255.0f;
            table[c][v] = range > 0.0f ? (uint8_t)(int)fminf(fmaxf(t, 0.0f), 255.0f) : (uint8_t)0;
        }
    }
    __syncthreads();
    const uint8_t* img = rgb + (int64_t)b * n;
    uint8_t* dst = out + (int64_t)b * n;
    const int npix = n / 3, groups = (n + 3 * RQ_GROUP - 1) / (3 * RQ_GROUP);
    for (int g = (int)blockIdx.x * RQ_THREADS + (int)threadIdx.x; g < groups; g += (int)gridDim.x * RQ_THREADS) {
        uint8_t v[3 * RQ_GROUP];
        rq_load(img, n, g, 0, v);
        const int left = n - g * (3 * RQ_GROUP);                       // bytes of this group inside the image (>= 48: all)
        if constexpr (!CHW) {
            Vec16<uint8_t> q[3];
#pragma unroll
            for (int e = 0; e < 3 * RQ_GROUP; ++e) q[e / 16].e[e % 16] = table[e % 3][v[e]];
            uint8_t* p = dst + (int64_t)g * (3 * RQ_GROUP);
            if (left >= 3 * RQ_GROUP && rq_al16(p)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) st16(p + 16 * k, q[k]);
            } else {
#pragma unroll
                for (int e = 0; e < 3 * RQ_GROUP; ++e)
                    if (e < left) p[e] = q[e / 16].e[e % 16];
            }
        } else {
            const int x0 = g * RQ_GROUP, pix = min(RQ_GROUP, npix - x0);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Vec16<uint8_t> q;
#pragma unroll
                for (int i = 0; i < RQ_GROUP; ++i) q.e[i] = table[c][v[3 * i + c]];
                uint8_t* p = dst + (int64_t)c * npix + x0;
                if (pix == RQ_GROUP && rq_al16(p)) {
                    st16(p, q);
                } else {
#pragma unroll
                    for (int i = 0; i < RQ_GROUP; ++i)
                        if (i < pix) p[i] = q.e[i];
                }
            }
        }
    }
}

static int np_shape_check(int batch, int height, int width, const char* who) {
    E2EFT_REQUIRE(batch > 0 && height > 0 && width > 0, "%s: shape %d x %d x %d", who, batch, height, width);
    E2EFT_REQUIRE(batch <= 65535, "%s: batch %d out of range (<= 65535: one grid plane per frame)", who, batch);
    E2EFT_REQUIRE((int64_t)height * width * 3 < ((int64_t)1 << 31) - 64, "%s: %d x %d x 3 elements per frame do not fit 31 bits", who, height, width);
    return E2EFT_OK;
}

}  // namespace e2eft

using namespace e2eft;

extern "C" int e2eft_normal_gt_prepare(const e2eft_normal_gt_desc* desc, const void* raw, float* normal, uint8_t* mask, int32_t* n_valid, void* stream) {
    E2EFT_REQUIRE(desc, "normal_gt_prepare: null descriptor");
    const e2eft_normal_gt_desc d = *desc;
    const int rc = np_shape_check(d.batch, d.height, d.width, "normal_gt_prepare");
    if (rc != E2EFT_OK) return rc;
    E2EFT_REQUIRE(d.raw_dtype == E2EFT_NORMAL_GT_U8 || d.raw_dtype == E2EFT_NORMAL_GT_F32, "normal_gt_prepare: raw_dtype %d (E2EFT_NORMAL_GT_U8 or E2EFT_NORMAL_GT_F32)", d.raw_dtype);
    E2EFT_REQUIRE(d.height <= 65535 * NG_ROWS, "normal_gt_prepare: height %d out of range (<= %d)", d.height, 65535 * NG_ROWS);
    E2EFT_REQUIRE(raw && normal && mask && n_valid, "normal_gt_prepare: null pointer");
    E2EFT_REQUIRE((d.raw_dtype == E2EFT_NORMAL_GT_U8 || ((uintptr_t)raw & 3) == 0) && ((uintptr_t)normal & 3) == 0 && ((uintptr_t)n_valid & 3) == 0,
                  "normal_gt_prepare: float32 raw, normal and n_valid must be aligned to 4 bytes");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(n_valid, 0, sizeof(int32_t) * (size_t)d.batch, s) != hipSuccess) return check_launch("normal_gt_prepare (clear n_valid)");
    const int np = NG_RUN_BYTES / (d.raw_dtype == E2EFT_NORMAL_GT_U8 ? 3 : 12);
    const dim3 grid((d.width + np - 1) / np, (d.height + NG_ROWS - 1) / NG_ROWS, d.batch);
    if (d.raw_dtype == E2EFT_NORMAL_GT_U8)
        hipLaunchKernelGGL((ng_kernel<uint8_t>), grid, dim3(NG_THREADS), 0, s, d.height, d.width, (const uint8_t*)raw, (uint32_t*)normal, mask, n_valid);
    else
        hipLaunchKernelGGL((ng_kernel<uint32_t>), grid, dim3(NG_THREADS), 0, s, d.height, d.width, (const uint32_t*)raw, (uint32_t*)normal, mask, n_valid);
    return check_launch("normal_gt_prepare");
}

extern "C" int e2eft_dsine_rgb_requantize(const e2eft_dsine_rgb_desc* desc, const uint8_t* rgb, uint8_t* out, int32_t* workspace, void* stream) {
    E2EFT_REQUIRE(desc, "dsine_rgb_requantize: null descriptor");
    const e2eft_dsine_rgb_desc d = *desc;
    const int rc = np_shape_check(d.batch, d.height, d.width, "dsine_rgb_requantize");
    if (rc != E2EFT_OK) return rc;
    E2EFT_REQUIRE(d.out_layout == E2EFT_RGB_HWC || d.out_layout == E2EFT_RGB_CHW, "dsine_rgb_requantize: out_layout %d (E2EFT_RGB_HWC or E2EFT_RGB_CHW)", d.out_layout);
    E2EFT_REQUIRE(rgb && out && workspace, "dsine_rgb_requantize: null pointer");
    E2EFT_REQUIRE(rgb != out, "dsine_rgb_requantize: out must not be the input");
    E2EFT_REQUIRE(((uintptr_t)workspace & 3) == 0, "dsine_rgb_requantize: workspace must be aligned to 4 bytes");
    hipStream_t s = (hipStream_t)stream;
    uint32_t* nlo = (uint32_t*)workspace;                              // [batch][3]: max of 255 - v
    uint32_t* hi = nlo + 3 * (size_t)d.batch;                          // [batch][3]: max of v
    if (hipMemsetAsync(workspace, 0, sizeof(uint32_t) * E2EFT_DSINE_RGB_WS_INTS * (size_t)d.batch, s) != hipSuccess)
        return check_launch("dsine_rgb_requantize (clear the range counters)");
    const int n = d.height * d.width * 3;
    const int groups = (n + 3 * RQ_GROUP - 1) / (3 * RQ_GROUP);
    const dim3 grid(std::min(std::max((groups + 4 * RQ_THREADS - 1) / (4 * RQ_THREADS), 1), 1024), d.batch);      // about four groups per lane: the table is rebuilt per block
    hipLaunchKernelGGL(rq_range_kernel, grid, dim3(RQ_THREADS), 0, s, n, rgb, nlo, hi);
    if (d.out_layout == E2EFT_RGB_HWC)
        hipLaunchKernelGGL((rq_map_kernel<false>), grid, dim3(RQ_THREADS), 0, s, n, rgb, (const uint32_t*)nlo, (const uint32_t*)hi, out);
    else
        hipLaunchKernelGGL((rq_map_kernel<true>), grid, dim3(RQ_THREADS), 0, s, n, rgb, (const uint32_t*)nlo, (const uint32_t*)hi, out);
    return check_launch("dsine_rgb_requantize");
}
