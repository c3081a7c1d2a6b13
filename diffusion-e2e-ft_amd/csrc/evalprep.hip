// evalprep.hip — decoded benchmark ground truth to evaluation inputs on the device: what the reference's evaluation dataset classes do to a depth file
// after decoding it (Marigold/src/dataset/base_depth_dataset.py:127-141,181-185 and the per-benchmark overrides nyu_dataset.py:27-43,
// kitti_dataset.py:35-105, eth3d_dataset.py:41-45, scannet_dataset.py:21-25, diode_dataset.py:65-68), for a batch of rasters in one launch.
//   decode       d = float(double(raw) / divisor): numpy's float64 division, then torch's .float(); a float32 raster with divisor 1 passes through bit for bit
//   ETH3D        d == +inf -> 0 (NaN stays NaN and is invalid by comparison)
//   crop         the output rectangle [crop_top, crop_top + crop_h) x [crop_left, crop_left + crop_w) of the raster (KITTI's benchmark crop)
//   validity     d > min_depth && d < max_depth in float32, inside the evaluation window (eigen / garg); or the file's own mask alone (DIODE)
//   count        n_valid[b]: the sum of the frame's mask
// One wave per 16-byte-chunk run of one output row: the row's first element sits anywhere in its chunk (an odd crop_left, an odd raster width: the
// alignment changes from row to row), so each lane takes the ALIGNED chunk that covers its elements — one 16-byte load when the whole chunk lies inside the
// row, element loads for the row's ragged first and last chunk (nothing outside the row is ever read).  The decoded values go through LDS so that the
// stores are one element per lane along the row, whatever the input alignment was.
// n_valid: each block adds ONE integer (its four waves' counts, summed in wave order) to the frame's counter with an integer atomic; integer addition is
// exact in any order, so the count is bit-reproducible.  The counter is cleared on the stream first.  No host read-back: capturable in a graph.
#include "common.h"

namespace e2eft {

constexpr int GP_ROWS = 4, GP_THREADS = 64 * GP_ROWS;

template <typename T> __device__ __forceinline__ float gp_decode(T v, double divisor) { return (float)((double)v / divisor); }
// float32 metres as stored (divisor 1): no conversion touches them, a NaN keeps its payload
template <> __device__ __forceinline__ float gp_decode<float>(float v, double divisor) { return divisor == 1.0 ? v : (float)((double)v / divisor); }

template <typename T>
__global__ __launch_bounds__(GP_THREADS) void gp_kernel(const e2eft_depth_gt_desc d, const T* __restrict__ raw, const uint8_t* __restrict__ ext,
                                                        float* __restrict__ depth, uint8_t* __restrict__ mask, int32_t* __restrict__ n_valid) {
    constexpr int E = 16 / sizeof(T);                                  // elements per 16-byte chunk: 8 (uint16) or 4 (int32, float32)
    __shared__ __attribute__((aligned(16))) float sd[GP_ROWS][64 * E];
    __shared__ __attribute__((aligned(16))) uint8_t sm[GP_ROWS][64 * E];
    __shared__ int cnt[GP_ROWS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.z, y = blockIdx.y * GP_ROWS + w;
    const bool live = y < d.crop_h;
    const int tile0 = (int)blockIdx.x * 64 * E;                        // first element slot of this block's run, counted from the row's first chunk
    const int64_t in_row = ((int64_t)b * d.h0 + d.crop_top + y) * d.w0 + d.crop_left;
    int head = 0;                                                      // elements of the first chunk that lie before the row's first element
    if (live) {
        const T* row = raw + in_row;
        head = (int)(((uintptr_t)row & 15) / sizeof(T));
        const int x0 = tile0 + lane * E - head;                        // output column of this lane's first element
        const T* chunk = row + x0;                                     // 16-byte aligned
        T v[E];
        if (x0 >= 0 && x0 + E <= d.crop_w) {
            const Vec16<T> q = ld16(chunk);
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = q.e[e];
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = (x0 + e >= 0 && x0 + e < d.crop_w) ? chunk[e] : (T)0;
        }
        const bool in_y = y >= d.win_y0 && y < d.win_y1;
        float o[E];
        uint32_t m[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            float f = gp_decode(v[e], d.divisor);
            if (d.inf_to_zero && f == __builtin_inff()) f = 0.0f;
            const int x = x0 + e;
            o[e] = f;
            m[e] = (f > d.min_depth && f < d.max_depth && in_y && x >= d.win_x0 && x < d.win_x1) ? 1u : 0u;
        }
#pragma unroll
        for (int q = 0; q < E / 4; ++q) {
            floatx4 t = {o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
            *reinterpret_cast<floatx4*>(&sd[w][lane * E + 4 * q]) = t;
            *reinterpret_cast<uint32_t*>(&sm[w][lane * E + 4 * q]) = m[4 * q] | (m[4 * q + 1] << 8) | (m[4 * q + 2] << 16) | (m[4 * q + 3] << 24);
        }
    }
    __syncthreads();
    int c = 0;
    if (live) {
        const int64_t out_row = ((int64_t)b * d.crop_h + y) * d.crop_w;
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int i = lane + 64 * j, x = tile0 + i - head;
            if (x >= 0 && x < d.crop_w) {
                const uint8_t ok = d.use_ext_mask ? (ext[in_row + x] != 0 ? 1 : 0) : sm[w][i];
                depth[out_row + x] = sd[w][i];
                mask[out_row + x] = ok;
                c += ok;
            }
        }
    }
    if (n_valid == nullptr) return;
    c = wave_sum(c);
    if (lane == 0) cnt[w] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int s = ((cnt[0] + cnt[1]) + cnt[2]) + cnt[3];
        if (s) atomicAdd(&n_valid[b], s);
    }
}

static int gp_check(const e2eft_depth_gt_desc* d, const char* who) {
    E2EFT_REQUIRE(d, "%s: null descriptor", who);
    E2EFT_REQUIRE(d->batch > 0 && d->h0 > 0 && d->w0 > 0, "%s: shape %d x %d x %d", who, d->batch, d->h0, d->w0);
    E2EFT_REQUIRE(d->batch <= 65535, "%s: batch %d out of range (<= 65535: one grid plane per frame)", who, d->batch);
    E2EFT_REQUIRE(d->raw_dtype == E2EFT_GT_U16 || d->raw_dtype == E2EFT_GT_I32 || d->raw_dtype == E2EFT_GT_F32,
                  "%s: raw_dtype %d (E2EFT_GT_U16, E2EFT_GT_I32 or E2EFT_GT_F32)", who, d->raw_dtype);
    E2EFT_REQUIRE(d->divisor > 0.0 && d->divisor < 1e300, "%s: divisor %g must be positive and finite", who, d->divisor);
    E2EFT_REQUIRE(d->crop_top >= 0 && d->crop_left >= 0 && d->crop_h > 0 && d->crop_w > 0 && d->crop_h <= d->h0 - d->crop_top && d->crop_w <= d->w0 - d->crop_left,
                  "%s: crop %d x %d at (%d, %d) lies outside the %d x %d raster", who, d->crop_h, d->crop_w, d->crop_top, d->crop_left, d->h0, d->w0);
    E2EFT_REQUIRE(d->crop_h <= 65535 * GP_ROWS, "%s: crop_h %d out of range (<= %d)", who, d->crop_h, 65535 * GP_ROWS);
    E2EFT_REQUIRE(d->win_y0 >= 0 && d->win_y0 <= d->win_y1 && d->win_y1 <= d->crop_h && d->win_x0 >= 0 && d->win_x0 <= d->win_x1 && d->win_x1 <= d->crop_w,
                  "%s: window rows %d:%d, cols %d:%d must be clamped to the %d x %d output", who, d->win_y0, d->win_y1, d->win_x0, d->win_x1, d->crop_h, d->crop_w);
    E2EFT_REQUIRE(!(d->min_depth != d->min_depth) && !(d->max_depth != d->max_depth), "%s: min_depth / max_depth must not be NaN", who);
    return E2EFT_OK;
}

}  // namespace e2eft

using namespace e2eft;

extern "C" int e2eft_depth_gt_prepare(const e2eft_depth_gt_desc* desc, const void* raw, const uint8_t* ext_mask, float* depth, uint8_t* mask, int32_t* n_valid,
                                      void* stream) {
    const int rc = gp_check(desc, "depth_gt_prepare");
    if (rc != E2EFT_OK) return rc;
    const e2eft_depth_gt_desc d = *desc;
    E2EFT_REQUIRE(!d.use_ext_mask || ext_mask, "depth_gt_prepare: use_ext_mask is set and ext_mask is null");
    E2EFT_REQUIRE(raw && depth && mask, "depth_gt_prepare: null pointer");
    const size_t esz = d.raw_dtype == E2EFT_GT_U16 ? 2 : 4;
    E2EFT_REQUIRE(((uintptr_t)raw & (esz - 1)) == 0 && ((uintptr_t)depth & 3) == 0 && ((uintptr_t)n_valid & 3) == 0,
                  "depth_gt_prepare: raw must be aligned to its element size, depth and n_valid to 4 bytes");
    hipStream_t s = (hipStream_t)stream;
    if (n_valid && hipMemsetAsync(n_valid, 0, sizeof(int32_t) * (size_t)d.batch, s) != hipSuccess) return check_launch("depth_gt_prepare (clear n_valid)");
    const int e = (int)(16 / esz);
    const int chunks = (d.crop_w + e - 1) / e + 1;                     // a row that starts mid-chunk spans one more
    const dim3 grid((chunks + 63) / 64, (d.crop_h + GP_ROWS - 1) / GP_ROWS, d.batch);
    if (d.raw_dtype == E2EFT_GT_U16)
        hipLaunchKernelGGL((gp_kernel<uint16_t>), grid, dim3(GP_THREADS), 0, s, d, (const uint16_t*)raw, ext_mask, depth, mask, n_valid);
    else if (d.raw_dtype == E2EFT_GT_I32)
        hipLaunchKernelGGL((gp_kernel<int32_t>), grid, dim3(GP_THREADS), 0, s, d, (const int32_t*)raw, ext_mask, depth, mask, n_valid);
    else
        hipLaunchKernelGGL((gp_kernel<float>), grid, dim3(GP_THREADS), 0, s, d, (const float*)raw, ext_mask, depth, mask, n_valid);
    return check_launch("depth_gt_prepare");
}
