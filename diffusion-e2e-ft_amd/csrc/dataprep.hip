// dataprep.hip — training-sample preparation on the GPU: what Hypersim.__getitem__ / VirtualKITTI2.__getitem__ do to a
// decoded, augmented sample (/root/reference/training/dataloaders/load.py:236-283 and :342-375, the same arithmetic twice):
//   valid = near < depth < far;  (lo, hi) = 2 % / 98 % quantiles of the valid depths (torch.quantile, linear interpolation);
//   depth -> clamp to [lo, hi], invalid pixels = hi (the metric target), then mapped to [-1, 1] and stacked x3 for the VAE;
//   rgb, normals -> [-1, 1], normals renormalised, invalid pixels zeroed; lo == hi or no valid pixel -> zeros and an empty mask.
// The quantiles are EXACT order statistics: the radix select of select.h over order_key(depth), two selections per image (the floor neighbour of
// each quantile, its successor where the rank has a fraction) — integer atomics only, so the result is deterministic.
#include "common.h"
#include "select.h"
#include <math.h>

namespace e2eft {

constexpr int DP_SEL = 2;             // selections per image: q_lo, q_hi
constexpr int DP_MAX_BLOCKS = 256;    // blocks per image of the digit and successor passes

struct DpLayout {
    SelState* state;      // [B][DP_SEL]
    uint32_t* hist;       // [B][DP_SEL][SEL_BINS]
    uint32_t* mpart;      // [B][DP_SEL][DP_MAX_BLOCKS] successor partials
};
static size_t dp_ws_bytes(int batch) { return (size_t)batch * DP_SEL * (sizeof(SelState) + (SEL_BINS + DP_MAX_BLOCKS) * sizeof(uint32_t)); }
static DpLayout dp_layout(void* ws, int batch) {
    DpLayout l;
    l.state = (SelState*)ws;
    l.hist = (uint32_t*)(l.state + (size_t)batch * DP_SEL);
    l.mpart = l.hist + (size_t)batch * DP_SEL * SEL_BINS;
    return l;
}

// torch.quantile: rank = q * (n - 1) in float32, floor / ceil neighbours, weight = the fractional part
struct DpQuantileRank {
    float q[DP_SEL];
    __device__ SelRank operator()(int64_t n, int sel) const {
        const float r = ((sel & 1) ? q[1] : q[0]) * (float)(n - 1);
        const float f = floorf(r);
        return SelRank{(int64_t)(unsigned)f, (unsigned)ceilf(r) != (unsigned)f, (double)(r - f)};
    }
};

__global__ void dp_init_kernel(int nsel, SelState* __restrict__ state, uint32_t* __restrict__ hist) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)nsel * SEL_BINS) hist[i] = 0;
    if (i < nsel) select_init(state + i, true);
}

// digit p of both selections over the valid pixels of image blockIdx.y.  grid (blocks, B)
__global__ __launch_bounds__(256) void dp_hist_kernel(int p, long n, float near, float far, const float* __restrict__ depth, const SelState* __restrict__ state,
                                                      uint32_t* __restrict__ hist) {
    DigitHist<uint32_t, DP_SEL> h(p, state + blockIdx.y * DP_SEL);
    if (!h.any) return;
    h.zero();
    const float* d = depth + (long)blockIdx.y * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = d[i];
        if (v > near && v < far) h.add(order_key(v));
    }
    h.flush(hist + (long)blockIdx.y * DP_SEL * SEL_BINS);
}

__global__ __launch_bounds__(256) void dp_min_kernel(long n, float near, float far, const float* __restrict__ depth, const SelState* __restrict__ state,
                                                     uint32_t* __restrict__ mpart) {
    SuccMin<uint32_t, DP_SEL> m(state + blockIdx.y * DP_SEL);
    if (!m.any()) return;
    const float* d = depth + (long)blockIdx.y * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = d[i];
        if (v > near && v < far) m.take(order_key(v));
    }
    m.store(mpart + (long)blockIdx.y * DP_SEL * DP_MAX_BLOCKS + blockIdx.x, DP_MAX_BLOCKS);
}

// one wave per image: the two interpolated quantiles and the ok flag
__global__ __launch_bounds__(64) void dp_finish_kernel(int nblk, const SelState* __restrict__ state, const uint32_t* __restrict__ mpart,
                                                       float* __restrict__ out /* [B][4] = lo, hi, count, ok */) {
    const SelState* st = state + blockIdx.x * DP_SEL;
    float q[DP_SEL];
#pragma unroll
    for (int j = 0; j < DP_SEL; ++j) {
        const uint32_t b = select_successor(st[j], mpart + ((long)blockIdx.x * DP_SEL + j) * DP_MAX_BLOCKS, nblk);
        q[j] = st[j].n ? quantile_lerp(order_value((uint32_t)st[j].prefix), order_value(b), (float)st[j].weight) : 0.f;
    }
    if (threadIdx.x != 0) return;
    const unsigned count = (unsigned)st[0].n;
    float* o = out + blockIdx.x * 4;
    o[0] = q[0]; o[1] = q[1]; o[2] = (float)count; o[3] = (count > 0 && q[0] != q[1]) ? 1.f : 0.f;
}

// the fused elementwise pass.  grid (blocks, B)
__global__ __launch_bounds__(256) void dp_prepare(long hw, float near, float far, const float* __restrict__ rgb, const float* __restrict__ depth,
                                                  const float* __restrict__ normal, const float* __restrict__ quant, float* __restrict__ o_rgb,
                                                  float* __restrict__ o_depth3, float* __restrict__ o_metric, float* __restrict__ o_normal,
                                                  uint8_t* __restrict__ o_mask) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const float lo = quant[b * 4], hi = quant[b * 4 + 1];
    const bool ok = quant[b * 4 + 3] != 0.f;
    const float range = hi - lo;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < hw; p += (long)gridDim.x * 256) {
        const float d = depth[(long)b * hw + p];
        const bool valid = ok && d > near && d < far;                       // load.py:236, :246 (mask emptied when lo == hi)
        float metric = 0.f, dn = 0.f;
        if (ok) {
            metric = fminf(fmaxf(d, lo), hi);                              // :249  clamp
            if (!valid) metric = hi;                                       // :250  invalid -> relative far plane
            dn = ((metric - lo) / range) * 2.0f - 1.0f;                    // :252
            dn = fminf(fmaxf(dn, -1.f), 1.f);
        }
        o_metric[(long)b * hw + p] = metric;
        o_mask[(long)b * hw + p] = valid ? 1 : 0;
        float n[3];
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long i = ((long)b * 3 + c) * hw + p;
            o_rgb[i] = rgb[i] * 2.0f - 1.0f;                               // :239
            o_depth3[i] = dn;                                              // :256  three identical channels
            n[c] = normal[i] * 2.0f - 1.0f;                                // :259
            ss += n[c] * n[c];
        }
        const float inv = fmaxf(sqrtf(ss), 1e-12f);                        // F.normalize(p=2, dim=0), eps = 1e-12
#pragma unroll
        for (int c = 0; c < 3; ++c) o_normal[((long)b * 3 + c) * hw + p] = valid ? n[c] / inv : 0.f;   // :260-264
    }
}

// Hypersim.__getitem__'s normal orientation fix (load.py:225-232 with align_normals / creat_uv_mesh, :185-204; Hypersim's stored normals do not always
// face the camera), on the DECODED uint8 normal image and the metric depth, in the reference's float64 arithmetic operation for operation (no contraction):
//   n = u8 / 255 * 2 - 1;  n.y, n.z *= -1;  P = depth * (invK [x, y, 1]^T);  if (n . P > 0) n = -n;  n = -n;  u8' = trunc((n + 1) / 2 * 255).
// One thread per pixel; 7 B read, 3 B written.
struct DpInvK { double m[9]; };
__global__ __launch_bounds__(256) void dp_align_normals(int h, int w, const uint8_t* __restrict__ nrm, const float* __restrict__ depth, DpInvK ik,
                                                        uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
    const long hw = (long)h * w;
    const long b = blockIdx.y;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < hw; p += (long)gridDim.x * 256) {
        const int y = (int)(p / w), x = (int)(p - (long)y * w);
        const uint8_t* src = nrm + (b * hw + p) * 3;
        double n[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) n[c] = ((double)src[c] / 255.0) * 2.0 - 1.0;
        n[1] *= -1.0;
        n[2] *= -1.0;
        const double d = (double)depth[b * hw + p];
        double dot = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double pr = (ik.m[3 * r] * (double)x + ik.m[3 * r + 1] * (double)y) + ik.m[3 * r + 2] * 1.0;      // (inv_K @ xy)[r], k in order
            const double t = n[r] * (d * pr);
            dot = r == 0 ? t : dot + t;
        }
        const double sgn = dot > 0.0 ? 1.0 : -1.0;          // flipped by the mask, then the whole map times -1: net +1 where the mask is set, -1 elsewhere
        uint8_t* dst = out + (b * hw + p) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = n[c] * sgn;
            dst[c] = (uint8_t)(int)(((v + 1.0) / 2.0) * 255.0);      // .astype(np.uint8): truncation
        }
    }
}

}  // namespace e2eft

using namespace e2eft;

extern "C" size_t e2eft_masked_quantiles_workspace_bytes(int32_t batch) {
    if (batch < 1) {
        fail(E2EFT_ERR_BAD_ARG, "masked_quantiles: batch = %d", (int)batch);
        return 0;
    }
    return dp_ws_bytes(batch);
}

extern "C" int e2eft_masked_quantiles(int32_t batch, int64_t n, const float* depth, float near_plane, float far_plane, float q_lo, float q_hi,
                                      float* out, void* workspace, size_t ws_bytes, void* stream) {
    E2EFT_REQUIRE(batch >= 1 && n >= 1 && n < 2147483647L && depth && out && workspace, "masked_quantiles: bad arguments");
    E2EFT_REQUIRE(q_lo >= 0.f && q_lo <= 1.f && q_hi >= 0.f && q_hi <= 1.f, "masked_quantiles: quantiles must lie in [0, 1]");
    E2EFT_REQUIRE(ws_bytes >= dp_ws_bytes(batch), "masked_quantiles: workspace %zu < %zu bytes", ws_bytes, dp_ws_bytes(batch));
    hipStream_t s = (hipStream_t)stream;
    const DpLayout l = dp_layout(workspace, batch);
    const int blocks = cdiv(n, 256 * 16) < DP_MAX_BLOCKS ? cdiv(n, 256 * 16) : DP_MAX_BLOCKS;
    const int nsel = batch * DP_SEL;
    hipLaunchKernelGGL(dp_init_kernel, dim3(nsel * (SEL_BINS / 256)), dim3(256), 0, s, nsel, l.state, l.hist);
    for (int p = 0; p < select_digits(32); ++p) {
        hipLaunchKernelGGL(dp_hist_kernel, dim3(blocks, batch), dim3(256), 0, s, p, (long)n, near_plane, far_plane, depth, (const SelState*)l.state, l.hist);
        hipLaunchKernelGGL((select_scan_kernel<uint32_t, DpQuantileRank>), dim3(nsel), dim3(SEL_BINS / 2), 0, s, p, l.hist, l.state, DpQuantileRank{{q_lo, q_hi}});
    }
    hipLaunchKernelGGL(dp_min_kernel, dim3(blocks, batch), dim3(256), 0, s, (long)n, near_plane, far_plane, depth, (const SelState*)l.state, l.mpart);
    hipLaunchKernelGGL(dp_finish_kernel, dim3(batch), dim3(64), 0, s, blocks, (const SelState*)l.state, (const uint32_t*)l.mpart, out);
    return check_launch("masked_quantiles");
}

extern "C" int e2eft_prepare_sample(int32_t batch, int64_t hw, const float* rgb01, const float* depth, const float* normal01, float near_plane,
                                    float far_plane, const float* quantiles, float* rgb, float* depth3, float* metric, float* normals,
                                    uint8_t* val_mask, void* stream) {
    E2EFT_REQUIRE(batch >= 1 && hw >= 1 && rgb01 && depth && normal01 && quantiles && rgb && depth3 && metric && normals && val_mask,
                  "prepare_sample: bad arguments");
    const int blocks = cdiv(hw, 256 * 4) < 1024 ? cdiv(hw, 256 * 4) : 1024;
    hipLaunchKernelGGL(dp_prepare, dim3(blocks, batch), dim3(256), 0, (hipStream_t)stream, (long)hw, near_plane, far_plane, rgb01, depth, normal01,
                       quantiles, rgb, depth3, metric, normals, val_mask);
    return check_launch("prepare_sample");
}

extern "C" int e2eft_align_normals_u8(int32_t batch, int32_t h, int32_t w, const uint8_t* normal_u8, const float* depth, const double* inv_k,
                                      uint8_t* out, void* stream) {
    E2EFT_REQUIRE(batch >= 1 && batch <= 65535 && h >= 1 && w >= 1 && normal_u8 && depth && inv_k && out, "align_normals: bad arguments");
    DpInvK ik;
    for (int i = 0; i < 9; ++i) ik.m[i] = inv_k[i];
    const long hw = (long)h * w;
    const int blocks = cdiv(hw, 256) < 4096 ? (int)cdiv(hw, 256) : 4096;
    hipLaunchKernelGGL(dp_align_normals, dim3(blocks, batch), dim3(256), 0, (hipStream_t)stream, (int)h, (int)w, normal_u8, depth, ik, out);
    return check_launch("align_normals");
}
