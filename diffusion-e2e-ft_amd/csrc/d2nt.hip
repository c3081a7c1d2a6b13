// d2nt.hip — surface normals from depth on the device: the D2NT "v3" translator the fine-tuning authors ran offline over Virtual KITTI 2
// (depth-to-normal-translator/python/gen_vkitti_normals.py:100-133 over utils/myApis.py:48-179, utils/apis.py:38-41).
// One fused kernel per 64 x 16 output tile (256 threads):
//   1. Z = depth * depth_scale (fp32) for the tile + a halo of 3 into LDS, reflect-101 at the image border (cv2.filter2D's default border);
//   2. the fp32 soft-min powers P = powf(e32, -|grad_l - grad_r|) (horizontal) and the vertical twin on the tile + 2 rings (the normal of a pixel
//      one outside the tile reads P one further out), 0 outside the image (soft_min's zero padding), and the fp32 DLF-alpha Laplacian L on the
//      tile + 1 ring, +inf outside the image (MRF_optim's padding);
//   3. per output pixel: the 5-way argmin over L (left, right, up, down, self; first index wins, a NaN at its first occurrence), then the fp64
//      normal of the CHOSEN pixel (refine = 1) or of the pixel itself (refine = 0), computed from the LDS maps — the normal is a pure function
//      of its location, so evaluating it where it is taken equals evaluating the whole ring first and gathering (and does one normal per output);
//   4. n *= -1; fp32 or the file's uint16 ((n + 1) * 32767.5 truncated, from the fp64 value) or its high byte, staged in LDS and written as whole
//      aligned dwords per tile row.
// Precision and order are the reference's (fp32 gradients / Laplacians / powf, fp64 after that); this file is built with -ffp-contract=off so
// that no FMA fuses a product the reference rounds.  powf is evaluated as float(exp(double(x) * log(double(e32)))): correctly rounded except
// within ~1e-14 of a float32 rounding boundary (numpy's own float32 power is SIMD-dispatched and differs from that by 1 ulp on a share of inputs).
#include "common.h"

namespace e2eft {

constexpr int DN_TW = 64, DN_TH = 16, DN_THREADS = 256;
constexpr int DN_ZW = DN_TW + 6, DN_ZH = DN_TH + 6;          // Z: halo 3
constexpr int DN_HW = DN_TW + 4, DN_HH = DN_TH + 2;          // P horizontal: columns -2 .. TW+1, rows -1 .. TH
constexpr int DN_VW = DN_TW + 2, DN_VH = DN_TH + 4;          // P vertical:   columns -1 .. TW, rows -2 .. TH+1
constexpr int DN_LW = DN_TW + 2, DN_LH = DN_TH + 2;          // L: tile + 1 ring
constexpr int DN_OROW = DN_TW * 12;                          // bytes of one staged output row (fp32 x 3 at most)

__device__ __forceinline__ int dn_reflect(int i, int n) {   // BORDER_REFLECT_101 for the one pixel beyond the edge that is ever used; clamped further out
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// powf(2.7182817f, -lap) rounded once from fp64 (myApis.py:59: np.power(np.e, -lap) on a float32 array stays float32)
__device__ __forceinline__ float dn_softpow(float lap) {
    const double ln_e32 = 0x1.fffffefb245eap-1;                // log((double)2.7182817f)
    return (float)exp((double)(-lap) * ln_e32);
}

// soft_min of one direction (myApis.py:63-64 / :69-70) for the pixel between neighbour powers a (left / up) and b (right / down), then the four
// sequential snapping lines (myApis.py:112-115 / :117-120)
__device__ __forceinline__ void dn_weights(float pa, float pb, double& la, double& lb) {
    const double eps = 1e-8, e = 2.718281828459045;
    const double a = (double)pa, b = (double)pb;
    const double den = (eps + a) + b;
    la = (a + eps * 0.5) / den;
    lb = (b + eps * 0.5) / den;
    if (la / (lb + eps) > e) la = 1.0;
    if (la / (lb + eps) > e) lb = 0.0;
    if (lb / (la + eps) > e) la = 0.0;
    if (lb / (la + eps) > e) lb = 1.0;
}

struct DnSmem {
    float z[DN_ZH][DN_ZW];
    float ph[DN_HH][DN_HW];
    float pv[DN_VH][DN_VW];
    float l[DN_LH][DN_LW];
    uint8_t out[DN_TH][DN_OROW];
};

template <int FMT>   // 0 fp32, 1 uint16, 2 uint8
__global__ __launch_bounds__(DN_THREADS) void d2nt_kernel(int H, int W, int refine, float depth_scale, const float* __restrict__ depth,
                                                          const float* __restrict__ intr, uint8_t* __restrict__ out) {
    constexpr int ES = FMT == 0 ? 4 : (FMT == 1 ? 2 : 1);
    constexpr int PB = 3 * ES;
    __shared__ DnSmem sm;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * DN_TW, y0 = blockIdx.y * DN_TH, b = blockIdx.z;
    const float* Zb = depth + (size_t)b * H * W;

    // 1. Z tile with halo 3 (local (i, j) <-> global (y0 - 3 + i, x0 - 3 + j))
    for (int k = tid; k < DN_ZH * DN_ZW; k += DN_THREADS) {
        const int i = k / DN_ZW, j = k - i * DN_ZW;
        const int gy = dn_reflect(y0 - 3 + i, H), gx = dn_reflect(x0 - 3 + j, W);
        sm.z[i][j] = __fmul_rn(Zb[(size_t)gy * W + gx], depth_scale);
    }
    __syncthreads();

    // 2. soft-min powers and the Laplacian.  grad_l = -Z[x-1] + Z[x], grad_r = -Z[x] + Z[x+1] (filter2D taps in row-major order), fp32
    for (int k = tid; k < DN_HH * DN_HW; k += DN_THREADS) {
        const int i = k / DN_HW, j = k - i * DN_HW;            // global (y0 - 1 + i, x0 - 2 + j); z index (i + 2, j + 1)
        const int gy = y0 - 1 + i, gx = x0 - 2 + j;
        float p = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float zl = sm.z[i + 2][j], zc = sm.z[i + 2][j + 1], zr = sm.z[i + 2][j + 2];
            const float gl = __fadd_rn(-zl, zc), gr = __fadd_rn(-zc, zr);
            p = dn_softpow(fabsf(__fsub_rn(gl, gr)));
        }
        sm.ph[i][j] = p;
    }
    for (int k = tid; k < DN_VH * DN_VW; k += DN_THREADS) {
        const int i = k / DN_VW, j = k - i * DN_VW;            // global (y0 - 2 + i, x0 - 1 + j); z index (i + 1, j + 2)
        const int gy = y0 - 2 + i, gx = x0 - 1 + j;
        float p = 0.0f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const float zu = sm.z[i][j + 2], zc = sm.z[i + 1][j + 2], zd = sm.z[i + 2][j + 2];
            const float gu = __fadd_rn(-zu, zc), gd = __fadd_rn(-zc, zd);
            p = dn_softpow(fabsf(__fsub_rn(gu, gd)));
        }
        sm.pv[i][j] = p;
    }
    if (refine) {
        for (int k = tid; k < DN_LH * DN_LW; k += DN_THREADS) {
            const int i = k / DN_LW, j = k - i * DN_LW;        // global (y0 - 1 + i, x0 - 1 + j); z index (i + 2, j + 2)
            const int gy = y0 - 1 + i, gx = x0 - 1 + j;
            float L = __builtin_inff();
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {     // |(((-up + -left) + 4c) + -right) + -down|  (lap_ker_alpha, myApis.py:20-22, :144)
                float s = __fadd_rn(-sm.z[i + 1][j + 2], -sm.z[i + 2][j + 1]);
                s = __fadd_rn(s, __fmul_rn(4.0f, sm.z[i + 2][j + 2]));
                s = __fadd_rn(s, -sm.z[i + 2][j + 3]);
                s = __fadd_rn(s, -sm.z[i + 3][j + 2]);
                L = fabsf(s);
            }
            sm.l[i][j] = L;
        }
    }
    __syncthreads();

    const double fx = (double)intr[4 * b + 0], fy = (double)intr[4 * b + 1], cx = (double)intr[4 * b + 2], cy = (double)intr[4 * b + 3];
    const int tw = min(DN_TW, W - x0), th = min(DN_TH, H - y0);
    for (int k = tid; k < DN_TW * DN_TH; k += DN_THREADS) {
        const int ty = k / DN_TW, tx = k - ty * DN_TW;
        if (ty >= th || tx >= tw) continue;
        // 3. MRF_optim's choice (myApis.py:151-158): [x-1, x+1, y-1, y+1, self]
        int sy = ty, sx = tx;
        if (refine) {
            const float c[5] = {sm.l[ty + 1][tx], sm.l[ty + 1][tx + 2], sm.l[ty][tx + 1], sm.l[ty + 2][tx + 1], sm.l[ty + 1][tx + 1]};
            int best = 0;
            float bv = c[0];
            if (!(bv == bv)) {
                best = 0;
            } else {
                for (int q = 1; q < 5; ++q) {
                    if (!(c[q] == c[q])) { best = q; break; }
                    if (c[q] < bv) { bv = c[q]; best = q; }
                }
            }
            const int dy[5] = {0, 0, -1, 1, 0}, dx[5] = {-1, 1, 0, 0, 0};
            sy += dy[best];
            sx += dx[best];
        }
        const int gy = y0 + sy, gx = x0 + sx;
        double nx = 0.0, ny = 0.0, nz = 0.0;                  // a chosen pixel outside the image contributes MRF_optim's zero padding
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int zi = sy + 3, zj = sx + 3;
            const float zc = sm.z[zi][zj];
            const float gl = __fadd_rn(-sm.z[zi][zj - 1], zc), gr = __fadd_rn(-zc, sm.z[zi][zj + 1]);
            const float gu = __fadd_rn(-sm.z[zi - 1][zj], zc), gd = __fadd_rn(-zc, sm.z[zi + 1][zj]);
            double l1, l2, l3, l4;
            dn_weights(sm.ph[sy + 1][sx + 1], sm.ph[sy + 1][sx + 3], l1, l2);     // P at (y, x - 1), (y, x + 1)
            dn_weights(sm.pv[sy + 1][sx + 1], sm.pv[sy + 3][sx + 1], l3, l4);     // P at (y - 1, x), (y + 1, x)
            const double Gu = l1 * (double)gl + l2 * (double)gr;                     // myApis.py:123-124
            const double Gv = l3 * (double)gu + l4 * (double)gd;
            const double u = (double)(gx + 1) - cx, v = (double)(gy + 1) - cy;      // gen_vkitti_normals.py:109-110 (1-based)
            nx = Gu * fx;
            ny = Gv * fy;
            nz = -(((double)zc + v * Gv) + u * Gu);
            const double d = sqrt((nx * nx + ny * ny) + nz * nz) + 1e-8;           // apis.py:38-41 (np.linalg.norm sums x2, y2, z2 in order)
            nx /= d;
            ny /= d;
            nz /= d;
        }
        nx = nx * -1.0;                                         // gen_vkitti_normals.py:127
        ny = ny * -1.0;
        nz = nz * -1.0;
        uint8_t* o = &sm.out[ty][tx * PB];
        const double n3[3] = {nx, ny, nz};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (FMT == 0) {
                const float f = (float)n3[c];
                const uint32_t u32 = __float_as_uint(f);
#pragma unroll
                for (int q = 0; q < 4; ++q) o[4 * c + q] = (uint8_t)(u32 >> (8 * q));
            } else {
                double t = (n3[c] + 1.0) * 32767.5;                                // :131, astype(uint16) truncates
                t = t < 0.0 ? 0.0 : (t > 65535.0 ? 65535.0 : t);
                const uint32_t q16 = (uint32_t)t;
                if (FMT == 1) {
                    o[2 * c] = (uint8_t)q16;
                    o[2 * c + 1] = (uint8_t)(q16 >> 8);
                } else {
                    o[c] = (uint8_t)(q16 >> 8);                                     // Image.open(p).convert('RGB') of a 48-bit PNG
                }
            }
        }
    }
    __syncthreads();

    // 4. each tile row is one contiguous byte range of the channels-last output: aligned dwords, single bytes at the two ends
    const int nb = tw * PB;
    constexpr int SLOTS = DN_OROW / 4 + 2;                      // dword slots per row (covers a misaligned start)
    for (int k = tid; k < th * SLOTS; k += DN_THREADS) {
        const int r = k / SLOTS, s = k - r * SLOTS;
        const size_t g0 = (((size_t)b * H + y0 + r) * W + x0) * PB;
        const int mis = (int)((4 - (((uintptr_t)out + g0) & 3)) & 3);
        const int lead = mis < nb ? mis : nb;
        const int nw = (nb - lead) >> 2;
        const uint8_t* src = sm.out[r];
        if (s < nw) {
            const int o = lead + 4 * s;
            const uint32_t v = (uint32_t)src[o] | ((uint32_t)src[o + 1] << 8) | ((uint32_t)src[o + 2] << 16) | ((uint32_t)src[o + 3] << 24);
            *reinterpret_cast<uint32_t*>(out + g0 + o) = v;
        } else if (s == SLOTS - 2) {
            for (int q = 0; q < lead; ++q) out[g0 + q] = src[q];
        } else if (s == SLOTS - 1) {
            for (int q = lead + 4 * nw; q < nb; ++q) out[g0 + q] = src[q];
        }
    }
}

}  // namespace e2eft

using namespace e2eft;

extern "C" int e2eft_depth_to_normals(const e2eft_d2nt_desc* desc, const float* depth, const float* intrinsics, void* out, void* stream) {
    E2EFT_REQUIRE(desc && depth && intrinsics && out, "depth_to_normals: null pointer");
    const e2eft_d2nt_desc d = *desc;
    E2EFT_REQUIRE(d.batch > 0 && d.height >= 2 && d.width >= 2, "depth_to_normals: shape %d x %d x %d (height and width >= 2)", d.batch, d.height, d.width);
    E2EFT_REQUIRE(d.batch <= 65535, "depth_to_normals: batch %d > 65535", d.batch);
    E2EFT_REQUIRE((int64_t)d.height * d.width <= ((int64_t)1 << 31) / 12, "depth_to_normals: %d x %d pixels per image too many", d.height, d.width);
    E2EFT_REQUIRE(d.refine == 0 || d.refine == 1, "depth_to_normals: refine %d (0 = v2, 1 = v3)", d.refine);
    E2EFT_REQUIRE(d.out_format >= E2EFT_D2NT_F32 && d.out_format <= E2EFT_D2NT_U8, "depth_to_normals: out_format %d", d.out_format);
    E2EFT_REQUIRE(((uintptr_t)depth & 3) == 0 && ((uintptr_t)intrinsics & 3) == 0, "depth_to_normals: depth and intrinsics must be 4-byte aligned");
    E2EFT_REQUIRE(((uintptr_t)out & (d.out_format == E2EFT_D2NT_F32 ? 3 : (d.out_format == E2EFT_D2NT_U16 ? 1 : 0))) == 0,
                  "depth_to_normals: output not aligned to its element");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((d.width + DN_TW - 1) / DN_TW, (d.height + DN_TH - 1) / DN_TH, d.batch);
    uint8_t* o = (uint8_t*)out;
    if (d.out_format == E2EFT_D2NT_F32)
        hipLaunchKernelGGL(d2nt_kernel<0>, grid, dim3(DN_THREADS), 0, s, d.height, d.width, d.refine, d.depth_scale, depth, intrinsics, o);
    else if (d.out_format == E2EFT_D2NT_U16)
        hipLaunchKernelGGL(d2nt_kernel<1>, grid, dim3(DN_THREADS), 0, s, d.height, d.width, d.refine, d.depth_scale, depth, intrinsics, o);
    else
        hipLaunchKernelGGL(d2nt_kernel<2>, grid, dim3(DN_THREADS), 0, s, d.height, d.width, d.refine, d.depth_scale, depth, intrinsics, o);
    return check_launch("depth_to_normals");
}
