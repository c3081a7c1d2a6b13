// noise.hip — device-side latent noise (training/train.py:483-518, training/util/noise.py:8-18, marigold_pipeline.py:76-86) and the x0 of a non-zero x_t.
//
// Generator (the CONTRACT — tests/noise_ref.py restates it on the host from this text, not from the code below):
//   Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85).  One round maps the counter
//   (c0,c1,c2,c3) under the key (k0,k1) to  ( hi(M1*c2) ^ c1 ^ k0,  lo(M1*c2),  hi(M0*c0) ^ c3 ^ k1,  lo(M0*c0) );  ten rounds, the key advanced by
//   (W0,W1) BEFORE each round but the first.
//   Element e of a tensor is its LOGICAL NCHW linear index ((b*C + ch)*H + y)*W + x — independent of memory layout and pixel stride.
//     q = e >> 2            counter = (q & 0xffffffff, q >> 32, slot, draw)            key = (seed & 0xffffffff, seed >> 32)            word = out[e & 3]
//     x = word >> 8,  u = (x + 0.5) * 2^-24      strictly inside (0, 1)
//   Box-Muller pairs the words (0,1) and (2,3) of ONE counter:  r = sqrt(-2 ln u_even),  theta = 2 pi u_odd;  the even word's element gets r cos(theta), the
//   odd word's r sin(theta).  fp32 arithmetic with the accurate logf / log1pf / sqrtf / sinf / cosf; rounded ONCE to the destination dtype at the store.
//   x + 0.5 has 25 significant bits once x >= 2^23, so the upper half of the u's are NOT fp32 numbers (x = 2^24 - 1 would round to u = 1, r = 0 instead of
//   2.4e-4).  Their complement 1 - u = ((2^24 - 1 - x) + 0.5) * 2^-24 is exact there, so for x >= 2^23 the kernel takes ln u = log1p(-(1 - u)) and
//   cos(2 pi u) = cos(2 pi (1 - u)), sin(2 pi u) = -sin(2 pi (1 - u)): every u enters the arithmetic exactly.
//   slot 0 is the base grid of a call, slot 1 + i the grid of pyramid level i; draw is the caller's per-call counter, passed by value — or, by e2eft_randn_fill_at,
//   read from device memory (the low 32 bits of an int64), which is what a captured graph needs to draw fresh noise on every replay.  The pyramid `_at` entry
//   points read `draw` AND the level table from int64 device words (e2eft_pyramid_table_set fills them); e2eft_randint_fill[_at] turns the raw word of an element
//   into an integer of [0, high):  t = ((uint64_t)word * (uint64_t)high) >> 32.
//
// Counter-based: any element of any grid is a pure function of (seed, draw, slot, e).  The pyramid kernel therefore evaluates the (at most four) bilinear
// corners of every level on the fly — no level grid is ever stored — and the result does not depend on the launch geometry.
#include "common.h"

namespace e2eft {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

__device__ __forceinline__ float half_unit(uint32_t x) { return ((float)x + 0.5f) * 5.9604644775390625e-08f; }      // (x + 0.5) * 2^-24, exact for x < 2^23

// Box-Muller on one word pair -> (r cos, r sin); u or 1 - u, whichever is exact in fp32 (header comment)
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float& zc, float& zs) {
    const uint32_t xa = wa >> 8, xb = wb >> 8;
    const float lnu = xa < (1u << 23) ? logf(half_unit(xa)) : log1pf(-half_unit(0xFFFFFFu - xa));
    const float r = sqrtf(-2.0f * lnu);
    const bool fold = xb >= (1u << 23);
    const float th = 6.283185307179586f * half_unit(fold ? 0xFFFFFFu - xb : xb);
    zc = r * cosf(th);
    zs = r * sinf(th);
    if (fold) zs = -zs;
}

// the four normals of quad q (elements 4q .. 4q+3)
__device__ __forceinline__ void normal_quad(uint64_t seed, uint32_t draw, uint32_t slot, uint64_t q, float z[4]) {
    uint32_t w[4];
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), slot, draw, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    box_muller(w[0], w[1], z[0], z[1]);
    box_muller(w[2], w[3], z[2], z[3]);
}

// the normal of ONE element (the other pair of its counter is not evaluated)
__device__ __forceinline__ float normal_at(uint64_t seed, uint32_t draw, uint32_t slot, uint64_t e) {
    uint32_t w[4];
    philox4x32_10((uint32_t)(e >> 2), (uint32_t)(e >> 34), slot, draw, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const bool hi = (e & 2) != 0;
    float zc, zs;
    box_muller(hi ? w[2] : w[0], hi ? w[3] : w[1], zc, zs);
    return (e & 1) ? zs : zc;
}

// c T-elements at p in one store (16 bytes of fp32, 8 bytes of a 16-bit type) — C == 4 only
template <typename T> __device__ __forceinline__ void store4(T* p, const float v[4]) {
    if constexpr (sizeof(T) == 4) {
        Vec16<T> o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o.e[k] = from_f<T>(v[k]);
        st16(p, o);
    } else {
        union {
            u32x2 raw;
            T e[4];
        } o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o.e[k] = from_f<T>(v[k]);
        *reinterpret_cast<u32x2*>(p) = o.raw;
    }
}

// ---- e2eft_randn_fill ----------------------------------------------------------------------------------------------------------------------------------
// C == 4, hw % 4 == 0, destination aligned: one thread owns four consecutive pixels of one image — four counters (one per channel, each yields that channel's
// four pixels), four whole-pixel stores.
template <typename T>
__global__ __launch_bounds__(256) void randn_fill4_kernel(long groups, int hw, int ldy, uint64_t seed, uint32_t draw, const int64_t* __restrict__ draw_at, uint32_t slot,
                                                          T* __restrict__ y) {
    if (draw_at) draw = (uint32_t)*draw_at;      // e2eft_randn_fill_at: the low 32 bits of a device int64 (uniform: one scalar load)
    const int gpi = hw >> 2;      // pixel groups per image
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < groups; it += (long)gridDim.x * 256) {
        const long b = it / gpi;
        const int g = (int)(it - b * gpi);
        float z[4][4];           // [channel][pixel of the group]
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) normal_quad(seed, draw, slot, (uint64_t)((b * 4 + ch) * gpi + g), z[ch]);
        T* dst = y + (b * hw + 4L * g) * ldy;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float v[4] = {z[0][p], z[1][p], z[2][p], z[3][p]};
            store4(dst + (long)p * ldy, v);
        }
    }
}

// any shape: one thread per quad of the logical NCHW index, element-wise stores
template <typename T>
__global__ __launch_bounds__(256) void randn_fill_kernel(long total, int c, int hw, int ldy, uint64_t seed, uint32_t draw, const int64_t* __restrict__ draw_at, uint32_t slot,
                                                         T* __restrict__ y) {
    if (draw_at) draw = (uint32_t)*draw_at;
    const long quads = (total + 3) >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
        float z[4];
        normal_quad(seed, draw, slot, (uint64_t)q, z);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long e = 4 * q + j;
            if (e < total) {
                const long plane = e / hw;                  // b * c + ch
                const long b = plane / c;
                y[(b * hw + (e - plane * hw)) * ldy + (plane - b * c)] = from_f<T>(z[j]);
            }
        }
    }
}

// ---- e2eft_pyramid_noise -------------------------------------------------------------------------------------------------------------------------------
struct PyrLevels {
    int n;
    int rows[E2EFT_PYRAMID_MAX_LEVELS], cols[E2EFT_PYRAMID_MAX_LEVELS];
    float weight[E2EFT_PYRAMID_MAX_LEVELS];      // discount^i
};

constexpr int PYR_MAX_BLOCKS = 1024;             // partial (sum, sum of squares) pairs of the first pass

// nn.Upsample(mode="bilinear"), align_corners=False: src = (in / out) * (dst + 0.5) - 0.5 clamped below at 0, i1 = min(i0 + 1, in - 1)
__device__ __forceinline__ void bilinear_tap(int dst, int in, int out, int& i0, int& i1, float& l1) {
    float src = ((float)in / (float)out) * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = min((int)src, in - 1);
    i1 = min(i0 + 1, in - 1);
    l1 = src - (float)i0;
}

__device__ __forceinline__ double block_sum_f64(double v, double* sh) {      // fixed-order tree over the 256 threads of a block; every thread gets the sum
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// pass 1: total = base + sum_i discount^i * bilinear_up(level_i) in fp32, stored pixel-major ([pixel][channel], dense) in the workspace; per-block partial sums.
// WEIGHTED (e2eft_pyramid_noise_weighted; GeoWizard/geowizard/training/train_depth_normal.py:286-296): level i of sample b enters with the weight
//   tw_b = (float)timesteps[b] / timestep_div          one fp32 division, timesteps[b] read from the device
//   acc  = fmaf(w_i * tw_b, up_i, acc)                 w_i = (float)discount^i; ONE fp32 product, then the fused multiply-add of the unweighted form
// — the CONTRACT of the weight (include/e2eft.h repeats it; tests/geowizard_pyramid_ref.py restates it from that text).  tw_b == 1 gives the unweighted bits,
// tw_b == 0 leaves the base grid.  The unweighted instantiation never touches `timesteps` and keeps its arithmetic.
// TABLE (the `_at` entry points): draw, the level count and the level sizes come from `table` = {draw, n_levels, rows_0, cols_0, .., rows_9, cols_9} (int64 device
// words, uniform loads) instead of `draw` / `lv.n` / `lv.rows` / `lv.cols`; the weights stay lv.weight (all ten are formed on the host: they do not depend on the
// table).  The host cannot see those words, so they are clamped here — n into [0, MAX_LEVELS], level rows into [1, rows], level cols into [1, cols] — and a stale
// table can overflow neither the level arrays nor the int index arithmetic (lr * lc <= rows * cols).  One body: the same values give the by-value bits.
__device__ __forceinline__ int clamp_word(long v, int lo, int hi) { return v < (long)lo ? lo : (v > (long)hi ? hi : (int)v); }

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void pyramid_total_kernel(long total, int c, int rows, int cols, PyrLevels lv, uint64_t seed, uint32_t draw,
                                                            const int64_t* __restrict__ table, const int64_t* __restrict__ timesteps, float timestep_div,
                                                            float* __restrict__ tot, double* __restrict__ partial) {
    __shared__ double sh[256];
    const int hw = rows * cols;
    int n_levels = lv.n;
    if (table) {
        draw = (uint32_t)table[0];
        n_levels = clamp_word(table[1], 0, E2EFT_PYRAMID_MAX_LEVELS);
    }
    float s1 = 0.f, s2 = 0.f;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const long gp = it / c;                  // b * hw + pix
        const int ch = (int)(it - gp * c);
        const long b = gp / hw;
        const int pix = (int)(gp - b * hw);
        const int yy = pix / cols, xx = pix - yy * cols;
        const long plane = b * c + ch;
        float tw = 1.f;
        if constexpr (WEIGHTED) tw = (float)timesteps[b] / timestep_div;
        float acc = normal_at(seed, draw, 0u, (uint64_t)(plane * hw + pix));
        for (int i = 0; i < n_levels; ++i) {
            const int lr = table ? clamp_word(table[2 + 2 * i], 1, rows) : lv.rows[i], lc = table ? clamp_word(table[3 + 2 * i], 1, cols) : lv.cols[i];
            int y0, y1, x0, x1;
            float ly, lx;
            bilinear_tap(yy, lr, rows, y0, y1, ly);
            bilinear_tap(xx, lc, cols, x0, x1, lx);
            const uint64_t base = (uint64_t)plane * (uint64_t)(lr * lc);
            const float wy[2] = {1.f - ly, ly}, wx[2] = {1.f - lx, lx};
            const int ys[2] = {y0, y1}, xs[2] = {x0, x1};
            float up = 0.f;
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const float w = wy[a] * wx[d];
                    if (w != 0.f) up = fmaf(w, normal_at(seed, draw, 1u + (uint32_t)i, base + (uint64_t)(ys[a] * lc + xs[d])), up);      // (a level of the output's own size: one corner)
                }
            if constexpr (WEIGHTED) acc = fmaf(lv.weight[i] * tw, up, acc);
            else acc = fmaf(lv.weight[i], up, acc);
        }
        tot[it] = acc;
        s1 += acc;
        s2 = fmaf(acc, acc, s2);
    }
    const double b1 = block_sum_f64((double)s1, sh), b2 = block_sum_f64((double)s2, sh);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = b1;
        partial[2 * blockIdx.x + 1] = b2;
    }
}

// pass 2: every block combines the partials in the same fixed order (fp64), then y = total / std (unbiased, whole tensor) for its share
template <typename T, bool VEC4>
__global__ __launch_bounds__(256) void pyramid_scale_kernel(long total, int c, int ldy, int nparts, const float* __restrict__ tot, const double* __restrict__ partial,
                                                            T* __restrict__ y) {
    __shared__ double sh[256];
    double p1 = 0.0, p2 = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 256) {
        p1 += partial[2 * k];
        p2 += partial[2 * k + 1];
    }
    const double S1 = block_sum_f64(p1, sh), S2 = block_sum_f64(p2, sh);
    const double var = (S2 - S1 * S1 / (double)total) / (double)(total - 1);
    const float sd = (float)sqrt(var);
    if constexpr (VEC4) {
        const long pixels = total >> 2;
        for (long gp = (long)blockIdx.x * 256 + threadIdx.x; gp < pixels; gp += (long)gridDim.x * 256) {
            const floatx4 t = *reinterpret_cast<const floatx4*>(tot + 4 * gp);
            const float v[4] = {t[0] / sd, t[1] / sd, t[2] / sd, t[3] / sd};
            store4(y + gp * ldy, v);
        }
    } else {
        for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
            const long gp = it / c;
            y[gp * ldy + (it - gp * c)] = from_f<T>(tot[it] / sd);
        }
    }
}

// ---- e2eft_pyramid_table_set ---------------------------------------------------------------------------------------------------------------------------
constexpr int PYR_TABLE_WORDS = 2 + 2 * E2EFT_PYRAMID_MAX_LEVELS;
struct PyrTableWords {
    int64_t w[PYR_TABLE_WORDS];
};

// one thread: the values travel as kernel arguments (no host-to-device copy, no staging buffer), plain stores
__global__ void pyramid_table_set_kernel(PyrTableWords v, int64_t* __restrict__ table) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < PYR_TABLE_WORDS; ++k) table[k] = v.w[k];
    }
}

// ---- e2eft_randint_fill --------------------------------------------------------------------------------------------------------------------------------
// element e < n takes word e & 3 of quad e >> 2 (the generator's raw uint32, tests/noise_ref.py::words): t = (word * high) >> 32 in [0, high), written to
// out[r * n + e] for r < repeat (the trainer's `randint(0, T, (b,)).repeat(2)`)
__global__ __launch_bounds__(256) void randint_fill_kernel(long n, int repeat, uint64_t high, uint64_t seed, uint32_t draw, const int64_t* __restrict__ draw_at,
                                                           uint32_t slot, int64_t* __restrict__ out) {
    if (draw_at) draw = (uint32_t)*draw_at;
    const long quads = (n + 3) >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long)gridDim.x * 256) {
        uint32_t w[4];
        philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), slot, draw, (uint32_t)seed, (uint32_t)(seed >> 32), w);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long e = 4 * q + j;
            if (e < n) {
                const int64_t t = (int64_t)(((uint64_t)w[j] * high) >> 32);
                for (int r = 0; r < repeat; ++r) out[(long)r * n + e] = t;
            }
        }
    }
}

// ---- e2eft_latent_x0 -----------------------------------------------------------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void latent_x0_kernel(long pixels, int c, int ldxt, int ldv, int ldo, float cx, float cv, const T* __restrict__ xt,
                                                        const T* __restrict__ v, T* __restrict__ o) {
    constexpr int EPC = VEC ? 16 / (int)sizeof(T) : 1;
    const int cch = c / EPC;
    const long total = pixels * cch;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const long pix = it / cch;
        const int ch = (int)(it - pix * cch) * EPC;
        if constexpr (VEC) {
            const Vec16<T> a = ld16(xt + pix * ldxt + ch), b = ld16(v + pix * ldv + ch);
            Vec16<T> r;
#pragma unroll
            for (int e = 0; e < EPC; ++e) r.e[e] = from_f<T>(fmaf(cx, to_f(a.e[e]), cv * to_f(b.e[e])));
            st16(o + pix * ldo + ch, r);
        } else {
            o[pix * ldo + ch] = from_f<T>(fmaf(cx, to_f(xt[pix * ldxt + ch]), cv * to_f(v[pix * ldv + ch])));
        }
    }
}

static unsigned blocks_for(long items, long cap) {
    long nb = (items + 255) / 256;
    return (unsigned)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

static size_t pyr_tot_bytes(long total) { return ((size_t)total * sizeof(float) + 15) & ~(size_t)15; }

}  // namespace e2eft

using namespace e2eft;

// draw_at == nullptr: `draw` by value (e2eft_randn_fill); otherwise the kernels read it from the device (e2eft_randn_fill_at) — one body, so both give the same bits
static int randn_fill_launch(const char* what, int32_t dtype, int32_t batch, int32_t c, int32_t hw, int32_t ldy, uint64_t seed, uint32_t draw, const int64_t* draw_at,
                             uint32_t slot, void* y, void* stream) {
    const long total = (long)batch * c * hw;
    hipStream_t s = (hipStream_t)stream;
    const size_t pixel_bytes = 4 * dtype_size(dtype);
    const bool vec = c == 4 && hw % 4 == 0 && ldy % 4 == 0 && ((uintptr_t)y % pixel_bytes) == 0;
    E2EFT_DISPATCH_DTYPE(dtype, T, {
        if (vec) {
            const long groups = (long)batch * (hw / 4);
            hipLaunchKernelGGL((randn_fill4_kernel<T>), dim3(blocks_for(groups, 16384)), dim3(256), 0, s, groups, hw, ldy, seed, draw, draw_at, slot, (T*)y);
        } else {
            hipLaunchKernelGGL((randn_fill_kernel<T>), dim3(blocks_for((total + 3) / 4, 16384)), dim3(256), 0, s, total, c, hw, ldy, seed, draw, draw_at, slot, (T*)y);
        }
    });
    return check_launch(what);
}

extern "C" int e2eft_randn_fill(int32_t dtype, int32_t batch, int32_t c, int32_t hw, int32_t ldy, uint64_t seed, uint32_t draw, uint32_t slot, void* y,
                                void* stream) {
    E2EFT_REQUIRE(y, "randn_fill: null pointer");
    E2EFT_REQUIRE(dtype >= 0 && dtype <= 2, "randn_fill: bad dtype");
    E2EFT_REQUIRE(batch > 0 && c > 0 && hw > 0 && ldy >= c, "randn_fill: shape");
    E2EFT_REQUIRE((long)batch * c * hw < (1L << 31), "randn_fill: more than 2^31 - 1 elements");
    return randn_fill_launch("randn_fill", dtype, batch, c, hw, ldy, seed, draw, nullptr, slot, y, stream);
}

extern "C" int e2eft_randn_fill_at(int32_t dtype, int32_t batch, int32_t c, int32_t hw, int32_t ldy, uint64_t seed, const int64_t* draw, uint32_t slot, void* y,
                                   void* stream) {
    E2EFT_REQUIRE(y && draw, "randn_fill_at: null pointer");
    E2EFT_REQUIRE(dtype >= 0 && dtype <= 2, "randn_fill_at: bad dtype");
    E2EFT_REQUIRE(batch > 0 && c > 0 && hw > 0 && ldy >= c, "randn_fill_at: shape");
    E2EFT_REQUIRE((long)batch * c * hw < (1L << 31), "randn_fill_at: more than 2^31 - 1 elements");
    return randn_fill_launch("randn_fill_at", dtype, batch, c, hw, ldy, seed, 0u, draw, slot, y, stream);
}

extern "C" size_t e2eft_pyramid_noise_workspace_bytes(int32_t batch, int32_t c, int32_t hw) {
    if (batch <= 0 || c <= 0 || hw <= 0 || (long)batch * c * hw >= (1L << 31)) return 0;
    return pyr_tot_bytes((long)batch * c * hw) + (size_t)PYR_MAX_BLOCKS * 2 * sizeof(double);
}

// timesteps == nullptr: e2eft_pyramid_noise; otherwise e2eft_pyramid_noise_weighted — one validation, one launcher, one pass-1 body (a template on "weighted").
// table != nullptr: the `_at` forms — draw, n_levels and level_sizes are not looked at (pass 0, 0, nullptr), the kernel reads and clamps them from the device words
static int pyramid_noise_launch(int32_t dtype, int32_t batch, int32_t c, int32_t rows, int32_t cols, int32_t ldy, uint64_t seed, uint32_t draw, float discount,
                                int32_t n_levels, const int32_t* level_sizes, const int64_t* table, const int64_t* timesteps, float timestep_div, void* y,
                                void* workspace, size_t workspace_bytes, void* stream) {
    E2EFT_REQUIRE(y && workspace && (level_sizes || n_levels == 0), "pyramid_noise: null pointer");
    E2EFT_REQUIRE(dtype >= 0 && dtype <= 2, "pyramid_noise: bad dtype");
    E2EFT_REQUIRE(batch > 0 && c > 0 && rows > 0 && cols > 0 && (long)rows * cols < (1L << 31) && ldy >= c, "pyramid_noise: shape");
    E2EFT_REQUIRE(n_levels >= 0 && n_levels <= E2EFT_PYRAMID_MAX_LEVELS, "pyramid_noise: at most %d levels", E2EFT_PYRAMID_MAX_LEVELS);
    const long total = (long)batch * c * rows * cols;
    E2EFT_REQUIRE(total >= 2 && total < (1L << 31), "pyramid_noise: the unbiased standard deviation needs 2 .. 2^31 - 1 elements");
    if (workspace_bytes < e2eft_pyramid_noise_workspace_bytes(batch, c, rows * cols)) return fail(E2EFT_ERR_WORKSPACE, "pyramid_noise: workspace too small");
    PyrLevels lv;
    lv.n = n_levels;
    double w = 1.0;
    for (int i = 0; i < E2EFT_PYRAMID_MAX_LEVELS; ++i) {
        lv.rows[i] = lv.cols[i] = 1;
        lv.weight[i] = 0.f;
        if (i < n_levels) {
            lv.rows[i] = level_sizes[2 * i];
            lv.cols[i] = level_sizes[2 * i + 1];
            E2EFT_REQUIRE(lv.rows[i] >= 1 && lv.cols[i] >= 1 && (long)lv.rows[i] * lv.cols[i] * batch * c < (1L << 31), "pyramid_noise: level %d size", i);
        }
        if (i < n_levels || table) {      // (a device table may hold any number of levels: all ten weights, the same running product)
            lv.weight[i] = (float)w;
            w *= (double)discount;
        }
    }
    E2EFT_REQUIRE(al16(workspace), "pyramid_noise: workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* tot = (float*)workspace;
    double* partial = (double*)((char*)workspace + pyr_tot_bytes(total));
    const unsigned g1 = blocks_for(total, PYR_MAX_BLOCKS);
    if (timesteps) hipLaunchKernelGGL((pyramid_total_kernel<true>), dim3(g1), dim3(256), 0, s, total, c, rows, cols, lv, seed, draw, table, timesteps, timestep_div, tot, partial);
    else hipLaunchKernelGGL((pyramid_total_kernel<false>), dim3(g1), dim3(256), 0, s, total, c, rows, cols, lv, seed, draw, table, (const int64_t*)nullptr, 1.f, tot, partial);
    const size_t pixel_bytes = 4 * dtype_size(dtype);
    const bool vec = c == 4 && ldy % 4 == 0 && ((uintptr_t)y % pixel_bytes) == 0;
    E2EFT_DISPATCH_DTYPE(dtype, T, {
        if (vec) hipLaunchKernelGGL((pyramid_scale_kernel<T, true>), dim3(blocks_for(total / 4, 16384)), dim3(256), 0, s, total, c, ldy, (int)g1, tot, partial, (T*)y);
        else hipLaunchKernelGGL((pyramid_scale_kernel<T, false>), dim3(blocks_for(total, 16384)), dim3(256), 0, s, total, c, ldy, (int)g1, tot, partial, (T*)y);
    });
    return check_launch("pyramid_noise");
}

extern "C" int e2eft_pyramid_noise(int32_t dtype, int32_t batch, int32_t c, int32_t rows, int32_t cols, int32_t ldy, uint64_t seed, uint32_t draw, float discount,
                                   int32_t n_levels, const int32_t* level_sizes, void* y, void* workspace, size_t workspace_bytes, void* stream) {
    return pyramid_noise_launch(dtype, batch, c, rows, cols, ldy, seed, draw, discount, n_levels, level_sizes, nullptr, nullptr, 1.f, y, workspace, workspace_bytes,
                                stream);
}

extern "C" int e2eft_pyramid_noise_weighted(int32_t dtype, int32_t batch, int32_t c, int32_t rows, int32_t cols, int32_t ldy, uint64_t seed, uint32_t draw,
                                            float discount, int32_t n_levels, const int32_t* level_sizes, const int64_t* timesteps, float timestep_div, void* y,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    E2EFT_REQUIRE(timesteps, "pyramid_noise_weighted: null timesteps");
    E2EFT_REQUIRE(timestep_div > 0.f, "pyramid_noise_weighted: timestep_div must be positive");
    return pyramid_noise_launch(dtype, batch, c, rows, cols, ldy, seed, draw, discount, n_levels, level_sizes, nullptr, timesteps, timestep_div, y, workspace,
                                workspace_bytes, stream);
}

extern "C" int e2eft_pyramid_noise_at(int32_t dtype, int32_t batch, int32_t c, int32_t rows, int32_t cols, int32_t ldy, uint64_t seed, const int64_t* table,
                                      float discount, void* y, void* workspace, size_t workspace_bytes, void* stream) {
    E2EFT_REQUIRE(table && ((uintptr_t)table & 7) == 0, "pyramid_noise_at: null or misaligned table");
    return pyramid_noise_launch(dtype, batch, c, rows, cols, ldy, seed, 0u, discount, 0, nullptr, table, nullptr, 1.f, y, workspace, workspace_bytes, stream);
}

extern "C" int e2eft_pyramid_noise_weighted_at(int32_t dtype, int32_t batch, int32_t c, int32_t rows, int32_t cols, int32_t ldy, uint64_t seed, const int64_t* table,
                                               float discount, const int64_t* timesteps, float timestep_div, void* y, void* workspace, size_t workspace_bytes,
                                               void* stream) {
    E2EFT_REQUIRE(table && ((uintptr_t)table & 7) == 0, "pyramid_noise_weighted_at: null or misaligned table");
    E2EFT_REQUIRE(timesteps, "pyramid_noise_weighted_at: null timesteps");
    E2EFT_REQUIRE(timestep_div > 0.f, "pyramid_noise_weighted_at: timestep_div must be positive");
    return pyramid_noise_launch(dtype, batch, c, rows, cols, ldy, seed, 0u, discount, 0, nullptr, table, timesteps, timestep_div, y, workspace, workspace_bytes, stream);
}

extern "C" int e2eft_pyramid_table_set(int64_t* table, uint32_t draw, int32_t n_levels, const int32_t* level_sizes, int32_t rows, int32_t cols, void* stream) {
    E2EFT_REQUIRE(table && ((uintptr_t)table & 7) == 0 && (level_sizes || n_levels == 0), "pyramid_table_set: null or misaligned pointer");
    E2EFT_REQUIRE(rows > 0 && cols > 0 && (long)rows * cols < (1L << 31), "pyramid_table_set: shape");
    E2EFT_REQUIRE(n_levels >= 0 && n_levels <= E2EFT_PYRAMID_MAX_LEVELS, "pyramid_table_set: at most %d levels", E2EFT_PYRAMID_MAX_LEVELS);
    PyrTableWords v;
    v.w[0] = (int64_t)draw;
    v.w[1] = n_levels;
    for (int i = 0; i < E2EFT_PYRAMID_MAX_LEVELS; ++i) {
        int lr = 1, lc = 1;
        if (i < n_levels) {
            lr = level_sizes[2 * i];
            lc = level_sizes[2 * i + 1];
            E2EFT_REQUIRE(lr >= 1 && lc >= 1, "pyramid_table_set: level %d size", i);
            E2EFT_REQUIRE(lr <= rows && lc <= cols, "pyramid_table_set: level %d (%d x %d) exceeds the output (%d x %d)", i, lr, lc, rows, cols);
        }
        v.w[2 + 2 * i] = lr;
        v.w[3 + 2 * i] = lc;
    }
    hipLaunchKernelGGL(pyramid_table_set_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, v, table);
    return check_launch("pyramid_table_set");
}

// draw_at == nullptr: e2eft_randint_fill; otherwise e2eft_randint_fill_at — one kernel body
static int randint_fill_launch(const char* what, int64_t n, int32_t repeat, int64_t high, uint64_t seed, uint32_t draw, const int64_t* draw_at, uint32_t slot,
                               int64_t* out, void* stream) {
    E2EFT_REQUIRE(out && ((uintptr_t)out & 7) == 0, "%s: null or misaligned pointer", what);
    E2EFT_REQUIRE(n >= 1 && n < (1L << 31) && repeat >= 1, "%s: n must be 1 .. 2^31 - 1 and repeat >= 1", what);
    E2EFT_REQUIRE(high >= 1 && high <= 0x7FFFFFFFL, "%s: high must be 1 .. 2^31 - 1", what);
    hipLaunchKernelGGL(randint_fill_kernel, dim3(blocks_for((n + 3) / 4, 16384)), dim3(256), 0, (hipStream_t)stream, (long)n, (int)repeat, (uint64_t)high, seed, draw,
                       draw_at, slot, out);
    return check_launch(what);
}

extern "C" int e2eft_randint_fill(int64_t n, int32_t repeat, int64_t high, uint64_t seed, uint32_t draw, uint32_t slot, int64_t* out, void* stream) {
    return randint_fill_launch("randint_fill", n, repeat, high, seed, draw, nullptr, slot, out, stream);
}

extern "C" int e2eft_randint_fill_at(int64_t n, int32_t repeat, int64_t high, uint64_t seed, const int64_t* draw, uint32_t slot, int64_t* out, void* stream) {
    E2EFT_REQUIRE(draw && ((uintptr_t)draw & 7) == 0, "randint_fill_at: null or misaligned draw");
    return randint_fill_launch("randint_fill_at", n, repeat, high, seed, 0u, draw, slot, out, stream);
}

extern "C" int e2eft_latent_x0(int32_t dtype, int64_t pixels, int32_t c, int32_t ldxt, int32_t ldv, int32_t ldo, float c_x, float c_v, const void* xt,
                               const void* v, void* x0, void* stream) {
    E2EFT_REQUIRE(xt && v && x0, "latent_x0: null pointer");
    E2EFT_REQUIRE(dtype >= 0 && dtype <= 2, "latent_x0: bad dtype");
    E2EFT_REQUIRE(pixels > 0 && c > 0 && ldxt >= c && ldv >= c && ldo >= c, "latent_x0: shape");
    const int epc = 16 / (int)dtype_size(dtype);
    const bool vec = c % epc == 0 && ldxt % epc == 0 && ldv % epc == 0 && ldo % epc == 0 && (((uintptr_t)xt | (uintptr_t)v | (uintptr_t)x0) & 15) == 0;
    hipStream_t s = (hipStream_t)stream;
    E2EFT_DISPATCH_DTYPE(dtype, T, {
        if (vec) hipLaunchKernelGGL((latent_x0_kernel<T, true>), dim3(blocks_for(pixels * (c / epc), 16384)), dim3(256), 0, s, (long)pixels, c, ldxt, ldv, ldo, c_x, c_v, (const T*)xt, (const T*)v, (T*)x0);
        else hipLaunchKernelGGL((latent_x0_kernel<T, false>), dim3(blocks_for(pixels * c, 16384)), dim3(256), 0, s, (long)pixels, c, ldxt, ldv, ldo, c_x, c_v, (const T*)xt, (const T*)v, (T*)x0);
    });
    return check_launch("latent_x0");
}
