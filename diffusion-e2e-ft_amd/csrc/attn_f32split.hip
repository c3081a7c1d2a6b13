// attn_f32split.hip — the second fp32 route of the d = 64 fused attention (forward with base-2 log-sum-exp, backward dK / dV and dQ), gfx950: every fp32
// product is made of three v_mfma_f32_32x32x16_f16 on two-term f16 splits of its operands.  Off by default (E2EFT_OPT_F32_SPLIT_ATTN); contract, launch
// geometry, owner-computes backward and the shared D = rowsum(dO o O) pass are attn32.hip's (attn32.h), fragments and operand order are attn.hip / attn_bwd.hip's.
//
// The split.  x -> (x0, x1) = (f16(x s), f16(x s - x0)) with s an exact power of two that brings the largest magnitude the scale covers into [2^14, 2^15);
// a b ~ (a0 b0 + a0 b1 + a1 b0) / (sa sb), the three products accumulated in fp32 by the matrix pipe, the scales removed exactly (they are powers of two);
// a1 b1 (2^-22 relative) is the only thing dropped.  x0 keeps 11 bits and x1 the next 11 as long as x1's last bit stays above f16's smallest subnormal 2^-24:
// a value within 2^-17 of its scale's maximum keeps 22 bits, a smaller one an absolute error of 2^-39 of that maximum.
// The split happens WHILE STAGING: the loader that brings a 64-row fp32 tile into LDS writes it as two row-major f16 planes (2 x 144-byte rows: the bytes of one
// padded fp32 tile), and operands that live in registers for the whole kernel (the lane's own q, k, v or dO row) are split once.  Which scale:
//  * an operand that lives in a lane's registers: one scale per ROW (the lane's 64 values) — it belongs to the result's column and factors out exactly;
//  * a staged tile: one scale per TILE (64 rows x 64 columns; four per-wave maxima through LDS, one extra barrier per tile).  A tile is read both along its rows
//    (contraction over d: S, dP) and, through ds_read_b64_tr_b16, along its columns (contraction over the tile's rows: O, dV, dK, dQ); only a scale that is
//    constant over the whole tile factors out of both;
//  * P lies in [0, 1]: p 2^14, no search;
//  * dS has no bound known in advance: one scale per lane (= per key in dK, per query in dQ) and 32-row block, from the block's own maximum.
//  An accumulator that runs over tiles whose scales differ (O, dV, dK, dQ) FOLLOWS them the way O follows the running maximum: it is kept in units of 2^-(282 - W)
//  with W = the largest (biased exponent of the tile scale + biased exponent of the register operand's scale) met so far; when W grows the accumulator is multiplied by
//  the (exact) power of two, and a block whose own W is smaller has the difference folded into its P / dS before they are split.
// Online softmax, exp2, lse and everything stored stay fp32.  No atomics, no host synchronisation, no allocation: graph-capturable like attn32.
#include "gfx950.h"
#include "attn32.h"

namespace e2eft {

namespace fsa {
constexpr int ROW = 144;                  // bytes per LDS row of a plane: 64 f16 + 16 (conflict-free ds_read_b128 of 16 rows; transpose reads see two-way conflicts)
constexpr int PLANE = 64 * ROW;           // one f16 plane of a 64-row tile
constexpr int TILE = 2 * PLANE;           // x0 plane | x1 plane: 18,432 B
constexpr float LN2 = 0.6931471805599453f;
constexpr int EMIN = 15;                  // smallest biased exponent a scale is taken from: 2^(141 - e) and 2^(e - 141) are both normal fp32 numbers for 15 <= e <= 255
using Mma = Mma32x32x16<f16>;
}  // namespace fsa

// biased fp32 exponent e of a maximum m >= 0 (m < 2^(e - 126)), clamped from below: zeros, subnormals and tiny values share the scale of 2^-112
__device__ __forceinline__ int fsa_exp_of(const float m) { return max((int)((__float_as_uint(m) >> 23) & 0xffu), fsa::EMIN); }
// 2^(e - 127) from its biased exponent; below the normal range: 0 (a contribution more than 2^127 below its accumulator's unit)
__device__ __forceinline__ float fsa_pow2(const int e) { return __uint_as_float((uint32_t)min(max(e, 0), 254) << 23); }
// the split scale of a maximum with biased exponent e is 2^(141 - e) (m s in [2^14, 2^15)) and its inverse 2^(e - 141)
__device__ __forceinline__ float fsa_scale(const int e) { return fsa_pow2(268 - e); }
__device__ __forceinline__ float fsa_inv_scale(const int e) { return fsa_pow2(e - 14); }
// an accumulator in units of 2^-(282 - W) -> the two exact factors that bring it back (W - 282 lies in [-252, 228]: one fp32 power of two cannot hold it)
__device__ __forceinline__ void fsa_unscale(const int W, float& f1, float& f2) {
    const int t = W - 282;
    f1 = fsa_pow2(127 + (t >> 1));
    f2 = fsa_pow2(127 + t - (t >> 1));
}

// eight fp32 values (already in the order of the eight 16-bit slots) -> four dwords of x0 and four of x1
__device__ __forceinline__ void fsa_split8(const floatx4 a, const floatx4 b, const float sc, u32x4& hi, u32x4& lo) {
    const float x[8] = {a[0] * sc, a[1] * sc, a[2] * sc, a[3] * sc, b[0] * sc, b[1] * sc, b[2] * sc, b[3] * sc};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t h = pack2<f16>(x[2 * w], x[2 * w + 1]);
        const half2v hv = __builtin_bit_cast(half2v, h);
        hi[w] = h;
        lo[w] = pack2<f16>(x[2 * w] - (float)hv[0], x[2 * w + 1] - (float)hv[1]);
    }
}
// the 16 registers of an accumulator block (P or dS, times the power of two f) -> the B operands of the block's two 16-row k-steps: dwords 4 s2 .. 4 s2 + 3
__device__ __forceinline__ void fsa_split16(const floatx16& v, const float f, uint32_t (&hi)[8], uint32_t (&lo)[8]) {
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const float x0 = v[2 * w] * f, x1 = v[2 * w + 1] * f;
        const uint32_t h = pack2<f16>(x0, x1);
        const half2v hv = __builtin_bit_cast(half2v, h);
        hi[w] = h;
        lo[w] = pack2<f16>(x0 - (float)hv[0], x1 - (float)hv[1]);
    }
}
// c += a b from the split operands of one k-step: the two cross terms first, the leading term last (the accumulating products O, dV, dK, dQ)
__device__ __forceinline__ floatx16 fsa_mma3(const u32x4& ah, const u32x4& al, const u32x4& bh, const u32x4& bl, floatx16 c) {
    c = fsa::Mma::run(al, bh, c);
    c = fsa::Mma::run(ah, bl, c);
    return fsa::Mma::run(ah, bh, c);
}
__device__ __forceinline__ floatx16 fsa_zero16() {
    floatx16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}
// accumulator row (within its 32-row block) of register r in half hh
__device__ __forceinline__ constexpr int fsa_arow(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// ---- the lane's own row (64 fp32 at `src`, times `mul`; zeros when !ok) as B operand: slots of k-step ds = elements 16 ds + 8 hh .. + 7; per-row scale
__device__ __forceinline__ void fsa_row_operand(const float* src, const bool ok, const float mul, const int hh, u32x4 (&xh)[4], u32x4 (&xl)[4], float& inv) {
    floatx4 a[8];
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const floatx4 z = {0.f, 0.f, 0.f, 0.f};
        floatx4 v = ok ? *reinterpret_cast<const floatx4*>(src + 16 * (j >> 1) + 8 * hh + 4 * (j & 1)) : z;
        v = v * mul;
#pragma unroll
        for (int e = 0; e < 4; ++e) m = fmaxf(m, fabsf(v[e]));
        a[j] = v;
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const int e = fsa_exp_of(m);
    inv = fsa_inv_scale(e);
    const float sc = fsa_scale(e);
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) fsa_split8(a[2 * ds], a[2 * ds + 1], sc, xh[ds], xl[ds]);
}

// ---- the tile loader all three kernels use: thread t moves columns 16 (t & 3) .. + 15 of tile row t >> 2 (attn32.hip's assignment).
// step 1, before the barrier: the wave's maximum of what it loaded goes to pmax[wave]
__device__ __forceinline__ void fsa_publish_max(const floatx4 (&r)[4], float* pmax, const int lane, const int wave) {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) m = fmaxf(m, fabsf(r[i][e]));
    m = wave_max(m);
    if (lane == 0) pmax[wave] = m;
}
// biased exponent of a tile's maximum from the four per-wave maxima
__device__ __forceinline__ int fsa_tile_exp(const float* pmax) {
    const floatx4 m = *reinterpret_cast<const floatx4*>(pmax);
    return fsa_exp_of(fmaxf(fmaxf(m[0], m[1]), fmaxf(m[2], m[3])));
}
// step 2, after the barrier: split with the tile's scale and store the thread's 16 values into both planes
__device__ __forceinline__ void fsa_store_split(char* tile, const floatx4 (&r)[4], const float sc, const int lrow, const int lcol) {
    char* dst = tile + lrow * fsa::ROW + lcol * 2;
    u32x4 h, l;
    fsa_split8(r[0], r[1], sc, h, l);
    *reinterpret_cast<u32x4*>(dst) = h;
    *reinterpret_cast<u32x4*>(dst + fsa::PLANE) = l;
    fsa_split8(r[2], r[3], sc, h, l);
    *reinterpret_cast<u32x4*>(dst + 16) = h;
    *reinterpret_cast<u32x4*>(dst + fsa::PLANE + 16) = l;
}
// A operand read along a tile's rows: row `row`, slots of k-step ds = columns 16 ds + 8 hh .. + 7
__device__ __forceinline__ void fsa_row_frag(const char* tile, const int row, const int hh, const int ds, u32x4& ah, u32x4& al) {
    const char* p = tile + row * fsa::ROW + hh * 16 + ds * 32;
    ah = *reinterpret_cast<const u32x4*>(p);
    al = *reinterpret_cast<const u32x4*>(p + fsa::PLANE);
}
// S / dP block: D[32 x 32] = A[32 tile rows x 64] B^T over d = 64, A = rows row0 .. + 31 of a staged tile, B = the lane's register operand.  The eight cross-term
// MFMAs come first and the four leading-term MFMAs last: the accumulator is rounded at the magnitude of the result four times instead of twelve (the cross terms
// are 2^-11 of it).  These blocks feed exp2 and the cancellation dP - D, where the accumulation error of a chain that alternates the terms showed (2.5e-3
// against 7.7e-4 on dK of tests/test_f32split_attn_gpu.py::test_range_per_channel).  BFIRST: b's x1 term first.  The forward and dQ compute S^T = K Q'^T with K
// as A, dK / dV computes S = Q' K^T with K as B and takes BFIRST: the three kernels then add the same products in the same order (K1 Q0, K0 Q1 per k-step, then
// K0 Q0), and as power-of-two scales commute with every rounding the recomputed score is the forward's bit for bit wherever both operands are inside their
// scales' 2^17 windows — P = 2^(S - lse) sees no difference between the two S (with |S| ~ 2^10 a last-bit difference is 2^-13 of a probability).
template <bool BFIRST = false>
__device__ __forceinline__ floatx16 fsa_rows_dot(const char* tile, const int row, const int hh, const u32x4 (&bh)[4], const u32x4 (&bl)[4]) {
    floatx16 c = fsa_zero16();
    u32x4 ah[4];
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) {
        u32x4 al;
        fsa_row_frag(tile, row, hh, ds, ah[ds], al);
        if (BFIRST) {
            c = fsa::Mma::run(ah[ds], bl[ds], c);
            c = fsa::Mma::run(al, bh[ds], c);
        } else {
            c = fsa::Mma::run(al, bh[ds], c);
            c = fsa::Mma::run(ah[ds], bl[ds], c);
        }
    }
#pragma unroll
    for (int ds = 0; ds < 4; ++ds) c = fsa::Mma::run(ah[ds], bh[ds], c);
    return c;
}
// A operand read along a tile's columns (transposed on the way out of LDS, attn.hip's V recipe): output row = column 32 dt + l31, slots = tile rows
// row0 + 4 hh + 0..3 and row0 + 8 + 4 hh + 0..3 — the register order of the accumulator block that supplies B.  tfrag = the lane's address inside a 16-row step.
__device__ __forceinline__ int fsa_tfrag(const int lane) {
    const int i16 = lane & 15, hh = lane >> 5;
    return ((i16 >> 2) + 4 * hh) * fsa::ROW + (16 * ((lane >> 4) & 1) + 4 * (i16 & 3)) * 2;
}
__device__ __forceinline__ void fsa_col_frag(const char* tile, const int tfrag, const int row0, const int dt, u32x4& ah, u32x4& al) {
    const char* p = tile + tfrag + row0 * fsa::ROW + dt * 64;
    const u32x2 h0 = lds_read_tr16(p), h1 = lds_read_tr16(p + 8 * fsa::ROW);
    const u32x2 l0 = lds_read_tr16(p + fsa::PLANE), l1 = lds_read_tr16(p + fsa::PLANE + 8 * fsa::ROW);
    ah = u32x4{h0[0], h0[1], h1[0], h1[1]};
    al = u32x4{l0[0], l0[1], l1[0], l1[1]};
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// forward: one 256-thread workgroup = 128 queries of one (image, head), a wave 32 queries (lane <-> query); 64-key tiles of K and V, two buffers.
//   S^T[key, q] = K Q'^T        A = K tile rows, B = the lane's Q' = c Q row;   O^T[d, q] += V^T P^T        A = V tile columns, B = P registers
__global__ __launch_bounds__(256, 2) void attn_f32split_fwd_kernel(const Attn32Params p) {
    using namespace fsa;
    constexpr int BUF = 2 * TILE;                                                  // K (x0 | x1), V (x0 | x1)
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF + 64];                // 73,792 B
    float* pmax = reinterpret_cast<float*>(smem + 2 * BUF);                        // [buffer][K | V][wave]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    int b, head, qblk;
    xcd_pair_block_map(p.batch, p.heads, p.nqb, b, head, qblk);
    const int qr = qblk * 128 + wave * 32 + l31;
    const bool qok = qr < p.nq;

    u32x4 qh[4], ql[4];
    float inv_q;
    fsa_row_operand(p.q + ((long)b * p.nq + (qok ? qr : 0)) * p.ldq + head * 64, qok, p.c, hh, qh, ql, inv_q);

    const int lrow = tid >> 2, lcol = 16 * (tid & 3);
    const int kvb0 = b % p.kv_bmod;
    floatx4 kreg[4], vreg[4];
    auto load_tile = [&](const int t, const int buf) {
        const int key = t * 64 + lrow;
        const bool ok = key < p.nk_total;
        const long row = (long)kvb0 * p.nk_seg + (ok ? key : 0);
        const float* kp = p.k + row * p.ldk + head * 64 + lcol;
        const float* vp = p.v + row * p.ldv + head * 64 + lcol;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const floatx4 z = {0.f, 0.f, 0.f, 0.f};
            kreg[i] = ok ? *reinterpret_cast<const floatx4*>(kp + 4 * i) : z;
            vreg[i] = ok ? *reinterpret_cast<const floatx4*>(vp + 4 * i) : z;
        }
        fsa_publish_max(kreg, pmax + buf * 8, lane, wave);
        fsa_publish_max(vreg, pmax + buf * 8 + 4, lane, wave);
    };
    auto store_tile = [&](const int buf) {
        fsa_store_split(smem + buf * BUF, kreg, fsa_scale(fsa_tile_exp(pmax + buf * 8)), lrow, lcol);
        fsa_store_split(smem + buf * BUF + TILE, vreg, fsa_scale(fsa_tile_exp(pmax + buf * 8 + 4)), lrow, lcol);
    };
    const int tfrag = fsa_tfrag(lane);

    const int nt = (p.nk_total + 63) / 64;
    load_tile(0, 0);
    __syncthreads();
    store_tile(0);
    __syncthreads();

    floatx16 o[2] = {fsa_zero16(), fsa_zero16()};
    float m_run = -INFINITY, l_run = 0.f;
    int ev_run = EMIN;                       // O^T is kept in units of 2^-(282 - (ev_run + 127)): V's largest tile scale so far, P's fixed 2^14
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        // the next tile goes global -> registers -> (maximum, barrier) -> split -> LDS in one go, before this tile's products: the staging registers are dead
        // while operands and accumulators work (attn32_bwd_dkdv_kernel's order); the other buffer is free since the barrier that closed iteration t - 1
        if (t + 1 < nt) {
            load_tile(t + 1, buf ^ 1);
            __syncthreads();
            store_tile(buf ^ 1);
        }
        const char* kt = smem + buf * BUF;
        const char* vt = kt + TILE;
        const int ek = fsa_tile_exp(pmax + buf * 8), ev = fsa_tile_exp(pmax + buf * 8 + 4);
        const float fs = fsa_inv_scale(ek) * inv_q;
        floatx16 s[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            s[kb] = fsa_rows_dot(kt, kb * 32 + l31, hh, qh, ql);
#pragma unroll
            for (int r = 0; r < 16; ++r) s[kb][r] *= fs;
        }
        if (t * 64 + 64 > p.nk_total) {
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (t * 64 + kb * 32 + fsa_arow(r, hh) >= p.nk_total) s[kb][r] = -INFINITY;
        }
        float mx = fmaxf(s[0][0], s[1][0]);
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, fmaxf(s[0][r], s[1][r]));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);                  // finite: every tile holds at least one key
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // first tile: 2^-inf = 0
        float lsum = 0.f;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[kb][r] = __builtin_amdgcn_exp2f(s[kb][r] - m_new);
                lsum += s[kb][r];
            }
        l_run = l_run * alpha + lsum;
        m_run = m_new;
        float oscale = alpha;
        if (ev > ev_run) {                                     // (uniform) a tile of V with a larger scale: O^T moves to its unit
            oscale *= fsa_pow2(127 + ev_run - ev);
            ev_run = ev;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) { o[0][r] *= oscale; o[1][r] *= oscale; }
        const float pf = fsa_pow2(141 + ev - ev_run);          // p 2^14, times this tile's unit relative to O^T's
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            uint32_t ph[8], pl[8];
            fsa_split16(s[kb], pf, ph, pl);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const u32x4 bh = {ph[4 * s2], ph[4 * s2 + 1], ph[4 * s2 + 2], ph[4 * s2 + 3]};
                const u32x4 bl = {pl[4 * s2], pl[4 * s2 + 1], pl[4 * s2 + 2], pl[4 * s2 + 3]};
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    u32x4 ah, al;
                    fsa_col_frag(vt, tfrag, kb * 32 + 16 * s2, dt, ah, al);
                    o[dt] = fsa_mma3(ah, al, bh, bl, o[dt]);
                }
            }
        }
        __syncthreads();
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.f / l_tot;
    float f1, f2;
    fsa_unscale(ev_run + 127, f1, f2);
    if (p.lse && hh == 0 && qok) p.lse[((long)b * p.heads + head) * p.nq + qr] = m_run + __builtin_amdgcn_logf(l_tot);
    if (qok) {
        float* dst = p.out + ((long)b * p.nq + qr) * p.ldo + head * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                floatx4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = o[dt][4 * g + e] * f1 * f2 * inv;
                *reinterpret_cast<floatx4*>(dst + dt * 32 + 8 * g + 4 * hh) = w;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// dK / dV: a workgroup owns 128 keys (a wave 32, lane <-> key); 64-query tiles of Q' = c Q and dO (plus their lse / D) stream through LDS.
//   S[q, key] = Q' K^T, dP[q, key] = dO V^T          A = tile rows, B = the lane's K / V row
//   P = 2^(S - lse[q]), dS = P o (dP - D[q])          registers = queries
//   dV^T[d, key] += dO^T P, dK^T[d, key] += Q'^T dS    A = tile columns, B = P / dS registers;   dK = ln 2 * dK' because Q' carries c = scale * log2 e
__global__ __launch_bounds__(256, 2) void attn_f32split_bwd_dkdv_kernel(const Attn32BwdParams p) {
    using namespace fsa;
    constexpr int BUF = 2 * TILE + 512;                                             // Q' (x0 | x1), dO (x0 | x1), lse[64], D[64]
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF + 64];                // 74,816 B
    float* pmax = reinterpret_cast<float*>(smem + 2 * BUF);                        // [buffer][Q' | dO][wave]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y;
    const int key = blockIdx.x * 128 + wave * 32 + l31;
    const bool kok = key < p.nk;
    u32x4 kh[4], kl[4], vh[4], vl[4];
    float inv_k, inv_v;
    fsa_row_operand(p.k + ((long)b * p.nk + (kok ? key : 0)) * p.ldk + head * 64, kok, 1.f, hh, kh, kl, inv_k);
    fsa_row_operand(p.v + ((long)b * p.nk + (kok ? key : 0)) * p.ldv + head * 64, kok, 1.f, hh, vh, vl, inv_v);

    const int lrow = tid >> 2, lcol = 16 * (tid & 3);
    floatx4 qreg[4], greg[4];
    float lreg = 0.f, dreg = 0.f;
    auto load_tile = [&](const int t, const int buf) {
        const int qi = t * 64 + lrow;
        const bool ok = qi < p.nq;
        const float* qp = p.q + ((long)b * p.nq + (ok ? qi : 0)) * p.ldq + head * 64 + lcol;
        const float* gp = p.dout + ((long)b * p.nq + (ok ? qi : 0)) * p.lddo + head * 64 + lcol;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const floatx4 z = {0.f, 0.f, 0.f, 0.f};
            const floatx4 a = ok ? *reinterpret_cast<const floatx4*>(qp + 4 * i) : z;
            qreg[i] = a * p.c;
            greg[i] = ok ? *reinterpret_cast<const floatx4*>(gp + 4 * i) : z;
        }
        if (tid < 64) {     // lse / D of query row `tid` of the tile; rows beyond nq: lse = +inf makes every probability of the row 0
            const int q2 = t * 64 + tid;
            const bool ok2 = q2 < p.nq;
            const long li = ((long)b * p.heads + head) * p.nq + (ok2 ? q2 : 0);
            lreg = ok2 ? p.lse[li] : INFINITY;
            dreg = ok2 ? p.dsum[li] : 0.f;
        }
        fsa_publish_max(qreg, pmax + buf * 8, lane, wave);
        fsa_publish_max(greg, pmax + buf * 8 + 4, lane, wave);
    };
    auto store_tile = [&](const int buf) {
        fsa_store_split(smem + buf * BUF, qreg, fsa_scale(fsa_tile_exp(pmax + buf * 8)), lrow, lcol);
        fsa_store_split(smem + buf * BUF + TILE, greg, fsa_scale(fsa_tile_exp(pmax + buf * 8 + 4)), lrow, lcol);
        if (tid < 64) {
            float* lt = reinterpret_cast<float*>(smem + buf * BUF + 2 * TILE);
            lt[tid] = lreg;
            lt[64 + tid] = dreg;
        }
    };
    const int tfrag = fsa_tfrag(lane);

    const int nt = (p.nq + 63) / 64;
    load_tile(0, 0);
    __syncthreads();
    store_tile(0);
    __syncthreads();
    floatx16 dv[2] = {fsa_zero16(), fsa_zero16()}, dk[2] = {fsa_zero16(), fsa_zero16()};
    int eg_run = EMIN;            // dV^T in units of 2^-(282 - (eg_run + 127)): dO's largest tile scale so far, P's fixed 2^14 (uniform)
    int wk = 2 * EMIN;            // dK^T in units of 2^-(282 - wk): per lane (= per key), the largest (Q' tile exponent + dS block exponent) so far
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        if (t + 1 < nt) {
            load_tile(t + 1, buf ^ 1);
            __syncthreads();
            store_tile(buf ^ 1);
        }
        const char* qt = smem + buf * BUF;
        const char* gt = qt + TILE;
        const float* lt = reinterpret_cast<const float*>(qt + 2 * TILE);
        const int eq = fsa_tile_exp(pmax + buf * 8), eg = fsa_tile_exp(pmax + buf * 8 + 4);
        const float fs = fsa_inv_scale(eq) * inv_k, fd = fsa_inv_scale(eg) * inv_v;
        if (eg > eg_run) {        // (uniform)
            const float f = fsa_pow2(127 + eg_run - eg);
#pragma unroll
            for (int r = 0; r < 16; ++r) { dv[0][r] *= f; dv[1][r] *= f; }
            eg_run = eg;
        }
        const float pf = fsa_pow2(141 + eg - eg_run);
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            floatx16 s = fsa_rows_dot<true>(qt, qb * 32 + l31, hh, kh, kl);      // registers = queries fsa_arow(r, hh) of the block
            floatx16 dp = fsa_rows_dot(gt, qb * 32 + l31, hh, vh, vl);
            float mds = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const floatx4 l4 = *reinterpret_cast<const floatx4*>(lt + qb * 32 + 8 * g + 4 * hh);
                const floatx4 d4 = *reinterpret_cast<const floatx4*>(lt + 64 + qb * 32 + 8 * g + 4 * hh);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float pr = __builtin_amdgcn_exp2f(s[4 * g + e] * fs - l4[e]);
                    s[4 * g + e] = pr;
                    dp[4 * g + e] = pr * (dp[4 * g + e] * fd - d4[e]);
                    mds = fmaxf(mds, fabsf(dp[4 * g + e]));
                }
            }
            mds = fmaxf(mds, __shfl_xor(mds, 32, 64));
            const int need = eq + fsa_exp_of(mds);
            if (__builtin_amdgcn_ballot_w64(need > wk) != 0) {      // some key's dK^T moves to a larger unit (rare after the first tiles)
                const int wn = max(wk, need);
                const float f = fsa_pow2(127 + wk - wn);
#pragma unroll
                for (int r = 0; r < 16; ++r) { dk[0][r] *= f; dk[1][r] *= f; }
                wk = wn;
            }
            uint32_t ph[8], pl[8], sh[8], sl[8];
            fsa_split16(s, pf, ph, pl);
            fsa_split16(dp, fsa_pow2(268 - wk + eq), sh, sl);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const u32x4 pbh = {ph[4 * s2], ph[4 * s2 + 1], ph[4 * s2 + 2], ph[4 * s2 + 3]};
                const u32x4 pbl = {pl[4 * s2], pl[4 * s2 + 1], pl[4 * s2 + 2], pl[4 * s2 + 3]};
                const u32x4 sbh = {sh[4 * s2], sh[4 * s2 + 1], sh[4 * s2 + 2], sh[4 * s2 + 3]};
                const u32x4 sbl = {sl[4 * s2], sl[4 * s2 + 1], sl[4 * s2 + 2], sl[4 * s2 + 3]};
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    u32x4 ah, al;
                    fsa_col_frag(gt, tfrag, qb * 32 + 16 * s2, dt, ah, al);
                    dv[dt] = fsa_mma3(ah, al, pbh, pbl, dv[dt]);
                    fsa_col_frag(qt, tfrag, qb * 32 + 16 * s2, dt, ah, al);
                    dk[dt] = fsa_mma3(ah, al, sbh, sbl, dk[dt]);
                }
            }
        }
        __syncthreads();
    }
    if (kok) {
        float v1, v2, k1, k2;
        fsa_unscale(eg_run + 127, v1, v2);
        fsa_unscale(wk, k1, k2);
        k2 *= LN2;
        float* dkp = p.dk + ((long)b * p.nk + key) * p.lddk + head * 64;
        float* dvp = p.dv + ((long)b * p.nk + key) * p.lddv + head * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                floatx4 a, c;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[e] = dk[dt][4 * g + e] * k1 * k2;
                    c[e] = dv[dt][4 * g + e] * v1 * v2;
                }
                *reinterpret_cast<floatx4*>(dkp + dt * 32 + 8 * g + 4 * hh) = a;
                *reinterpret_cast<floatx4*>(dvp + dt * 32 + 8 * g + 4 * hh) = c;
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// dQ: the forward's structure (lane <-> query, 64-key tiles of K and V in LDS).
//   S^T[key, q] = K Q'^T, dP^T[key, q] = V dO^T        A = tile rows, B = the lane's Q' / dO row
//   dS^T = P^T o (dP^T - D[q])                          lane-local lse / D
//   dQ^T[d, q] += K^T dS^T                              A = K tile columns, B = dS^T registers;   dQ = scale * dQ'
__global__ __launch_bounds__(256, 2) void attn_f32split_bwd_dq_kernel(const Attn32BwdParams p) {
    using namespace fsa;
    constexpr int BUF = 2 * TILE;
    __shared__ __attribute__((aligned(16))) char smem[2 * BUF + 64];
    float* pmax = reinterpret_cast<float*>(smem + 2 * BUF);                        // [buffer][K | V][wave]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z, head = blockIdx.y;
    const int qr = blockIdx.x * 128 + wave * 32 + l31;
    const bool qok = qr < p.nq;
    u32x4 qh[4], ql[4], gh[4], gl[4];
    float inv_q, inv_g;
    fsa_row_operand(p.q + ((long)b * p.nq + (qok ? qr : 0)) * p.ldq + head * 64, qok, p.c, hh, qh, ql, inv_q);
    fsa_row_operand(p.dout + ((long)b * p.nq + (qok ? qr : 0)) * p.lddo + head * 64, qok, 1.f, hh, gh, gl, inv_g);
    const long li = ((long)b * p.heads + head) * p.nq + (qok ? qr : 0);
    const float lse_q = qok ? p.lse[li] : INFINITY, d_q = qok ? p.dsum[li] : 0.f;

    const int lrow = tid >> 2, lcol = 16 * (tid & 3);
    floatx4 kreg[4], vreg[4];
    auto load_tile = [&](const int t, const int buf) {
        const int key = t * 64 + lrow;
        const bool ok = key < p.nk;
        const float* kp = p.k + ((long)b * p.nk + (ok ? key : 0)) * p.ldk + head * 64 + lcol;
        const float* vp = p.v + ((long)b * p.nk + (ok ? key : 0)) * p.ldv + head * 64 + lcol;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const floatx4 z = {0.f, 0.f, 0.f, 0.f};
            kreg[i] = ok ? *reinterpret_cast<const floatx4*>(kp + 4 * i) : z;
            vreg[i] = ok ? *reinterpret_cast<const floatx4*>(vp + 4 * i) : z;
        }
        fsa_publish_max(kreg, pmax + buf * 8, lane, wave);
        fsa_publish_max(vreg, pmax + buf * 8 + 4, lane, wave);
    };
    auto store_tile = [&](const int buf) {
        fsa_store_split(smem + buf * BUF, kreg, fsa_scale(fsa_tile_exp(pmax + buf * 8)), lrow, lcol);
        fsa_store_split(smem + buf * BUF + TILE, vreg, fsa_scale(fsa_tile_exp(pmax + buf * 8 + 4)), lrow, lcol);
    };
    const int tfrag = fsa_tfrag(lane);

    const int nt = (p.nk + 63) / 64;
    load_tile(0, 0);
    __syncthreads();
    store_tile(0);
    __syncthreads();
    floatx16 dq[2] = {fsa_zero16(), fsa_zero16()};
    int wq = 2 * EMIN;            // dQ^T in units of 2^-(282 - wq): per lane (= per query), the largest (K tile exponent + dS^T block exponent) so far
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        if (t + 1 < nt) {
            load_tile(t + 1, buf ^ 1);
            __syncthreads();
            store_tile(buf ^ 1);
        }
        const char* kt = smem + buf * BUF;
        const char* vt = kt + TILE;
        const int ek = fsa_tile_exp(pmax + buf * 8), ev = fsa_tile_exp(pmax + buf * 8 + 4);
        const float fs = fsa_inv_scale(ek) * inv_q, fd = fsa_inv_scale(ev) * inv_g;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            floatx16 s = fsa_rows_dot(kt, kb * 32 + l31, hh, qh, ql);
            floatx16 dp = fsa_rows_dot(vt, kb * 32 + l31, hh, gh, gl);
            float mds = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool in = t * 64 + kb * 32 + fsa_arow(r, hh) < p.nk;
                const float pr = in ? __builtin_amdgcn_exp2f(s[r] * fs - lse_q) : 0.f;
                dp[r] = pr * (dp[r] * fd - d_q);
                mds = fmaxf(mds, fabsf(dp[r]));
            }
            mds = fmaxf(mds, __shfl_xor(mds, 32, 64));
            const int need = ek + fsa_exp_of(mds);
            if (__builtin_amdgcn_ballot_w64(need > wq) != 0) {
                const int wn = max(wq, need);
                const float f = fsa_pow2(127 + wq - wn);
#pragma unroll
                for (int r = 0; r < 16; ++r) { dq[0][r] *= f; dq[1][r] *= f; }
                wq = wn;
            }
            uint32_t sh[8], sl[8];
            fsa_split16(dp, fsa_pow2(268 - wq + ek), sh, sl);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const u32x4 sbh = {sh[4 * s2], sh[4 * s2 + 1], sh[4 * s2 + 2], sh[4 * s2 + 3]};
                const u32x4 sbl = {sl[4 * s2], sl[4 * s2 + 1], sl[4 * s2 + 2], sl[4 * s2 + 3]};
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    u32x4 ah, al;
                    fsa_col_frag(kt, tfrag, kb * 32 + 16 * s2, dt, ah, al);
                    dq[dt] = fsa_mma3(ah, al, sbh, sbl, dq[dt]);
                }
            }
        }
        __syncthreads();
    }
    if (qok) {
        float f1, f2;
        fsa_unscale(wq, f1, f2);
        f2 *= p.scale;
        float* dst = p.dq + ((long)b * p.nq + qr) * p.lddq + head * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                floatx4 w;
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = dq[dt][4 * g + e] * f1 * f2;
                *reinterpret_cast<floatx4*>(dst + dt * 32 + 8 * g + 4 * hh) = w;
            }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------
int attn_f32split_fwd(const E2eftAttnDesc* d, const void* q, const void* k, const void* v, void* out, float* lse, void* stream) {
    Attn32Params p;
    const int rc = attn32_fwd_params(d, q, k, v, out, lse, &p);
    if (rc != E2EFT_OK) return rc;
    hipLaunchKernelGGL(attn_f32split_fwd_kernel, dim3((unsigned)((long)d->batch * d->heads * p.nqb)), dim3(256), 0, (hipStream_t)stream, p);
    tag_kernel("attn_f32split_fwd_kernel");
    return check_launch("attn_fwd (fp32, f16 splits)");
}

int attn_f32split_bwd(const E2eftAttnDesc* d, const void* q, const void* k, const void* v, const void* out, const void* dout, int32_t lddo, const float* lse,
                      void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv, int32_t lddv, void* workspace, void* stream) {
    Attn32BwdParams p;
    const int rc = attn32_bwd_params(d, q, k, v, out, dout, lddo, lse, dq, lddq, dk, lddk, dv, lddv, workspace, &p);
    if (rc != E2EFT_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    attn32_bwd_prep(d, out, dout, lddo, (float*)workspace, s);
    hipLaunchKernelGGL(attn_f32split_bwd_dkdv_kernel, dim3(cdiv(p.nk, 128), d->heads, d->batch), dim3(256), 0, s, p);
    hipLaunchKernelGGL(attn_f32split_bwd_dq_kernel, dim3(cdiv(p.nq, 128), d->heads, d->batch), dim3(256), 0, s, p);
    tag_kernel("attn_f32split_bwd_dkdv_kernel + attn_f32split_bwd_dq_kernel");
    return check_launch("attn_bwd (fp32, f16 splits)");
}

}  // namespace e2eft

// Pure host arithmetic: does the split route take this attention (backward != 0: e2eft_attn_bwd)?  Self- and cross-attention of any query / key count;
// GeoWizard's joint keys (kv_nseg > 1, forward only) stay on attn32.hip.
extern "C" int32_t e2eft_attn_f32split_supported(const E2eftAttnDesc* d, int32_t backward) {
    using namespace e2eft;
    if (!d || option(E2EFT_OPT_F32_SPLIT_ATTN) != 1 || d->dtype != E2EFT_F32) return 0;
    if (d->batch <= 0 || d->heads <= 0 || d->nq <= 0 || d->nk_seg <= 0 || d->kv_bmod <= 0) return 0;
    if (d->kv_nseg != 1) return 0;
    if (backward && d->kv_bmod != d->batch) return 0;
    return 1;
}
