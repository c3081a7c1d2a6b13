// igemm_epilogue.h — every epilogue of the implicit-GEMM family: out = alpha * (acc + bias + rowadd[img]) + residual, optionally with the GroupNorm
// statistics (n, mean, M2) of the tile that was written (IgemmParams::gn_partial).
//   * igemm_epilogue / igemm_epilogue_rows: igemm2's workgroup-wide epilogue (the whole fp32 tile staged in LDS, then row passes);
//   * epilogue_packed / epilogue / epilogue_f32 / combine: the wave-private epilogues of the persistent kernels (igemm5.hip, igemm6.hip, convin.hip) and the
//     merge of their statistics deposits.  Everything they use is a parameter, a member of EpiCtx or a template argument.
#pragma once
#include "igemm.h"
#include <type_traits>

namespace e2eft {

// ---- GroupNorm statistics: pivot sums -> (n, mean, M2) ------------------------------------------------------------------------------------------------------
struct GnTriple { float n, mean, m2; };
// fold a block of n values, summed about a pivot (s1 = sum (x - pv), s2 = sum (x - pv)^2), into the running triple t (t.n == 0: the first block) with Chan's
// formula.  n is a power of two at every call, so the divisions by it are exact scalings
__device__ __forceinline__ void gn_add_pivot_sums(GnTriple& t, const float n, const float s1, const float s2, const float pv) {
    const float mb = pv + s1 / n;
    const float m2b = fmaxf(s2 - s1 * s1 / n, 0.f);
    if (t.n == 0.f) { t = GnTriple{n, mb, m2b}; return; }
    const float nt = t.n + n, dl = mb - t.mean;
    t.mean += dl * (n / nt);
    t.m2 += m2b + dl * dl * (t.n * n / nt);
    t.n = nt;
}

// ---------------------------------------------------------------------------------------------------------------
// igemm2: the 32x32 MFMA accumulator layout (lane = column, registers = rows) would give 2-byte scattered
// stores and one dependent residual load per element.  Instead the fp32 tile goes through LDS once (the k-loop is
// finished, its buffers are free) and is written back row-wise: every thread owns 8 consecutive columns of a row,
// residual / output move as 16-byte vectors, a wave covers 4 full 256-byte rows per instruction.
// Optionally (p.gn_partial) the full-tile path also emits the GroupNorm statistics of the tile it just wrote — per column, shifted sums
// over each thread's rows, butterfly + LDS merge over the workgroup — so that the consuming GroupNorm skips its statistics
// pass over HBM (one of its three passes).
template <typename T, int BM_, int BN_, int NT_>
__device__ __forceinline__ void igemm_epilogue_rows(const IgemmParams& p, char* smem, int m0, int n0, int zo, int zi);

template <typename T, int BM_, int BN_, int NT_>
__device__ __forceinline__ void igemm_epilogue(const IgemmParams& p, char* smem, floatx16 (&acc)[2][2], int wm, int wn, int l31,
                                               int h, int m0, int n0, int zo, int zi) {
    constexpr int LDT = BN_ + 4;            // fp32 row stride of the staged tile (528 B for BN = 128)
    float* tile = reinterpret_cast<float*>(smem);
    __syncthreads();                        // every wave is done reading the last k-tile
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                tile[(wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * LDT + wn * 64 + j * 32 + l31] = acc[i][j][r];
    __syncthreads();
    E2EFT_STAMP(3);
    igemm_epilogue_rows<T, BM_, BN_, NT_>(p, smem, m0, n0, zo, zi);
}

// the row passes over a tile that is already staged in LDS as fp32 [BM_][BN_ + 4] (all threads past a barrier): bias / rowadd / alpha /
// residual, rounding, 16-byte stores, optional GroupNorm statistics.
template <typename T, int BM_, int BN_, int NT_>
__device__ __forceinline__ void igemm_epilogue_rows(const IgemmParams& p, char* smem, int m0, int n0, int zo, int zi) {
    constexpr int EPC = 16 / (int)sizeof(T);
    constexpr int LDT = BN_ + 4;            // fp32 row stride of the staged tile (528 B for BN = 128)
    constexpr int CPR = BN_ / 8;            // 8-column chunks per row
    constexpr int RPP = NT_ / CPR;          // rows per pass
    constexpr int NPASS = BM_ / RPP;        // rows per thread
    constexpr int NWV = NT_ / 64;
    float* tile = reinterpret_cast<float*>(smem);
    float* gst = tile + BM_ * LDT;          // [NWV][16 chunks][8 cols][2] wave partials of the GroupNorm statistics

    const T* __restrict__ bias = (const T*)p.bias;
    const T* __restrict__ rowadd = (const T*)p.rowadd;
    const T* __restrict__ res = p.residual ? (const T*)p.residual + zo * p.sr_o + zi * p.sr_i : nullptr;
    T* __restrict__ out = (T*)p.out + zo * p.so_o + zi * p.so_i;
    const int chunk = threadIdx.x % CPR, rbase = threadIdx.x / CPR;
    const int n = n0 + chunk * 8;
    const bool col_ok = n < p.N;
    const bool vec = (p.N % 8 == 0) && (p.ldo % EPC == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0) &&
                     (!res || (p.ldr % EPC == 0 && (reinterpret_cast<uintptr_t>(res) & 15) == 0));
    const bool stats = p.gn_partial != nullptr;   // the host (launch2 of igemm2.hip) keeps gn_partial only where `full` below holds for every tile
    const int nv = min(8, p.N - n);
    float bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = (bias && !p.bias_along_m && col_ok && e < nv) ? to_f(bias[n + e]) : 0.f;

    // ---- fast path: vector epilogue on a tile that lies completely inside the problem; every condition is workgroup-uniform and
    // hoisted, so the pass loop is straight-line code: x = fma(acc, alpha, bias*alpha) [+ rowadd*alpha] [+ residual], one
    // v_cvt_pk per column pair, one 16-byte store per row chunk.  (The generic loop below costs ~9k cycles per 256x128 tile in
    // exec-mask branches and scalar fallbacks even when none is taken — scripts/stamp_bench.py.)
    const bool full = vec && m0 + BM_ <= p.M && !(bias && p.bias_along_m);   // a ragged last N-tile only idles the threads of its missing chunks
    if (full) {
        const float al = p.alpha;
        float bva[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) bva[e] = bv[e] * al;
        const bool one_img = p.rows_per_img % BM_ == 0 || p.rows_per_img >= p.M;
        const int img0 = rowadd ? m0 / p.rows_per_img : 0;
        T* __restrict__ orow = out + (long)(m0 + rbase) * p.ldo + n;
        const T* __restrict__ rrow = res ? res + (long)(m0 + rbase) * p.ldr + n : nullptr;
        const long ostep = (long)RPP * p.ldo, rstep = (long)RPP * p.ldr;
        // GroupNorm statistics: every thread of a column accumulates sum(x - pv), sum((x - pv)^2) about the same pivot pv (the tile's
        // first row before rowadd / residual: any value near the data does), so partial results merge by plain addition.  They are
        // taken from the fp32 value; rounding to T adds a variance of ~2^-22 x^2 (fp16) / 2^-16 x^2 (bf16) — below the kernels' noise.
        float pv[8];
        if (stats) {
            const floatx4 q0 = *reinterpret_cast<const floatx4*>(tile + chunk * 8);
            const floatx4 q1 = *reinterpret_cast<const floatx4*>(tile + chunk * 8 + 4);
            const float pr[8] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]};
#pragma unroll
            for (int e = 0; e < 8; ++e) pv[e] = fmaf(pr[e], al, bva[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) pv[e] = 0.f;
        }
        // The row passes work on float2 values: explicit packed math (v_pk_fma_f32 / v_pk_add_f32 on NATURAL register pairs — the pairs
        // are the dword pairs of the ds_read_b128 results, so no operand swizzle is needed; the swizzled forms the SLP vectorizer used
        // to generate here are the ones that misread on gfx950, DESIGN.md §3.6, and build.py keeps that vectorizer off).  The
        // statistics cost 4.6k cycles per 256x128 tile as scalar code (3 VALU per element) against 3.6k packed.
        typedef float f2 __attribute__((ext_vector_type(2)));
        const f2 al2 = {al, al};
        f2 bva2[4], pv2[4], sm2[4], sq2[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bva2[q] = f2{bva[2 * q], bva[2 * q + 1]};
            pv2[q] = f2{pv[2 * q], pv[2 * q + 1]};
            sm2[q] = f2{0.f, 0.f};
            sq2[q] = f2{0.f, 0.f};
        }
        // p.out_seg > 0 (e2eft_upconv2x_fwd: one parity phase of a 2x-upsampled image): GEMM row m lands on output row m + (m / out_seg) * out_seg
        auto seg_off = [&](const int row) -> long { return p.out_seg > 0 ? (long)((m0 + row) / p.out_seg) * p.out_seg * p.ldo : 0L; };
        auto run = [&](auto has_res, auto has_ra) {
            constexpr bool HAS_RES = decltype(has_res)::value, HAS_RA = decltype(has_ra)::value;
#pragma unroll
            for (int pass = 0; pass < NPASS; ++pass) {
                const int row = rbase + pass * RPP;
                const floatx4 t0 = *reinterpret_cast<const floatx4*>(tile + row * LDT + chunk * 8);
                const floatx4 t1 = *reinterpret_cast<const floatx4*>(tile + row * LDT + chunk * 8 + 4);
                f2 x2[4] = {f2{t0[0], t0[1]}, f2{t0[2], t0[3]}, f2{t1[0], t1[1]}, f2{t1[2], t1[3]}};
#pragma unroll
                for (int q = 0; q < 4; ++q) x2[q] = __builtin_elementwise_fma(x2[q], al2, bva2[q]);
                if constexpr (HAS_RA) {
                    const int img = one_img ? img0 : (m0 + row) / p.rows_per_img;
                    const T* ra = rowadd + (long)img * p.N + n;
#pragma unroll
                    for (int q = 0; q < 8 / EPC; ++q) {
                        const Vec16<T> t = ld16(ra + q * EPC);
#pragma unroll
                        for (int e = 0; e < EPC; e += 2) {
                            const int j = (q * EPC + e) >> 1;
                            x2[j] = __builtin_elementwise_fma(f2{to_f(t.e[e]), to_f(t.e[e + 1])}, al2, x2[j]);
                        }
                    }
                }
                if constexpr (HAS_RES) {
#pragma unroll
                    for (int q = 0; q < 8 / EPC; ++q) {
                        const Vec16<T> t = ld16(rrow + pass * rstep + q * EPC);
#pragma unroll
                        for (int e = 0; e < EPC; e += 2) {
                            const int j = (q * EPC + e) >> 1;
                            x2[j] += f2{to_f(t.e[e]), to_f(t.e[e + 1])};
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < 8 / EPC; ++q) {
                    Vec16<T> o;
#pragma unroll
                    for (int e = 0; e < EPC; ++e) o.e[e] = from_f<T>(x2[(q * EPC + e) >> 1][(q * EPC + e) & 1]);
                    st16(orow + pass * ostep + seg_off(row) + q * EPC, o);
                }
                if (stats) {   // uniform: shifted sums about a per-column pivot shared by the whole tile (sm2 = sum, sq2 = sum of squares)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f2 d = x2[q] - pv2[q];
                        sm2[q] += d;
                        sq2[q] = __builtin_elementwise_fma(d, d, sq2[q]);
                    }
                }
            }
        };
        if (col_ok) {
            if (res) {
                if (rowadd) run(std::true_type{}, std::true_type{});
                else run(std::true_type{}, std::false_type{});
            } else {
                if (rowadd) run(std::false_type{}, std::true_type{});
                else run(std::false_type{}, std::false_type{});
            }
        }
        if (stats) {   // uniform.  lanes l, l^16, l^32, l^48 own the same 8 columns: add; then the waves through LDS
            float s_sum[8], s_sq[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s_sum[2 * q] = sm2[q][0]; s_sum[2 * q + 1] = sm2[q][1];
                s_sq[2 * q] = sq2[q][0]; s_sq[2 * q + 1] = sq2[q][1];
            }
#pragma unroll
            for (int off = 16; off <= 32; off <<= 1)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    s_sum[e] += __shfl_xor(s_sum[e], off, 64);
                    s_sq[e] += __shfl_xor(s_sq[e], off, 64);
                }
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
            float* piv = gst + NWV * 16 * 8 * 2;
            if (lane < 16) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    gst[((wv * 16 + lane) * 8 + e) * 2] = s_sum[e];
                    gst[((wv * 16 + lane) * 8 + e) * 2 + 1] = s_sq[e];
                    if (wv == 0) piv[lane * 8 + e] = pv[e];
                }
            }
            __syncthreads();
            if (threadIdx.x < BN_ && n0 + (int)threadIdx.x < p.N) {
                const int c = threadIdx.x;
                float su = 0.f, sq = 0.f;
#pragma unroll
                for (int w = 0; w < NWV; ++w) {
                    su += gst[((w * 16 + c / 8) * 8 + (c & 7)) * 2];
                    sq += gst[((w * 16 + c / 8) * 8 + (c & 7)) * 2 + 1];
                }
                GnTriple t = {0.f, 0.f, 0.f};
                gn_add_pivot_sums(t, (float)BM_, su, sq, piv[c]);
                const int img = m0 / p.rows_per_img;
                const int slab = (m0 - img * p.rows_per_img) / BM_;
                float* o = p.gn_partial + (((long)img * p.gn_nslabs + slab) * p.N + n0 + c) * 3;
                o[0] = t.n; o[1] = t.mean; o[2] = t.m2;
            }
        }
        return;
    }
    // ---- generic path: ragged M, unaligned rows, bias along M.  No statistics: launch2 drops gn_partial for every launch that can get here
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
        const int row = rbase + pass * RPP;
        const int m = m0 + row;
        if (m >= p.M || !col_ok) continue;
        const floatx4 t0 = *reinterpret_cast<const floatx4*>(tile + row * LDT + chunk * 8);
        const floatx4 t1 = *reinterpret_cast<const floatx4*>(tile + row * LDT + chunk * 8 + 4);
        float v[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
        const float bm = (bias && p.bias_along_m) ? to_f(bias[m]) : 0.f;
        const T* ra = rowadd ? rowadd + (long)(m / p.rows_per_img) * p.N + n : nullptr;
        if (vec) {
            float rv[8];
            if (res) {
#pragma unroll
                for (int q = 0; q < 8 / EPC; ++q) {
                    Vec16<T> t = ld16(res + (long)m * p.ldr + n + q * EPC);
#pragma unroll
                    for (int e = 0; e < EPC; ++e) rv[q * EPC + e] = to_f(t.e[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float x = v[e] + bv[e] + bm;
                if (ra) x += to_f(ra[e]);
                x *= p.alpha;
                if (res) x += rv[e];
                v[e] = x;
            }
#pragma unroll
            for (int q = 0; q < 8 / EPC; ++q) {
                Vec16<T> o;
#pragma unroll
                for (int e = 0; e < EPC; ++e) o.e[e] = from_f<T>(v[q * EPC + e]);
                st16(out + ((long)m + (p.out_seg > 0 ? (long)(m / p.out_seg) * p.out_seg : 0L)) * p.ldo + n + q * EPC, o);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e < nv) {
                    float x = v[e] + bv[e] + bm;
                    if (ra) x += to_f(ra[e]);
                    x *= p.alpha;
                    if (res) x += to_f(res[(long)m * p.ldr + n + e]);
                    out[((long)m + (p.out_seg > 0 ? (long)(m / p.out_seg) * p.out_seg : 0L)) * p.ldo + n + e] = from_f<T>(x);
                }
            }
        }
    }
}

// =============================================================================================================================================================
// The persistent kernels (igemm5.hip, igemm6.hip, convin.hip): a wave sends its own 64 x 64 accumulator block through a private 2 x 2 KiB window in LDS.
//   epilogue_packed  launches WITHOUT a residual: everything per column is done in the accumulator layout, two rounded rows share a dword through LDS
//   epilogue         16-bit launches with a residual: eight fp32 slices, row-wise readers
//   epilogue_f32     fp32 bias / residual / output (csrc/f32split.hip), the same slices
//   combine          merge of the four row-waves' statistics deposits of a tile, one thread per column
// M16: the accumulators are the 4 x 4 x floatx4 layout of v_mfma_f32_16x16x32 (a lane owns columns 16 j + (lane & 15), rows 4 (lane >> 4) + e of 16-row block i)
// instead of the 2 x 2 x floatx16 of v_mfma_f32_32x32x16 (columns 32 j + (lane & 31)).
typedef float f2 __attribute__((ext_vector_type(2)));
enum EpiKind { EPI_PACKED, EPI_ROWS, EPI_F32 };

// first row (inside the wave's 64-row block) of slice s of the fp32-window epilogues, for the lane that reads window row 0 of the slice
template <bool M16> __device__ __forceinline__ constexpr int epi_srow(const int s) { return M16 ? 16 * (s >> 1) + 2 * (s & 1) : 8 * s; }

// ---- row maps: rofs(r) = pixel-row offset of row r (a multiple of 8) of the wave's 64-row block relative to its row 0; rows_left(er): rows of the problem from
// this lane's row `er` of the block on (slice s exists while epi_srow(s) < rows_left)
// consecutive GEMM rows (igemm5).  p.out_seg > 0 (e2eft_upconv2x_fwd): row r may lie in a later output segment than row 0 — every segment passed adds out_seg
// pixel rows (wave-uniform: one float-reciprocal division per slice).  mb: first GEMM row of the wave's block, seg0: the output segment it starts in
struct RowsConsecutive {
    const IgemmParams& p;
    const int& mb;
    const int& seg0;
    __device__ __forceinline__ long rofs(const int r) const {
        if (p.out_seg <= 0) return (long)r;
        return (long)r + (long)(fast_div(mb + r, p.out_seg) - seg0) * p.out_seg;
    }
    __device__ __forceinline__ int rows_left(const int er) const { return p.M - (mb + er); }   // (the ragged last tile of the fp32-split launches)
};
// an 8 x 32-pixel block of one image (igemm6, convin): a wave's 64 rows are two image rows, `stride` pixels apart; tiles are whole blocks
struct RowsBlock {
    const int stride;
    __device__ __forceinline__ long rofs(const int r) const { return (long)(r & 31) + (long)(r >> 5) * stride; }
    __device__ __forceinline__ int rows_left(const int) const { return 0x40000000; }
};

// ---- epilogue operands requested ahead of their use (inside the k-loop), and how many VMEM instructions a request issues: the k-loops' counted waits depend on it.
// Every lane requests (columns beyond N read the tile's first chunk / column instead): the count must not depend on exec.
template <typename T, bool M16> struct EpiOperands {
    static constexpr int NJ = M16 ? 4 : 2;            // columns a lane owns in the accumulator layout
    Vec16<T> res[4], bias, ra;                        // EPI_ROWS: residual rows of slices 0-3, bias and rowadd chunk of this lane
    T col_bias[NJ], col_ra[NJ];                       // EPI_PACKED: bias / rowadd of the lane's columns
    template <EpiKind KIND> static __device__ __forceinline__ int vmem_count(const bool has_bias, const bool has_ra) {
        const int per = (has_bias ? 1 : 0) + (has_ra ? 1 : 0);
        return KIND == EPI_F32 ? 0 : KIND == EPI_ROWS ? 4 + per : NJ * per;      // (epilogue_f32 requests its operands itself)
    }
    // rrow: element offset of this lane's residual row of slice 0, ncl: first column of its chunk (clamped), img: the tile's image (rowadd)
    __device__ __forceinline__ void request_rows(const IgemmParams& p, const T* bias_, const T* rowadd, const bool has_ra, const long rrow, const int ncl, const int img) {
#pragma unroll
        for (int s = 0; s < 4; ++s) res[s] = ld16((const T*)p.residual + rrow + (long)epi_srow<M16>(s) * p.ldr);
        if (bias_) bias = ld16(bias_ + ncl);
        if (has_ra) ra = ld16(rowadd + (long)img * p.N + ncl);
    }
    // col0: first column of the wave's 64, n0: the tile's first column
    __device__ __forceinline__ void request_cols(const IgemmParams& p, const T* bias_, const T* rowadd, const bool has_ra, const int lane, const int n0, const int col0, const int img) {
        int nj[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int cj = col0 + (M16 ? 16 * j + (lane & 15) : 32 * j + (lane & 31));
            nj[j] = cj < p.N ? cj : n0;
        }
        // the issue order each layout's kernels were measured with: column by column (M16), operand by operand (32x32)
#pragma unroll
        for (int k = 0; k < 2 * NJ; ++k) {
            const int j = M16 ? k >> 1 : k % NJ;
            const bool ra_turn = M16 ? (k & 1) != 0 : k >= NJ;
            if (!ra_turn) { if (bias_) col_bias[j] = bias_[nj[j]]; }
            else if (has_ra) col_ra[j] = rowadd[(long)img * p.N + nj[j]];
        }
    }
};

// ---- what an epilogue reads from its kernel: built once per kernel; the members that change per tile are references
template <typename T_, bool M16_, typename Acc, typename Rows> struct EpiCtx {
    using T = T_;
    static constexpr bool M16 = M16_;
    const IgemmParams& p;
    char* smem;
    Acc& acc;                               // floatx16[2][2], or (M16) floatx4[4][4]
    const EpiOperands<T_, M16_>& ops;
    const Rows& rows;
    const int wave, lane;                   // the kernel's lane coordinates (its own values, so that the compiler sees one definition of each):
    const int l31, h, er, ec;               // lane & 31, lane >> 5 (accumulator layout); lane >> 3, lane & 7 (row and 8-column chunk of the row-wise readers)
    const T_* bias;                         // null: no bias
    const bool has_ra, stats;               // a row vector is added / statistics are deposited
    const long& orow;                       // element offset of this lane's output row of slice 0 (packed: of round 0) at its 8-column chunk
    const bool& colok;                      // that chunk lies inside N
};
struct NoStamp { __device__ __forceinline__ void operator()(int) const {} };

// physical dword of a lane's first value inside a window.  fp32 windows (hstride 128): 16-byte unit U = ((x >> 2) & 1) * 64 + row * 8 + (x >> 3) for logical (row, column x) —
// the row-wise readers take units `lane` and `64 + lane` (two conflict-free contiguous kilobytes), the accumulator lanes write 2-way (free on ds_write_b32).  Packed windows
// (hstride 64): dword of (row pair rp8, column x) = ((x >> 2) & 1) * 256 + rp8 * 32 + (x >> 3) * 4 + (x & 3).  M16: a lane's rows are 4 (lane >> 4) + e, i.e. window rows
// 2 (lane >> 4) + e of a two-rows-per-block slice or row pairs 2 (lane >> 4) + t — the same offset in both windows (these writes are 4-way on a bank)
template <bool M16> __device__ __forceinline__ int epi_wofs(const int lane, const int l31, const int h, const int hstride) {
    if constexpr (M16) return (((lane & 15) >> 2) & 1) * 256 + (lane >> 4) * 64 + ((lane & 15) >> 3) * 4 + (lane & 3);
    else return ((l31 >> 2) & 1) * 256 + h * hstride + (l31 >> 3) * 4 + (l31 & 3);
}

// ---- the epilogue of a tile WITHOUT a residual: out = alpha * (acc + bias + rowadd[img]), eight slices per wave
// Everything that is per column (alpha, bias, row vector, GroupNorm statistics) is done in the accumulator layout, where a lane owns NJ columns; the values are
// rounded to T there and two rows of a column share a dword, so the LDS transpose moves half the bytes (the ds_write_b32 rate of 64 B/clk is what bounds the
// epilogue) and the row-wise readers only un-interleave and store.  Rounds of 16 rows: window = 8 row pairs x 64 columns of packed dwords (2 KiB as one fp32
// slice), two windows in flight.  DEP: LDS offset of the per-wave statistics deposits
template <int DEP, typename Ctx>
__device__ __forceinline__ void epilogue_packed(const Ctx& c, const int sfree, const long zoff_o) {
    using T = typename Ctx::T;
    constexpr bool M16 = Ctx::M16;
    const IgemmParams& p = c.p;
    const int lane = c.lane, l31 = c.l31, h = c.h;
    unsigned* win = reinterpret_cast<unsigned*>(c.smem + sfree + c.wave * 4096);
    const float al = p.alpha;
    T* __restrict__ out = (T*)p.out + zoff_o;
    const f2 al2 = {al, al};
    constexpr int NJ = M16 ? 4 : 2;
    f2 bva[NJ], rav[NJ], pv[NJ], sm[NJ], sq[NJ];   // per owned column j: bias * alpha, row vector, pivot, shifted sums (pairs = two rows at a time)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        // association as in the fp32 epilogue below and igemm2's vector row pass: fma(rowadd, alpha, fma(acc, alpha, bias * alpha))
        const float bj = c.bias ? to_f(c.ops.col_bias[j]) * al : 0.f, rj = c.has_ra ? to_f(c.ops.col_ra[j]) : 0.f;
        bva[j] = f2{bj, bj}; rav[j] = f2{rj, rj};
        pv[j] = f2{0.f, 0.f}; sm[j] = f2{0.f, 0.f}; sq[j] = f2{0.f, 0.f};
    }
    const int wofs = epi_wofs<M16>(lane, l31, h, 64);   // + qq * 128 + t * 32 + j * 16; M16 (a round is one 16-row block): + t * 32 + j * 8
    // (the two accumulator layouts keep a written-out body each: one shared lambda for a row pair's arithmetic, statistics and packed dword changed the address-space
    // inference of convin's bias loads — flat instead of global loads)
    auto wr = [&](auto rc_) {
        constexpr int r = decltype(rc_)::value, i = r >> 1;
        unsigned* wb = win + (r & 1) * 512 + wofs;
        if constexpr (M16) {
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f2 x = {c.acc[r][j][2 * t], c.acc[r][j][2 * t + 1]};
                    x = __builtin_elementwise_fma(x, al2, bva[j]);
                    if (c.has_ra) x = __builtin_elementwise_fma(rav[j], al2, x);
                    if (c.stats) {
                        if (r == 0 && t == 0) {   // pivot of a column: its first value in the wave (held by the lane >> 4 = 0 lane)
                            const float p0 = __shfl(x[0], lane & 15, 64);
                            pv[j] = f2{p0, p0};
                        }
                        const f2 d = x - pv[j];
                        sm[j] += d;
                        sq[j] = __builtin_elementwise_fma(d, d, sq[j]);
                    }
                    T e2[2] = {from_f<T>(x[0]), from_f<T>(x[1])};
                    unsigned u;
                    __builtin_memcpy(&u, e2, 4);
                    wb[t * 32 + j * 8] = u;
                }
            return;
        }
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) {
            const int q = 2 * (r & 1) + qq;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f2 x = {c.acc[i][j][4 * q + 2 * t], c.acc[i][j][4 * q + 2 * t + 1]};
                    x = __builtin_elementwise_fma(x, al2, bva[j]);
                    if (c.has_ra) x = __builtin_elementwise_fma(rav[j], al2, x);
                    if (c.stats) {
                        if (r == 0 && qq == 0 && t == 0) {   // pivot of a column: its first value in the wave (held by the h = 0 lane)
                            const float p0 = __shfl(x[0], l31, 64);
                            pv[j] = f2{p0, p0};
                        }
                        const f2 d = x - pv[j];
                        sm[j] += d;
                        sq[j] = __builtin_elementwise_fma(d, d, sq[j]);
                    }
                    T e2[2] = {from_f<T>(x[0]), from_f<T>(x[1])};
                    unsigned u;
                    __builtin_memcpy(&u, e2, 4);
                    wb[qq * 128 + t * 32 + j * 16] = u;
                }
        }
    };
    const int rp8 = lane >> 3;                                   // reader: row pair of the round, chunk lane & 7
    auto round = [&](auto rc_) {
        constexpr int r = decltype(rc_)::value;
        if constexpr (r < 3) wr(IConst<r + 1>{});
        if constexpr (r == 2) __builtin_amdgcn_s_waitcnt(0x0F70);   // the next tile's first two k-tiles have landed (as slice 4 of the fp32 epilogue)
        const unsigned* rb = win + (r & 1) * 512 + lane * 4;
        const u32x4 t0 = *reinterpret_cast<const u32x4*>(rb);       // columns 8 ec .. +3, rows (2 rp8, 2 rp8 + 1) interleaved
        const u32x4 t1 = *reinterpret_cast<const u32x4*>(rb + 256); // columns 8 ec + 4 .. +7
        u32x4 lo, hi;
        lo[0] = __builtin_amdgcn_perm(t0[1], t0[0], 0x05040100u); hi[0] = __builtin_amdgcn_perm(t0[1], t0[0], 0x07060302u);
        lo[1] = __builtin_amdgcn_perm(t0[3], t0[2], 0x05040100u); hi[1] = __builtin_amdgcn_perm(t0[3], t0[2], 0x07060302u);
        lo[2] = __builtin_amdgcn_perm(t1[1], t1[0], 0x05040100u); hi[2] = __builtin_amdgcn_perm(t1[1], t1[0], 0x07060302u);
        lo[3] = __builtin_amdgcn_perm(t1[3], t1[2], 0x05040100u); hi[3] = __builtin_amdgcn_perm(t1[3], t1[2], 0x07060302u);
        if (c.colok) {
            T* o = out + c.orow + (c.rows.rofs(16 * r) + rp8) * p.ldo;   // orow is row `rp8` of the wave's block: + rp8 more rows = row 2 rp8 of round r
            *reinterpret_cast<u32x4*>(o) = lo;
            *reinterpret_cast<u32x4*>(o + p.ldo) = hi;
        }
    };
    wr(IConst<0>{});
    round(IConst<0>{}); round(IConst<1>{}); round(IConst<2>{}); round(IConst<3>{});
    if (c.stats) {   // uniform: per column totals = both halves of the pair accumulators + the other lanes of the column (32x32: the other half-wave; M16: the four
        // lanes lane & 15, a fixed butterfly); the lanes that own the block's row 0 deposit their NJ columns
        float* dep = reinterpret_cast<float*>(c.smem + DEP);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float su = sm[j][0] + sm[j][1], s2 = sq[j][0] + sq[j][1];
            if constexpr (M16) {
                su += __shfl_xor(su, 16, 64);
                s2 += __shfl_xor(s2, 16, 64);
            }
            su += __shfl_xor(su, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (M16 ? lane < 16 : h == 0) {
                float* d3 = dep + (c.wave * 64 + (M16 ? 16 * j + lane : 32 * j + l31)) * 3;
                d3[0] = su; d3[1] = s2; d3[2] = pv[j][0];
            }
        }
    }
}

// ---- the row-wise (fp32-window) epilogues: eight slices of eight rows per wave, two 2-KiB slice windows — slice s + 1 is written while slice s is read back row-wise.
// (Opened by the barrier embedded in the last k-tile: every wave is done reading that k-tile, its stage is scratch now.)  M16: all lanes write every slice when slice
// s = rows 4 q + 2 (s & 1) + e (q = 0 .. 3, e = 0, 1) of the 16-row block s >> 1: window row 2 q + e, so the reader of window row `er` holds row
// 4 (er >> 1) + (er & 1) + epi_srow(s) of the wave's block (orow / rrow are that row's).
// slice S of the accumulators into its window
template <bool M16, int S, typename Acc>
__device__ __forceinline__ void epi_window_write(float* win, const int wofs, const Acc& acc) {
    float* wb = win + (S & 1) * 512 + wofs;
    if constexpr (M16) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 2; ++e) wb[e * 32 + j * 8] = acc[S >> 1][j][2 * (S & 1) + e];
    } else {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) wb[e * 32 + j * 16] = acc[S >> 2][j][4 * (S & 3) + e];
    }
}
// statistics of a slice's row: shifted sums about the pivot — the wave's first row (first = slice 0), broadcast down the eight row-lanes of every chunk
__device__ __forceinline__ void epi_stats_row(const f2 (&x2)[4], const bool first, const int ec, f2 (&pv2)[4], f2 (&sm2)[4], f2 (&sq2)[4]) {
    if (first) {
#pragma unroll
        for (int q = 0; q < 4; ++q) pv2[q] = f2{__shfl(x2[q][0], ec, 64), __shfl(x2[q][1], ec, 64)};
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f2 d = x2[q] - pv2[q];
        sm2[q] += d;
        sq2[q] = __builtin_elementwise_fma(d, d, sq2[q]);
    }
}
// statistics of the row-wise epilogues, after the last slice: 16 values (8 sums, 8 sums of squares) over the 8 row-lanes of a chunk — a reduce-scatter butterfly,
// each step a lane hands half of its values to its partner and adds the partner's other half (14 exchanges instead of 48) — and the deposits (sum, sum of squares,
// pivot) per column of the wave at LDS offset DEP
template <int DEP>
__device__ __forceinline__ void epi_deposit_rowwise(char* smem, const int wave, const int er, const int ec, const f2 (&sm2)[4], const f2 (&sq2)[4], const f2 (&pv2)[4]) {
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) { v[2 * q] = sm2[q][0]; v[2 * q + 1] = sm2[q][1]; v[8 + 2 * q] = sq2[q][0]; v[8 + 2 * q + 1] = sq2[q][1]; }
    const bool b0 = (er & 1) != 0, b1 = (er & 2) != 0, b2 = (er & 4) != 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float keep = b0 ? v[k + 8] : v[k], send = b0 ? v[k] : v[k + 8];
        v[k] = keep + __shfl_xor(send, 8, 64);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float keep = b1 ? v[k + 4] : v[k], send = b1 ? v[k] : v[k + 4];
        v[k] = keep + __shfl_xor(send, 16, 64);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float keep = b2 ? v[k + 2] : v[k], send = b2 ? v[k] : v[k + 2];
        v[k] = keep + __shfl_xor(send, 32, 64);
    }
    // this lane now holds statistic (er & 1) of columns e0, e0 + 1 of its chunk, e0 = 4 * bit1 + 2 * bit2
    const int e0 = ((er >> 1) & 1) * 4 + (er >> 2) * 2;
    float pva[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) pva[e] = pv2[e >> 1][e & 1];
    const float pe0 = b1 ? (b2 ? pva[6] : pva[4]) : (b2 ? pva[2] : pva[0]);
    const float pe1 = b1 ? (b2 ? pva[7] : pva[5]) : (b2 ? pva[3] : pva[1]);
    // (sum or sum of squares at + b0; the b0 = 0 lanes add the pivots: one address serves both)
    float* d3 = reinterpret_cast<float*>(smem + DEP) + (wave * 64 + ec * 8 + e0) * 3 + (int)b0;
    d3[0] = v[0];
    d3[3] = v[1];
    if (!b0) { d3[2] = pe0; d3[5] = pe1; }
}

// 16-bit launches with a residual: out = alpha * (acc + bias + rowadd[img]) + residual.  The residual rows of slices 0-3, the bias and the rowadd chunk arrive in c.ops
// (requested inside the k-loop), the rows of slices 4-7 are requested at slice 0.  rrow: element offset of this lane's residual row of slice 0 (with the batch offset)
template <int DEP, typename Ctx, typename Stamp = NoStamp>
__device__ __forceinline__ void epilogue(const Ctx& c, const int sfree, const long zoff_o, const long rrow, const Stamp& stamp = Stamp{}) {
    using T = typename Ctx::T;
    constexpr bool M16 = Ctx::M16;
    const IgemmParams& p = c.p;
    const int lane = c.lane, ec = c.ec;
    float* win = reinterpret_cast<float*>(c.smem + sfree + c.wave * 4096);
    const int wofs = epi_wofs<M16>(lane, c.l31, c.h, 128);      // in floats; + e * 32 + j * 16 (M16: + e * 32 + j * 8)
    const float al = p.alpha;
    T* __restrict__ out = (T*)p.out + zoff_o;
    const T* __restrict__ res = (const T*)p.residual;
    f2 bva2[4], ra2[4], pv2[4], sm2[4], sq2[4];
    const f2 al2 = {al, al};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        bva2[q] = c.bias ? f2{to_f(c.ops.bias.e[2 * q]) * al, to_f(c.ops.bias.e[2 * q + 1]) * al} : f2{0.f, 0.f};
        ra2[q] = c.has_ra ? f2{to_f(c.ops.ra.e[2 * q]), to_f(c.ops.ra.e[2 * q + 1])} : f2{0.f, 0.f};
        pv2[q] = f2{0.f, 0.f}; sm2[q] = f2{0.f, 0.f}; sq2[q] = f2{0.f, 0.f};
    }
    Vec16<T> late_res[4];
    auto slice = [&](auto sc_) {
        constexpr int s = decltype(sc_)::value;
        if constexpr (s == 0) {   // residual rows of slices 4-7: consumed four slices from now
#pragma unroll
            for (int t = 0; t < 4; ++t) late_res[t] = ld16(res + rrow + c.rows.rofs(epi_srow<M16>(4 + t)) * p.ldr);
        }
        if constexpr (s < 7) epi_window_write<M16, s + 1>(win, wofs, c.acc);
        // the next tile's first two k-tiles (issued >= 1 k-tile + 4 slices ago) have landed.  The BUILTIN, not inline asm: the compiler's
        // waitcnt pass then knows that nothing is pending and does not drain again in front of later register / LDS reuse
        if constexpr (s == 4) __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), expcnt / lgkmcnt untouched
        const float* rb = win + (s & 1) * 512 + lane * 4;
        const floatx4 t0 = *reinterpret_cast<const floatx4*>(rb);
        const floatx4 t1 = *reinterpret_cast<const floatx4*>(rb + 256);
        f2 x2[4] = {f2{t0[0], t0[1]}, f2{t0[2], t0[3]}, f2{t1[0], t1[1]}, f2{t1[2], t1[3]}};
#pragma unroll
        for (int q = 0; q < 4; ++q) x2[q] = __builtin_elementwise_fma(x2[q], al2, bva2[q]);
        if (c.has_ra) {
#pragma unroll
            for (int q = 0; q < 4; ++q) x2[q] = __builtin_elementwise_fma(ra2[q], al2, x2[q]);
        }
        const Vec16<T>& rv = s < 4 ? c.ops.res[s & 3] : late_res[s & 3];
#pragma unroll
        for (int q = 0; q < 4; ++q) x2[q] += f2{to_f(rv.e[2 * q]), to_f(rv.e[2 * q + 1])};
        Vec16<T> o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.e[e] = from_f<T>(x2[e >> 1][e & 1]);
        if (c.colok) st16(out + c.orow + c.rows.rofs(epi_srow<M16>(s)) * p.ldo, o);
        if (c.stats) epi_stats_row(x2, s == 0, ec, pv2, sm2, sq2);
    };
    epi_window_write<M16, 0>(win, wofs, c.acc);
    slice(IConst<0>{});
    stamp(5);
    slice(IConst<1>{}); slice(IConst<2>{}); slice(IConst<3>{});
    stamp(6);
    slice(IConst<4>{}); slice(IConst<5>{}); slice(IConst<6>{}); slice(IConst<7>{});
    if (c.stats) epi_deposit_rowwise<DEP>(c.smem, c.wave, c.er, ec, sm2, sq2, pv2);   // uniform
}

// fp32 bias / residual / output (csrc/f32split.hip; the 32x32 layout only): out = acc * al + bias + residual, al = alpha / (activation split scale).  A lane's 8-column
// chunk of a row is two 16-byte units; bias and the residual rows of slices 0-3 are requested on entry (the staging of slice 0 covers their latency), slices 4-7 behind
// slice 3.  Slice s handles this lane's row 8 s of the wave's block: it exists while 8 s < rows_left (ragged last tile of igemm5).  Statistics as the 16-bit epilogue
// (of the fp32 values that are stored).  ncl: first column of the lane's chunk
template <int DEP, typename Ctx>
__device__ __forceinline__ void epilogue_f32(const Ctx& c, const int sfree, const float al_f32, const long rrow, const int ncl) {
    static_assert(!Ctx::M16, "the fp32-output variants exist in the 32x32 layout only");
    const IgemmParams& p = c.p;
    const int lane = c.lane, er = c.er, ec = c.ec;
    float* win = reinterpret_cast<float*>(c.smem + sfree + c.wave * 4096);
    const int wofs = epi_wofs<false>(lane, c.l31, c.h, 128);
    float* __restrict__ out = (float*)p.out;
    const float* __restrict__ res = (const float*)p.residual;
    const float* __restrict__ bias32 = (const float*)p.bias;
    const bool hres = res != nullptr;
    const int rows_left = c.rows.rows_left(er);
    const f2 al2 = {al_f32, al_f32};
    f2 bv2[4], pv2[4], sm2[4], sq2[4];
    {
        floatx4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
        if (bias32) { b0 = *reinterpret_cast<const floatx4*>(bias32 + ncl); b1 = *reinterpret_cast<const floatx4*>(bias32 + ncl + 4); }
        bv2[0] = f2{b0[0], b0[1]}; bv2[1] = f2{b0[2], b0[3]}; bv2[2] = f2{b1[0], b1[1]}; bv2[3] = f2{b1[2], b1[3]};
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { pv2[q] = f2{0.f, 0.f}; sm2[q] = f2{0.f, 0.f}; sq2[q] = f2{0.f, 0.f}; }
    floatx4 rr[4][2];
    auto req = [&](const int s0) {
        if (hres) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float* r = res + rrow + c.rows.rofs((s0 + t) * 8) * p.ldr;
                if ((s0 + t) * 8 < rows_left) {
                    rr[t][0] = *reinterpret_cast<const floatx4*>(r);
                    rr[t][1] = *reinterpret_cast<const floatx4*>(r + 4);
                }
            }
        }
    };
    auto slice = [&](auto sc_) {
        constexpr int s = decltype(sc_)::value;
        if constexpr (s < 7) epi_window_write<false, s + 1>(win, wofs, c.acc);
        if constexpr (s == 4) __builtin_amdgcn_s_waitcnt(0x0F70);   // (as the 16-bit epilogue: the next tile's first pieces have landed; also the residual rows)
        const float* rb = win + (s & 1) * 512 + lane * 4;
        const floatx4 t0 = *reinterpret_cast<const floatx4*>(rb);
        const floatx4 t1 = *reinterpret_cast<const floatx4*>(rb + 256);
        f2 x2[4] = {f2{t0[0], t0[1]}, f2{t0[2], t0[3]}, f2{t1[0], t1[1]}, f2{t1[2], t1[3]}};
#pragma unroll
        for (int q = 0; q < 4; ++q) x2[q] = __builtin_elementwise_fma(x2[q], al2, bv2[q]);
        if (hres) {
            const floatx4 r0 = rr[s & 3][0], r1 = rr[s & 3][1];
            x2[0] += f2{r0[0], r0[1]}; x2[1] += f2{r0[2], r0[3]}; x2[2] += f2{r1[0], r1[1]}; x2[3] += f2{r1[2], r1[3]};
        }
        if (c.colok && s * 8 < rows_left) {
            float* o = out + c.orow + c.rows.rofs(s * 8) * p.ldo;
            *reinterpret_cast<floatx4*>(o) = floatx4{x2[0][0], x2[0][1], x2[1][0], x2[1][1]};
            *reinterpret_cast<floatx4*>(o + 4) = floatx4{x2[2][0], x2[2][1], x2[3][0], x2[3][1]};
        }
        if constexpr (s == 3) req(4);      // (rr is free: slice 3 was its last reader)
        if (c.stats) epi_stats_row(x2, s == 0, ec, pv2, sm2, sq2);
    };
    req(0);
    epi_window_write<false, 0>(win, wofs, c.acc);
    slice(IConst<0>{}); slice(IConst<1>{}); slice(IConst<2>{}); slice(IConst<3>{});
    slice(IConst<4>{}); slice(IConst<5>{}); slice(IConst<6>{}); slice(IConst<7>{});
    if (c.stats) epi_deposit_rowwise<DEP>(c.smem, c.wave, c.er, ec, sm2, sq2, pv2);   // uniform
}

// merge of the four row-waves' deposits (at `dep`) of the tile at column n0, one thread per column (after a barrier that follows the deposits)
__device__ __forceinline__ void combine(const IgemmParams& p, const float* dep, const int tid, const int bn, const int img, const int slab, const int n0) {
    if (tid < bn && n0 + tid < p.N) {
        const int cw = tid >> 6, cc = tid & 63;
        GnTriple t = {0.f, 0.f, 0.f};
#pragma unroll
        for (int w4 = 0; w4 < 4; ++w4) {
            const float* d3 = dep + ((w4 * 2 + cw) * 64 + cc) * 3;
            gn_add_pivot_sums(t, 64.f, d3[0], d3[1], d3[2]);
        }
        float* o = p.gn_partial + (((long)img * (p.gn_islabs > 0 ? p.gn_islabs : p.gn_nslabs) + slab) * p.N + n0 + tid) * 3;
        o[0] = t.n; o[1] = t.mean; o[2] = t.m2;
    }
}

}  // namespace e2eft
