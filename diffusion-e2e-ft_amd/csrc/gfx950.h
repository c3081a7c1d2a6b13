// gfx950.h — the hardware primitives the matrix-pipe / LDS-DMA kernels share: ONE definition each, so that a hardware finding (a wait state, an operand
// swizzle) is applied in one place.  Wrappers and address helpers only — no kernel logic; the elementwise files have no use for it and common.h does not include it.
#pragma once
#include "common.h"
#include <type_traits>

namespace e2eft {

template <int V> using IConst = std::integral_constant<int, V>;      // a compile-time int as a lambda argument (static stage / piece / slice indices)

// ---- v_mfma_f32_32x32x16_{f16,bf16}: A and B are 8 sixteen-bit k-slots per lane in four dwords, C / D 16 fp32 per lane.
template <typename T> struct Mma32x32x16;
template <> struct Mma32x32x16<f16> {
    __device__ static __forceinline__ floatx16 run(const u32x4& a, const u32x4& b, floatx16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
    }
};
template <> struct Mma32x32x16<bf16> {
    __device__ static __forceinline__ floatx16 run(const u32x4& a, const u32x4& b, floatx16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bhalf8, a), __builtin_bit_cast(bhalf8, b), c, 0, 0, 0);
    }
};

// ---- v_mfma_f32_16x16x32_{f16,bf16}: A and B as above (lane = row / column lane & 15, k-slots 8 (lane >> 4) .. + 7), C / D 4 fp32 per lane: column lane & 15,
// rows 4 (lane >> 4) + register.  Same flops per matrix-pipe cycle as the 32x32x16 form; it holds the SIMD's vector issue for 8 of its 16 cycles.
template <typename T> struct Mma16x16x32;
template <> struct Mma16x16x32<f16> {
    __device__ static __forceinline__ floatx4 run(const u32x4& a, const u32x4& b, floatx4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
    }
};
template <> struct Mma16x16x32<bf16> {
    __device__ static __forceinline__ floatx4 run(const u32x4& a, const u32x4& b, floatx4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bhalf8, a), __builtin_bit_cast(bhalf8, b), c, 0, 0, 0);
    }
};

// ---- two fp32 -> one dword of T with a single v_cvt_pk_{f16,bf16}_f32 (lo in bits 0-15)
typedef float float2v __attribute__((ext_vector_type(2)));
typedef __bf16 bhalf2v __attribute__((ext_vector_type(2)));
template <typename T> __device__ __forceinline__ uint32_t pack2(float lo, float hi);
template <> __device__ __forceinline__ uint32_t pack2<f16>(float lo, float hi) {
    const float2v f = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, half2v));
}
template <> __device__ __forceinline__ uint32_t pack2<bf16>(float lo, float hi) {
    const float2v f = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bhalf2v));
}

// ---- n / d for 0 <= n < 2^31, d >= 1 with a quotient below 2^22 (rows / image size, pixels / row length, tiles / tiles per row): float estimate
// (relative error ~2^-22, so off by at most one) + one correction — 8 instructions instead of the ~25 of the generic unsigned division, eight of
// which sit in front of the first DMA of every workgroup.
__device__ __forceinline__ int fast_div(int n, int d) {
    int q = (int)((float)n * __builtin_amdgcn_rcpf((float)d));
    const int r = n - q * d;
    if (r < 0) --q;
    else if (r >= d) ++q;
    return q;
}

// ---- LDS
typedef __attribute__((address_space(3))) void* lds_ptr_t;      // (unsigned)(uintptr_t)(lds_ptr_t)smem = the LDS byte address m0 / the DMA builtin take

// ds_read_b64_tr_b16: lane i of a 16-lane group supplies the address of 4 consecutive 16-bit elements (row i >> 2, columns 4 (i & 3) .. + 3 of a
// 4 x 16 block) and receives column i of the block, rows 0 .. 3 — a tile stays row-major in LDS and is transposed on the way to the MFMA's A operand
__device__ __forceinline__ u32x2 lds_read_tr16(const char* p) {
    typedef short short4v __attribute__((ext_vector_type(4)));
    return __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) short4v*)p));
}

// ---- buffer descriptors for LDS-DMA.  One descriptor spans "everything above the base": SRD_RECORDS bytes, raw addressing (flags 0x00020000); a lane that
// must fetch zeros (padding, ragged edge) passes the byte offset SRD_OOB, beyond the records, and the buffer bounds check writes zeros.  Launchers take these
// kernels only when every valid offset stays below SRD_RECORDS.  (wgrad.hip and attn512.hip build exact-range descriptors of their own: there the range
// check itself does the masking.)
constexpr unsigned int SRD_RECORDS = 0xE0000000u;
constexpr unsigned int SRD_OOB = 0xF0000000u;
// what the launchers hold the kernels' offsets to (host side): everything one descriptor addresses from its base — the images a tile's rows may touch —
// below SRD_SPAN_MAX, and the rows of one tile, whose offsets are formed in 32 bits before the k-loop advances them, below SRD_TILE_MAX
constexpr long SRD_SPAN_MAX = 0xD0000000L, SRD_TILE_MAX = 0x40000000L;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t whole_range_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, SRD_RECORDS, 0x00020000);
}

// One LDS-DMA piece (64 lanes x 16 B -> 1 KiB at LDS byte address lds_addr, wave-uniform; lane l lands at lds_addr + 16 l), issued from asm.
// Two forms of the same instruction are in use, on purpose:
//  * igemm2 / igemm5 / igemm6 call __builtin_amdgcn_raw_ptr_buffer_load_lds: the compiler counts those pieces and the kernels' counted
//    `s_waitcnt vmcnt(N)` agree with its bookkeeping;
//  * attn (DMA kernel), attn512 and wgrad use THIS asm form: the compiler's waitcnt pass drains vmcnt(0) in front of every LDS read it cannot prove
//    disjoint from a pending LDS-DMA it knows of — what it does not see it does not wait for; these kernels count their own pieces.
// "s_nop 0": m0 written by SALU -> LDS-DMA needs one wait state, and inside an asm statement nobody pads.  m0 is compiler-reserved: saved and restored.
// `volatile` + "memory" keep the piece where the source puts it; the scalar temporary is early-clobber (it is written before %3 is read).
// The offset that makes a lane fetch zeros belongs to the DESCRIPTOR, not to the piece: SRD_OOB with whole_range_rsrc, 0xFFFFFFF0 with the exact-range
// descriptors of wgrad.hip and attn512.hip (any offset beyond their records) — these are different on purpose.
__device__ __forceinline__ void lds_dma_piece(const __amdgpu_buffer_rsrc_t& rs, const unsigned voff, const unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(rs), "s"(lds_addr) : "memory");
}

// ---- XCD-aware map of a 1-D grid of nqb * heads * batch workgroups -> (image, head, query block): pair = (image, head); pairs are dealt to the eight
// XCDs round-robin (block id mod 8 = XCD), each XCD walks its pairs' query blocks — so all query blocks of one pair run on ONE XCD and the head's K / V
// (2.4 MB at 9216 keys) is fetched into one L2 instead of eight: PMC had 3.5x the algorithmic HBM bytes with the plain map.
__device__ __forceinline__ void xcd_pair_block_map(const int batch, const int heads, const int nqb, int& b, int& head, int& qblk) {
    const int npair = batch * heads;
    const int L = blockIdx.x, full = (npair >> 3) << 3;          // pairs covered by complete rounds of eight
    if (L < full * nqb) {
        const int xcd = L & 7, idx = L >> 3;
        const int pr = (idx / nqb) * 8 + xcd;
        qblk = idx - (idx / nqb) * nqb;
        b = pr / heads; head = pr - b * heads;
    } else {                                                      // the remaining (< 8) pairs: plain order
        const int r = L - full * nqb;
        const int pr = full + r / nqb;
        qblk = r - (r / nqb) * nqb;
        b = pr / heads; head = pr - b * heads;
    }
}

}  // namespace e2eft
