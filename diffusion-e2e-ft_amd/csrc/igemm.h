// igemm.h — parameter block, stamp macros, planner and launcher declarations of the implicit-GEMM kernel variants (their epilogues: igemm_epilogue.h).
#pragma once
#include "gfx950.h"

namespace e2eft {

// -DE2EFT_STAMPS (build.py build_stamps(): lib/libe2eft_stamps.so, scripts/stamp_bench.py): thread 0 of every workgroup records the
// shader clock at the phase boundaries of igemm2_kernel — start, k-loop entry, k-loop exit, accumulators staged, end.
#ifdef E2EFT_STAMPS
static __device__ long long g_stamps[65536 * 8];
static __device__ long long g_stamps_rt[65536 * 2];   // the constant 100 MHz counter (s_memrealtime) at stamps 0 and 4: shader clock = cycles / ticks * 100 MHz
#define E2EFT_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < 65536) { g_stamps[blockIdx.x * 8 + (i)] = __builtin_readcyclecounter(); \
    if ((i) == 0 || (i) == 4) g_stamps_rt[blockIdx.x * 2 + ((i) >> 2)] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define E2EFT_STAMP(i) do { } while (0)
#endif

struct IgemmParams {
    const void* x1;
    const void* x2;
    const void* w;
    const void* bias;
    const void* rowadd;
    const void* residual;
    void* out;
    int M, N, K;
    int ldx1, ldx2, c1, cin;
    int hin, win, hl, wl, kh, kw, stride, pad_t, pad_l, hout, wout;
    float up_sh, up_sw;
    int zins;            // > 1: the source is read through a zero-insertion grid (dgrad of a strided conv): logical (y, x) is
                         // source (y / zins, x / zins) when both are multiples of zins and zero otherwise
    int ldw, ldr, ldo;
    int bias_along_m;
    int rows_per_img;
    float alpha;
    int nzi;
    long sa_o, sa_i, sw_o, sw_i, so_o, so_i, sr_o, sr_i;
    int mtiles, ntiles;
    float* gn_partial;   // optional: [img][gn_nslabs][N][3] (n, mean, M2) GroupNorm partials of the output.  Every epilogue that emits them (igemm_epilogue.h: the full-tile
                         // path of igemm_epilogue_rows, the persistent kernels' epilogues) takes them from the fp32 value BEFORE it is rounded to the output
                         // type; the hosts keep gn_partial for full, vector-aligned tiles only.  tests/gn_stats_model.py: TARGET
    int gn_nslabs;       // row slabs (one per M-tile) per image
    int ksplit_taps;     // conv split-K: batch index zi covers filter taps [zi * ksplit_taps, (zi + 1) * ksplit_taps) (0 = whole K)
    const float* nrm_ad; // optional (igemm6 only): the A operand is read through GroupNorm(+SiLU): [image][cin][2] fp32 (a, mean) pairs of e2eft_groupnorm_fwd_stats ...
    const void* nrm_beta; // ... and the norm's beta [cin] (or null): value = (x - mean) * a + beta, then SiLU if nrm_silu
    int nrm_silu;
    int out_seg;         // > 0 (igemm5 only, e2eft_upconv2x_fwd): the output rows are laid out in SEGMENTS of out_seg consecutive GEMM rows, segment g starting
                         // 2 * out_seg pixel rows (of ldo elements) after segment g - 1: output row of GEMM row m = m + (m / out_seg) * out_seg.  That is one
                         // parity phase of a 2x-upsampled image: GEMM rows = low-resolution pixels (b, Y, X), out_seg = W, ldo = 2 * (pixel stride of the full
                         // image), so consecutive X land on every other pixel and consecutive Y on every other row.  Multiple of 16.
    int gn_islabs;       // > 0: statistics slabs per image in gn_partial (the image stride), when it differs from gn_nslabs (four phases share one buffer)
    // round 6 (igemm6 only, e2eft_conv2d_fwd_f32split): an fp32 convolution on the f16 matrix pipe.  The A operand is the two-term f16 split of an fp32 tensor,
    // planes [x0 | x1] side by side in one pixel (x * s = x0 + x1 to 22 bits, s a power of two); K runs over THREE blocks of split_c channels per tap — (x0, w0), (x0, w1),
    // (x1, w0) — so chunk channel ch reads plane channel ch - split_c once ch >= split_c; the weights arrive laid out that way.  Bias / residual / output are fp32:
    // out = acc * (alpha * *alpha_dev) + bias + residual   (alpha_dev: device scalar 1 / s of the activation split; alpha carries 1 / s_w and the caller's factor)
    int split_c;         // > 0: channels of one plane (cin = 3 * split_c)
    const float* alpha_dev;
    const float* alpha_dev2;   // a second optional device factor (1 / s_w of weights that were split on the device)
    int debug_flags;     // instrumented build (-DE2EFT_STAMPS) only: bit 0 / 1 / 2 = the persistent kernel issues its A-operand LDS-DMA never / on the
                         // first tap of a filter row only / on the first tap of a 64-channel chunk only (WRONG results; the price of operand
                         // delivery: profiles/r03d_a_operand_delivery_probe.txt, "what an A-reuse scheme could buy at most")
};

// ---- host side: one planner for the family (definitions and the dispatch order: igemm.hip) ---------------------------------------------------------------
// Eligibility tests READ the parameter block and fill a TilePlan; only the launcher that takes the launch applies the plan to the block it launches.
struct TilePlan { int grid; long total; int mtiles, ntiles, gn_nslabs; };
inline void apply_plan(IgemmParams& p, const TilePlan& t) {
    p.mtiles = t.mtiles;
    p.ntiles = t.ntiles;
    if (p.gn_partial) p.gn_nslabs = t.gn_nslabs;
}
// workgroups of a persistent launch: the CUs of the current device, or the grid option when that is smaller (tests: a small grid sends small problems through
// the persistent kernels); 0 = no device.  The only reader of that option outside api.hip.
int persistent_grid();
// the common tail of the persistent kernels' tests: bm x bn tiles on `grid` workgroups, at least min_tiles4 / 4 of them (the caller's bar), tile and row indices within
// the kernels' float-reciprocal splits (quotients below 2^22), one statistics slab per M tile
bool plan_tiles(const IgemmParams& p, int nz, int bm, int bn, int grid, long min_tiles4, TilePlan& t);
// the 16-bit vector epilogues of the persistent kernels (igemm_epilogue.h): whole 16-byte units of output, residual and bias
inline bool vec_epilogue_ok(const IgemmParams& p) {
    return p.N % 8 == 0 && p.ldo % 8 == 0 && al16(p.out) && (!p.residual || (p.ldr % 8 == 0 && al16(p.residual))) && (!p.bias || al16(p.bias));
}
// FAST operand path (LDS-DMA through whole_range_rsrc, es = element size): do all valid offsets stay inside the descriptor?  The 256 rows of a convolution's tile may
// lie in several images, all addressed from the first one's base.
inline bool conv_window_in_range(long hin, long win, long ldx, long rows_per_img, long es) { return hin * win * ldx * es * (256 / rows_per_img + 2) < SRD_SPAN_MAX; }
inline bool fast_operands_in_range(int mode, const IgemmParams& p, long es) {
    if (128L * p.ldw * es >= SRD_TILE_MAX) return false;
    return mode == 0 ? 256L * p.ldx1 * es < SRD_TILE_MAX : conv_window_in_range(p.hin, p.win, p.ldx1 > p.ldx2 ? p.ldx1 : p.ldx2, (long)p.hout * p.wout, es);
}

// v2: 256x128 tile, 8 waves, LDS-DMA (global_load_lds) 3-stage ring — igemm2.hip
int launch_igemm_v2(int dtype, int mode, IgemmParams& p, int nz, hipStream_t s);
// igemm5.hip: persistent workgroups walking a tile sequence (16-bit FAST path, M % 256 == 0, >= 2 tiles per CU); -1 when not eligible
int launch_igemm_persistent(int dtype, int mode, IgemmParams& p, int nz, hipStream_t s);
bool igemm_persistent_eligible(int dtype, int mode, const IgemmParams& p, int nz, TilePlan& t);   // its host-side test alone: pure arithmetic
// igemm6.hip: persistent, the A operand of a 3x3 / stride-1 / pad-1 convolution as a 2-D halo patch in LDS; -1 when not eligible
int launch_igemm_patch(int dtype, int mode, IgemmParams& p, int nz, hipStream_t s);
bool igemm_patch_eligible(int dtype, int mode, const IgemmParams& p, int nz, TilePlan& t);
// convin.hip: 3x3 / stride-1 / pad-1 convolutions with eight input channels (operands straight from global memory, persistent); -1 when not eligible
int launch_conv_thin_in(int dtype, int mode, IgemmParams& p, int nz, hipStream_t s);
// the persistent family in its one order — halo patch, else persistent tiles (a fused normalisation exists on the patch kernel alone); -1 when neither takes the launch
int launch_persistent_family(int dtype, int mode, IgemmParams& p, int nz, hipStream_t s);
// ... and its const twin: would the family take this geometry with 16-byte aligned operands (normed: read through a fused GroupNorm)?
bool persistent_family_eligible(int dtype, int mode, const IgemmParams& geometry, int nz, bool normed = false);

// E2eftConvDesc -> the geometry of its implicit GEMM (no pointers); phase ph of a 2x-upsampler convolution as the 2x2 convolution of e2eft_upconv2x_fwd (split = 3: the
// operands are f16 split planes of an fp32 tensor, three K blocks per tap)
IgemmParams conv_params(const E2eftConvDesc* d);
IgemmParams upconv2x_phase_params(const E2eftConvDesc* d, int ph, int split);
// the four phases of one upsampler convolution.  io carries x1, w (all four phase weights), bias, out (the full-resolution image), alpha_dev / alpha_dev2 and gn_partial
// (null: no statistics); persistent = false sends the phases to igemm2.  `who` opens the error messages.
int run_upconv2x_phases(const E2eftConvDesc* d, int dtype, int split, const IgemmParams& io, bool persistent, int32_t* slab_rows, const char* who, hipStream_t s);
// the GroupNorm statistics buffer [images][128-row slabs][n][3] fp32: E2EFT_OK, or E2EFT_ERR_WORKSPACE when `have` bytes do not hold it
int check_gn_partial(const char* who, size_t have, long images, long rows_per_img, long n);

}  // namespace e2eft
