// attn32.h — what the two fp32 routes of the d = 64 fused attention share (attn32.hip: v_mfma_f32_32x32x2_f32; attn_f32split.hip: two-term f16 splits on
// v_mfma_f32_32x32x16_f16): the parameter blocks, the argument checks that fill them, and the D = rowsum(dO o O) pass of the backward.  Defined in attn32.hip.
#pragma once
#include "common.h"

namespace e2eft {

struct Attn32Params {
    const float* q;
    const float* k;
    const float* v;
    float* out;
    int batch, heads, nq, nk_seg, kv_nseg, kv_bmod, nk_total, nqb;
    int ldq, ldk, ldv, ldo;
    float c;        // scale * log2(e)
    float* lse;     // optional [batch][heads][nq]: base-2 log-sum-exp of the scaled scores
};

struct Attn32BwdParams {
    const float* q;
    const float* k;
    const float* v;
    const float* dout;
    const float* lse;
    const float* dsum;
    float* dq;
    float* dk;
    float* dv;
    int batch, heads, nq, nk;
    int ldq, ldk, ldv, lddo, lddq, lddk, lddv;
    float c, scale;
};

// stride / alignment / grid checks of the fp32 forward and backward (E2EFT_ERR_BAD_ARG with a message on failure) and the filled parameter block
int attn32_fwd_params(const E2eftAttnDesc* d, const void* q, const void* k, const void* v, void* out, float* lse, Attn32Params* p);
int attn32_bwd_params(const E2eftAttnDesc* d, const void* q, const void* k, const void* v, const void* out, const void* dout, int32_t lddo, const float* lse,
                      void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv, int32_t lddv, void* workspace, Attn32BwdParams* p);
// enqueue D[b][h][q] = sum_d dO[b, q, h, d] O[b, q, h, d] into dsum (= the backward's workspace)
void attn32_bwd_prep(const E2eftAttnDesc* d, const void* out, const void* dout, int32_t lddo, float* dsum, hipStream_t s);

}  // namespace e2eft
