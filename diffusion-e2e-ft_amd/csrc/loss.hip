// loss.hip — E2E-FT task losses (forward), fp32 I/O with fp64 reductions.
//   ScaleAndShiftInvariantLoss  — /root/reference/training/util/loss.py:13-47
//   AngularLoss                 — /root/reference/training/util/loss.py:51-67
#include "common.h"

namespace e2eft {

// pass 1: per-image masked sums a00=sum m p^2, a01=sum m p, a11=sum m, b0=sum m p t, b1=sum m t   (loss.py:33-38)
__global__ __launch_bounds__(256) void ssi_sums_kernel(int hw, const float* __restrict__ pred, const float* __restrict__ tgt,
                                                       const uint8_t* __restrict__ mask, double* __restrict__ part /* [B][nb][5] */) {
    const int b = blockIdx.y;
    const float* p = pred + (long)b * hw;
    const float* t = tgt + (long)b * hw;
    const uint8_t* m = mask + (long)b * hw;
    double v[5] = {0, 0, 0, 0, 0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
        if (m[i]) {
            const double pp = p[i], tt = t[i];
            v[0] += pp * pp; v[1] += pp; v[2] += 1.0; v[3] += pp * tt; v[4] += tt;
        }
    }
    block_sums<5>(v, part + ((long)b * gridDim.x + blockIdx.x) * 5);
}

// per image: the nb partials summed in index order -> sums[b][5] (the backward reads them), then the 2x2 system in fp32 exactly as loss.py:39-46
// (det > 0 guard, zeros otherwise)
__global__ void ssi_solve_kernel(int batch, int nb, const double* __restrict__ part, double* __restrict__ sums /* [B][5] */, float* __restrict__ ss /* [B][2] */) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double t[5] = {0, 0, 0, 0, 0};
#pragma unroll 4
    for (int k = 0; k < nb; ++k)
        for (int i = 0; i < 5; ++i) t[i] += part[((long)b * nb + k) * 5 + i];
    for (int i = 0; i < 5; ++i) sums[b * 5 + i] = t[i];
    const float a00 = (float)t[0], a01 = (float)t[1], a11 = (float)t[2], b0 = (float)t[3], b1 = (float)t[4];
    const float det = a00 * a11 - a01 * a01;
    float x0 = 0.f, x1 = 0.f;
    if (det > 0.f) {
        x0 = (a11 * b0 - a01 * b1) / det;
        x1 = (-a01 * b0 + a00 * b1) / det;
    }
    ss[b * 2] = x0;
    ss[b * 2 + 1] = x1;
}

// pass 2: sum over valid pixels of |scale_b p + shift_b - t| and the valid count (loss.py:26-28)
__global__ __launch_bounds__(256) void ssi_l1_kernel(int hw, const float* __restrict__ pred, const float* __restrict__ tgt,
                                                     const uint8_t* __restrict__ mask, const float* __restrict__ ss,
                                                     double* __restrict__ part /* [B * nb][2] */) {
    const int b = blockIdx.y;
    const float sc = ss[b * 2], sh = ss[b * 2 + 1];
    const float* p = pred + (long)b * hw;
    const float* t = tgt + (long)b * hw;
    const uint8_t* m = mask + (long)b * hw;
    double v[2] = {0, 0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
        if (m[i]) {
            v[0] += (double)fabsf(sc * p[i] + sh - t[i]);
            v[1] += 1.0;
        }
    }
    block_sums<2>(v, part + ((long)b * gridDim.x + blockIdx.x) * 2);
}

// mean over the valid pixels.  No valid pixel -> 0 (the reference skips the loss term: `if val_mask.any()`, training/train.py:504);
// a NaN sum -> 0 as well (`if not torch.isnan(...)`, train.py:548,552): the term contributes neither loss nor gradient (bwd.hip).
// One block: thread t adds partials t, t + 256, ... in order, block_sums gives acc[0..1] (sum, valid count: the backward reads them).
__global__ __launch_bounds__(256) void mean_kernel(int nparts, const double* __restrict__ part, double* __restrict__ acc, float* __restrict__ out) {
    __shared__ double tot[2];
    double v[2] = {0, 0};
    for (int k = threadIdx.x; k < nparts; k += 256) {
        v[0] += part[(long)k * 2];
        v[1] += part[(long)k * 2 + 1];
    }
    block_sums<2>(v, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        acc[0] = tot[0];
        acc[1] = tot[1];
        out[0] = (tot[1] > 0.0 && !isnan(tot[0])) ? (float)(tot[0] / tot[1]) : 0.f;
    }
}

__global__ __launch_bounds__(256) void angular_kernel(int hw, const float* __restrict__ pred, const float* __restrict__ tgt,
                                                      const uint8_t* __restrict__ mask, double* __restrict__ part /* [B * nb][2] */) {
    const int b = blockIdx.y;
    const float* p = pred + (long)b * 3 * hw;
    const float* t = tgt + (long)b * 3 * hw;
    const uint8_t* m = mask + (long)b * hw;
    double v[2] = {0, 0};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
        if (m[i]) {
            float d = p[i] * t[i] + p[hw + i] * t[hw + i] + p[2 * hw + i] * t[2 * hw + i];
            d = isnan(d) ? d : fminf(fmaxf(d, -1.f), 1.f);   // torch.clamp propagates NaN (fminf / fmaxf would swallow it, loss.py:62)
            v[0] += (double)acosf(d);
            v[1] += 1.0;
        }
    }
    block_sums<2>(v, part + ((long)b * gridDim.x + blockIdx.x) * 2);
}

}  // namespace e2eft

using namespace e2eft;

// forward workspace of the SSI loss: sums [B][5] | acc [2] | partials [B][LOSS_NBLK][5] (doubles; pass 2 reuses the partials as [B][nb][2]) | scale/shift [B][2] floats.
// The backward (bwd.hip) reads sums and acc.
extern "C" size_t e2eft_ssi_loss_workspace_bytes(int32_t batch) {
    return batch > 0 ? ((size_t)batch * 5 + 2 + (size_t)batch * LOSS_NBLK * 5) * sizeof(double) + (size_t)batch * 2 * sizeof(float) : 0;
}

extern "C" int e2eft_ssi_loss_fwd(int32_t batch, int32_t hw, const float* pred, const float* target, const uint8_t* mask,
                                  float* out_loss, float* out_scale_shift, void* workspace, size_t ws_bytes, void* stream) {
    E2EFT_REQUIRE(pred && target && mask && out_loss && workspace, "ssi_loss: null pointer");
    E2EFT_REQUIRE(batch > 0 && batch <= 65535 && hw > 0, "ssi_loss: shape");
    const size_t need = e2eft_ssi_loss_workspace_bytes(batch);
    if (ws_bytes < need) return fail(E2EFT_ERR_WORKSPACE, "ssi_loss: workspace %zu < %zu", ws_bytes, need);
    E2EFT_REQUIRE(((uintptr_t)workspace & 7) == 0, "ssi_loss: workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    double* sums = (double*)workspace;
    double* acc = sums + (size_t)batch * 5;
    double* part = acc + 2;
    float* ss = out_scale_shift ? out_scale_shift : (float*)(part + (size_t)batch * LOSS_NBLK * 5);
    int nb = cdiv(hw, 256 * 8);
    if (nb > LOSS_NBLK) nb = LOSS_NBLK;
    hipLaunchKernelGGL(ssi_sums_kernel, dim3(nb, batch), dim3(256), 0, s, hw, pred, target, mask, part);
    hipLaunchKernelGGL(ssi_solve_kernel, dim3(cdiv(batch, 64)), dim3(64), 0, s, batch, nb, part, sums, ss);
    hipLaunchKernelGGL(ssi_l1_kernel, dim3(nb, batch), dim3(256), 0, s, hw, pred, target, mask, ss, part);
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, batch * nb, part, acc, out_loss);
    return check_launch("ssi_loss");
}

// forward workspace of the angular loss: acc [2] (the backward reads it) | partials [B][LOSS_NBLK][2] doubles
extern "C" size_t e2eft_angular_loss_workspace_bytes(int32_t batch) { return batch > 0 ? (2 + (size_t)batch * LOSS_NBLK * 2) * sizeof(double) : 0; }

extern "C" int e2eft_angular_loss_fwd(int32_t batch, int32_t hw, const float* pred, const float* target, const uint8_t* mask,
                                      float* out_loss, void* workspace, size_t ws_bytes, void* stream) {
    E2EFT_REQUIRE(pred && target && mask && out_loss && workspace, "angular_loss: null pointer");
    E2EFT_REQUIRE(batch > 0 && batch <= 65535 && hw > 0, "angular_loss: shape");
    const size_t need = e2eft_angular_loss_workspace_bytes(batch);
    if (ws_bytes < need) return fail(E2EFT_ERR_WORKSPACE, "angular_loss: workspace %zu < %zu", ws_bytes, need);
    E2EFT_REQUIRE(((uintptr_t)workspace & 7) == 0, "angular_loss: workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    double* acc = (double*)workspace;
    int nb = cdiv(hw, 256 * 8);
    if (nb > LOSS_NBLK) nb = LOSS_NBLK;
    hipLaunchKernelGGL(angular_kernel, dim3(nb, batch), dim3(256), 0, s, hw, pred, target, mask, acc + 2);
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, batch * nb, acc + 2, acc, out_loss);
    return check_launch("angular_loss");
}
