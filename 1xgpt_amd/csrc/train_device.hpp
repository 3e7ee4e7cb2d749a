// Device code that kernels_train.hip and kernels_muon.hip share, stated once: the 128 x 128 x 16 operand tile of the general f32
// matrix-core GEMM (either operand in either orientation) and the per-element pieces of the optimizers.
#pragma once
#include "kernels.hpp"

namespace genie {

// 128x128x16 tile, 4 waves (2x2) x 64x64, double-buffered LDS.  Row-major operands use the k-permuted
// ds_read_b128 fetch of gemm_f32_nt_kernel (kernels_exact.hip); k-major operands are staged as they lie
// ([16][128] floats, coalesced float4) and fetched with one conflict-free ds_read_b32 per MFMA -- the f32 MFMA
// issues every 64 cycles per SIMD, so four narrow LDS reads per four MFMAs stay hidden.
constexpr int GG_BM = 128, GG_BK = 16, GG_LD = GG_BK + 4, GG_TLD = GG_BM + 4;
constexpr int GG_TILE = GG_BM * GG_LD;  // 2560 floats >= 16 * 132

// BRANCH: the bounds guard as a branch around the load instead of a select on its result.  The select form leaves the staging registers
// in scratch memory (96 bytes per lane, one round trip per k-tile); gemm_f32_gen_kernel keeps it, as every training measurement was taken
// with it, and the batched products of kernels_muon.hip take the branch form (no scratch).  The values loaded are the same.
template <bool TR, bool BRANCH = false>
__device__ __forceinline__ void gg_stage_load(const float* __restrict__ G, long ld, int row0, int limit, int k0, int tid,
                                              float4 (&regs)[2]) {
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if constexpr (BRANCH) {
            const int row = row0 + (tid >> 2) + p * 64, kr = (tid >> 5) + p * 8, c4 = (tid & 31) << 2;
            regs[p] = z4;
            if constexpr (!TR) {
                if (row < limit) regs[p] = *reinterpret_cast<const float4*>(G + (size_t)row * ld + k0 + ((tid & 3) << 2));
            } else {
                if ((row0 + c4) < limit) regs[p] = *reinterpret_cast<const float4*>(G + (size_t)(k0 + kr) * ld + row0 + c4);
            }
        } else if constexpr (!TR) {
            const int row = row0 + (tid >> 2) + p * 64;
            regs[p] = row < limit ? *reinterpret_cast<const float4*>(G + (size_t)row * ld + k0 + ((tid & 3) << 2)) : z4;
        } else {
            const int kr = (tid >> 5) + p * 8, c4 = (tid & 31) << 2;
            regs[p] = (row0 + c4) < limit ? *reinterpret_cast<const float4*>(G + (size_t)(k0 + kr) * ld + row0 + c4) : z4;
        }
    }
}
template <bool TR>
__device__ __forceinline__ void gg_stage_store(float* s, int tid, const float4 (&regs)[2]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if constexpr (!TR)
            *reinterpret_cast<float4*>(&s[((tid >> 2) + p * 64) * GG_LD + ((tid & 3) << 2)]) = regs[p];
        else
            *reinterpret_cast<float4*>(&s[((tid >> 5) + p * 8) * GG_TLD + ((tid & 31) << 2)]) = regs[p];
    }
}
// the four k-values (8kk + 4h + j, j = 0..3) of operand row `row` that MFMA j consumes
template <bool TR>
__device__ __forceinline__ float4 gg_frag(const float* s, int row, int kk, int h) {
    if constexpr (!TR) return *reinterpret_cast<const float4*>(&s[row * GG_LD + kk * 8 + 4 * h]);
    const float* p = s + (kk * 8 + 4 * h) * GG_TLD + row;
    return make_float4(p[0], p[GG_TLD], p[2 * GG_TLD], p[3 * GG_TLD]);
}

// grad_mult times the clip coefficient of clip_grad_norm_: min(1, max_norm / (total_norm + 1e-6))
__device__ __forceinline__ float adamw_coef(float grad_mult, const double* __restrict__ sumsq, float max_norm) {
    float coef = grad_mult;
    if (sumsq && max_norm > 0.f) {
        const float tn = (float)sqrt(*sumsq) * grad_mult;
        coef *= fminf(1.0f, max_norm / (tn + 1e-6f));
    }
    return coef;
}
// LitEma.forward's line (include/genie_hip.h, "EMA of the weights"): three f32 operations, each rounded on its own
__device__ __forceinline__ float ema_element(float e, float p, float omd) {
    return __fsub_rn(e, __fmul_rn(omd, __fsub_rn(e, p)));
}

}  // namespace genie
