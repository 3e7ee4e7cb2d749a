// Kernels of the training step: what autograd derives for STMaskGIT.forward
// (genie/st_mask_git.py:231-279) plus the optimizer of train.py:426-441, 628-633.  Everything here is f32 and serves all
// three precisions (LayerNorm / attention / loss / embedding backward, reductions, AdamW); the Linear products of the
// "exact" precision run on v_mfma_f32_32x32x2_f32 through ONE general GEMM that reads either operand in either orientation,
// so no activation or weight is ever physically transposed for a backward product (the 16-bit precisions take the NT GEMM
// of kernels_bf16.hip with the operand copies of kernels_train16.hip instead):
//     forward   Y  = X . W^T          A = X  [rows][k]      B = W  [cols][k]
//     dgrad     dX = dY . W           A = dY [rows][k]      B = W  [k][cols]   (TB)
//     wgrad     dW = dY^T . X         A = dY [k][rows] (TA) B = X  [k][cols]   (TB), split over the token axis
// All reductions that feed a gradient (split-K partials, LayerNorm / bias column sums, embedding scatter) are
// two-stage with a fixed summation order: a training step is bit-reproducible run to run.
#include "train_device.hpp"

namespace genie {

// ------------------------------------------------------------------------------------------------
// C[b1][b2][M,N] = alpha * sum_k A(m,k) B(n,k) (+ bias[n]) (+ R[m,n])
//   TA: A(m,k) = A[k*lda + m] else A[m*lda + k];   TB: B(n,k) = W[k*ldw + n] else W[n*ldw + k]
//   blockIdx.y = b1, blockIdx.z = b2 * nsplit + split; split s contracts k in [s*K/nsplit, (s+1)*K/nsplit) and
//   writes its own slab C + s*sCsplit (no bias / residual there; splitk_reduce adds the slabs in order).
// The 128x128x16 operand tile (gg_stage_load / gg_stage_store / gg_frag) is stated in train_device.hpp, which the batched
// products of kernels_muon.hip share.
// ------------------------------------------------------------------------------------------------

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_f32_gen_kernel(const float* __restrict__ A, long lda, long sA1, long sA2,
                                                           const float* __restrict__ W, long ldw, long sW1, long sW2,
                                                           const float* __restrict__ bias, const float* R,
                                                           float* C, long ldc, long sC1, long sC2, int M, int N, int K,
                                                           float alpha, int nsplit, long sCsplit) {
    __shared__ __attribute__((aligned(16))) float sA[2][GG_TILE];
    __shared__ __attribute__((aligned(16))) float sB[2][GG_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int r = lane & 31, h = lane >> 5;
    const int n_tiles = (N + GG_BM - 1) / GG_BM;
    const int m0 = (blockIdx.x / n_tiles) * GG_BM, n0 = (blockIdx.x % n_tiles) * GG_BM;
    const int b2 = blockIdx.z / nsplit, sp = blockIdx.z - b2 * nsplit;
    A += (size_t)blockIdx.y * sA1 + (size_t)b2 * sA2;
    W += (size_t)blockIdx.y * sW1 + (size_t)b2 * sW2;
    const size_t coff = (size_t)blockIdx.y * sC1 + (size_t)b2 * sC2 + (size_t)sp * sCsplit;
    C += coff;
    if (R) R += coff;
    const int kc = K / nsplit, kbeg = sp * kc;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    float4 ra[2], rb[2];
    const int nk = kc / GG_BK;
    gg_stage_load<TA>(A, lda, m0, M, kbeg, tid, ra);
    gg_stage_load<TB>(W, ldw, n0, N, kbeg, tid, rb);
    gg_stage_store<TA>(sA[0], tid, ra);
    gg_stage_store<TB>(sB[0], tid, rb);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) {
            gg_stage_load<TA>(A, lda, m0, M, kbeg + (kt + 1) * GG_BK, tid, ra);
            gg_stage_load<TB>(W, ldw, n0, N, kbeg + (kt + 1) * GG_BK, tid, rb);
        }
#pragma unroll
        for (int kk = 0; kk < GG_BK / 8; ++kk) {
            float4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = gg_frag<TA>(sA[buf], wm * 64 + i * 32 + r, kk, h);
                b[i] = gg_frag<TB>(sB[buf], wn * 64 + i * 32 + r, kk, h);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
                }
        }
        if (kt + 1 < nk) {
            gg_stage_store<TA>(sA[buf ^ 1], tid, ra);
            gg_stage_store<TB>(sB[buf ^ 1], tid, rb);
        }
        __syncthreads();
    }
    // C/D map of the 32x32 MFMA: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 64 + j * 32 + r;
            if (col >= N) continue;
            const float bcol = bias ? bias[col] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (row >= M) continue;
                const size_t idx = (size_t)row * ldc + col;
                float v = acc[i][j][e] * alpha + bcol;
                if (R) v += R[idx];
                C[idx] = v;
            }
        }
}

int launch_gemm_f32_gen(bool ta, bool tb, const float* A, long lda, long sA1, long sA2, const float* W, long ldw, long sW1,
                        long sW2, const float* bias, const float* R, float* C, long ldc, long sC1, long sC2, int M, int N,
                        int K, int batch1, int batch2, int nsplit, long sCsplit, float alpha, hipStream_t st) {
    GENIE_CHECK_SHAPE(K > 0 && nsplit > 0 && K % (GG_BK * nsplit) == 0,
                      "gemm_gen: K=%d must be a positive multiple of %d", K, GG_BK * nsplit);
    GENIE_CHECK_SHAPE(lda % 4 == 0 && ldw % 4 == 0, "gemm_gen: leading dims must be multiples of 4 floats");
    GENIE_CHECK_SHAPE((!ta || M % 4 == 0) && (!tb || N % 4 == 0), "gemm_gen: k-major operands need row counts % 4 == 0");
    if (M <= 0 || N <= 0 || batch1 <= 0 || batch2 <= 0) return GENIE_OK;
    const int mt = (M + GG_BM - 1) / GG_BM, nt = (N + GG_BM - 1) / GG_BM;
    dim3 grid(mt * nt, batch1, batch2 * nsplit);
    const double mn = (double)M * N * batch1 * batch2;
    ProfScope prof(GENIE_KC_GEMM, 2.0 * mn * K,
                   4.0 * (((double)M * K + (double)N * K) * batch1 * batch2 + mn * nsplit * (R ? 2 : 1)), st,
                   "gemm_f32_gen_kernel");
#define GG_LAUNCH(TA_, TB_)                                                                                          \
    gemm_f32_gen_kernel<TA_, TB_><<<grid, 256, 0, st>>>(A, lda, sA1, sA2, W, ldw, sW1, sW2, bias, R, C, ldc, sC1, sC2, \
                                                        M, N, K, alpha, nsplit, sCsplit)
    if (!ta && !tb) GG_LAUNCH(false, false);
    else if (!ta && tb) GG_LAUNCH(false, true);
    else if (ta && tb) GG_LAUNCH(true, true);
    else GG_LAUNCH(true, false);
#undef GG_LAUNCH
    GENIE_LAUNCH_CHECK("gemm_f32_gen");
    return GENIE_OK;
}

// out[i] = beta * out[i] + sum_{s < ns} part[s*n + i].  Fixed order: thread group g (0..3) of a block sums slabs
// g, g+4, g+8, ... of its 64 columns with 4 independent chains, then the 4 group sums are added 0+1+2+3.
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ part, int ns, size_t n,
                                                          float* __restrict__ out, float beta) {
    __shared__ float red[4][64];
    const int col = threadIdx.x & 63, g = threadIdx.x >> 6;
    const size_t i = (size_t)blockIdx.x * 64 + col;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (i < n) {
        int k = g;
        for (; k + 12 < ns; k += 16) {
            s0 += part[(size_t)k * n + i];
            s1 += part[(size_t)(k + 4) * n + i];
            s2 += part[(size_t)(k + 8) * n + i];
            s3 += part[(size_t)(k + 12) * n + i];
        }
        for (; k < ns; k += 4) s0 += part[(size_t)k * n + i];
    }
    red[g][col] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (g == 0 && i < n) {
        const float s = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
        out[i] = (beta != 0.f ? beta * out[i] : 0.f) + s;
    }
}
int launch_slab_reduce(const float* part, int ns, size_t n, float* out, float beta, hipStream_t st, const char* what) {
    if (!n) return GENIE_OK;
    if (what) {   // a named reduction is bracketed for the profile; the others stay outside it, as they always were
        ProfScope prof(GENIE_KC_OTHER, 0.0, 4.0 * ((double)ns + 1.0) * (double)n, st, what);
        slab_reduce_kernel<<<(unsigned)((n + 63) / 64), 256, 0, st>>>(part, ns, n, out, beta);
    } else {
        slab_reduce_kernel<<<(unsigned)((n + 63) / 64), 256, 0, st>>>(part, ns, n, out, beta);
    }
    GENIE_LAUNCH_CHECK("slab_reduce");
    return GENIE_OK;
}

// dW[N,K] (beta*dW +)= alpha * dY[M,N]^T . X[M,K], contraction over the M tokens split into slabs
int launch_wgrad_f32(const float* dY, long ldy, const float* X, long ldx, float* dW, int Mtok, int N, int K, float alpha,
                     float beta, float* slabs, size_t slab_floats, hipStream_t st) {
    const int tiles = ((N + 127) / 128) * ((K + 127) / 128);
    int ns = 1;
    while (ns < 64 && tiles * ns < 512 && Mtok % (GG_BK * ns * 2) == 0 && (size_t)(ns * 2) * N * K <= slab_floats) ns *= 2;
    if (ns == 1)
        return launch_gemm_f32_gen(true, true, dY, ldy, 0, 0, X, ldx, 0, 0, nullptr, beta != 0.f ? dW : nullptr, dW, K, 0, 0,
                                   N, K, Mtok, 1, 1, 1, 0, alpha, st);
    GENIE_CHECK_ARG(beta == 0.f || beta == 1.f, "wgrad: beta must be 0 or 1");
    GENIE_TRY(launch_gemm_f32_gen(true, true, dY, ldy, 0, 0, X, ldx, 0, 0, nullptr, nullptr, slabs, K, 0, 0, N, K, Mtok, 1,
                                  1, ns, (long)N * K, alpha, st));
    return launch_slab_reduce(slabs, ns, (size_t)N * K, dW, beta, st);
}

// ------------------------------------------------------------------------------------------------
// column sums (bias gradients): part[chunk][N] = sum over the chunk's rows, then slab_reduce
// ------------------------------------------------------------------------------------------------
__global__ void colsum_partial_kernel(const float* __restrict__ Y, long ld, long rows, int N, float* __restrict__ part) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const long per = (rows + gridDim.y - 1) / gridDim.y;
    const long r0 = (long)blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
    float s = 0.f;
    for (long r = r0; r < r1; ++r) s += Y[(size_t)r * ld + c];
    part[(size_t)blockIdx.y * N + c] = s;
}
// the same restricted to the rows whose id equals `key` (gradient of the mask-token embedding)
__global__ void colsum_where_partial_kernel(const float* __restrict__ Y, long ld, long rows, int N,
                                            const int64_t* __restrict__ ids, int64_t key, float* __restrict__ part) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= N) return;
    const long per = (rows + gridDim.y - 1) / gridDim.y;
    const long r0 = (long)blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
    float s = 0.f;
    for (long r = r0; r < r1; ++r)
        if (ids[r] == key) s += Y[(size_t)r * ld + c];
    part[(size_t)blockIdx.y * N + c] = s;
}
int launch_colsum_where(const float* Y, long ld, long rows, int N, const int64_t* ids, int64_t key, float* out, float beta,
                        float* part, hipStream_t st) {
    if (rows <= 0 || N <= 0) return GENIE_OK;
    colsum_where_partial_kernel<<<dim3((N + 255) / 256, COLSUM_CHUNKS), 256, 0, st>>>(Y, ld, rows, N, ids, key, part);
    GENIE_LAUNCH_CHECK("colsum_where");
    return launch_slab_reduce(part, COLSUM_CHUNKS, (size_t)N, out, beta, st);
}
int launch_colsum(const float* Y, long ld, long rows, int N, float* out, float beta, float* part, hipStream_t st) {
    if (rows <= 0 || N <= 0) return GENIE_OK;
    colsum_partial_kernel<<<dim3((N + 255) / 256, COLSUM_CHUNKS), 256, 0, st>>>(Y, ld, rows, N, part);
    GENIE_LAUNCH_CHECK("colsum");
    return launch_slab_reduce(part, COLSUM_CHUNKS, (size_t)N, out, beta, st);
}

// ------------------------------------------------------------------------------------------------
// LayerNorm backward (nn.LayerNorm(C, eps), biased variance): one wave per row, statistics recomputed from x.
//   dxout[row] += (gy - mean(gy) - xhat * mean(gy * xhat)) * rstd,  gy = dy * gamma
//   part[block][0][C] = sum_rows dy * xhat, part[block][1][C] = sum_rows dy   (then slab_reduce -> dgamma, dbeta)
// ------------------------------------------------------------------------------------------------
constexpr int LNB_MAXI = 16;  // C <= 1024
constexpr int LNB_BLOCKS = 512;
// PARAMS = false (both parameter gradients frozen): dxout alone -- no dg / db accumulators, no LDS, `part` is not touched
template <bool PARAMS>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ dy, float* __restrict__ dxout,
                                                     float* __restrict__ part, long rows, int C, float eps) {
    extern __shared__ float red[];  // [4][2][C]
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float dg[LNB_MAXI], db[LNB_MAXI], gm[LNB_MAXI];
#pragma unroll
    for (int i = 0; i < LNB_MAXI; ++i) {
        if constexpr (PARAMS) { dg[i] = 0.f; db[i] = 0.f; }
        const int c = lane + 64 * i;
        gm[i] = c < C ? gamma[c] : 0.f;
    }
    const float invC = 1.0f / (float)C;
    for (long row = (long)blockIdx.x * 4 + wid; row < rows; row += (long)gridDim.x * 4) {
        const float* xr = x + (size_t)row * C;
        const float* dr = dy + (size_t)row * C;
        float xv[LNB_MAXI], dv[LNB_MAXI];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < LNB_MAXI; ++i) {
            const int c = lane + 64 * i;
            xv[i] = c < C ? xr[c] : 0.f;
            dv[i] = c < C ? dr[c] : 0.f;
            s += xv[i];
        }
        const float mean = wave_sum(s) * invC;
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < LNB_MAXI; ++i) {
            const int c = lane + 64 * i;
            const float xc = c < C ? xv[i] - mean : 0.f;
            xv[i] = xc;
            v += xc * xc;
        }
        const float rstd = 1.0f / sqrtf(wave_sum(v) * invC + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < LNB_MAXI; ++i) {
            xv[i] *= rstd;  // xhat
            const float gy = dv[i] * gm[i];
            s1 += gy;
            s2 += gy * xv[i];
            if constexpr (PARAMS) { dg[i] += dv[i] * xv[i]; db[i] += dv[i]; }
        }
        s1 = wave_sum(s1) * invC;
        s2 = wave_sum(s2) * invC;
        float* o = dxout + (size_t)row * C;
#pragma unroll
        for (int i = 0; i < LNB_MAXI; ++i) {
            const int c = lane + 64 * i;
            if (c < C) o[c] += (dv[i] * gm[i] - s1 - xv[i] * s2) * rstd;
        }
    }
    if constexpr (PARAMS) {
#pragma unroll
        for (int i = 0; i < LNB_MAXI; ++i) {
            const int c = lane + 64 * i;
            if (c < C) { red[(wid * 2 + 0) * C + c] = dg[i]; red[(wid * 2 + 1) * C + c] = db[i]; }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < 2 * C; c += 256) {
            const int which = c / C, cc = c - which * C;
            float s = 0.f;
            for (int w = 0; w < 4; ++w) s += red[(w * 2 + which) * C + cc];
            part[(size_t)blockIdx.x * 2 * C + c] = s;  // [block][which][C]
        }
    }
}
// The same for C = 256 / 512 with the access pattern of layer_norm_fast_kernel: a lane owns VPL = C/64 contiguous
// channels (float4 loads / read-modify-write of dxout instead of 4-byte strided ones), the next row's x and dy are in
// flight while the current row is reduced.
template <int VPL, bool PARAMS>
__global__ __launch_bounds__(256) void ln_bwd_fast_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ dy, float* __restrict__ dxout,
                                                          float* __restrict__ part, long rows, float eps) {
    constexpr int C = 64 * VPL;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float dg[VPL], db[VPL], gm[VPL], xv[VPL], dv[VPL], xn[VPL], dn[VPL];
    auto load = [&](const float* p, float (&v)[VPL]) {
#pragma unroll
        for (int k = 0; k < VPL; k += 4) {
            const float4 t = *reinterpret_cast<const float4*>(p + lane * VPL + k);
            v[k] = t.x; v[k + 1] = t.y; v[k + 2] = t.z; v[k + 3] = t.w;
        }
    };
    load(gamma, gm);
    if constexpr (PARAMS) {
#pragma unroll
        for (int k = 0; k < VPL; ++k) { dg[k] = 0.f; db[k] = 0.f; }
    }
    const long stride = (long)gridDim.x * 4;
    long row = (long)blockIdx.x * 4 + wid;
    if (row < rows) { load(x + (size_t)row * C, xv); load(dy + (size_t)row * C, dv); }
    for (; row < rows; row += stride) {
        const long nrow = row + stride;
        if (nrow < rows) { load(x + (size_t)nrow * C, xn); load(dy + (size_t)nrow * C, dn); }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < VPL; ++k) s += xv[k];
        const float mean = wave_sum(s) * (1.0f / C);
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < VPL; ++k) { xv[k] -= mean; v += xv[k] * xv[k]; }
        const float rstd = 1.0f / sqrtf(wave_sum(v) * (1.0f / C) + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < VPL; ++k) {
            xv[k] *= rstd;  // xhat
            const float gy = dv[k] * gm[k];
            s1 += gy;
            s2 += gy * xv[k];
            if constexpr (PARAMS) { dg[k] += dv[k] * xv[k]; db[k] += dv[k]; }
        }
        s1 = wave_sum(s1) * (1.0f / C);
        s2 = wave_sum(s2) * (1.0f / C);
        float* o = dxout + (size_t)row * C + lane * VPL;
#pragma unroll
        for (int k = 0; k < VPL; k += 4) {
            float4 t = *reinterpret_cast<const float4*>(o + k);
            t.x += (dv[k] * gm[k] - s1 - xv[k] * s2) * rstd;
            t.y += (dv[k + 1] * gm[k + 1] - s1 - xv[k + 1] * s2) * rstd;
            t.z += (dv[k + 2] * gm[k + 2] - s1 - xv[k + 2] * s2) * rstd;
            t.w += (dv[k + 3] * gm[k + 3] - s1 - xv[k + 3] * s2) * rstd;
            *reinterpret_cast<float4*>(o + k) = t;
        }
#pragma unroll
        for (int k = 0; k < VPL; ++k) { xv[k] = xn[k]; dv[k] = dn[k]; }
    }
    if constexpr (PARAMS) {
        __shared__ float red[4][2][C];
#pragma unroll
        for (int k = 0; k < VPL; ++k) { red[wid][0][lane * VPL + k] = dg[k]; red[wid][1][lane * VPL + k] = db[k]; }
        __syncthreads();
        for (int c = threadIdx.x; c < 2 * C; c += 256) {
            const int which = c / C, cc = c - which * C;
            part[(size_t)blockIdx.x * 2 * C + c] = ((red[0][which][cc] + red[1][which][cc]) + red[2][which][cc]) + red[3][which][cc];
        }
    }
}

// part slabs are [block][2][C]: dgamma = reduce of the first C, dbeta of the second C.  A NULL dgamma / dbeta is a frozen tensor
// (include/genie_hip.h, "Frozen tensors"): its half is not reduced; both NULL: the parameter-free kernels and no reduction at all
int launch_ln_bwd(const float* x, const float* gamma, const float* dy, float* dxout, float* dgamma, float* dbeta,
                  long rows, int C, float eps, float beta, float* part, hipStream_t st) {
    GENIE_CHECK_SHAPE(C <= 64 * LNB_MAXI, "ln_bwd: C=%d > %d", C, 64 * LNB_MAXI);
    if (rows <= 0) return GENIE_OK;
    ProfScope prof(GENIE_KC_LAYERNORM, 12.0 * rows * C, 16.0 * rows * C, st);
    if (!dgamma && !dbeta) {
        if (C == 512) ln_bwd_fast_kernel<8, false><<<LNB_BLOCKS, 256, 0, st>>>(x, gamma, dy, dxout, nullptr, rows, eps);
        else if (C == 256) ln_bwd_fast_kernel<4, false><<<LNB_BLOCKS, 256, 0, st>>>(x, gamma, dy, dxout, nullptr, rows, eps);
        else ln_bwd_kernel<false><<<LNB_BLOCKS, 256, 0, st>>>(x, gamma, dy, dxout, nullptr, rows, C, eps);
        GENIE_LAUNCH_CHECK("ln_bwd");
        return GENIE_OK;
    }
    if (C == 512) ln_bwd_fast_kernel<8, true><<<LNB_BLOCKS, 256, 0, st>>>(x, gamma, dy, dxout, part, rows, eps);
    else if (C == 256) ln_bwd_fast_kernel<4, true><<<LNB_BLOCKS, 256, 0, st>>>(x, gamma, dy, dxout, part, rows, eps);
    else ln_bwd_kernel<true><<<LNB_BLOCKS, 256, (size_t)8 * C * sizeof(float), st>>>(x, gamma, dy, dxout, part, rows, C, eps);
    GENIE_LAUNCH_CHECK("ln_bwd");
    // the two halves of each slab are contiguous ([2][C]), so one reduce of 2C columns serves both when dbeta follows
    // dgamma in memory; they need not, so reduce separately through strided views
    float* tmp = part + (size_t)LNB_BLOCKS * 2 * C;  // [2][C] reduced
    GENIE_TRY(launch_slab_reduce(part, LNB_BLOCKS, (size_t)2 * C, tmp, 0.f, st, "slab_reduce_norm"));
    if (dgamma) GENIE_TRY(launch_slab_reduce(tmp, 1, (size_t)C, dgamma, beta, st, "slab_reduce_norm"));
    return dbeta ? launch_slab_reduce(tmp + C, 1, (size_t)C, dbeta, beta, st, "slab_reduce_norm") : GENIE_OK;
}
size_t ln_bwd_scratch_floats(int C) { return (size_t)(LNB_BLOCKS + 1) * 2 * C; }

// ------------------------------------------------------------------------------------------------
// erf-GELU forward (saving the pre-activation) and backward: dz = dh * (Phi(z) + z * phi(z))
// ------------------------------------------------------------------------------------------------
__global__ void gelu_fwd_kernel(const float4* __restrict__ z, float4* __restrict__ h, size_t n4) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float4 v = z[i];
    v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w);
    h[i] = v;
}
__device__ __forceinline__ float gelu_grad(float z) {
    const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * z * z) * 0.39894228040143267794f;
    return cdf + z * pdf;
}
__global__ void gelu_bwd_kernel(const float4* __restrict__ z, float4* __restrict__ g, size_t n4) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const float4 zz = z[i];
    float4 v = g[i];
    v.x *= gelu_grad(zz.x); v.y *= gelu_grad(zz.y); v.z *= gelu_grad(zz.z); v.w *= gelu_grad(zz.w);
    g[i] = v;
}
int launch_gelu_fwd(const float* z, float* h, size_t n, hipStream_t st) {
    GENIE_CHECK_SHAPE(n % 4 == 0, "gelu: n %% 4");
    if (!n) return GENIE_OK;
    gelu_fwd_kernel<<<(unsigned)((n / 4 + 255) / 256), 256, 0, st>>>((const float4*)z, (float4*)h, n / 4);
    GENIE_LAUNCH_CHECK("gelu_fwd");
    return GENIE_OK;
}
int launch_gelu_bwd(const float* z, float* g, size_t n, hipStream_t st) {
    GENIE_CHECK_SHAPE(n % 4 == 0, "gelu: n %% 4");
    if (!n) return GENIE_OK;
    gelu_bwd_kernel<<<(unsigned)((n / 4 + 255) / 256), 256, 0, st>>>((const float4*)z, (float4*)g, n / 4);
    GENIE_LAUNCH_CHECK("gelu_bwd");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// embedding backward (factorization_utils.py:29-52, st_mask_git.py:257-261), scatter-free and ordered:
//   dpos[t,s,:]  = sum_b dx[b,t,s,:]
//   row v of table f (block f*vf + v): sum over tokens n (ascending) with factor_f(id_n) == v and id_n != MASK
//   mask row: a predicated column sum over the tokens with id_n == MASK (they are a large fraction of a training
//   batch, so they get the chunked two-stage reduction instead of one block)
// ------------------------------------------------------------------------------------------------
struct EmbedTables { float* p[4]; };
__global__ void embed_bwd_pos_kernel(const float* __restrict__ dx, float* __restrict__ dpos, int B, size_t per_clip,
                                     float beta) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per_clip) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dx[(size_t)b * per_clip + i];
    dpos[i] = (beta != 0.f ? beta * dpos[i] : 0.f) + s;
}
__global__ __launch_bounds__(256) void embed_bwd_tables_kernel(const float* __restrict__ dx, const int64_t* __restrict__ ids,
                                                               long n_tok, int d, int vf, int nfac, int64_t mask_id,
                                                               EmbedTables tables, float* __restrict__ dmask,
                                                               float beta) {
    // One block per table row (and one for the mask row).  The block sweeps the ids 1024 at a time: every thread tests
    // 4 tokens, wave ballots give an ORDERED match list (token index ascending), and the (rare: 1/vf) matching rows
    // of dx are summed channel-parallel in that order -- no atomics, no sort, bit-reproducible.
    __shared__ unsigned long long masks[4][4];  // [k][wave]: tokens base + k*256 + wave*64 + bit
    const int blk = blockIdx.x;
    constexpr bool is_mask_row = false;
    const int f = blk / vf, v = blk - f * vf;
    if (!tables.p[f]) return;   // a frozen table: the whole block leaves, in front of every barrier
    int64_t div = 1;
    for (int k = 0; k < f; ++k) div *= vf;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};  // channels threadIdx.x + 256*k, d <= 1024
    for (long base = 0; base < n_tok; base += 1024) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long i = base + k * 256 + threadIdx.x;
            bool m = false;
            if (i < n_tok) {
                const int64_t id = ids[i];
                m = is_mask_row ? (id == mask_id) : (id != mask_id && (int)((id / div) % vf) == v);
            }
            const unsigned long long bal = __ballot(m);
            if (lane == 0) masks[k][wid] = bal;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                unsigned long long bits = masks[k][w];
                while (bits) {
                    const int bit = __ffsll((long long)bits) - 1;
                    bits &= bits - 1;
                    const float* r = dx + (size_t)(base + k * 256 + w * 64 + bit) * d;
#pragma unroll
                    for (int c4 = 0; c4 < 4; ++c4) {
                        const int c = threadIdx.x + 256 * c4;
                        if (c < d) acc[c4] += r[c];
                    }
                }
            }
        __syncthreads();
    }
    float* out = is_mask_row ? dmask : tables.p[f] + (size_t)v * d;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = threadIdx.x + 256 * k;
        if (c < d) out[c] = (beta != 0.f ? beta * out[c] : 0.f) + acc[k];
    }
}
int launch_embed_bwd(const genie_cfg& c, const float* dx, const int64_t* ids, int B, float* dpos, float* dmask,
                     float* const* tables_host, float beta, float* colpart, hipStream_t st) {
    // dpos, dmask and each table may be NULL: a frozen tensor (include/genie_hip.h, "Frozen tensors"), whose part is skipped
    EmbedTables tables_dev;
    bool any_table = false;
    for (int j = 0; j < 4; ++j) {
        tables_dev.p[j] = j < c.num_factored ? tables_host[j] : nullptr;
        any_table = any_table || tables_dev.p[j];
    }
    GENIE_CHECK_SHAPE(c.d_model <= 1024, "embed backward: d_model > 1024");
    const size_t per_clip = (size_t)c.T * c.S * c.d_model;
    if (dpos) {
        embed_bwd_pos_kernel<<<(unsigned)((per_clip + 255) / 256), 256, 0, st>>>(dx, dpos, B, per_clip, beta);
        GENIE_LAUNCH_CHECK("embed_bwd_pos");
    }
    if (any_table) {
        embed_bwd_tables_kernel<<<c.num_factored * c.factored_vocab, 256, 0, st>>>(
            dx, ids, (long)B * c.T * c.S, c.d_model, c.factored_vocab, c.num_factored, (int64_t)c.image_vocab_size, tables_dev,
            dmask, beta);
        GENIE_LAUNCH_CHECK("embed_bwd_tables");
    }
    if (!dmask) return GENIE_OK;
    return launch_colsum_where(dx, c.d_model, (long)B * c.T * c.S, c.d_model, ids, (int64_t)c.image_vocab_size, dmask, beta,
                               colpart, st);
}

// action-table gradient (per-frame action conditioning, genie_frame_cond): the action row of frame (b, t) is added to every
// token of that frame, so
//   stage 1: fs[b*T + t, :] = sum_s dx[b, t, s, :]                (s ascending; one thread per (frame, channel))
//   stage 2: d_table[k, :]  = sum over frames n (ascending) with act_ids[n] == k of fs[n, :]
// stage 2 is embed_bwd_tables_kernel's ordered ballot walk over the B*T frame ids, one block per action: no atomics.
__global__ void frame_sum_kernel(const float* __restrict__ dx, float* __restrict__ fs, long n_frames, int S, int d) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_frames * d) return;
    const long f = i / d;
    const int c = (int)(i - f * d);
    const float* r = dx + (size_t)f * S * d + c;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += r[(size_t)k * d];
    fs[i] = s;
}
__global__ __launch_bounds__(256) void action_bwd_kernel(const float* __restrict__ fs, const int64_t* __restrict__ act_ids,
                                                         long n_frames, int d, float* __restrict__ d_table, float beta) {
    __shared__ unsigned long long masks[4];  // [wave]: frames base + wave*64 + bit
    const int64_t k = blockIdx.x;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};  // channels threadIdx.x + 256*j, d <= 1024
    for (long base = 0; base < n_frames; base += 256) {
        const long i = base + threadIdx.x;
        const unsigned long long bal = __ballot(i < n_frames && act_ids[i] == k);
        if (lane == 0) masks[wid] = bal;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned long long bits = masks[w];
            while (bits) {
                const int bit = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                const float* r = fs + (size_t)(base + w * 64 + bit) * d;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = threadIdx.x + 256 * j;
                    if (c < d) acc[j] += r[c];
                }
            }
        }
        __syncthreads();
    }
    float* out = d_table + (size_t)k * d;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = threadIdx.x + 256 * j;
        if (c < d) out[c] = (beta != 0.f ? beta * out[c] : 0.f) + acc[j];
    }
}
int launch_action_embed_bwd(const genie_cfg& c, const float* dx, const int64_t* act_ids, int n_act, int B, float* d_table,
                            float beta, float* frame_sums, hipStream_t st) {
    GENIE_CHECK_SHAPE(c.d_model <= 1024, "action embed backward: d_model > 1024");
    const long n_frames = (long)B * c.T;
    frame_sum_kernel<<<(unsigned)((n_frames * c.d_model + 255) / 256), 256, 0, st>>>(dx, frame_sums, n_frames, c.S, c.d_model);
    GENIE_LAUNCH_CHECK("frame_sum");
    action_bwd_kernel<<<(unsigned)n_act, 256, 0, st>>>(frame_sums, act_ids, n_frames, c.d_model, d_table, beta);
    GENIE_LAUNCH_CHECK("action_embed_bwd");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// optimizer: sum of squares (two-stage, f64) and torch.optim.AdamW's update with clip_grad_norm_ folded in
// ------------------------------------------------------------------------------------------------
constexpr int SUMSQ_BLOCKS = 1024;
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ x, size_t n, double* __restrict__ part) {
    __shared__ double red[4];
    double s = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double v = x[i];
        s += v * v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void sumsq_final_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double s = 0;
        for (int i = 0; i < n; ++i) s += part[i];
        *out += s;
    }
}
int launch_sumsq(const float* x, size_t n, double* out, double* scratch, hipStream_t st) {
    if (!n) return GENIE_OK;
    sumsq_partial_kernel<<<SUMSQ_BLOCKS, 256, 0, st>>>(x, n, scratch);
    GENIE_LAUNCH_CHECK("sumsq");
    sumsq_final_kernel<<<1, 64, 0, st>>>(scratch, SUMSQ_BLOCKS, out);
    GENIE_LAUNCH_CHECK("sumsq_final");
    return GENIE_OK;
}

// The AdamW update of one element, stated once for adamw_kernel and adamw_ema_kernel (the build does not contract: -ffp-contract=off).
struct AdamwScalars {
    float beta1, beta2, eps, decay, step_size, inv_sqrt_bc2;
};
// (adamw_coef, grad_mult times the clip coefficient of clip_grad_norm_, is stated in train_device.hpp: the Muon step shares it)
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, float coef, const AdamwScalars& a) {
    const float gi = g * coef;
    const float pi = p * a.decay;  // decoupled weight decay: p *= 1 - lr*wd
    const float mi = a.beta1 * m + (1.0f - a.beta1) * gi;
    const float vi = a.beta2 * v + (1.0f - a.beta2) * gi * gi;
    m = mi;
    v = vi;
    const float denom = sqrtf(vi) * a.inv_sqrt_bc2 + a.eps;
    p = pi - a.step_size * (mi / denom);
}
// (ema_element, LitEma.forward's line, is stated in train_device.hpp as well)

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                             float* __restrict__ v, size_t n, AdamwScalars a, float grad_mult, const double* __restrict__ sumsq,
                             float max_norm) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float pi = p[i], mi = m[i], vi = v[i];
    adamw_element(pi, g[i], mi, vi, adamw_coef(grad_mult, sumsq, max_norm), a);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
}
static AdamwScalars adamw_scalars(float lr, float beta1, float beta2, float eps, float weight_decay, int step) {
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    return {beta1, beta2, eps, (float)(1.0 - (double)lr * weight_decay), (float)(lr / bc1), (float)(1.0 / sqrt(bc2))};
}
int launch_adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int step, float grad_mult, const double* sumsq, float max_norm, hipStream_t st) {
    if (!n) return GENIE_OK;
    adamw_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(p, g, m, v, n, adamw_scalars(lr, beta1, beta2, eps, weight_decay, step),
                                                             grad_mult, sumsq, max_norm);
    GENIE_LAUNCH_CHECK("adamw");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// EMA of the weights: three streaming kernels of one shape.  Every thread walks float4 groups [0, n4) with a grid stride, 16 bytes per
// load and store, then the elements [4 n4, n) one at a time; the host gives n4 = n / 4 when every base pointer is 16-byte aligned and
// n4 = 0 (all of the range on the one-element path) when one is not.  The grid is capped at STREAM_MAX_BLOCKS workgroups of 256.
// No LDS, no atomics: the same bytes run to run.
// ------------------------------------------------------------------------------------------------
constexpr unsigned STREAM_MAX_BLOCKS = 2048;
struct StreamShape {
    size_t n4;
    unsigned blocks;
};
template <typename... P>
static StreamShape stream_shape(size_t n, const P*... base) {
    const bool aligned = (((uintptr_t)base | ...) & 15) == 0;
    const size_t n4 = aligned ? n / 4 : 0;
    const size_t items = n4 > n - 4 * n4 ? n4 : n - 4 * n4;   // the longer of the two loops
    const size_t blocks = (items + 255) / 256;
    return {n4, (unsigned)(blocks < STREAM_MAX_BLOCKS ? (blocks ? blocks : 1) : STREAM_MAX_BLOCKS)};
}

__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ ema, size_t n, size_t n4,
                                                        AdamwScalars a, float grad_mult, const double* __restrict__ sumsq,
                                                        float max_norm, float omd) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    const float coef = adamw_coef(grad_mult, sumsq, max_norm);
    for (size_t i = tid; i < n4; i += stride) {
        float4 p4 = reinterpret_cast<const float4*>(p)[i], m4 = reinterpret_cast<const float4*>(m)[i];
        float4 v4 = reinterpret_cast<const float4*>(v)[i], e4 = reinterpret_cast<const float4*>(ema)[i];
        const float4 g4 = reinterpret_cast<const float4*>(g)[i];
        adamw_element(p4.x, g4.x, m4.x, v4.x, coef, a);
        adamw_element(p4.y, g4.y, m4.y, v4.y, coef, a);
        adamw_element(p4.z, g4.z, m4.z, v4.z, coef, a);
        adamw_element(p4.w, g4.w, m4.w, v4.w, coef, a);
        e4.x = ema_element(e4.x, p4.x, omd);
        e4.y = ema_element(e4.y, p4.y, omd);
        e4.z = ema_element(e4.z, p4.z, omd);
        e4.w = ema_element(e4.w, p4.w, omd);
        reinterpret_cast<float4*>(m)[i] = m4;
        reinterpret_cast<float4*>(v)[i] = v4;
        reinterpret_cast<float4*>(p)[i] = p4;
        reinterpret_cast<float4*>(ema)[i] = e4;
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) {
        float pi = p[i], mi = m[i], vi = v[i];
        adamw_element(pi, g[i], mi, vi, coef, a);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
        ema[i] = ema_element(ema[i], pi, omd);
    }
}
int launch_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, size_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, float grad_mult, const double* sumsq, float max_norm, float omd, hipStream_t st) {
    if (!n) return GENIE_OK;
    const StreamShape s = stream_shape(n, p, g, m, v, ema);
    adamw_ema_kernel<<<s.blocks, 256, 0, st>>>(p, g, m, v, ema, n, s.n4, adamw_scalars(lr, beta1, beta2, eps, weight_decay, step),
                                               grad_mult, sumsq, max_norm, omd);
    GENIE_LAUNCH_CHECK("adamw_ema");
    return GENIE_OK;
}

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, size_t n, size_t n4,
                                                         float omd) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < n4; i += stride) {
        float4 e4 = reinterpret_cast<const float4*>(ema)[i];
        const float4 p4 = reinterpret_cast<const float4*>(p)[i];
        e4.x = ema_element(e4.x, p4.x, omd);
        e4.y = ema_element(e4.y, p4.y, omd);
        e4.z = ema_element(e4.z, p4.z, omd);
        e4.w = ema_element(e4.w, p4.w, omd);
        reinterpret_cast<float4*>(ema)[i] = e4;
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) ema[i] = ema_element(ema[i], p[i], omd);
}
int launch_ema_update(float* ema, const float* p, size_t n, float omd, hipStream_t st) {
    if (!n) return GENIE_OK;
    const StreamShape s = stream_shape(n, ema, p);
    ema_update_kernel<<<s.blocks, 256, 0, st>>>(ema, p, n, s.n4, omd);
    GENIE_LAUNCH_CHECK("ema_update");
    return GENIE_OK;
}

// a <-> b elementwise (the ranges do not overlap: checked by the entry point)
__global__ __launch_bounds__(256) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, size_t n, size_t n4) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < n4; i += stride) {
        const float4 a4 = reinterpret_cast<const float4*>(a)[i], b4 = reinterpret_cast<const float4*>(b)[i];
        reinterpret_cast<float4*>(a)[i] = b4;
        reinterpret_cast<float4*>(b)[i] = a4;
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) {
        const float ai = a[i], bi = b[i];
        a[i] = bi;
        b[i] = ai;
    }
}
int launch_swap_f32(float* a, float* b, size_t n, hipStream_t st) {
    if (!n) return GENIE_OK;
    const StreamShape s = stream_shape(n, a, b);
    swap_f32_kernel<<<s.blocks, 256, 0, st>>>(a, b, n, s.n4);
    GENIE_LAUNCH_CHECK("swap_f32");
    return GENIE_OK;
}

}  // namespace genie
