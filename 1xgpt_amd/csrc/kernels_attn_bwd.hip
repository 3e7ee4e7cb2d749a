// The f32 attention backward of the training step (kernels_train.hip holds the rest of it): the materialised-scores softmax
// pair, the causal temporal backward (an MFMA kernel for T = 16, its tiled form for T = 32 / 64, a scalar LDS kernel for the
// other geometries), the fused spatial backward, and the qk-norm forward / backward pair.  All three precisions take the
// temporal backward and qk-norm here; the bf16 precision has its own spatial backward (kernels_attn_bwd16.hip).
#include <type_traits>

#include "kernels.hpp"

namespace genie {

// ------------------------------------------------------------------------------------------------
// row softmax (in place) and its backward dS = P * (dP - sum_j P dP) (in place on dP); one wave per row
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void softmax_rows_kernel(float* __restrict__ P, long rows, int N) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float* p = P + (size_t)row * N;
    float m = -INFINITY;
    for (int j = lane; j < N; j += 64) m = fmaxf(m, p[j]);
    m = wave_max(m);
    float s = 0.f;
    for (int j = lane; j < N; j += 64) { const float e = expf(p[j] - m); p[j] = e; s += e; }
    const float inv = 1.0f / wave_sum(s);
    for (int j = lane; j < N; j += 64) p[j] *= inv;
}
__global__ __launch_bounds__(256) void softmax_bwd_rows_kernel(const float* __restrict__ P, float* __restrict__ dP,
                                                               long rows, int N) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* p = P + (size_t)row * N;
    float* g = dP + (size_t)row * N;
    float s = 0.f;
    for (int j = lane; j < N; j += 64) s += p[j] * g[j];
    s = wave_sum(s);
    for (int j = lane; j < N; j += 64) g[j] = p[j] * (g[j] - s);
}
int launch_softmax_rows(float* P, long rows, int N, hipStream_t st) {
    if (rows <= 0) return GENIE_OK;
    softmax_rows_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(P, rows, N);
    GENIE_LAUNCH_CHECK("softmax_rows");
    return GENIE_OK;
}
int launch_softmax_bwd_rows(const float* P, float* dP, long rows, int N, hipStream_t st) {
    if (rows <= 0) return GENIE_OK;
    softmax_bwd_rows_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(P, dP, rows, N);
    GENIE_LAUNCH_CHECK("softmax_bwd_rows");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// Temporal (causal, N = T <= 16 frames) attention backward on the frame-strided rows of (B,T,S,3d) -- the
// "(B S) T C" view of st_transformer.py:77 without a transpose.  One thread per (sequence, head, frame i);
// a block holds GPB (sequence, head) groups of 16 threads; q (pre-scaled), k, v, dO rows sit in LDS.
//   p_ij = softmax_j(scale q_i.k_j), j <= i;  dp_ij = dO_i.v_j;  ds_ij = p_ij (dp_ij - sum_j p_ij dp_ij)
//   dq_i = scale sum_j ds_ij k_j;  dk_j = scale sum_{i>=j} ds_ij q_i;  dv_j = sum_{i>=j} p_ij dO_i
// ------------------------------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(64) void attn_temporal_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ qk,
                                                               long qk_ld, const float* __restrict__ dO,
                                                               float* __restrict__ dqkv, int B, int T, int S, int d, int H,
                                                               float scale) {
    constexpr int GPB = 4, NMAX = 16, DHP = DH + 4;  // padded rows: threads of a group read different rows, same column
    extern __shared__ float sm[];
    const int g = threadIdx.x >> 4, i = threadIdx.x & 15;
    float* sq = sm + (size_t)g * (4 * NMAX * DHP + 2 * NMAX * NMAX);
    float* sk = sq + NMAX * DHP;
    float* sv = sk + NMAX * DHP;
    float* sd = sv + NMAX * DHP;
    float* sp = sd + NMAX * DHP;  // [i][j]
    float* sds = sp + NMAX * NMAX;
    const long grp = (long)blockIdx.x * GPB + g;  // (b, s, head)
    const long n_grp = (long)B * S * H;
    const bool active = grp < n_grp && i < T;
    long row = 0;
    int head = 0;
    if (active) {
        head = (int)(grp % H);
        const long bs = grp / H;
        const long b = bs / S, s = bs - b * S;
        row = (b * T + i) * (long)S + s;
        const float* base = qkv + (size_t)row * 3 * d + head * DH;
        const float* qb = qk + (size_t)row * qk_ld + head * DH;  // q at column 0, k at column d of the (normalised) source
        const float* dob = dO + (size_t)row * d + head * DH;
#pragma unroll 4
        for (int c = 0; c < DH; c += 4) {
            float4 q4 = *reinterpret_cast<const float4*>(qb + c);
            q4.x *= scale; q4.y *= scale; q4.z *= scale; q4.w *= scale;
            *reinterpret_cast<float4*>(sq + i * DHP + c) = q4;
            *reinterpret_cast<float4*>(sk + i * DHP + c) = *reinterpret_cast<const float4*>(qb + d + c);
            *reinterpret_cast<float4*>(sv + i * DHP + c) = *reinterpret_cast<const float4*>(base + 2 * d + c);
            *reinterpret_cast<float4*>(sd + i * DHP + c) = *reinterpret_cast<const float4*>(dob + c);
        }
    }
    __syncthreads();
    float acc[DH];
    if (active) {
        float p[NMAX], dp[NMAX];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            float s = 0.f, t = 0.f;
            if (j <= i) {
#pragma unroll 8
                for (int c = 0; c < DH; ++c) {
                    s = fmaf(sq[i * DHP + c], sk[j * DHP + c], s);
                    t = fmaf(sd[i * DHP + c], sv[j * DHP + c], t);
                }
                m = fmaxf(m, s);
            }
            p[j] = s; dp[j] = t;
        }
        float l = 0.f;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            p[j] = j <= i ? expf(p[j] - m) : 0.f;
            l += p[j];
        }
        const float inv = 1.0f / l;
        float dsum = 0.f;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) { p[j] *= inv; dsum += p[j] * dp[j]; }
#pragma unroll
        for (int c = 0; c < DH; ++c) acc[c] = 0.f;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            const float ds = p[j] * (dp[j] - dsum);  // p[j] = 0 beyond the causal bound
            sp[i * NMAX + j] = p[j];
            sds[i * NMAX + j] = ds;
            if (j <= i) {
#pragma unroll 8
                for (int c = 0; c < DH; ++c) acc[c] = fmaf(ds, sk[j * DHP + c], acc[c]);
            }
        }
        float* o = dqkv + (size_t)row * 3 * d + head * DH;
#pragma unroll 4
        for (int c = 0; c < DH; c += 4)
            *reinterpret_cast<float4*>(o + c) =
                make_float4(acc[c] * scale, acc[c + 1] * scale, acc[c + 2] * scale, acc[c + 3] * scale);
    }
    __syncthreads();
    if (active) {
        const int j = i;
        float* o = dqkv + (size_t)row * 3 * d + head * DH;
        // dk_j: sq holds scale*q, so sum_i ds_ij * sq_i is already the scaled product
#pragma unroll
        for (int c = 0; c < DH; ++c) acc[c] = 0.f;
        for (int ii = j; ii < T; ++ii) {
            const float ds = sds[ii * NMAX + j];
#pragma unroll 8
            for (int c = 0; c < DH; ++c) acc[c] = fmaf(ds, sq[ii * DHP + c], acc[c]);
        }
#pragma unroll 4
        for (int c = 0; c < DH; c += 4)
            *reinterpret_cast<float4*>(o + d + c) = make_float4(acc[c], acc[c + 1], acc[c + 2], acc[c + 3]);
#pragma unroll
        for (int c = 0; c < DH; ++c) acc[c] = 0.f;
        for (int ii = j; ii < T; ++ii) {
            const float pp = sp[ii * NMAX + j];
#pragma unroll 8
            for (int c = 0; c < DH; ++c) acc[c] = fmaf(pp, sd[ii * DHP + c], acc[c]);
        }
#pragma unroll 4
        for (int c = 0; c < DH; c += 4)
            *reinterpret_cast<float4*>(o + 2 * d + c) = make_float4(acc[c], acc[c + 1], acc[c + 2], acc[c + 3]);
    }
}
// ------------------------------------------------------------------------------------------------
// The same backward for the production geometry (T = 16 frames, head_dim 32 / 64) on v_mfma_f32_16x16x4_f32: one
// WAVE per (b, s, head), no LDS.  The 16x16 MFMA D tile puts D[4g+e][r] in lane (r = lane&15, g = lane>>4), so a
// 16x16 score matrix is available in two register layouts, chosen by operand order:
//     T-layout  mfma(k, q)  -> lane (r,g) holds X[i = r][j = 4g+e]   (row i across the 4 lane groups; the forward's)
//     N-layout  mfma(q, k)  -> lane (r,g) holds X[i = 4g+e][j = r]
// and a tile held in T-layout is directly the A operand (row r, contraction index 4g+e) of a product contracted over
// j, one held in N-layout of a product contracted over i.  So:  P, dP, dS are computed in BOTH layouts (4 x DH/4
// MFMAs); dQ = scale dS K uses the T copy, dK = scale dS^T Q and dV = P^T dO the N copy; row statistics (max, 1/sum,
// D_i = sum_j P dP) are reduced once in the T layout and fetched by lane index for the N layout.
// Feature permutation of the forward kernel: MFMA output column r of chunk c is feature NV*r + c (NV = DH/16), so
// every global access is NV contiguous floats per lane.
// The T = 32 / 64 kernel behind it is made of the same steps, stated once here for both (NT tiles of 16 keys to a tile row; the
// T = 16 kernel is NT = 1, I = 0).  The other steps stay written out in each kernel; as shared functions the row-operand loads and
// the gradient products take the (head_dim 64, T = 64) instantiation past its 480 registers, and the row statistics and the
// N-layout P / dS measured slower (profiles/attn_bwd_refactor_ab.txt).
// ------------------------------------------------------------------------------------------------
// NV contiguous features of one row as one 8- or 16-byte access: the B operands and the outputs
template <int NV>
__device__ __forceinline__ void load_nv(const float* __restrict__ p, float (&o)[NV]) {
    if constexpr (NV == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    } else {
        const float2 a = *reinterpret_cast<const float2*>(p);
        o[0] = a.x; o[1] = a.y;
    }
}
template <int NV>
__device__ __forceinline__ void store_nv(float* __restrict__ p, const f32x4 (&x)[NV], int e, float mul) {
    if constexpr (NV == 4)
        *reinterpret_cast<float4*>(p) = make_float4(x[0][e] * mul, x[1][e] * mul, x[2][e] * mul, x[3][e] * mul);
    else
        *reinterpret_cast<float2*>(p) = make_float2(x[0][e] * mul, x[1][e] * mul);
}
// S and dP of one 16 x 16 tile in both layouts, as CHAINS accumulator chains per product (c mod CHAINS), added at the end
template <int CHAINS, int PER>
__device__ __forceinline__ void score_tile(const float (&q)[PER], const float (&k)[PER], const float (&v)[PER],
                                           const float (&go)[PER], f32x4& sT, f32x4& pT, f32x4& sN, f32x4& pN) {
    f32x4 a[CHAINS][4];
#pragma unroll
    for (int h = 0; h < CHAINS; ++h)
#pragma unroll
        for (int m = 0; m < 4; ++m) a[h][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        f32x4(&x)[4] = a[c % CHAINS];
        x[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(k[c], q[c], x[0], 0, 0, 0);   // S[i=r][j=4g+e]
        x[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[c], go[c], x[1], 0, 0, 0);  // dP[i=r][j=4g+e]
        x[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(q[c], k[c], x[2], 0, 0, 0);   // S[i=4g+e][j=r]
        x[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(go[c], v[c], x[3], 0, 0, 0);  // dP[i=4g+e][j=r]
    }
    if constexpr (CHAINS == 2) {
        sT = a[0][0] + a[1][0]; pT = a[0][1] + a[1][1]; sN = a[0][2] + a[1][2]; pN = a[0][3] + a[1][3];
    } else {
        sT = a[0][0]; pT = a[0][1]; sN = a[0][2]; pN = a[0][3];
    }
}
// The statistics of row 16I + 4g+e for the N layout come from lane 4g+e (any group holds them)
__device__ __forceinline__ void fetch_row_stat(float mx, float inv, float dsum, int i, float& mi, float& ii, float& di) {
    mi = __shfl(mx, i); ii = __shfl(inv, i); di = __shfl(dsum, i);
}

template <int DH>
__global__ __launch_bounds__(256) void attn_temporal_bwd_mfma_kernel(const float* __restrict__ qkv,
                                                                     const float* __restrict__ qk, long qk_ld,
                                                                     const float* __restrict__ dO,
                                                                     float* __restrict__ dqkv, long n_bs, int S, int d,
                                                                     int H, float scale) {
    constexpr int T = 16, PER = DH / 4, NV = DH / 16;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, g = lane >> 4;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long bs = wave / H;
    const int head = (int)(wave - bs * H);
    if (bs >= n_bs) return;
    const long b = bs / S, s = bs - b * S;
    const size_t row0 = (size_t)(b * T) * S + s;  // token row of frame 0; frame t is row0 + t*S
    const float* qb = qk + row0 * qk_ld + head * DH;          // q at column 0, k at column d
    const float* vb = qkv + row0 * 3 * d + 2 * d + head * DH;
    const float* ob = dO + row0 * d + head * DH;
    const long qs = (long)S * qk_ld, vs = (long)S * 3 * d, os = (long)S * d;
    // ---- row operands: lane (r,g) holds features g*PER .. of row r
    float q[PER], k[PER], v[PER], go[PER];
#pragma unroll
    for (int c = 0; c < PER; c += 4) {
        const float4 a = *reinterpret_cast<const float4*>(qb + (size_t)r * qs + g * PER + c);
        const float4 bb = *reinterpret_cast<const float4*>(qb + (size_t)r * qs + d + g * PER + c);
        const float4 cc = *reinterpret_cast<const float4*>(vb + (size_t)r * vs + g * PER + c);
        const float4 dd = *reinterpret_cast<const float4*>(ob + (size_t)r * os + g * PER + c);
        q[c] = a.x * scale; q[c + 1] = a.y * scale; q[c + 2] = a.z * scale; q[c + 3] = a.w * scale;
        k[c] = bb.x; k[c + 1] = bb.y; k[c + 2] = bb.z; k[c + 3] = bb.w;
        v[c] = cc.x; v[c + 1] = cc.y; v[c + 2] = cc.z; v[c + 3] = cc.w;
        go[c] = dd.x; go[c + 1] = dd.y; go[c + 2] = dd.z; go[c + 3] = dd.w;
    }
    f32x4 sT, pT, sN, pN;
    score_tile<1, PER>(q, k, v, go, sT, pT, sN, pN);
    // ---- softmax statistics of row i = r in the T layout (causal: j <= i)
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (4 * g + e > r) sT[e] = -INFINITY;
        mx = fmaxf(mx, sT[e]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { sT[e] = expf(sT[e] - mx); sum += sT[e]; }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    float dsum = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { sT[e] *= inv; dsum += sT[e] * pT[e]; }
    dsum += __shfl_xor(dsum, 16);
    dsum += __shfl_xor(dsum, 32);
    f32x4 dsT, dsN, prN;
#pragma unroll
    for (int e = 0; e < 4; ++e) dsT[e] = sT[e] * (pT[e] - dsum);  // masked entries: P = 0
    // ---- the same in the N layout
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = 4 * g + e;
        float mi, ii, di;
        fetch_row_stat(mx, inv, dsum, i, mi, ii, di);
        const float p = r <= i ? expf(sN[e] - mi) * ii : 0.f;
        prN[e] = p;
        dsN[e] = p * (pN[e] - di);
    }
    // ---- dQ = scale dS K,  dK = scale dS^T Q,  dV = P^T dO: B operands are rows 4g+e, features NV*r .. NV*r+NV-1
    float kk[4][NV], qq[4][NV], dd[4][NV];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const size_t t = (size_t)(4 * g + e);
        load_nv<NV>(qb + t * qs + d + NV * r, kk[e]);
        load_nv<NV>(qb + t * qs + NV * r, qq[e]);
        load_nv<NV>(ob + t * os + NV * r, dd[e]);
    }
    f32x4 dq[NV], dk[NV], dv[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        dq[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        dk[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        dv[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dq[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsT[e], kk[e][c], dq[c], 0, 0, 0);
            dk[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsN[e], qq[e][c], dk[c], 0, 0, 0);
            dv[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(prN[e], dd[e][c], dv[c], 0, 0, 0);
        }
    }
    // D map: lane (r,g) holds rows 4g+e, features NV*r + c
    float* outb = dqkv + row0 * 3 * d + head * DH + NV * r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float* o = outb + (size_t)(4 * g + e) * vs;
        store_nv<NV>(o, dq, e, scale);
        store_nv<NV>(o + d, dk, e, scale);
        store_nv<NV>(o + 2 * d, dv, e, 1.0f);
    }
}

// ------------------------------------------------------------------------------------------------
// The same backward for T = 16 NT frames, NT = 2 / 4 (T = 32 / 64), head_dim 32 / 64: still one wave per (b, s, head) and no
// LDS; the T x T scores are the lower triangle of NT x NT tiles of 16 x 16, each computed as in the T = 16 kernel (both layouts,
// the same operand fragments and feature permutation).  Tile row I (queries 16I .. 16I+15) is the outer loop:
//   S and dP of its I+1 tiles in both layouts stay in registers (<= 64 VGPRs); only the diagonal tile J = I is masked;
//   max, 1/sum and D_i run over the whole tile row in the T layout (in-lane over tiles and e, then the two cross-group
//   shuffles) and are fetched by lane index for the N layout;
//   dQ_I = scale sum_J dS_IJ K_J is complete when the row ends and is stored once;
//   dK_J += dS_IJ^T Q_I and dV_J += P_IJ^T dO_I accumulate in NT x 2 x NV register quads (128 VGPRs at T = 64, head_dim 64),
//   in increasing I, and are stored once after the last row.
// Nothing is kept between tiles but those: the K / V fragments of tile J are read again for every I >= J (L2 hits: a head's
// rows are DH contiguous floats per frame, at most 3 x 16 KB per wave).  Every loop is unrolled (register arrays).
// ------------------------------------------------------------------------------------------------
template <int DH, int NT>
__global__ __launch_bounds__(256) void attn_temporal_bwd_tiled_kernel(const float* __restrict__ qkv,
                                                                      const float* __restrict__ qk, long qk_ld,
                                                                      const float* __restrict__ dO,
                                                                      float* __restrict__ dqkv, long n_bs, int S, int d,
                                                                      int H, float scale) {
    constexpr int T = 16 * NT, PER = DH / 4, NV = DH / 16;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, g = lane >> 4;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long bs = wave / H;
    const int head = (int)(wave - bs * H);
    if (bs >= n_bs) return;
    const long b = bs / S, s = bs - b * S;
    const size_t row0 = (size_t)(b * T) * S + s;  // token row of frame 0; frame t is row0 + t*S
    const float* qb = qk + row0 * qk_ld + head * DH;          // q at column 0, k at column d
    const float* vb = qkv + row0 * 3 * d + 2 * d + head * DH;
    const float* ob = dO + row0 * d + head * DH;
    float* outb = dqkv + row0 * 3 * d + head * DH + NV * r;   // D map: lane (r,g) holds rows 4g+e, features NV*r + c
    const long qs = (long)S * qk_ld, vs = (long)S * 3 * d, os = (long)S * d;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 dk[NT][NV], dv[NT][NV];
#pragma unroll
    for (int J = 0; J < NT; ++J)
#pragma unroll
        for (int c = 0; c < NV; ++c) { dk[J][c] = zero; dv[J][c] = zero; }
#pragma unroll
    for (int I = 0; I < NT; ++I) {
        // ---- row operands of the tile row: lane (r,g) holds features g*PER .. of frame 16I + r
        float q[PER], go[PER];
        {
            const size_t t = (size_t)(16 * I + r);
#pragma unroll
            for (int c = 0; c < PER; c += 4) {
                const float4 a = *reinterpret_cast<const float4*>(qb + t * qs + g * PER + c);
                const float4 dd = *reinterpret_cast<const float4*>(ob + t * os + g * PER + c);
                q[c] = a.x * scale; q[c + 1] = a.y * scale; q[c + 2] = a.z * scale; q[c + 3] = a.w * scale;
                go[c] = dd.x; go[c + 1] = dd.y; go[c + 2] = dd.z; go[c + 3] = dd.w;
            }
        }
        f32x4 sT[NT], pT[NT], sN[NT], pN[NT];
#pragma unroll
        for (int J = 0; J < NT; ++J) {
            if (J > I) continue;
            const size_t t = (size_t)(16 * J + r);
            float k[PER], v[PER];
#pragma unroll
            for (int c = 0; c < PER; c += 4) {
                const float4 bb = *reinterpret_cast<const float4*>(qb + t * qs + d + g * PER + c);
                const float4 cc = *reinterpret_cast<const float4*>(vb + t * vs + g * PER + c);
                k[c] = bb.x; k[c + 1] = bb.y; k[c + 2] = bb.z; k[c + 3] = bb.w;
                v[c] = cc.x; v[c + 1] = cc.y; v[c + 2] = cc.z; v[c + 3] = cc.w;
            }
            // two accumulator chains per product (even / odd c), added at the end: half the chain length -- with sharp softmax rows
            // (|s| ~ 16) the rounding of a DH/4-long f32 chain in the scores was the largest error of the whole backward
            score_tile<2, PER>(q, k, v, go, sT[J], pT[J], sN[J], pN[J]);
            // keep the next tile's operand loads behind this tile: hoisted across the unrolled tiles they cost more registers than
            // one wave has (T = 64, head_dim 64)
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- softmax statistics of row i = 16I + r in the T layout (causal: only the diagonal tile has j > i)
        float mx = -INFINITY;
#pragma unroll
        for (int J = 0; J < NT; ++J) {
            if (J > I) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (J == I && 4 * g + e > r) sT[J][e] = -INFINITY;
                mx = fmaxf(mx, sT[J][e]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int J = 0; J < NT; ++J) {
            if (J > I) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) { sT[J][e] = expf(sT[J][e] - mx); sum += sT[J][e]; }
        }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
        float dsum = 0.f;
#pragma unroll
        for (int J = 0; J < NT; ++J) {
            if (J > I) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) { sT[J][e] *= inv; dsum += sT[J][e] * pT[J][e]; }
        }
        dsum += __shfl_xor(dsum, 16);
        dsum += __shfl_xor(dsum, 32);
        // ---- ... and those of row 16I + 4g+e for the N layout
        float mi[4], ii[4], di[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) fetch_row_stat(mx, inv, dsum, 4 * g + e, mi[e], ii[e], di[e]);
        // ---- B operands of the tile row's frames 16I + 4g+e, features NV*r .. NV*r+NV-1
        float qq[4][NV], dd[4][NV];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const size_t t = (size_t)(16 * I + 4 * g + e);
            load_nv<NV>(qb + t * qs + NV * r, qq[e]);
            load_nv<NV>(ob + t * os + NV * r, dd[e]);
        }
        f32x4 dq[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) dq[c] = zero;
#pragma unroll
        for (int J = 0; J < NT; ++J) {
            if (J > I) continue;
            f32x4 dsT, dsN, prN;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dsT[e] = sT[J][e] * (pT[J][e] - dsum);  // masked entries: P = 0
                const float p = (J < I || r <= 4 * g + e) ? expf(sN[J][e] - mi[e]) * ii[e] : 0.f;
                prN[e] = p;
                dsN[e] = p * (pN[J][e] - di[e]);
            }
            float kk[4][NV];
#pragma unroll
            for (int e = 0; e < 4; ++e) load_nv<NV>(qb + (size_t)(16 * J + 4 * g + e) * qs + d + NV * r, kk[e]);
#pragma unroll
            for (int c = 0; c < NV; ++c) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dq[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsT[e], kk[e][c], dq[c], 0, 0, 0);
                    dk[J][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(dsN[e], qq[e][c], dk[J][c], 0, 0, 0);
                    dv[J][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(prN[e], dd[e][c], dv[J][c], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) store_nv<NV>(outb + (size_t)(16 * I + 4 * g + e) * vs, dq, e, scale);
    }
    // qq holds the UNSCALED q (the scores used scale*q), so dK takes the scale here, as dQ does
#pragma unroll
    for (int J = 0; J < NT; ++J) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float* o = outb + (size_t)(16 * J + 4 * g + e) * vs;
            store_nv<NV>(o + d, dk[J], e, scale);
            store_nv<NV>(o + 2 * d, dv[J], e, 1.0f);
        }
    }
}

// Runs f(std::integral_constant<int, V>()) for the V among VS that equals v; false: v is not among VS
template <int... VS, class F>
static bool for_value(int v, F&& f) {
    return ((v == VS && (f(std::integral_constant<int, VS>()), true)) || ...);
}

int launch_attn_temporal_bwd(const float* qkv, const float* qk, long qk_ld, const float* dO, float* dqkv, int B, int T,
                             int S, int d, int H, int Dh, float scale, hipStream_t st) {
    GENIE_CHECK_SHAPE(T <= 64, "temporal attention backward: T=%d > 64", T);
    GENIE_CHECK_SHAPE(T <= 16 || ((T == 32 || T == 64) && (Dh == 32 || Dh == 64)),
                      "temporal attention backward: T=%d > 16 needs T in {32, 64} and head_dim in {32, 64}, not %d", T, Dh);
    const long n_grp = (long)B * S * H;
    if (n_grp <= 0) return GENIE_OK;
    ProfScope prof(GENIE_KC_ATTN_TEMPORAL, 10.0 * n_grp * T * T * Dh, 4.0 * n_grp * T * Dh * 7, st, "attn_temporal_bwd");
    const unsigned blocks = (unsigned)((n_grp + 3) / 4);
    if (T >= 16 && (Dh == 64 || Dh == 32)) {   // T is 16, 32 or 64 here
        const long n_bs = (long)B * S;
        for_value<32, 64>(Dh, [&](auto dh) {
            constexpr int DH = decltype(dh)::value;
            if (T == 16) {
                attn_temporal_bwd_mfma_kernel<DH><<<blocks, 256, 0, st>>>(qkv, qk, qk_ld, dO, dqkv, n_bs, S, d, H, scale);
            } else {
                for_value<2, 4>(T / 16, [&](auto nt) {
                    constexpr int NT = decltype(nt)::value;
                    attn_temporal_bwd_tiled_kernel<DH, NT><<<blocks, 256, 0, st>>>(qkv, qk, qk_ld, dO, dqkv, n_bs, S, d, H, scale);
                });
            }
        });
        GENIE_LAUNCH_CHECK(T == 16 ? "attn_temporal_bwd_mfma" : "attn_temporal_bwd_tiled");
        return GENIE_OK;
    }
#define TB_LAUNCH(DH_)                                                                                       \
    {                                                                                                        \
        const size_t lds = (size_t)4 * (4 * 16 * (DH_ + 4) + 2 * 16 * 16) * sizeof(float);                        \
        (void)hipFuncSetAttribute((const void*)attn_temporal_bwd_kernel<DH_>,                                \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                     \
        attn_temporal_bwd_kernel<DH_><<<blocks, 64, lds, st>>>(qkv, qk, qk_ld, dO, dqkv, B, T, S, d, H, scale); \
    }
    if (Dh == 64) TB_LAUNCH(64)
    else if (Dh == 32) TB_LAUNCH(32)
    else if (Dh == 128) TB_LAUNCH(128)
    else {
        set_error("temporal attention backward: head_dim %d not in {32, 64, 128}", Dh);
        return GENIE_E_UNSUPPORTED;
    }
#undef TB_LAUNCH
    GENIE_LAUNCH_CHECK("attn_temporal_bwd");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// Spatial attention backward, fused (S = 256 tokens of one frame, head_dim 32 / 64, non-causal): one workgroup of 4
// waves per (b, t, head); K and V of the head stay in LDS (2 x 68 KB at head_dim 64, rows padded to DH+4 floats so
// the k-permuted ds_read_b128 fragments are conflict-free), queries are streamed in blocks of 32 rows.  Wave w owns
// keys [64w, 64w+64).  Per query block, on v_mfma_f32_32x32x2_f32:
//   [two passes over the query blocks -- pass A: T layout, statistics and dQ; pass B: N layout, dK and dV -- so that only
//   one layout's tiles are live at a time (the single-pass form needed all 512 registers and spilled)]
//   S = scale Q K^T and dP = dO V^T in BOTH register layouts (the same operand fragments, swapped): T-layout = one
//     query row per lane (softmax statistics: in-lane + one cross-half shuffle + a 3-value exchange between the 4 waves,
//     combined like an online softmax), N-layout = one key column per lane;
//   dS = P (dP - D), D_i = sum_j P dP;   dQ_i += dS K (A = dS in T-layout, partial over the wave's 64 keys, reduced over
//     the 4 waves through LDS in a FIXED order);   dK += dS^T Q_i and dV += P^T dO_i (A = N-layout tiles), accumulated in
//     registers over the 8 query blocks and written once.
// Nothing of size S x S ever touches HBM: 7 d floats per token in, 3 d out.  ~450 VGPRs at one wave per SIMD.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rowmap32(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

template <int DH>
__global__ __launch_bounds__(256, 1) void attn_spatial_bwd_fused_kernel(const float* __restrict__ qkv,
                                                                        const float* __restrict__ qk, long qk_ld,
                                                                        const float* __restrict__ dO,
                                                                        float* __restrict__ dqkv, int d, int H,
                                                                        float scale) {
    constexpr int S = 256, LD = DH + 4, IB = 32, NF = DH / 32, NKK = DH / 8, NPF = IB * DH / 4 / 256;
    static_assert(NPF >= 1, "head_dim >= 32");
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* sK = sm;
    float* sV = sK + S * LD;
    float* sQ = sV + S * LD;
    float* sdO = sQ + IB * LD;
    float* sPM = sdO + IB * LD;  // per-wave partial statistics [4][32]
    float* sPL = sPM + 128;
    float* sPD = sPL + 128;
    float* stM = sPD + 128;      // final row max (log2 units) / 1/sum / D for all 256 query rows (pass A -> pass B)
    float* stI = stM + S;
    float* stD = stI + S;
    float* red = sQ;             // dQ reduction buffer [4][16][DH], aliases sQ | sdO
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane & 31, h = lane >> 5;
    const long bt = blockIdx.x / H;
    const int head = (int)(blockIdx.x - bt * H);
    const size_t row0 = (size_t)bt * S;
    const float* qb = qk + row0 * qk_ld + head * DH;
    const float* kb = qb + d;
    const float* vb = qkv + row0 * 3 * d + 2 * d + head * DH;
    const float* ob = dO + row0 * d + head * DH;
    float* outb = dqkv + row0 * 3 * d + head * DH;
    // scores are carried as s*log2(e) so that every exponential is one v_exp_f32 (the probabilities are the same)
    const float scale_l2 = scale * 1.4426950408889634f;

    for (int idx = tid; idx < S * DH / 4; idx += 256) {
        const int row = idx / (DH / 4), c4 = (idx % (DH / 4)) * 4;
        *reinterpret_cast<float4*>(&sK[row * LD + c4]) = *reinterpret_cast<const float4*>(kb + (size_t)row * qk_ld + c4);
        *reinterpret_cast<float4*>(&sV[row * LD + c4]) = *reinterpret_cast<const float4*>(vb + (size_t)row * 3 * d + c4);
    }
    float4 pq[NPF], pd[NPF];
    auto fetch = [&](int ib) {
#pragma unroll
        for (int p = 0; p < NPF; ++p) {
            const int idx = tid + 256 * p, row = idx / (DH / 4), c4 = (idx % (DH / 4)) * 4;
            pq[p] = *reinterpret_cast<const float4*>(qb + (size_t)(ib * IB + row) * qk_ld + c4);
            pd[p] = *reinterpret_cast<const float4*>(ob + (size_t)(ib * IB + row) * d + c4);
        }
    };
    auto publish = [&]() {  // prefetched Q_i, dO_i -> LDS
#pragma unroll
        for (int p = 0; p < NPF; ++p) {
            const int idx = tid + 256 * p, row = idx / (DH / 4), c4 = (idx % (DH / 4)) * 4;
            *reinterpret_cast<float4*>(&sQ[row * LD + c4]) = pq[p];
            *reinterpret_cast<float4*>(&sdO[row * LD + c4]) = pd[p];
        }
    };

    // ================= pass A: T layout (one query row per lane): row statistics and dQ =================
    fetch(0);
    for (int ib = 0; ib < S / IB; ++ib) {
        publish();
        __syncthreads();  // Q_i, dO_i (and K, V on the first pass) are in LDS
        fetch(ib + 1 < S / IB ? ib + 1 : 0);  // next block; after the last one: block 0 again for pass B
        f32x16 sT[2], pT[2];
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) { sT[jt][e] = 0.f; pT[jt][e] = 0.f; }
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
            const int jrow = w * 64 + jt * 32 + c;
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                const float4 kf = *reinterpret_cast<const float4*>(&sK[jrow * LD + kk * 8 + 4 * h]);
                const float4 vf = *reinterpret_cast<const float4*>(&sV[jrow * LD + kk * 8 + 4 * h]);
                const float4 qf = *reinterpret_cast<const float4*>(&sQ[c * LD + kk * 8 + 4 * h]);
                const float4 of = *reinterpret_cast<const float4*>(&sdO[c * LD + kk * 8 + 4 * h]);
#define SP_STEP(X)                                                              \
    sT[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.X, qf.X, sT[jt], 0, 0, 0); \
    pT[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.X, of.X, pT[jt], 0, 0, 0);
                SP_STEP(x) SP_STEP(y) SP_STEP(z) SP_STEP(w)
#undef SP_STEP
            }
        }
        // lane (c, h) holds S[i = c][j = 64w + 32jt + rowmap(e, h)]: statistics of row c over this wave's keys
        float m = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) { sT[jt][e] *= scale_l2; m = fmaxf(m, sT[jt][e]); }
        m = fmaxf(m, __shfl_xor(m, 32));
        float l = 0.f, ds = 0.f;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = __builtin_amdgcn_exp2f(sT[jt][e] - m);
                sT[jt][e] = p;
                l += p;
                ds += p * pT[jt][e];
            }
        l += __shfl_xor(l, 32);
        ds += __shfl_xor(ds, 32);
        if (h == 0) { sPM[w * 32 + c] = m; sPL[w * 32 + c] = l; sPD[w * 32 + c] = ds; }
        __syncthreads();
        float gm = sPM[c];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww) gm = fmaxf(gm, sPM[ww * 32 + c]);
        float gl = 0.f, gd = 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) {
            const float f = __builtin_amdgcn_exp2f(sPM[ww * 32 + c] - gm);
            gl += sPL[ww * 32 + c] * f;
            gd += sPD[ww * 32 + c] * f;
        }
        const float inv = 1.0f / gl, Di = gd * inv;
        if (w == 0 && h == 0) { stM[ib * IB + c] = gm; stI[ib * IB + c] = inv; stD[ib * IB + c] = Di; }
        const float corr = __builtin_amdgcn_exp2f(m - gm) * inv;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) sT[jt][e] = sT[jt][e] * corr * (pT[jt][e] - Di);  // dS
        // dQ partial over this wave's 64 keys: A = dS (row c, contraction index = key rowmap(e, h))
        f32x16 dq[NF];
#pragma unroll
        for (int ft = 0; ft < NF; ++ft)
#pragma unroll
            for (int e = 0; e < 16; ++e) dq[ft][e] = 0.f;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float* kr = &sK[(w * 64 + jt * 32 + rowmap32(e, h)) * LD + c];
#pragma unroll
                for (int ft = 0; ft < NF; ++ft)
                    dq[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(sT[jt][e], kr[32 * ft], dq[ft], 0, 0, 0);
            }
        __syncthreads();  // every wave is done with sQ / sdO and the partial statistics
#pragma unroll
        for (int round = 0; round < 2; ++round) {
#pragma unroll
            for (int ft = 0; ft < NF; ++ft)
#pragma unroll
                for (int e8 = 0; e8 < 8; ++e8) {
                    const int e = 8 * round + e8;
                    red[(w * 16 + rowmap32(e, h) - 16 * round) * DH + 32 * ft + c] = dq[ft][e];
                }
            __syncthreads();
            if (tid < 16 * DH / 4) {
                const int row = tid / (DH / 4), f4 = (tid % (DH / 4)) * 4;
                float4 a = *reinterpret_cast<const float4*>(&red[row * DH + f4]);
#pragma unroll
                for (int ww = 1; ww < 4; ++ww) {
                    const float4 b = *reinterpret_cast<const float4*>(&red[(ww * 16 + row) * DH + f4]);
                    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
                }
                a.x *= scale; a.y *= scale; a.z *= scale; a.w *= scale;
                *reinterpret_cast<float4*>(outb + (size_t)(ib * IB + 16 * round + row) * 3 * d + f4) = a;
            }
            __syncthreads();
        }
    }

    // ================= pass B: N layout (one key column per lane): dK and dV =================
    f32x16 dk[2][NF], dv[2][NF];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int ft = 0; ft < NF; ++ft)
#pragma unroll
            for (int e = 0; e < 16; ++e) { dk[jt][ft][e] = 0.f; dv[jt][ft][e] = 0.f; }
    for (int ib = 0; ib < S / IB; ++ib) {
        publish();
        __syncthreads();
        if (ib + 1 < S / IB) fetch(ib + 1);
        f32x16 sN[2], pN[2];
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) { sN[jt][e] = 0.f; pN[jt][e] = 0.f; }
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
            const int jrow = w * 64 + jt * 32 + c;
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                const float4 kf = *reinterpret_cast<const float4*>(&sK[jrow * LD + kk * 8 + 4 * h]);
                const float4 vf = *reinterpret_cast<const float4*>(&sV[jrow * LD + kk * 8 + 4 * h]);
                const float4 qf = *reinterpret_cast<const float4*>(&sQ[c * LD + kk * 8 + 4 * h]);
                const float4 of = *reinterpret_cast<const float4*>(&sdO[c * LD + kk * 8 + 4 * h]);
#define SP_STEP(X)                                                              \
    sN[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(qf.X, kf.X, sN[jt], 0, 0, 0); \
    pN[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(of.X, vf.X, pN[jt], 0, 0, 0);
                SP_STEP(x) SP_STEP(y) SP_STEP(z) SP_STEP(w)
#undef SP_STEP
            }
        }
        // lane (c, h) holds X[i = rowmap(e, h)][j = 64w + 32jt + c]; the statistics of row i were published by pass A
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = ib * IB + rowmap32(e, h);
            const float mi = stM[i], ii = stI[i], di = stD[i];
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
                const float p = __builtin_amdgcn_exp2f(fmaf(sN[jt][e], scale_l2, -mi)) * ii;
                sN[jt][e] = p;                        // P
                pN[jt][e] = p * (pN[jt][e] - di);     // dS
            }
        }
#pragma unroll
        for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int rr = rowmap32(e, h);
                const float* qr = &sQ[rr * LD + c];
                const float* orow = &sdO[rr * LD + c];
#pragma unroll
                for (int ft = 0; ft < NF; ++ft) {
                    dk[jt][ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(pN[jt][e], qr[32 * ft], dk[jt][ft], 0, 0, 0);
                    dv[jt][ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(sN[jt][e], orow[32 * ft], dv[jt][ft], 0, 0, 0);
                }
            }
        __syncthreads();  // sQ / sdO are rewritten by the next block
    }
#pragma unroll
    for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int ft = 0; ft < NF; ++ft)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                float* o = outb + (size_t)(w * 64 + jt * 32 + rowmap32(e, h)) * 3 * d + 32 * ft + c;
                o[d] = dk[jt][ft][e] * scale;
                o[2 * d] = dv[jt][ft][e];
            }
}

// GENIE_E_UNSUPPORTED for other geometries (the caller then takes the materialised-scores path)
int launch_attn_spatial_bwd_fused(const float* qkv, const float* qk, long qk_ld, const float* dO, float* dqkv, long n_bt, int S,
                                  int d, int H, int Dh, float scale, hipStream_t st) {
    if (!attn_spatial_bwd_fused_takes(S, Dh)) return GENIE_E_UNSUPPORTED;
    if (n_bt <= 0) return GENIE_OK;
    const size_t lds = (size_t)((2 * 256 + 2 * 32) * (Dh + 4) + 12 * 32 + 3 * 256) * sizeof(float);
    ProfScope prof(GENIE_KC_ATTN_SPATIAL, 14.0 * S * S * Dh * (double)n_bt * H, 4.0 * 10 * S * Dh * (double)n_bt * H, st,
                   "attn_spatial_bwd_fused_kernel");
    if (Dh == 64) {
        (void)hipFuncSetAttribute((const void*)attn_spatial_bwd_fused_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        attn_spatial_bwd_fused_kernel<64><<<(unsigned)(n_bt * H), 256, lds, st>>>(qkv, qk, qk_ld, dO, dqkv, d, H, scale);
    } else {
        (void)hipFuncSetAttribute((const void*)attn_spatial_bwd_fused_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        attn_spatial_bwd_fused_kernel<32><<<(unsigned)(n_bt * H), 256, lds, st>>>(qkv, qk, qk_ld, dO, dqkv, d, H, scale);
    }
    GENIE_LAUNCH_CHECK("attn_spatial_bwd_fused");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// qk-norm (attention.py:42-47): LayerNorm over head_dim of every q and k head row, ONE affine shared by q, k and all
// heads.  Forward writes the normalised operands qkn (M, 2d) = [LN(q) | LN(k)] for the score GEMMs of the backward;
// backward turns d/d(normalised) into d/d(raw) in place on the q,k columns of dqkv and emits the affine's gradient
// partials.  DH/4 lanes per (row, q|k, head) item, float4 each.
// ------------------------------------------------------------------------------------------------
template <int LPI>
__device__ __forceinline__ float sub_sum(float v) {
#pragma unroll
    for (int o = LPI / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <int DH>
__global__ __launch_bounds__(256) void qk_norm_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ qkn,
                                                          const float* __restrict__ nw, const float* __restrict__ nb,
                                                          long n_items, int H, int d) {
    constexpr int LPI = DH / 4, IPB = 256 / LPI;
    const long item = (long)blockIdx.x * IPB + threadIdx.x / LPI;
    const int sub = threadIdx.x % LPI;
    if (item >= n_items) return;
    const long row = item / (2 * H);
    const int rem = (int)(item - row * 2 * H), which = rem / H, head = rem - which * H;
    const float4 v = *reinterpret_cast<const float4*>(qkv + (size_t)row * 3 * d + which * d + head * DH + sub * 4);
    const float mean = sub_sum<LPI>(v.x + v.y + v.z + v.w) * (1.0f / DH);
    const float a = v.x - mean, b = v.y - mean, c = v.z - mean, e = v.w - mean;
    const float rstd = 1.0f / sqrtf(sub_sum<LPI>(a * a + b * b + c * c + e * e) * (1.0f / DH) + 1e-5f);
    const float4 g = *reinterpret_cast<const float4*>(nw + sub * 4), bb = *reinterpret_cast<const float4*>(nb + sub * 4);
    *reinterpret_cast<float4*>(qkn + (size_t)row * 2 * d + which * d + head * DH + sub * 4) =
        make_float4(a * rstd * g.x + bb.x, b * rstd * g.y + bb.y, c * rstd * g.z + bb.z, e * rstd * g.w + bb.w);
}
constexpr int QKN_BLOCKS = 512;
// PARAMS = false (the shared affine's two gradients frozen): dqkv alone -- no dg / db accumulators, no LDS, `part` is not touched
template <int DH, bool PARAMS>
__global__ __launch_bounds__(256) void qk_norm_bwd_kernel(const float* __restrict__ qkv, float* __restrict__ dqkv,
                                                          const float* __restrict__ nw, float* __restrict__ part,
                                                          long n_items, int H, int d) {
    constexpr int LPI = DH / 4, IPB = 256 / LPI;
    const int sub = threadIdx.x % LPI;
    const float4 g = *reinterpret_cast<const float4*>(nw + sub * 4);
    float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
    for (long item = (long)blockIdx.x * IPB + threadIdx.x / LPI; item < n_items; item += (long)gridDim.x * IPB) {
        const long row = item / (2 * H);
        const int rem = (int)(item - row * 2 * H), which = rem / H, head = rem - which * H;
        const size_t off = (size_t)row * 3 * d + which * d + head * DH + sub * 4;
        const float4 v = *reinterpret_cast<const float4*>(qkv + off);
        const float4 dy = *reinterpret_cast<const float4*>(dqkv + off);
        const float mean = sub_sum<LPI>(v.x + v.y + v.z + v.w) * (1.0f / DH);
        float xh[4] = {v.x - mean, v.y - mean, v.z - mean, v.w - mean};
        const float rstd =
            1.0f / sqrtf(sub_sum<LPI>(xh[0] * xh[0] + xh[1] * xh[1] + xh[2] * xh[2] + xh[3] * xh[3]) * (1.0f / DH) + 1e-5f);
        const float dyv[4] = {dy.x, dy.y, dy.z, dy.w}, gv[4] = {g.x, g.y, g.z, g.w};
        float gy[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            xh[k] *= rstd;
            gy[k] = dyv[k] * gv[k];
            s1 += gy[k];
            s2 += gy[k] * xh[k];
            if constexpr (PARAMS) { dg[k] += dyv[k] * xh[k]; db[k] += dyv[k]; }
        }
        s1 = sub_sum<LPI>(s1) * (1.0f / DH);
        s2 = sub_sum<LPI>(s2) * (1.0f / DH);
        *reinterpret_cast<float4*>(dqkv + off) = make_float4((gy[0] - s1 - xh[0] * s2) * rstd, (gy[1] - s1 - xh[1] * s2) * rstd,
                                                            (gy[2] - s1 - xh[2] * s2) * rstd, (gy[3] - s1 - xh[3] * s2) * rstd);
    }
    if constexpr (PARAMS) {
        __shared__ float red[256][8];
#pragma unroll
        for (int k = 0; k < 4; ++k) { red[threadIdx.x][k] = dg[k]; red[threadIdx.x][4 + k] = db[k]; }
        __syncthreads();
        if (threadIdx.x < 2 * DH) {  // part[block][which][DH]: channel c is held by the threads with sub == c/4
            const int which = threadIdx.x / DH, c = threadIdx.x - which * DH;
            float s = 0.f;
            for (int t = c / 4; t < 256; t += LPI) s += red[t][which * 4 + (c & 3)];
            part[(size_t)blockIdx.x * 2 * DH + threadIdx.x] = s;
        }
    }
}
int launch_qk_norm_fwd(const float* qkv, float* qkn, const float* nw, const float* nb, long M, int H, int Dh, int d,
                       hipStream_t st) {
    const long n_items = M * 2 * H;
    if (n_items <= 0) return GENIE_OK;
    const unsigned blocks = (unsigned)((n_items + (1024 / Dh) - 1) / (1024 / Dh));
    if (Dh == 64) qk_norm_fwd_kernel<64><<<blocks, 256, 0, st>>>(qkv, qkn, nw, nb, n_items, H, d);
    else if (Dh == 32) qk_norm_fwd_kernel<32><<<blocks, 256, 0, st>>>(qkv, qkn, nw, nb, n_items, H, d);
    else if (Dh == 128) qk_norm_fwd_kernel<128><<<blocks, 256, 0, st>>>(qkv, qkn, nw, nb, n_items, H, d);
    else { set_error("qk-norm: head_dim %d not in {32, 64, 128}", Dh); return GENIE_E_UNSUPPORTED; }
    GENIE_LAUNCH_CHECK("qk_norm_fwd");
    return GENIE_OK;
}
// in place on the q,k columns of dqkv; dnw/dnb (Dh) = beta * old + sums over rows, q and k, and heads.  A NULL dnw / dnb is a frozen
// tensor (include/genie_hip.h, "Frozen tensors"): its half is not reduced; both NULL: the parameter-free kernel and no reduction at all
int launch_qk_norm_bwd(const float* qkv, float* dqkv, const float* nw, float* dnw, float* dnb, long M, int H, int Dh,
                       int d, float beta, float* part, hipStream_t st) {
    const long n_items = M * 2 * H;
    if (n_items <= 0) return GENIE_OK;
    if (!dnw && !dnb) {
        if (Dh == 64) qk_norm_bwd_kernel<64, false><<<QKN_BLOCKS, 256, 0, st>>>(qkv, dqkv, nw, nullptr, n_items, H, d);
        else if (Dh == 32) qk_norm_bwd_kernel<32, false><<<QKN_BLOCKS, 256, 0, st>>>(qkv, dqkv, nw, nullptr, n_items, H, d);
        else if (Dh == 128) qk_norm_bwd_kernel<128, false><<<QKN_BLOCKS, 256, 0, st>>>(qkv, dqkv, nw, nullptr, n_items, H, d);
        else { set_error("qk-norm: head_dim %d not in {32, 64, 128}", Dh); return GENIE_E_UNSUPPORTED; }
        GENIE_LAUNCH_CHECK("qk_norm_bwd");
        return GENIE_OK;
    }
    if (Dh == 64) qk_norm_bwd_kernel<64, true><<<QKN_BLOCKS, 256, 0, st>>>(qkv, dqkv, nw, part, n_items, H, d);
    else if (Dh == 32) qk_norm_bwd_kernel<32, true><<<QKN_BLOCKS, 256, 0, st>>>(qkv, dqkv, nw, part, n_items, H, d);
    else if (Dh == 128) qk_norm_bwd_kernel<128, true><<<QKN_BLOCKS, 256, 0, st>>>(qkv, dqkv, nw, part, n_items, H, d);
    else { set_error("qk-norm: head_dim %d not in {32, 64, 128}", Dh); return GENIE_E_UNSUPPORTED; }
    GENIE_LAUNCH_CHECK("qk_norm_bwd");
    float* tmp = part + (size_t)QKN_BLOCKS * 2 * Dh;
    GENIE_TRY(launch_slab_reduce(part, QKN_BLOCKS, (size_t)2 * Dh, tmp, 0.f, st, "slab_reduce_norm"));
    if (dnw) GENIE_TRY(launch_slab_reduce(tmp, 1, (size_t)Dh, dnw, beta, st, "slab_reduce_norm"));
    return dnb ? launch_slab_reduce(tmp + Dh, 1, (size_t)Dh, dnb, beta, st, "slab_reduce_norm") : GENIE_OK;
}
// part[QKN_BLOCKS][2][Dh] and the reduced [2][Dh] behind it
size_t qk_norm_bwd_scratch_floats(int Dh) {
    return (Dh == 32 || Dh == 64 || Dh == 128) ? (size_t)(QKN_BLOCKS + 1) * 2 * Dh : 0;
}

}  // namespace genie
