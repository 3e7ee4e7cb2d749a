// Causal temporal attention for gfx950, every precision: the f32-MFMA kernel of a whole clip (T <= 16 frames), its teacher-forced
// prefix form with the generic-geometry fallback, and the single-query decode step of the temporal KV cache (ordinary and fan-out).
// The arithmetic is f32 throughout; inputs are f32 or bf16 rows, outputs f32, bf16 or split-f16 planes.
#include <type_traits>

#include "common.hpp"
#include "kernels.hpp"

namespace genie {

// N contiguous values of a temporal qkv row as f32: from an f32 buffer (exact, f16x3) or from a bf16 one (GENIE_PREC_BF16 keeps
// its temporal qkv / KV cache in bf16: half the bytes of these HBM-bound kernels; the arithmetic below stays f32)
template <int N>
__device__ __forceinline__ void load_vals(const float* p, float* v) {
    if constexpr (N >= 4) {
#pragma unroll
        for (int c = 0; c < N / 4; ++c) {
            const float4 a = *reinterpret_cast<const float4*>(p + 4 * c);
            v[4 * c] = a.x; v[4 * c + 1] = a.y; v[4 * c + 2] = a.z; v[4 * c + 3] = a.w;
        }
    } else {
        const float2 a = *reinterpret_cast<const float2*>(p);
        v[0] = a.x; v[1] = a.y;
    }
}
template <int N>
__device__ __forceinline__ void load_vals(const uint16_t* p, float* v) {
    if constexpr (N >= 8) {
#pragma unroll
        for (int c = 0; c < N / 8; ++c) {
            const uint4 a = *reinterpret_cast<const uint4*>(p + 8 * c);
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[8 * c + 2 * j] = __uint_as_float(w[j] << 16);
                v[8 * c + 2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u);
            }
        }
    } else if constexpr (N == 4) {
        const uint2 a = *reinterpret_cast<const uint2*>(p);
        v[0] = __uint_as_float(a.x << 16); v[1] = __uint_as_float(a.x & 0xFFFF0000u);
        v[2] = __uint_as_float(a.y << 16); v[3] = __uint_as_float(a.y & 0xFFFF0000u);
    } else {
        const uint32_t a = *reinterpret_cast<const uint32_t*>(p);
        v[0] = __uint_as_float(a << 16); v[1] = __uint_as_float(a & 0xFFFF0000u);
    }
}
__device__ __forceinline__ float load_val(const float* p) { return *p; }
__device__ __forceinline__ float load_val(const uint16_t* p) { return bf16_to_f32(*p); }

// NV (1, 2 or 4) contiguous outputs of one row: f32, bf16 (plane == 0) or split-f16 planes
template <int NV>
__device__ __forceinline__ void store_row_chunk(float* out, uint16_t* out16, size_t plane, size_t oi, const float* v) {
    if (!out16) {
        if constexpr (NV == 4) *reinterpret_cast<float4*>(out + oi) = make_float4(v[0], v[1], v[2], v[3]);
        else if constexpr (NV == 2) *reinterpret_cast<float2*>(out + oi) = make_float2(v[0], v[1]);
        else out[oi] = v[0];
    } else if (plane) {
        uint16_t hi[NV], lo[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) split_f16(v[c], hi[c], lo[c]);
        if constexpr (NV == 4) {
            *reinterpret_cast<uint2*>(out16 + oi) = make_uint2((uint32_t)hi[0] | ((uint32_t)hi[1] << 16), (uint32_t)hi[2] | ((uint32_t)hi[3] << 16));
            *reinterpret_cast<uint2*>(out16 + plane + oi) = make_uint2((uint32_t)lo[0] | ((uint32_t)lo[1] << 16), (uint32_t)lo[2] | ((uint32_t)lo[3] << 16));
        } else if constexpr (NV == 2) {
            *reinterpret_cast<uint32_t*>(out16 + oi) = (uint32_t)hi[0] | ((uint32_t)hi[1] << 16);
            *reinterpret_cast<uint32_t*>(out16 + plane + oi) = (uint32_t)lo[0] | ((uint32_t)lo[1] << 16);
        } else {
            out16[oi] = hi[0];
            out16[plane + oi] = lo[0];
        }
    } else {
        if constexpr (NV == 4)
            *reinterpret_cast<uint2*>(out16 + oi) = make_uint2((uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16),
                                                               (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16));
        else if constexpr (NV == 2)
            *reinterpret_cast<uint32_t*>(out16 + oi) = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
        else
            out16[oi] = f32_to_bf16(v[0]);
    }
}

// Runs f(std::integral_constant<int, DH>, TI()) for the DH among DHS that equals Dh and the element type TI of the temporal qkv rows
// (in16: bf16 as uint16_t, else float): the one place a launcher chooses its kernel instantiation.  false: Dh is not among DHS.
template <int... DHS, class F>
static bool for_head_dim_and_type(int Dh, bool in16, F&& f) {
    return ((Dh == DHS && ((in16 ? f(std::integral_constant<int, DHS>(), uint16_t()) : f(std::integral_constant<int, DHS>(), float())), true)) || ...);
}

// ------------------------------------------------------------------------------------------------
// a8  Temporal causal attention on the f32 matrix cores, T = 16 frames, one wavefront per (b, s, head),
// operands straight from HBM into MFMA fragments -- no LDS, no "(B S) T C" transpose (st_transformer.py:77).
//
//   S^T = K Q^T : v_mfma_f32_16x16x4_f32, lane (r = lane&15, g = lane>>4) holds K[r][16g..16g+15] and
//                 Q[r][16g..16g+15] (4 float4 each, 256 B contiguous per token across the 4 lane groups);
//                 MFMA step s consumes element s of every lane, i.e. k in {s, 16+s, 32+s, 48+s}: the k-sum
//                 is order-free so 16 steps cover Dh = 64.  Result: lane (i = r, g) holds scores of query i
//                 against keys j = 4g + e -> causal mask + softmax = 4 in-lane values + 2 cross-group shuffles.
//   O = P V     : same trick on the key axis: step e feeds P[i][4g+e] and V[4g+e][16*dt + r].
//
// The steps the plain and the prefix kernel share are stated once, below.
// ------------------------------------------------------------------------------------------------
// the wave's (clip b, position s, head) and the lane's tile coordinates (r, g); false: a wave past the last (b, s, head)
struct TemporalWave {
    long b, s;
    int head, r, g;
};
__device__ __forceinline__ bool temporal_wave(long n_bs, int S, int H, TemporalWave& w) {
    const int lane = threadIdx.x & 63;
    w.r = lane & 15;
    w.g = lane >> 4;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long bs = wave / H;
    w.head = (int)(wave - bs * H);
    w.b = bs / S;
    w.s = bs - w.b * S;
    return bs < n_bs;
}

// qk-norm of N head rows (q, k[, kc]), f32, one shared affine (attention.py:42-47); a row is spread over the 4 lane groups, PER values in
// lane group g.  Per row: sum, mean, centred squares, 1 / sqrt(var / DH + eps), affine.  The rows take the affine step together: its
// weights are fetched once, after the last reduction (a call per row kept them in registers across the next row's reductions).
template <int DH, int N>
__device__ __forceinline__ void qk_norm_rows(float* const (&v)[N], int g, const float* nw, const float* nb) {
    constexpr int PER = DH / 4;
    float mean[N], rstd[N];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < PER; ++c) sum += v[n][c];
        sum += __shfl_xor(sum, 16); sum += __shfl_xor(sum, 32);
        mean[n] = sum / DH;
        float var = 0.f;
#pragma unroll
        for (int c = 0; c < PER; ++c) { const float a = v[n][c] - mean[n]; var += a * a; }
        var += __shfl_xor(var, 16); var += __shfl_xor(var, 32);
        rstd[n] = 1.0f / sqrtf(var / DH + 1e-5f);
    }
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        const float w_ = nw[g * PER + c], b_ = nb[g * PER + c];
#pragma unroll
        for (int n = 0; n < N; ++n) v[n][c] = (v[n][c] - mean[n]) * rstd[n] * w_ + b_;
    }
}

// Mask (attention.py:51-55: -finfo.max before softmax -> exact zeros) and softmax numerators over the keys of an S^T tile: the lane holds the
// scores of its query against keys j = 4g + e, of which j < n_keys are visible.  mx: in, a further score every lane of the query holds
// (the prefix kernel's diagonal; -INFINITY: none); out, the row maximum.  st becomes exp(score - mx); returns the sum over the tile's keys.
__device__ __forceinline__ float softmax_keys(f32x4& st, int g, int n_keys, float& mx) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (4 * g + e >= n_keys) st[e] = -INFINITY;
        mx = fmaxf(mx, st[e]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { st[e] = expf(st[e] - mx); sum += st[e]; }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    return sum;
}

// O = P V and the store of the T query rows.  Feature permutation: MFMA column r of "d-tile" c is feature NV*r + c, so a lane fetches NV
// CONTIGUOUS features of V[4g+e] (16 lanes = one 4*DH-byte row segment: vv[e]) and stores NV contiguous outputs.
// C/D map: col = lane&15 (-> features NV*r..NV*r+NV-1 over c), row = 4*(lane>>4) + e (query frame); obase: the lane's features of frame 0.
// SELF: query row i adds p_self * vs, its own value row; p_self_lane is that weight of query r, held by every lane with r == i.
template <int NV, bool SELF>
__device__ __forceinline__ void pv_store_rows(const f32x4& st, float inv, const float (*vv)[NV], const float (*vs)[NV], float p_self_lane,
                                              int g, int T, float* out, uint16_t* out16, size_t plane, size_t obase, size_t row_stride) {
    float p_self[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (SELF) {
#pragma unroll
        for (int e = 0; e < 4; ++e) p_self[e] = __shfl(p_self_lane, 4 * g + e);  // lane index 4g+e has r = 4g+e
    }
    f32x4 o[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(st[e] * inv, vv[e][c], o[c], 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (4 * g + e >= T) continue;
        float ov[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            if constexpr (SELF) ov[c] = fmaf(p_self[e], vs[e][c], o[c][e]);
            else ov[c] = o[c][e];
        }
        store_row_chunk<NV>(out, out16, plane, obase + (size_t)(4 * g + e) * row_stride, ov);
    }
}

template <int DH, typename TI>
__global__ __launch_bounds__(256) void attn_temporal_f32_mfma_kernel(const TI* __restrict__ qkv,
                                                                     float* __restrict__ out, long n_bs, int S,
                                                                     int d, int H, int T, int Tq, float scale,
                                                                     const float* __restrict__ nw,
                                                                     const float* __restrict__ nb,
                                                                     uint16_t* __restrict__ out16, size_t plane) {
    // Tq: frames per clip in the layout of `qkv` (>= T; the output is dense (B,T,S,d))
    constexpr int PER = DH / 4;  // floats per lane per row; T <= 16 frames fill a 16x16 tile (rows >= T are padding:
                                 // they repeat frame T-1 on the load side and are never stored)
    TemporalWave w;
    if (!temporal_wave(n_bs, S, H, w)) return;
    const int r = w.r, g = w.g;
    const long tok_stride = (long)S * 3 * d;                       // frame t -> t+1
    const TI* base = qkv + ((size_t)(w.b * Tq) * S + w.s) * 3 * d + w.head * DH;
    const TI* qp = base + (size_t)(r < T ? r : T - 1) * tok_stride + g * PER;     // row t = r
    float q[PER], k[PER];
    load_vals<PER>(qp, q);
    load_vals<PER>(qp + d, k);
    if (nw) {
        float* const rows[2] = {q, k};
        qk_norm_rows<DH>(rows, g, nw, nb);
    }
    f32x4 st = {0.f, 0.f, 0.f, 0.f};  // S^T: row = key j = 4g + e, col = query i = r
#pragma unroll
    for (int c = 0; c < PER; ++c) st = __builtin_amdgcn_mfma_f32_16x16x4f32(k[c], q[c] * scale, st, 0, 0, 0);
    float mx = -INFINITY;
    const float inv = 1.0f / softmax_keys(st, g, r + 1, mx);   // causal: keys j <= i
    constexpr int NV = DH / 16;
    const TI* vp = base + 2 * d + NV * r;
    float vv[4][NV];
#pragma unroll
    for (int e = 0; e < 4; ++e) load_vals<NV>(vp + (size_t)(4 * g + e < T ? 4 * g + e : T - 1) * tok_stride, vv[e]);
    pv_store_rows<NV, false>(st, inv, vv, nullptr, 0.f, g, T, out, out16, plane, ((size_t)(w.b * T) * S + w.s) * d + w.head * DH + NV * r,
                             (size_t)S * d);
}

// Temporal attention over 8 <= T <= 16 frames on a (B,T,S,3d) buffer; GENIE_E_UNSUPPORTED for other geometries.
// in16: `qkv` holds bf16 values (GENIE_PREC_BF16's temporal qkv); any 1 <= T <= 16 then (there is no other bf16-input kernel:
// rows >= T of the 16x16 tile are padding whatever T is).
int launch_attn_temporal_f32_mfma(const float* qkv, float* out, int B, int T, int S, int d, int H, int Dh, float scale,
                                  const float* nw, const float* nb, hipStream_t st, uint16_t* out16, size_t plane, int Tq,
                                  bool in16) {
    if (T > 16 || T < (in16 ? 1 : 8) || (Dh != 32 && Dh != 64)) return GENIE_E_UNSUPPORTED;
    if (Tq <= 0) Tq = T;
    const long n_bs = (long)B * S, waves = n_bs * H;
    ProfScope prof(GENIE_KC_ATTN_TEMPORAL, 4.0 * T * T * Dh * (double)waves,
                   (double)waves * T * Dh * (in16 ? 8.0 : 16.0), st);
    const unsigned blocks = (unsigned)((waves + 3) / 4);
    for_head_dim_and_type<32, 64>(Dh, in16, [&](auto dh, auto ti) {
        using TI = decltype(ti);
        attn_temporal_f32_mfma_kernel<decltype(dh)::value, TI><<<blocks, 256, 0, st>>>(reinterpret_cast<const TI*>(qkv), out, n_bs, S, d, H, T, Tq,
                                                                                       scale, nw, nb, out16, plane);
    });
    GENIE_LAUNCH_CHECK("attn_temporal_f32_mfma");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// Teacher-forced prefix reuse: temporal attention of "frame t in timeline t".
// In the evaluator's timeline t the frames < t are ground truth, and because temporal attention is causal
// and everything else is per-frame, their activations are those of ONE clean pass over the ground-truth clip.
// So query frame i attends keys j < i taken from the clean pass's cached temporal qkv (`cache`, same layout
// (B,T,S,3d)) and key j = i from the current buffer `cur`; current frames never see each other.
//   scores_j<i = scale q_i . kc_j   (MFMA, as attn_temporal_f32_mfma_kernel)      diag = scale q_i . k_i
//   o_i = sum_j<i p_ij vc_j  +  p_ii v_i
// ------------------------------------------------------------------------------------------------
template <int DH, typename TI>
__global__ __launch_bounds__(256) void attn_temporal_prefix_f32_mfma_kernel(
    const TI* __restrict__ cur, const TI* __restrict__ cache, float* __restrict__ out, long n_bs, int S, int d,
    int H, int T, int sh, float scale, const float* __restrict__ nw, const float* __restrict__ nb,
    uint16_t* __restrict__ out16, size_t plane) {
    // T <= 16 frame slots in `cur` and in `cache` (tile rows / columns >= T are padding: loads repeat slot T-1, nothing is
    // stored); query slot i sees cached slots j < i + sh (sh = 0: cur and cache hold the same frames; sh = 1: cur holds
    // clip frames 1..T, cache clip frames 0..T-1)
    constexpr int PER = DH / 4;
    TemporalWave w;
    if (!temporal_wave(n_bs, S, H, w)) return;
    const int r = w.r, g = w.g;
    const long tok_stride = (long)S * 3 * d;
    const size_t off0 = ((size_t)(w.b * T) * S + w.s) * 3 * d + w.head * DH;
    const int rr = r < T ? r : T - 1;
    const TI* qp = cur + off0 + (size_t)rr * tok_stride + g * PER;
    const TI* kcp = cache + off0 + (size_t)rr * tok_stride + d + g * PER;
    float q[PER], k[PER], kc[PER];
    load_vals<PER>(qp, q);
    load_vals<PER>(qp + d, k);
    load_vals<PER>(kcp, kc);
    if (nw) {
        float* const rows[3] = {q, k, kc};
        qk_norm_rows<DH>(rows, g, nw, nb);
    }
    f32x4 st = {0.f, 0.f, 0.f, 0.f};  // row = cached key j = 4g + e, col = query i = r
    float dg = 0.f;                   // diagonal: q_i . k_i (same q*scale products as the MFMA path)
#pragma unroll
    for (int c = 0; c < PER; ++c) {
        const float qs = q[c] * scale;
        st = __builtin_amdgcn_mfma_f32_16x16x4f32(kc[c], qs, st, 0, 0, 0);
        dg = fmaf(k[c], qs, dg);
    }
    dg += __shfl_xor(dg, 16);
    dg += __shfl_xor(dg, 32);
    float mx = dg;
    const float sum = softmax_keys(st, g, min(r + sh, T), mx);   // strictly earlier clip frames only
    const float pd = expf(dg - mx);
    const float inv = 1.0f / (sum + pd);
    const float pdn = pd * inv;  // weight of the query's own (current) frame, held by every lane with r == i
    constexpr int NV = DH / 16;  // feature permutation as in attn_temporal_f32_mfma_kernel
    const TI* vcp = cache + off0 + 2 * d + NV * r;
    const TI* vp = cur + off0 + 2 * d + NV * r;
    float vc[4][NV], vs[4][NV];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const size_t fo = (size_t)(4 * g + e < T ? 4 * g + e : T - 1) * tok_stride;
        load_vals<NV>(vcp + fo, vc[e]);
        load_vals<NV>(vp + fo, vs[e]);
    }
    pv_store_rows<NV, true>(st, inv, vc, vs, pdn, g, T, out, out16, plane, ((size_t)(w.b * T) * S + w.s) * d + w.head * DH + NV * r, (size_t)S * d);
}

// generic geometry (any T <= 64, Dh in {8,16,32,64}): one thread per (b, s, head, frame)
template <int DH>
__global__ void attn_temporal_prefix_generic_kernel(const float* __restrict__ cur, const float* __restrict__ cache,
                                                    float* __restrict__ out, long n, int T, int sh, int S, int d, int H,
                                                    float scale, const float* __restrict__ nw,
                                                    const float* __restrict__ nb) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int i = (int)(idx % T);
    long rest = idx / T;
    const int head = (int)(rest % H);
    rest /= H;
    const long s = rest % S, b = rest / S;
    const long tok_stride = (long)S * 3 * d;
    const size_t off0 = ((size_t)(b * T) * S + s) * 3 * d + head * DH;
    auto load_norm = [&](const float* p, float* v) {
        float m = 0.f;
#pragma unroll
        for (int c = 0; c < DH; ++c) { v[c] = p[c]; m += v[c]; }
        if (nw) {
            m /= DH;
            float var = 0.f;
#pragma unroll
            for (int c = 0; c < DH; ++c) { float t = v[c] - m; var += t * t; }
            const float rs = 1.0f / sqrtf(var / DH + 1e-5f);
#pragma unroll
            for (int c = 0; c < DH; ++c) v[c] = (v[c] - m) * rs * nw[c] + nb[c];
        }
    };
    float q[DH], kk[DH], o[DH];
    load_norm(cur + off0 + (size_t)i * tok_stride, q);
#pragma unroll
    for (int c = 0; c < DH; ++c) { q[c] *= scale; o[c] = 0.f; }
    float sc[65];
    float mx = -INFINITY;
    const int nc = i + sh;  // cached slots 0..nc-1, then the query's own (current) slot
    for (int j = 0; j <= nc; ++j) {
        const float* src = (j < nc ? cache + off0 + (size_t)j * tok_stride : cur + off0 + (size_t)i * tok_stride) + d;
        load_norm(src, kk);
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < DH; ++c) a = fmaf(q[c], kk[c], a);
        sc[j] = a;
        mx = fmaxf(mx, a);
    }
    float sum = 0.f;
    for (int j = 0; j <= nc; ++j) { sc[j] = expf(sc[j] - mx); sum += sc[j]; }
    const float inv = 1.0f / sum;
    for (int j = 0; j <= nc; ++j) {
        const float* vsrc = (j < nc ? cache + off0 + (size_t)j * tok_stride : cur + off0 + (size_t)i * tok_stride) + 2 * d;
        const float p = sc[j] * inv;
#pragma unroll
        for (int c = 0; c < DH; ++c) o[c] = fmaf(p, vsrc[c], o[c]);
    }
    float* op = out + ((size_t)(b * T + i) * S + s) * d + head * DH;
#pragma unroll
    for (int c = 0; c < DH; ++c) op[c] = o[c];
}

// out16/plane as in launch_attn_temporal_f32_mfma; the generic fallback writes f32 `out` only
// (returns GENIE_E_UNSUPPORTED if a 16-bit output is requested for a geometry without an MFMA instantiation).
int launch_attn_temporal_prefix(const float* cur, const float* cache, float* out, int B, int T, int S, int d, int H,
                                int Dh, float scale, const float* nw, const float* nb, hipStream_t st,
                                uint16_t* out16, size_t plane, int sh, bool in16) {
    // T frame slots in both buffers; query slot i sees cached slots j < i + sh and itself (sh in {0, 1})
    // in16: both buffers hold bf16 values (GENIE_PREC_BF16); MFMA kernel only, any 1 <= T <= 16
    GENIE_CHECK_SHAPE(sh == 0 || sh == 1, "prefix attention: shift %d", sh);
    const long n_bs = (long)B * S, waves = n_bs * H;
    ProfScope prof(GENIE_KC_ATTN_TEMPORAL, 4.0 * T * T * Dh * (double)waves,
                   (double)waves * T * Dh * (in16 ? 14.0 : 28.0), st);
    if (T <= 16 && T >= (in16 ? 1 : 8) && (Dh == 32 || Dh == 64)) {
        const unsigned blocks = (unsigned)((waves + 3) / 4);
        for_head_dim_and_type<32, 64>(Dh, in16, [&](auto dh, auto ti) {
            using TI = decltype(ti);
            attn_temporal_prefix_f32_mfma_kernel<decltype(dh)::value, TI><<<blocks, 256, 0, st>>>(
                reinterpret_cast<const TI*>(cur), reinterpret_cast<const TI*>(cache), out, n_bs, S, d, H, T, sh, scale, nw, nb, out16, plane);
        });
        GENIE_LAUNCH_CHECK("attn_temporal_prefix_mfma");
        return GENIE_OK;
    }
    if (out16 || in16) return GENIE_E_UNSUPPORTED;
    GENIE_CHECK_SHAPE(T <= 64, "prefix attention: T=%d > 64", T);
    const long n = waves * T;
    const unsigned blocks = (unsigned)((n + 127) / 128);
    switch (Dh) {
        case 8: attn_temporal_prefix_generic_kernel<8><<<blocks, 128, 0, st>>>(cur, cache, out, n, T, sh, S, d, H, scale, nw, nb); break;
        case 16: attn_temporal_prefix_generic_kernel<16><<<blocks, 128, 0, st>>>(cur, cache, out, n, T, sh, S, d, H, scale, nw, nb); break;
        case 32: attn_temporal_prefix_generic_kernel<32><<<blocks, 128, 0, st>>>(cur, cache, out, n, T, sh, S, d, H, scale, nw, nb); break;
        case 64: attn_temporal_prefix_generic_kernel<64><<<blocks, 128, 0, st>>>(cur, cache, out, n, T, sh, S, d, H, scale, nw, nb); break;
        default: set_error("prefix attention: head_dim %d unsupported", Dh); return GENIE_E_SHAPE;
    }
    GENIE_LAUNCH_CHECK("attn_temporal_prefix_generic");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// Temporal attention of ONE query frame t against the cached qkv of frames 0..t (the frame's own qkv has just been
// written into slot t): the decode step of the temporal KV cache used by generate().  One wavefront per
// (b, s, head), lane = feature; T <= 64 scores live in registers: static indices for t < 16, score j in lane j for t >= 16
// (no indexed array, so no scratch).
// out: dense (B, S, d) f32 / bf16 / split-f16.
// FAN: the split cache of a fan-out decode pass (FanSplit, kernels.hpp) -- `cache` is the branch slice with T = Tb slots per clip,
// slots below fan.P0 come from the parent's clip of the trunk; the base pointer is chosen per frame, after the clamp (fan_slot).
// FAN = false is the same kernel without the split.
// ------------------------------------------------------------------------------------------------
template <int DH, typename TI, bool FAN>
__global__ __launch_bounds__(256) void attn_temporal_single_kernel(const TI* __restrict__ cache,
                                                                   float* __restrict__ out, long n_items, int T, int S,
                                                                   int t, int d, int H, float scale,
                                                                   const float* __restrict__ nw,
                                                                   const float* __restrict__ nb,
                                                                   uint16_t* __restrict__ out16, size_t plane, FanSplit<FAN> fan) {
    const int lane = threadIdx.x & 63;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= n_items) return;
    const int head = (int)(item % H);
    const long bs = item / H;
    const long b = bs / S, s = bs - b * S;
    const bool act = lane < DH;
    const size_t tok_stride = (size_t)S * 3 * d;
    const TI* base = cache + ((size_t)(b * T) * S + s) * 3 * d + head * DH + (act ? lane : 0);
    const TI* tbase = nullptr;   // FAN: the same (position, head, lane) of the parent's clip of the trunk
    int P0 = 0;
    if constexpr (FAN) {
        tbase = static_cast<const TI*>(fan.trunk) + ((size_t)((b / fan.K) * fan.T) * S + s) * 3 * d + head * DH + (act ? lane : 0);
        P0 = fan.P0;
    }
    const size_t oi = (size_t)bs * d + head * DH + lane;   // the lane's output feature (act lanes only)
    auto norm = [&](float v) {  // qk-norm over the DH active lanes
        if (!nw) return v;
        const float mu = wave_sum(act ? v : 0.f) / DH;
        const float c = act ? v - mu : 0.f;
        const float var = wave_sum(c * c) / DH;
        return c * (1.0f / sqrtf(var + 1e-5f)) * nw[act ? lane : 0] + nb[act ? lane : 0];
    };
    if constexpr (DH >= 16) {
        if (t < 16 && !nw) {
            // The shipped window without qk-norm: lane (j = lane / 4, c = lane % 4) takes frame j's key, features [c CH, (c + 1) CH):
            // all t + 1 scores come out of ONE pass -- a CH-long dot product per lane and two cross-lane adds -- instead of t + 1
            // 64-lane reductions one after the other (the kernel was bound by that chain: 58 us at 16 clips for 200 MB of cache);
            // max / sum over the 16 frame groups are four butterfly steps each.  P.V stays lane = feature with p_j broadcast from
            // lane 4 j; every key and value load is issued before the first use.
            constexpr int CH = DH / 4;
            const int j = lane >> 2, c4 = lane & 3;
            const TI* hb = cache + ((size_t)(b * T) * S + s) * 3 * d + head * DH;
            const TI* thb = nullptr;
            if constexpr (FAN) thb = static_cast<const TI*>(fan.trunk) + ((size_t)((b / fan.K) * fan.T) * S + s) * 3 * d + head * DH;
            float qv[CH], kv[CH], vj[16];
            load_vals<CH>(fan_slot<FAN>(hb, thb, t, P0, tok_stride) + c4 * CH, qv);
            load_vals<CH>(fan_slot<FAN>(hb, thb, j <= t ? j : t, P0, tok_stride) + d + c4 * CH, kv);
#pragma unroll
            for (int jj = 0; jj < 16; ++jj)   // (frames past t re-read frame t, branch-free: their probability is 0)
                vj[jj] = load_val(fan_slot<FAN>(hb, thb, jj <= t ? jj : t, P0, tok_stride) + 2 * d + (act ? lane : 0));
            // (ties the score arithmetic behind the issue of the value loads: one memory round trip, not two)
            asm volatile("" : "+v"(qv[0]), "+v"(kv[0]) :: "memory");
            float part = 0.f;
#pragma unroll
            for (int e = 0; e < CH; ++e) part = fmaf(qv[e], kv[e], part);
            part += __shfl_xor(part, 1);
            part += __shfl_xor(part, 2);
            const float sc = j <= t ? part * scale : -INFINITY;
            float mxs = sc;
#pragma unroll
            for (int o = 4; o < 64; o <<= 1) mxs = fmaxf(mxs, __shfl_xor(mxs, o));
            const float pe = j <= t ? expf(sc - mxs) : 0.f;
            float sm = pe;
#pragma unroll
            for (int o = 4; o < 64; o <<= 1) sm += __shfl_xor(sm, o);
            const float pn = pe * (1.0f / sm);
            float o16 = 0.f;
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) o16 = fmaf(__shfl(pn, 4 * jj), vj[jj], o16);
            if (act) store_row_chunk<1>(out, out16, plane, oi, &o16);
            return;
        }
    }
    float q = norm(load_val(fan_slot<FAN>(base, tbase, t, P0, tok_stride))) * scale;
    if (!act) q = 0.f;
    if (t < 16) {
        // the shipped window (T = 16): every cached key / value of the (position, head) is fetched up front -- 2 (t + 1)
        // independent 4-byte-per-lane loads in flight instead of a load -> reduce -> load chain -- and the scores live in
        // registers (static indices)
        float kj[16], vj[16], sc16[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            kj[j] = 0.f; vj[j] = 0.f;
            if (j <= t) { kj[j] = load_val(fan_slot<FAN>(base, tbase, j, P0, tok_stride) + d); vj[j] = load_val(fan_slot<FAN>(base, tbase, j, P0, tok_stride) + 2 * d); }
        }
        float mx16 = -INFINITY;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j <= t) {
                const float a = wave_sum(act ? q * norm(kj[j]) : 0.f);
                sc16[j] = a;
                mx16 = fmaxf(mx16, a);
            }
        }
        float sum16 = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j <= t) { sc16[j] = expf(sc16[j] - mx16); sum16 += sc16[j]; }
        const float inv16 = 1.0f / sum16;
        float o16 = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j <= t) o16 = fmaf(sc16[j] * inv16, vj[j], o16);
        if (act) store_row_chunk<1>(out, out16, plane, oi, &o16);
        return;
    }
    // t >= 16: every lane holds the same wave_sum, so lane j keeps score j; exp runs once per lane, and the sum and P.V read lane j's
    // value in the order j = 0 .. t
    float mine = 0.f, mx = -INFINITY;
    for (int j = 0; j <= t; ++j) {
        const float kj = norm(load_val(fan_slot<FAN>(base, tbase, j, P0, tok_stride) + d));
        const float a = wave_sum(act ? q * kj : 0.f);
        mine = lane == j ? a : mine;
        mx = fmaxf(mx, a);
    }
    mine = expf(mine - mx);
    float sum = 0.f;
    for (int j = 0; j <= t; ++j) sum += __shfl(mine, j);
    const float inv = 1.0f / sum;
    float o = 0.f;
    for (int j = 0; j <= t; ++j) o = fmaf(__shfl(mine, j) * inv, load_val(fan_slot<FAN>(base, tbase, j, P0, tok_stride) + 2 * d), o);
    if (act) store_row_chunk<1>(out, out16, plane, oi, &o);
}

// fan != NULL: the fan-out flavour (launch_attn_temporal_single_fanout)
static int attn_temporal_single_launch(const float* cache, float* out, int B, int T, int S, int t, int d, int H, int Dh, float scale,
                                       const float* nw, const float* nb, hipStream_t st, uint16_t* out16, size_t plane, bool in16,
                                       const FanSplit<true>* fan) {
    const long n = (long)B * S * H;
    ProfScope prof(GENIE_KC_ATTN_TEMPORAL, 4.0 * (t + 1) * Dh * (double)n, (double)n * Dh * (in16 ? 2.0 : 4.0) * (2 * t + 4), st);
    const unsigned blocks = (unsigned)((n + 3) / 4);
    auto with_split = [&](auto split) {   // split: the FanSplit of the flavour
        return for_head_dim_and_type<8, 16, 32, 64>(Dh, in16, [&](auto dh, auto ti) {
            using TI = decltype(ti);
            constexpr bool FAN = std::is_same<decltype(split), FanSplit<true>>::value;
            attn_temporal_single_kernel<decltype(dh)::value, TI, FAN><<<blocks, 256, 0, st>>>(
                reinterpret_cast<const TI*>(cache), out, n, T, S, t, d, H, scale, nw, nb, out16, plane, split);
        });
    };
    if (!(fan ? with_split(*fan) : with_split(FanSplit<false>()))) {
        set_error("temporal_single: head_dim %d unsupported", Dh);
        return GENIE_E_SHAPE;
    }
    GENIE_LAUNCH_CHECK("attn_temporal_single");
    return GENIE_OK;
}

int launch_attn_temporal_single(const float* cache, float* out, int B, int T, int S, int t, int d, int H, int Dh,
                                float scale, const float* nw, const float* nb, hipStream_t st, uint16_t* out16,
                                size_t plane, bool in16) {
    GENIE_CHECK_SHAPE(T <= 64 && t >= 0 && t < T, "temporal_single: bad frame %d of %d", t, T);
    return attn_temporal_single_launch(cache, out, B, T, S, t, d, H, Dh, scale, nw, nb, st, out16, plane, in16, nullptr);
}

int launch_attn_temporal_single_fanout(const float* cache, float* out, int B, int T, int S, int t, int d, int H, int Dh, float scale,
                                       const float* nw, const float* nb, hipStream_t st, uint16_t* out16, size_t plane, bool in16,
                                       const FanSplit<true>& fan) {
    GENIE_CHECK_SHAPE(fan.T <= 64 && fan.K >= 1 && B % fan.K == 0 && fan.P0 >= 0 && fan.P0 <= t && t - fan.P0 < T && t < fan.T,
                      "temporal_single (fan-out): frame %d, trunk slots [0, %d) of %d, %d branch slots, %d clips in branches of %d", t, fan.P0,
                      fan.T, T, B, fan.K);
    return attn_temporal_single_launch(cache, out, B, T, S, t, d, H, Dh, scale, nw, nb, st, out16, plane, in16, &fan);
}

}  // namespace genie
