// MLP dropout of the training step (genie_dropout in include/genie_hip.h; reference: st_transformer.py:22-25, one nn.Dropout used
// behind the GELU -- site 0 -- and behind fc2 -- site 1).  The keep masks are a pure function of counters, made in registers by
// every kernel that applies them and never stored: the recomputing backward and the backward of the saving mode draw the bits the
// forward drew.
//
// Law: Philox4x32-10, key = (seed lo, seed hi), counter = (g lo, g hi, layer * 2 + site, call), g = e / 4: the four output words
// serve elements 4g .. 4g + 3 of the row-major (M, hidden) / (M, d_model) matrix; element e is kept iff its word >= thr,
// thr = floor((double)p * 2^32).  Integer only, so a NumPy restatement is bit-exact (tests/dropout_model.py).
//
// The step's four kernels report to the profiler (genie_profile_*) in class GENIE_KC_OTHER with the bytes they move.
// All kernels are elementwise streams: one Philox call per four elements (about 60 integer VALU instructions, 40 of them the 32x32
// multiplies), 16-byte accesses on the f32 side.  Where the scale 1 / (1 - p) can ride in the alpha of the GEMM behind the mask
// (site 0: fc2 and its two backward products) the kernel only zeroes elements, which is exact in every operand form.
#include "kernels.hpp"

namespace genie {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                       uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// keep[j] of elements 4g + j
__device__ __forceinline__ void keep4(const DropKey& k, size_t g, bool (&keep)[4]) {
    uint32_t w[4];
    philox4x32_10((uint32_t)g, (uint32_t)((uint64_t)g >> 32), k.stream, k.call, k.k0, k.k1, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) keep[j] = w[j] >= k.thr;
}

// (the derivative the saving and the undropped backward use: gelu_grad of kernels_train.hip, restated because that file's kernels stay as they are)
__device__ __forceinline__ float drop_gelu_grad(float z) {
    const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * z * z) * 0.39894228040143267794f;
    return cdf + z * pdf;
}

// exact, site 0 forward: h = m * gelu(z) (launch_gelu_fwd with the mask; the scale travels in fc2's alpha)
__global__ __launch_bounds__(256) void drop_gelu_fwd_kernel(const float4* __restrict__ z, float4* __restrict__ h, size_t n4, DropKey k) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    bool m[4];
    keep4(k, i, m);
    float4 v = z[i];
    v.x = m[0] ? gelu_erf(v.x) : 0.f; v.y = m[1] ? gelu_erf(v.y) : 0.f;
    v.z = m[2] ? gelu_erf(v.z) : 0.f; v.w = m[3] ? gelu_erf(v.w) : 0.f;
    h[i] = v;
}
// exact, site 0 backward: dz = m * dh * gelu'(z), in place on dh (launch_gelu_bwd with the mask)
__global__ __launch_bounds__(256) void drop_gelu_bwd_kernel(const float4* __restrict__ z, float4* __restrict__ g, size_t n4, DropKey k) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    bool m[4];
    keep4(k, i, m);
    const float4 zz = z[i];
    float4 v = g[i];
    v.x = m[0] ? v.x * drop_gelu_grad(zz.x) : 0.f; v.y = m[1] ? v.y * drop_gelu_grad(zz.y) : 0.f;
    v.z = m[2] ? v.z * drop_gelu_grad(zz.z) : 0.f; v.w = m[3] ? v.w * drop_gelu_grad(zz.w) : 0.f;
    g[i] = v;
}

// out = (add) + m * (s * in), f32; OP 1 / 2: also `out` in operand form (bf16 / f16 split planes, the roundings of launch_cast16).
// in == out and add == out are allowed (every thread reads its four elements before it writes them), hence no __restrict__.
template <int OP>
__global__ __launch_bounds__(256) void drop_axpy_kernel(const float4* in, const float4* add, float4* out, uint16_t* out16, size_t plane,
                                                         size_t n4, float s, DropKey k) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    bool m[4];
    keep4(k, i, m);
    float4 v = in[i];
    v.x = m[0] ? v.x * s : 0.f; v.y = m[1] ? v.y * s : 0.f; v.z = m[2] ? v.z * s : 0.f; v.w = m[3] ? v.w * s : 0.f;
    if (add) {
        const float4 r = add[i];
        v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    out[i] = v;
    if constexpr (OP == 1) {
        *reinterpret_cast<uint2*>(out16 + 4 * i) = make_uint2(f32x2_to_bf16x2(v.x, v.y), f32x2_to_bf16x2(v.z, v.w));
    } else if constexpr (OP == 2) {
        uint16_t h[4], l[4];
        split_f16(v.x, h[0], l[0]); split_f16(v.y, h[1], l[1]); split_f16(v.z, h[2], l[2]); split_f16(v.w, h[3], l[3]);
        *reinterpret_cast<uint2*>(out16 + 4 * i) = make_uint2(h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16);
        *reinterpret_cast<uint2*>(out16 + plane + 4 * i) = make_uint2(l[0] | (uint32_t)l[1] << 16, l[2] | (uint32_t)l[3] << 16);
    }
}

// 16-bit, site 0 forward: zero the dropped elements of the h operand in place (NPL planes `plane` elements apart); 8 elements =
// two Philox calls and one 16-byte access per plane and thread
template <int NPL>
__global__ __launch_bounds__(256) void drop_zero16_kernel(uint16_t* h16, size_t plane, size_t n8, DropKey k) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    bool a[4], b[4];
    keep4(k, 2 * i, a);
    keep4(k, 2 * i + 1, b);
    auto pair = [](bool lo, bool hi) { return (lo ? 0x0000FFFFu : 0u) | (hi ? 0xFFFF0000u : 0u); };
    const uint32_t mask[4] = {pair(a[0], a[1]), pair(a[2], a[3]), pair(b[0], b[1]), pair(b[2], b[3])};
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) {
        uint4* p = reinterpret_cast<uint4*>(h16 + pl * plane + 8 * i);
        uint4 v = *p;
        v.x &= mask[0]; v.y &= mask[1]; v.z &= mask[2]; v.w &= mask[3];
        *p = v;
    }
}

// the keep bytes themselves (genie_dropout_mask, the tests' window on the law); any n
__global__ __launch_bounds__(256) void dropout_mask_kernel(uint8_t* __restrict__ keep, size_t n, DropKey k) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (4 * g >= n) return;
    bool m[4];
    keep4(k, g, m);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * g + j < n) keep[4 * g + j] = m[j] ? 1 : 0;
}

static inline unsigned blocks_of(size_t threads) { return (unsigned)((threads + 255) / 256); }

int launch_drop_gelu_fwd(const float* z, float* h, size_t n, const DropKey& k, hipStream_t st) {
    GENIE_CHECK_SHAPE(n % 4 == 0, "dropout gelu: n %% 4");
    if (!n) return GENIE_OK;
    ProfScope prof(GENIE_KC_OTHER, 0.0, 8.0 * n, st, "drop_gelu_fwd_kernel");
    drop_gelu_fwd_kernel<<<blocks_of(n / 4), 256, 0, st>>>((const float4*)z, (float4*)h, n / 4, k);
    GENIE_LAUNCH_CHECK("drop_gelu_fwd");
    return GENIE_OK;
}
int launch_drop_gelu_bwd(const float* z, float* g, size_t n, const DropKey& k, hipStream_t st) {
    GENIE_CHECK_SHAPE(n % 4 == 0, "dropout gelu: n %% 4");
    if (!n) return GENIE_OK;
    ProfScope prof(GENIE_KC_OTHER, 0.0, 12.0 * n, st, "drop_gelu_bwd_kernel");
    drop_gelu_bwd_kernel<<<blocks_of(n / 4), 256, 0, st>>>((const float4*)z, (float4*)g, n / 4, k);
    GENIE_LAUNCH_CHECK("drop_gelu_bwd");
    return GENIE_OK;
}
int launch_drop_axpy(int npl_out, const float* in, const float* add, float* out, uint16_t* out16, size_t n, float s, const DropKey& k,
                     hipStream_t st) {
    GENIE_CHECK_SHAPE(n % 4 == 0, "dropout: n %% 4");
    GENIE_CHECK_ARG(npl_out >= 0 && npl_out <= 2 && (npl_out == 0 || out16), "dropout: operand form %d without its output", npl_out);
    if (!n) return GENIE_OK;
    const float4 *i4 = (const float4*)in, *a4 = (const float4*)add;
    ProfScope prof(GENIE_KC_OTHER, 0.0, (8.0 + (add ? 4.0 : 0.0) + 2.0 * npl_out) * n, st, "drop_axpy_kernel");
    if (npl_out == 0) drop_axpy_kernel<0><<<blocks_of(n / 4), 256, 0, st>>>(i4, a4, (float4*)out, nullptr, 0, n / 4, s, k);
    else if (npl_out == 1) drop_axpy_kernel<1><<<blocks_of(n / 4), 256, 0, st>>>(i4, a4, (float4*)out, out16, 0, n / 4, s, k);
    else drop_axpy_kernel<2><<<blocks_of(n / 4), 256, 0, st>>>(i4, a4, (float4*)out, out16, n, n / 4, s, k);
    GENIE_LAUNCH_CHECK("drop_axpy");
    return GENIE_OK;
}
int launch_drop_zero16(int npl, uint16_t* h16, size_t n, const DropKey& k, hipStream_t st) {
    GENIE_CHECK_SHAPE(n % 8 == 0, "dropout (16-bit): n %% 8");
    if (!n) return GENIE_OK;
    ProfScope prof(GENIE_KC_OTHER, 0.0, 4.0 * npl * n, st, "drop_zero16_kernel");
    if (npl == 1) drop_zero16_kernel<1><<<blocks_of(n / 8), 256, 0, st>>>(h16, 0, n / 8, k);
    else drop_zero16_kernel<2><<<blocks_of(n / 8), 256, 0, st>>>(h16, n, n / 8, k);
    GENIE_LAUNCH_CHECK("drop_zero16");
    return GENIE_OK;
}
int launch_dropout_mask(uint8_t* keep, size_t n, const DropKey& k, hipStream_t st) {
    if (!n) return GENIE_OK;
    dropout_mask_kernel<<<blocks_of((n + 3) / 4), 256, 0, st>>>(keep, n, k);
    GENIE_LAUNCH_CHECK("dropout_mask");
    return GENIE_OK;
}

}  // namespace genie
