// MaskGIT sampling half with a tempered, top-k / top-p filtered law (genie_sample_ex, include/genie_hip.h).
// Reference counterpart: st_mask_git.py:171-190, which has neither filter and whose `temperature` only switches arg-max to
// sampling (Categorical(probs / T) renormalises).  One wavefront per token, as sample_kernel / sample_rows_kernel
// (kernels_exact.hip): lane l owns the contiguous vocabulary slice [l * per, (l + 1) * per), so index order = lane order.
//
// Per factored vocabulary (most significant first), z = logit * (1 / tau):
//   1. wave max / arg-max, wave sum of exp(z - max): the tempered UNFILTERED softmax, which the confidence is taken from
//   2. top-k: bitwise bisection on the order-preserving integer image of z for the k-th largest value (32 rounds of one
//      compare per entry + one wave count); ties at the threshold are admitted in index order by a lane prefix count
//   3. top-p: the same bisection on the value with mass(z >= t) in place of the count (monotone in t); ties likewise
//   4. inverse-CDF pick in index order over the kept entries on the caller's uniform: position = #{kept prefix sums < u * total},
//      then the kept entry at that position (the last kept one if the position runs past them)
// With every filter off the operations on the values, and their order, are those of sample_kernel: same samples, same bits of conf.
// The tail lane writes samples / conf and, when asked, the "confidence"-mode unmasking key log(conf) + scale * gumbel(noise).
//
// The two flavours share every line but the fetch: Rows keeps the 64 * PER token-major values of a factor in registers
// (16-byte loads, one read of the logits), Strided re-reads them per pass through the layout's strides (any vocabulary size).
//
// Classifier-free guidance (genie_guidance, genie_sample_guided) is a third and a fourth fetch: the Guided flavours read the
// conditional and the null row of the same token and form g = (w * c) + ((1 - w) * u) -- three separately rounded f32 operations --
// where the unguided ones read one logit; everything from z = g * (1 / tau) on is the code above, in the same launch.
#include "kernels.hpp"

// the per-entry loops ask for unrolling: complete in the Rows flavour (compile-time trip count, values in registers); in the
// Strided flavour the trip count is a run-time value and the request is declined, which -Wall would report
#pragma clang diagnostic ignored "-Wpass-failed"

namespace genie {

typedef float f32x4s __attribute__((ext_vector_type(4)));

struct SampleFilter {
    float inv_tau;   // 1.0f / logit_temperature
    int top_k;       // 0 = off
    float top_p;     // >= 1 = off
};

// order-preserving image of an f32 in uint32 (-0 == +0, as the float compare has it)
__device__ __forceinline__ uint32_t order_key(float z) {
    const uint32_t b = z == 0.f ? 0u : __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float order_key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// wave reductions of the bisection rounds on DPP row operations (four in-row steps, then the four row totals through
// v_readlane): a __shfl_xor butterfly is six dependent LDS-crossbar round trips, 64 times per token.  Every lane gets the same bits.
template <int CTRL>
__device__ __forceinline__ int dpp_mov(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += __int_as_float(dpp_mov<0xB1>(__float_as_int(v)));    // quad_perm [1,0,3,2]
    v += __int_as_float(dpp_mov<0x4E>(__float_as_int(v)));    // quad_perm [2,3,0,1]
    v += __int_as_float(dpp_mov<0x141>(__float_as_int(v)));   // row_half_mirror
    v += __int_as_float(dpp_mov<0x140>(__float_as_int(v)));   // row_mirror: every lane holds its row's 16-lane sum
    const int i = __float_as_int(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(i, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(i, 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(i, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(i, 48));
    return (r0 + r1) + (r2 + r3);
}
__device__ __forceinline__ int wave_isum_dpp(int v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
           (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}
// entries of the lanes below this one (exclusive prefix over lanes)
__device__ __forceinline__ int lane_prefix(int v, int lane) {
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    return incl - v;
}

// the values of one factor as a lane sees them: entry q of the lane is vocabulary index lane * per() + q
template <int PER>
struct RowsVals {   // token-major, vf == 64 * PER: registers
    float zr[PER];
    int lane;
    __device__ __forceinline__ void load(const float* lf, float inv_tau) {
#pragma unroll
        for (int q = 0; q < PER; q += 4) {
            const f32x4s t = *reinterpret_cast<const f32x4s*>(lf + lane * PER + q);
            zr[q] = t.x * inv_tau; zr[q + 1] = t.y * inv_tau; zr[q + 2] = t.z * inv_tau; zr[q + 3] = t.w * inv_tau;
        }
    }
    __device__ __forceinline__ int per() const { return PER; }
    __device__ __forceinline__ bool valid(int) const { return true; }
    __device__ __forceinline__ int idx(int q) const { return lane * PER + q; }
    __device__ __forceinline__ float z(int q) const { return zr[q]; }
};
struct StridedVals {   // any layout, any vocabulary size: memory
    const float* lf;
    long vstride;
    int lane, vf, n_per;
    float inv_tau;
    __device__ __forceinline__ int per() const { return n_per; }
    __device__ __forceinline__ bool valid(int q) const { return lane * n_per + q < vf; }
    __device__ __forceinline__ int idx(int q) const { return lane * n_per + q; }
    __device__ __forceinline__ float z(int q) const { return lf[(size_t)(lane * n_per + q) * vstride] * inv_tau; }
};

// guided logit: g = (w * c) + (omw * u), omw = 1.0f - w from the host; three roundings, never an FMA
struct Guide {
    float w, omw;
};
__device__ __forceinline__ float guide(float c, float u, Guide g) { return __fadd_rn(__fmul_rn(g.w, c), __fmul_rn(g.omw, u)); }

template <int PER>
struct GuidedRowsVals {   // RowsVals on two rows: two 16-byte loads per four entries, combined into the same registers
    float zr[PER];
    int lane;
    __device__ __forceinline__ void load(const float* lc, const float* lu, Guide g, float inv_tau) {
#pragma unroll
        for (int q = 0; q < PER; q += 4) {
            const f32x4s a = *reinterpret_cast<const f32x4s*>(lc + lane * PER + q);
            const f32x4s b = *reinterpret_cast<const f32x4s*>(lu + lane * PER + q);
            zr[q] = guide(a.x, b.x, g) * inv_tau; zr[q + 1] = guide(a.y, b.y, g) * inv_tau;
            zr[q + 2] = guide(a.z, b.z, g) * inv_tau; zr[q + 3] = guide(a.w, b.w, g) * inv_tau;
        }
    }
    __device__ __forceinline__ int per() const { return PER; }
    __device__ __forceinline__ bool valid(int) const { return true; }
    __device__ __forceinline__ int idx(int q) const { return lane * PER + q; }
    __device__ __forceinline__ float z(int q) const { return zr[q]; }
};
struct GuidedStridedVals {   // StridedVals on two bases with the same strides
    const float* lc;
    const float* lu;
    long vstride;
    int lane, vf, n_per;
    float inv_tau;
    Guide g;
    __device__ __forceinline__ int per() const { return n_per; }
    __device__ __forceinline__ bool valid(int q) const { return lane * n_per + q < vf; }
    __device__ __forceinline__ int idx(int q) const { return lane * n_per + q; }
    __device__ __forceinline__ float z(int q) const {
        const size_t o = (size_t)(lane * n_per + q) * vstride;
        return guide(lc[o], lu[o], g) * inv_tau;
    }
};

// survivors of top-k: key above the threshold, or equal to it and among the first `room` such entries in index order
struct KeepK {
    uint32_t thr;
    int room;
    __device__ __forceinline__ bool operator()(uint32_t key, int& ties) const {
        if (key > thr) return true;
        if (key != thr) return false;
        return ties++ < room;
    }
};
// ... of top-p among them: mass of the better-ranked survivors below the target
struct KeepP {
    uint32_t thr;
    float above, e_thr, target;   // mass(key > thr), exp of the threshold value, top_p * mass of the top-k survivors
    __device__ __forceinline__ bool operator()(uint32_t key, int& ties) const {
        if (key > thr) return true;
        if (key != thr) return false;
        const int r = ties++;
        return above + (float)r * e_thr < target || (r == 0 && above == 0.f);   // the best entry is always kept
    }
};

// One factor of one token: pick and its probability under the tempered unfiltered softmax.
template <class Vals>
__device__ __forceinline__ void sample_factor(const Vals& X, const int lane, const int vf, const bool draw, const SampleFilter f,
                                              const float uniform, int& pick_out, float& p_out) {
    float mx = -INFINITY;
    int mi = 0;
#pragma unroll
    for (int q = 0; q < X.per(); ++q)
        if (X.valid(q)) {
            const float z = X.z(q);
            if (z > mx) { mx = z; mi = X.idx(q); }
        }
    wave_argmax(mx, mi);
    float part = 0.f;
#pragma unroll
    for (int q = 0; q < X.per(); ++q)
        if (X.valid(q)) part += expf(X.z(q) - mx);
    const float tot = wave_sum(part);
    pick_out = mi;
    p_out = 1.0f / tot;
    if (!draw) return;   // arg-max: no filter can change it

    // ---- top-k
    KeepK kk{0u, 0x7fffffff};
    int tie_base_k = 0;
    if (f.top_k > 0 && f.top_k < vf) {
        uint32_t thr = 0;
#pragma unroll 1
        for (int bit = 31; bit >= 0; --bit) {   // the largest t with #{key >= t} >= k is the k-th largest key
            const uint32_t cand = thr | (1u << bit);
            int c = 0;
#pragma unroll
            for (int q = 0; q < X.per(); ++q)
                if (X.valid(q)) c += order_key(X.z(q)) >= cand ? 1 : 0;
            if (wave_isum_dpp(c) >= f.top_k) thr = cand;
        }
        int above = 0, ties = 0;
#pragma unroll
        for (int q = 0; q < X.per(); ++q)
            if (X.valid(q)) {
                const uint32_t key = order_key(X.z(q));
                above += key > thr ? 1 : 0;
                ties += key == thr ? 1 : 0;
            }
        kk.thr = thr;
        kk.room = f.top_k - wave_isum_dpp(above);
        tie_base_k = lane_prefix(ties, lane);
    }

    // ---- top-p among the survivors
    KeepP kp{0u, 0.f, 0.f, INFINITY};
    int tie_base_p = 0;
    if (f.top_p > 0.f && f.top_p < 1.f) {
        float m = 0.f;
        int tk = tie_base_k;
#pragma unroll
        for (int q = 0; q < X.per(); ++q)
            if (X.valid(q)) {
                const float z = X.z(q);
                m += kk(order_key(z), tk) ? expf(z - mx) : 0.f;
            }
        const float target = f.top_p * wave_sum_dpp(m);
        uint32_t thr = 0;
#pragma unroll 1
        for (int bit = 31; bit >= 0; --bit) {   // the largest t with mass(key >= t) >= target: the value the nucleus ends in
            const uint32_t cand = thr | (1u << bit);
            m = 0.f;
            tk = tie_base_k;
#pragma unroll
            for (int q = 0; q < X.per(); ++q)
                if (X.valid(q)) {
                    const float z = X.z(q);
                    const uint32_t key = order_key(z);
                    const float e = kk(key, tk) ? expf(z - mx) : 0.f;
                    m += key >= cand ? e : 0.f;
                }
            if (wave_sum_dpp(m) >= target) thr = cand;
        }
        m = 0.f;
        tk = tie_base_k;
        int ties = 0;
#pragma unroll
        for (int q = 0; q < X.per(); ++q)
            if (X.valid(q)) {
                const float z = X.z(q);
                const uint32_t key = order_key(z);
                const bool in_k = kk(key, tk);
                m += (in_k && key > thr) ? expf(z - mx) : 0.f;
                ties += (in_k && key == thr) ? 1 : 0;
            }
        kp.thr = thr;
        kp.above = wave_sum_dpp(m);
        kp.e_thr = expf(order_key_value(thr) - mx);
        kp.target = target;
        tie_base_p = lane_prefix(ties, lane);
    }

    // ---- inverse CDF in index order over the kept entries (the scheme of sample_kernel)
    float part_k = 0.f;
    int n_kept = 0;
    {
        int tk = tie_base_k, tp = tie_base_p;
#pragma unroll
        for (int q = 0; q < X.per(); ++q)
            if (X.valid(q)) {
                const float z = X.z(q);
                const uint32_t key = order_key(z);
                const bool kept = kk(key, tk) && kp(key, tp);
                part_k += kept ? expf(z - mx) : 0.f;
                n_kept += kept ? 1 : 0;
            }
    }
    const float u = uniform * wave_sum(part_k);
    float incl = part_k;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    float run = incl - part_k;
    int cntl = 0;
    {
        int tk = tie_base_k, tp = tie_base_p;
#pragma unroll
        for (int q = 0; q < X.per(); ++q)
            if (X.valid(q)) {
                const float z = X.z(q);
                const uint32_t key = order_key(z);
                const bool kept = kk(key, tk) && kp(key, tp);
                run += kept ? expf(z - mx) : 0.f;
                cntl += (kept && run < u) ? 1 : 0;
            }
    }
    int pos = wave_isum_dpp(cntl);
    const int total_kept = wave_isum_dpp(n_kept);   // >= 1: the arg-max survives every filter
    pos = pos < total_kept - 1 ? pos : total_kept - 1;
    // the kept entry number `pos` in index order
    int seen = lane_prefix(n_kept, lane);
    int found_idx = -1;
    float found_e = 0.f;
    {
        int tk = tie_base_k, tp = tie_base_p;
#pragma unroll
        for (int q = 0; q < X.per(); ++q)
            if (X.valid(q)) {
                const float z = X.z(q);
                const uint32_t key = order_key(z);
                if (kk(key, tk) && kp(key, tp)) {
                    if (seen == pos) { found_idx = X.idx(q); found_e = expf(z - mx); }
                    ++seen;
                }
            }
    }
    const unsigned long long owner = __ballot(found_idx >= 0);   // exactly one lane
    const int src = owner ? __ffsll((long long)owner) - 1 : 0;
    pick_out = __shfl(found_idx, src);
    p_out = __shfl(found_e, src) / tot;
}

// the unmasking key of the "confidence" mode: log(conf) + scale * g, g = -log(-log(u)) on the caller's clamped U[0,1) draw
__device__ __forceinline__ float confidence_key(float cf, float noise, float scale) {
    const float u = fminf(fmaxf(noise, 0x1p-24f), 1.0f - 0x1p-24f);
    return logf(cf) + scale * (-logf(-logf(u)));
}

template <int PER>
__global__ __launch_bounds__(256) void sample_filtered_rows_kernel(const float* __restrict__ logits, long n_tok, long V, int vf, int nfac,
                                                                   float temperature, SampleFilter f,
                                                                   const float* __restrict__ uniforms, int64_t* __restrict__ samples,
                                                                   float* conf, float* keys_out, const float* __restrict__ noise,
                                                                   float key_scale) {
    static_assert(PER % 4 == 0, "16-byte loads");
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    const float* lp = logits + (size_t)n * V;
    const bool draw = temperature > 1e-8f;
    int64_t sample = 0;
    float cf = 1.0f;
    for (int k = 0; k < nfac; ++k) {
        const int fac = nfac - 1 - k;  // flip(2): hi factor first (st_mask_git.py:179)
        RowsVals<PER> X;
        X.lane = lane;
        X.load(lp + (size_t)fac * vf, f.inv_tau);
        int pick;
        float p;
        sample_factor(X, lane, vf, draw, f, draw ? uniforms[(size_t)k * n_tok + n] : 0.f, pick, p);
        sample = sample * vf + pick;
        cf *= p;
    }
    if (lane == 0) {
        samples[n] = sample;
        if (keys_out != conf) conf[n] = cf;
        if (keys_out) keys_out[n] = confidence_key(cf, noise[n], key_scale);
    }
}

__global__ __launch_bounds__(256) void sample_filtered_kernel(const float* __restrict__ logits, long tok_stride_b, long tok_stride_s,
                                                              long vstride, int B, int S, int vf, int nfac, float temperature,
                                                              SampleFilter f, const float* __restrict__ uniforms,
                                                              int64_t* __restrict__ samples, float* conf, float* keys_out,
                                                              const float* __restrict__ noise, float key_scale) {
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= (long)B * S) return;
    const long b = n / S, s = n - b * S;
    const float* lp = logits + (size_t)b * tok_stride_b + (size_t)s * tok_stride_s;
    const bool draw = temperature > 1e-8f;
    int64_t sample = 0;
    float cf = 1.0f;
    for (int k = 0; k < nfac; ++k) {
        const int fac = nfac - 1 - k;
        const StridedVals X{lp + (size_t)fac * vf * vstride, vstride, lane, vf, (vf + 63) / 64, f.inv_tau};
        int pick;
        float p;
        sample_factor(X, lane, vf, draw, f, draw ? uniforms[((size_t)k * B + b) * S + s] : 0.f, pick, p);
        sample = sample * vf + pick;
        cf *= p;
    }
    if (lane == 0) {
        samples[n] = sample;
        if (keys_out != conf) conf[n] = cf;
        if (keys_out) keys_out[n] = confidence_key(cf, noise[n], key_scale);
    }
}

// the two kernels above with the guided fetch: token n of the B * S reads row n of both logits tensors
template <int PER>
__global__ __launch_bounds__(256) void sample_guided_rows_kernel(const float* __restrict__ logits_c, const float* __restrict__ logits_u,
                                                                 Guide g, long n_tok, long V, int vf, int nfac, float temperature,
                                                                 SampleFilter f, const float* __restrict__ uniforms,
                                                                 int64_t* __restrict__ samples, float* conf, float* keys_out,
                                                                 const float* __restrict__ noise, float key_scale) {
    static_assert(PER % 4 == 0, "16-byte loads");
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= n_tok) return;
    const float* lc = logits_c + (size_t)n * V;
    const float* lu = logits_u + (size_t)n * V;
    const bool draw = temperature > 1e-8f;
    int64_t sample = 0;
    float cf = 1.0f;
    for (int k = 0; k < nfac; ++k) {
        const int fac = nfac - 1 - k;
        GuidedRowsVals<PER> X;
        X.lane = lane;
        X.load(lc + (size_t)fac * vf, lu + (size_t)fac * vf, g, f.inv_tau);
        int pick;
        float p;
        sample_factor(X, lane, vf, draw, f, draw ? uniforms[(size_t)k * n_tok + n] : 0.f, pick, p);
        sample = sample * vf + pick;
        cf *= p;
    }
    if (lane == 0) {
        samples[n] = sample;
        if (keys_out != conf) conf[n] = cf;
        if (keys_out) keys_out[n] = confidence_key(cf, noise[n], key_scale);
    }
}

__global__ __launch_bounds__(256) void sample_guided_kernel(const float* __restrict__ logits_c, const float* __restrict__ logits_u, Guide g,
                                                            long tok_stride_b, long tok_stride_s, long vstride, int B, int S, int vf,
                                                            int nfac, float temperature, SampleFilter f,
                                                            const float* __restrict__ uniforms, int64_t* __restrict__ samples, float* conf,
                                                            float* keys_out, const float* __restrict__ noise, float key_scale) {
    const int lane = threadIdx.x & 63;
    const long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= (long)B * S) return;
    const long b = n / S, s = n - b * S;
    const size_t tok = (size_t)b * tok_stride_b + (size_t)s * tok_stride_s;
    const bool draw = temperature > 1e-8f;
    int64_t sample = 0;
    float cf = 1.0f;
    for (int k = 0; k < nfac; ++k) {
        const int fac = nfac - 1 - k;
        const size_t o = tok + (size_t)fac * vf * vstride;
        const GuidedStridedVals X{logits_c + o, logits_u + o, vstride, lane, vf, (vf + 63) / 64, f.inv_tau, g};
        int pick;
        float p;
        sample_factor(X, lane, vf, draw, f, draw ? uniforms[((size_t)k * B + b) * S + s] : 0.f, pick, p);
        sample = sample * vf + pick;
        cf *= p;
    }
    if (lane == 0) {
        samples[n] = sample;
        if (keys_out != conf) conf[n] = cf;
        if (keys_out) keys_out[n] = confidence_key(cf, noise[n], key_scale);
    }
}

// out[r][i] = guide(cond[r][i], null[r][i]) for `rows` rows of `len` values (row strides in elements): the guided step-0 logits
__global__ __launch_bounds__(256) void guide_logits_kernel(const float* __restrict__ cond, const float* __restrict__ null_, float* __restrict__ out,
                                                           long rows, long len, long in_stride, long out_stride, Guide g) {
    const long total = rows * len;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / len, j = i - r * len;
        out[r * out_stride + j] = guide(cond[r * in_stride + j], null_[r * in_stride + j], g);
    }
}

bool sampling_is_neutral(const genie_sampling* sp, int vf) {
    return !sp || (sp->logit_temperature == 1.0f && (sp->top_k <= 0 || sp->top_k >= vf) && !(sp->top_p > 0.f && sp->top_p < 1.f));
}

// the kernels' view of a law (NULL = every field off) and the scale of the confidence-mode key
static SampleFilter make_filter(const genie_sampling* sp, int vf, float anneal, float& key_scale) {
    SampleFilter f{1.0f, 0, 1.0f};
    key_scale = 0.f;
    if (sp) {
        f.inv_tau = 1.0f / sp->logit_temperature;
        f.top_k = (sp->top_k > 0 && sp->top_k < vf) ? sp->top_k : 0;
        f.top_p = (sp->top_p > 0.f && sp->top_p < 1.f) ? sp->top_p : 1.0f;
        key_scale = sp->choice_temperature * anneal;
    }
    return f;
}

int launch_sample_ex(const genie_cfg& c, const float* logits, int layout, int B, float temperature, const float* uniforms,
                     int64_t* samples, float* conf, const genie_sampling* sp, float* keys_out, const float* noise, float anneal,
                     hipStream_t st) {
    const int vf = c.factored_vocab;
    if (sampling_is_neutral(sp, vf) && !keys_out)   // today's kernels, bit for bit
        return launch_sample(c, logits, layout, B, temperature, uniforms, samples, conf, st);
    float key_scale;
    const SampleFilter f = make_filter(sp, vf, anneal, key_scale);
    const long V = (long)vf * c.num_factored, n = (long)B * c.S;
    if (layout == GENIE_LAYOUT_TOKEN_MAJOR && vf == 512 && ((uintptr_t)logits & 15) == 0) {
        sample_filtered_rows_kernel<8><<<(unsigned)((n + 3) / 4), 256, 0, st>>>(logits, n, V, vf, c.num_factored, temperature, f, uniforms,
                                                                                samples, conf, keys_out, noise, key_scale);
        GENIE_LAUNCH_CHECK("sample_filtered_rows");
        return GENIE_OK;
    }
    long sb = (long)c.S * V, ss, vs;
    if (layout == GENIE_LAYOUT_TOKEN_MAJOR) { ss = V; vs = 1; }
    else { ss = 1; vs = c.S; }
    sample_filtered_kernel<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(logits, sb, ss, vs, B, c.S, vf, c.num_factored, temperature, f,
                                                                     uniforms, samples, conf, keys_out, noise, key_scale);
    GENIE_LAUNCH_CHECK("sample_filtered");
    return GENIE_OK;
}

int launch_sample_guided(const genie_cfg& c, const float* logits_c, const float* logits_u, int layout, int B, float temperature,
                         const float* uniforms, int64_t* samples, float* conf, const genie_sampling* sp, float* keys_out,
                         const float* noise, float anneal, float scale, hipStream_t st) {
    if (scale == 1.0f)   // g = c: the unguided launch, the null logits are not read
        return launch_sample_ex(c, logits_c, layout, B, temperature, uniforms, samples, conf, sp, keys_out, noise, anneal, st);
    const int vf = c.factored_vocab;
    float key_scale;
    const SampleFilter f = make_filter(sp, vf, anneal, key_scale);
    const Guide g{scale, 1.0f - scale};
    const long V = (long)vf * c.num_factored, n = (long)B * c.S;
    if (layout == GENIE_LAYOUT_TOKEN_MAJOR && vf == 512 && (((uintptr_t)logits_c | (uintptr_t)logits_u) & 15) == 0) {
        sample_guided_rows_kernel<8><<<(unsigned)((n + 3) / 4), 256, 0, st>>>(logits_c, logits_u, g, n, V, vf, c.num_factored, temperature, f,
                                                                              uniforms, samples, conf, keys_out, noise, key_scale);
        GENIE_LAUNCH_CHECK("sample_guided_rows");
        return GENIE_OK;
    }
    long sb = (long)c.S * V, ss, vs;
    if (layout == GENIE_LAYOUT_TOKEN_MAJOR) { ss = V; vs = 1; }
    else { ss = 1; vs = c.S; }
    sample_guided_kernel<<<(unsigned)((n + 3) / 4), 256, 0, st>>>(logits_c, logits_u, g, sb, ss, vs, B, c.S, vf, c.num_factored, temperature,
                                                                   f, uniforms, samples, conf, keys_out, noise, key_scale);
    GENIE_LAUNCH_CHECK("sample_guided");
    return GENIE_OK;
}

int launch_guide_logits(const float* cond, const float* null_, float* out, long rows, long len, long in_stride, long out_stride, float scale,
                        hipStream_t st) {
    const long total = rows * len;
    if (total <= 0) return GENIE_OK;
    const long blocks = (total + 255) / 256;
    guide_logits_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, st>>>(cond, null_, out, rows, len, in_stride, out_stride,
                                                                                      Guide{scale, 1.0f - scale});
    GENIE_LAUNCH_CHECK("guide_logits");
    return GENIE_OK;
}

}  // namespace genie
