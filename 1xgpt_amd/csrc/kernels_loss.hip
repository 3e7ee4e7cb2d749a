// Loss and scoring kernels: everything that turns a token's factored logits row (nfac factors of vf logits, token-major unless said
// otherwise) into a loss.  All of it is f32 per token with f64 sums; a token is one wave (lane l takes classes l, l + 64, ...) except
// in ce_bcthw_kernel.  The contracts:
//
//   evaluator CE (genie_factored_ce / genie_readout_ce; st_mask_git.py:231-253, eval_utils.py:72-77), read-only logits:
//     sums += [sum ce, sum all-factors-argmax-correct, n] over the tokens of frames [t0, t1) whose weight id is MASK (all without
//     weight_ids).  One atomicAdd per sum and workgroup.  count_equal_kernel files the evaluator's metric vector beside it.
//   scoring (genie_score_logits / genie_score_fanout), read-only logits: the same per-token loss kept apart per row -- nll, hits
//     (f64, one per row) and optionally every token's loss (f32); fixed-order sums, no atomics: the same bits launch to launch.
//   training losses, d loss / d logits REPLACING each logits row; counted(token) = frame >= 1 and input id == MASK, an uncounted
//   token's row becomes zero; the count kernel of each runs first and writes the normaliser the loss kernel divides by:
//     neutral step (st_mask_git.py:231-253, 276): sums = [sum ce, sum hits, n];  row <- (softmax_f - onehot_f) / n
//     objective (include/genie_hip.h, "Training objective": label smoothing eps, z-loss zeta, per-frame weights w_t):
//       sums = [sum w_t l_n, sum hits, W = sum_t w_t c_t, sum plain nll, n = sum_t c_t]; hits and plain nll over ALL counted tokens
//       row <- w_t > 0 ? (p (1 + 2 zeta lse) - q) (float)(w_t / W) : 0
//     distillation (include/genie_hip.h, "Distillation"): the objective with a read-only row of TEACHER logits beside every row
//       l_f = (1 - alpha) hard_f + alpha tau^2 KL(r || pt) + zeta lse^2,   r = softmax(u / tau), pt = softmax(z / tau)
//       d l_f / d z_k = (1 - alpha)(p_k - q_k) + 2 zeta lse p_k + alpha tau (pt_k - r_k)
//       sums = the objective's five + [sum plain kd, sum teacher plain nll]; entries 1, 3, 5, 6 over ALL counted tokens
//   No atomics on d logits (the same bytes run to run); the accumulated sums use double atomics, so they depend on arrival order.
//
// The steps the kernels share are stated once, in front of them: a factor's streaming log-sum-exp, a token's cross-entropy, the
// training losses' token head and the workgroup's tail.
#include <algorithm>

#include "kernels.hpp"

namespace genie {

// ------------------------------------------------------------------------------------------------
// The shared steps
// ------------------------------------------------------------------------------------------------
// One factor's log-sum-exp, streamed from memory by one wave: first-max-wins arg-max, then sum of expf(v - max); lse = logf(se) + mx.
// SUMZ: sz is this LANE's sum of the logits, riding in the first pass (the smoothing term; its wave_sum is the caller's).
struct FactorLse {
    float mx, se, sz;
    int mi;
};
template <bool SUMZ>
__device__ __forceinline__ FactorLse factor_lse(const float* lf, int vf, int lane) {
    FactorLse r{-INFINITY, 0.f, 0.f, 0};
    for (int k = lane; k < vf; k += 64) {
        const float x = lf[k];
        if constexpr (SUMZ) r.sz += x;
        if (x > r.mx) { r.mx = x; r.mi = k; }
    }
    wave_argmax(r.mx, r.mi);
    for (int k = lane; k < vf; k += 64) r.se += expf(lf[k] - r.mx);
    r.se = wave_sum(r.se);
    return r;
}

// A token's cross-entropy summed over its factors, and whether every factor's arg-max is the target's.  The target is decomposed
// unsigned: the same factors as the signed form for every id >= 0 (a negative id indexes outside the row in either).
__device__ __forceinline__ float token_ce(const float* __restrict__ lp, uint64_t tgt, int vf, int nfac, int lane, bool& all_ok) {
    float loss = 0.f;
    all_ok = true;
    if (vf == 512 && nfac == 2) {
        // the shipped vocabulary (2 x 512): a lane owns 8 consecutive logits of each factor -- all four 16-byte loads of the token are
        // in flight before the first use (the strided dword loop below waits on a memory round trip per 64 logits: 1.2 ms for 1 GB of
        // logits, 0.45 TB/s).  Same arithmetic: first-max-wins argmax, sum of expf(v - max), logf.
        typedef float ce4 __attribute__((ext_vector_type(4)));
        ce4 v[2][2];
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int q = 0; q < 2; ++q) v[f][q] = *reinterpret_cast<const ce4*>(lp + f * 512 + lane * 8 + q * 4);
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            const int tf = (int)(tgt % 512);
            tgt /= 512;
            float mx = -INFINITY;
            int mi = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float x = v[f][q >> 2][q & 3];
                if (x > mx) { mx = x; mi = lane * 8 + q; }
            }
            wave_argmax(mx, mi);
            float se = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) se += expf(v[f][q >> 2][q & 3] - mx);
            se = wave_sum(se);
            float tv = 0.f;   // the target's logit sits in lane tf / 8, slot tf % 8
#pragma unroll
            for (int q = 0; q < 8; ++q) tv = (tf & 7) == q ? v[f][q >> 2][q & 3] : tv;
            tv = __shfl(tv, tf >> 3);
            loss += (logf(se) + mx) - tv;
            all_ok = all_ok && (mi == tf);
        }
        return loss;
    }
    for (int f = 0; f < nfac; ++f) {
        const int tf = (int)(tgt % (uint64_t)vf);
        tgt /= (uint64_t)vf;
        const float* lf = lp + f * vf;
        const FactorLse s = factor_lse<false>(lf, vf, lane);
        loss += (logf(s.se) + s.mx) - lf[tf];
        all_ok = all_ok && (s.mi == tf);
    }
    return loss;
}

// The head of a training-loss token (one wave): t is its frame, and it is counted when t >= 1 and its input id is MASK; the wave zeroes
// the `row` logits of a token that is not.
__device__ __forceinline__ bool token_counted(float* lp, const int64_t* __restrict__ ids, long n, int T, int S, int64_t mask_id, int row,
                                              int lane, int& t) {
    t = (int)((n / S) % T);
    const bool counted = t >= 1 && ids[n] == mask_id;
    if (!counted)
        for (int k = lane; k < row; k += 64) lp[k] = 0.f;
    return counted;
}

// The tail of a 256-thread workgroup: the values of lane 0 of each wave (LANES: of all its lanes, butterflied first) are added in wave
// order by thread 0, which adds each sum that is not zero to sums[SLOT].  Every addend is >= 0 and the sums start at +0, so a skipped
// zero changes no bit.
template <bool LANES, int... SLOT, typename... V>
__device__ __forceinline__ void block_add_sums(double* sums, V... v) {
    constexpr int K = sizeof...(SLOT);
    static_assert(sizeof...(V) == K, "one value per slot");
    constexpr int slot[K] = {SLOT...};
    __shared__ double red[K][4];
    double a[K] = {v...};
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if constexpr (LANES) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int i = 0; i < K; ++i) a[i] += __shfl_xor(a[i], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < K; ++i) red[i][wid] = a[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            a[i] = 0;
            for (int w = 0; w < 4; ++w) a[i] += red[i][w];
        }
#pragma unroll
        for (int i = 0; i < K; ++i)
            if (a[i] != 0.0) atomicAdd(&sums[slot[i]], a[i]);
    }
}

// ------------------------------------------------------------------------------------------------
// a12  factored cross-entropy + "all factors argmax-correct" (st_mask_git.py:231-253, eval_utils.py:72-77)
// token-major: one wavefront per token (V contiguous, 2 KB per factor, coalesced).
// BCTHW: one lane per token, 64 consecutive tokens per wave, loop over the vocab (coalesced across lanes).
// ------------------------------------------------------------------------------------------------
// logits token-major (B, nt, S, V): token index n = (b*nt + tt)*S + s
__global__ __launch_bounds__(256) void ce_token_major_kernel(const float* __restrict__ logits,
                                                             const int64_t* __restrict__ targets,
                                                             const int64_t* __restrict__ weight_ids, long n_tok,
                                                             int nt, int S, int T, int t0, int vf, int nfac,
                                                             int64_t mask_id, double* sums) {
    const int lane = threadIdx.x & 63;
    double ce = 0, hit = 0, cnt = 0;
    // grid-stride over tokens: the three f64 atomics per block all land on the same addresses (~6 ns each at the L2), so one
    // block per four tokens made the atomics, not the 4 KB of logits per token, the kernel's time (1.2 ms for 246 k tokens)
    for (long n = (long)blockIdx.x * 4 + (threadIdx.x >> 6); n < n_tok; n += (long)gridDim.x * 4) {
        long b = n / ((long)nt * S);
        long rem = n - b * (long)nt * S;
        long gi = (b * T + t0) * (long)S + rem;  // index into the full (B,T,S) clip
        bool counted = weight_ids ? (weight_ids[gi] == mask_id) : true;
        if (counted) {
            bool all_ok;
            const float loss = token_ce(logits + (size_t)n * vf * nfac, (uint64_t)targets[gi], vf, nfac, lane, all_ok);
            if (lane == 0) { ce += loss; hit += all_ok ? 1.0 : 0.0; cnt += 1.0; }
        }
    }
    block_add_sums<true, 0, 1, 2>(sums, ce, hit, cnt);
}

// logits BCTHW (B, V, nt, S): element (b, v, tt, s) at ((b*V + v)*nt + tt)*S + s
__global__ __launch_bounds__(256) void ce_bcthw_kernel(const float* __restrict__ logits,
                                                       const int64_t* __restrict__ targets,
                                                       const int64_t* __restrict__ weight_ids, long n_tok, int nt,
                                                       int S, int T, int t0, int vf, int nfac, int64_t mask_id,
                                                       double* sums) {
    long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    double ce = 0, hit = 0, cnt = 0;
    if (n < n_tok) {
        long b = n / ((long)nt * S);
        long rem = n - b * (long)nt * S;  // tt*S + s
        long gi = (b * T + t0) * (long)S + rem;
        bool counted = weight_ids ? (weight_ids[gi] == mask_id) : true;
        if (counted) {
            int64_t tgt = targets[gi];
            const long vstride = (long)nt * S;
            const float* lp = logits + (size_t)b * vf * nfac * vstride + rem;
            float loss = 0.f;
            bool all_ok = true;
            for (int f = 0; f < nfac; ++f) {
                int tf = (int)(tgt % vf);
                tgt /= vf;
                const float* lf = lp + (size_t)f * vf * vstride;
                float mx = -INFINITY;
                int mi = 0;
                for (int k = 0; k < vf; ++k) {
                    float v = lf[(size_t)k * vstride];
                    if (v > mx) { mx = v; mi = k; }
                }
                float se = 0.f;
                for (int k = 0; k < vf; ++k) se += expf(lf[(size_t)k * vstride] - mx);
                loss += (logf(se) + mx) - lf[(size_t)tf * vstride];
                all_ok = all_ok && (mi == tf);
            }
            ce = loss; hit = all_ok ? 1.0 : 0.0; cnt = 1.0;
        }
    }
    block_add_sums<true, 0, 1, 2>(sums, ce, hit, cnt);
}

// sampled-token accuracy numerator of the evaluator (evaluate.py:176-179: (samples == ground truth).sum()): a (batch, n) view
// with batch stride `sa` against b (batch, n) with stride `sb`; the count is ADDED to sums6[2].  Block 0 also files the rest
// of the metric vector: sums6 = [sum CE, n CE tokens, hits, n tokens, n frames, n clips] with the CE pair taken from the
// 3-vector genie_factored_ce accumulated (ce3 = [sum CE, sum argmax-correct, n]; NULL = leave sums6[0..1] alone).
__global__ __launch_bounds__(256) void count_equal_kernel(const int64_t* __restrict__ a, long sa, const int64_t* __restrict__ b,
                                                          long sb, long n, long total, const double* __restrict__ ce3,
                                                          double* sums6, double n_tokens, double n_frames, double n_clips) {
    __shared__ int wsum[4];
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int hit = 0;
    if (i < total) {
        const long bi = i / n, r = i - bi * n;
        hit = a[bi * sa + r] == b[bi * sb + r];
    }
    const unsigned long long m = __ballot(hit);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int c = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (c) atomicAdd(&sums6[2], (double)c);  // integer-valued addends: the f64 sum is exact in any order
        if (blockIdx.x == 0) {
            if (ce3) { sums6[0] = ce3[0]; sums6[1] = ce3[2]; }
            sums6[3] = n_tokens; sums6[4] = n_frames; sums6[5] = n_clips;
        }
    }
}
int launch_count_equal(const int64_t* a, long sa, const int64_t* b, long sb, int batch, long n, const double* ce3, double* sums6,
                       double n_tokens, double n_frames, double n_clips, hipStream_t st) {
    const long total = (long)batch * n;
    if (total <= 0) return GENIE_OK;
    count_equal_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(a, sa, b, sb, n, total, ce3, sums6, n_tokens, n_frames,
                                                                        n_clips);
    GENIE_LAUNCH_CHECK("count_equal");
    return GENIE_OK;
}

int launch_factored_ce(const genie_cfg& c, const float* logits, int layout, const int64_t* targets,
                       const int64_t* weight_ids, int B, int t0, int t1, double* sums, hipStream_t st) {
    int nt = t1 - t0;
    long n_tok = (long)B * nt * c.S;
    if (n_tok <= 0) return GENIE_OK;
    if (layout == GENIE_LAYOUT_TOKEN_MAJOR) {
        const long blocks_all = (n_tok + 3) / 4;
        ce_token_major_kernel<<<(unsigned)(blocks_all < 2048 ? blocks_all : 2048), 256, 0, st>>>(
            logits, targets, weight_ids, n_tok, nt, c.S, c.T, t0, c.factored_vocab, c.num_factored,
            (int64_t)c.image_vocab_size, sums);
    } else {
        ce_bcthw_kernel<<<(unsigned)((n_tok + 255) / 256), 256, 0, st>>>(
            logits, targets, weight_ids, n_tok, nt, c.S, c.T, t0, c.factored_vocab, c.num_factored,
            (int64_t)c.image_vocab_size, sums);
    }
    GENIE_LAUNCH_CHECK("factored_ce");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// Per-row negative log-likelihood of observed tokens (genie_score_logits / genie_score_fanout): the per-token loss of
// ce_token_major_kernel, kept apart per row instead of summed over the batch.  Row i of the token-major (N, S, V) logits of ONE frame
// is scored against the S targets at targets + (i / K) * target_clip_stride: the K branches of a clip share their parent's tokens.
// One workgroup per row, one wave per token; wave w takes tokens w, w + nw, ... and keeps its own f64 partial, and thread 0 adds the nw
// partials in wave order -- a fixed order and no atomics, so two launches give the same bits.
// ------------------------------------------------------------------------------------------------
#define GENIE_SCORE_MAX_WAVES 16
__global__ __launch_bounds__(64 * GENIE_SCORE_MAX_WAVES) void score_rows_kernel(const float* __restrict__ logits,
                                                                                const int64_t* __restrict__ targets, long target_clip_stride,
                                                                                int K, int S, int vf, int nfac, double* __restrict__ nll,
                                                                                long nll_stride, double* __restrict__ hits,
                                                                                float* __restrict__ token_nll, long token_stride) {
    __shared__ double red[2][GENIE_SCORE_MAX_WAVES];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const long row = blockIdx.x;
    const int64_t* tg = targets + (row / K) * target_clip_stride;
    const float* lrow = logits + (size_t)row * S * vf * nfac;
    double acc = 0, hit = 0;
    for (int s = wid; s < S; s += nw) {
        bool ok;
        const float loss = token_ce(lrow + (size_t)s * vf * nfac, (uint64_t)tg[s], vf, nfac, lane, ok);
        acc += (double)loss;
        hit += ok ? 1.0 : 0.0;
        if (token_nll && lane == 0) token_nll[row * token_stride + s] = loss;
    }
    if (lane == 0) { red[0][wid] = acc; red[1][wid] = hit; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0, h = 0;
        for (int w = 0; w < nw; ++w) { a += red[0][w]; h += red[1][w]; }
        nll[row * nll_stride] = a;
        if (hits) hits[row * nll_stride] = h;
    }
}

int launch_score_rows(const genie_cfg& c, const float* logits, const int64_t* targets, long target_clip_stride, int K, long N, double* nll,
                      long nll_stride, double* hits, float* token_nll, long token_stride, hipStream_t st) {
    if (N <= 0) return GENIE_OK;
    GENIE_CHECK_SHAPE(N <= 0x7fffffffL, "score_rows: %ld rows", N);
    int nw = c.S / 4;   // four tokens per wave at the least: S = 16 runs 4 waves, S >= 64 all 16
    nw = nw < 1 ? 1 : (nw > GENIE_SCORE_MAX_WAVES ? GENIE_SCORE_MAX_WAVES : nw);
    score_rows_kernel<<<(unsigned)N, 64 * nw, 0, st>>>(logits, targets, target_clip_stride, K, c.S, c.factored_vocab, c.num_factored, nll,
                                                       nll_stride, hits, token_nll, token_stride);
    GENIE_LAUNCH_CHECK("score_rows");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// The neutral training step's loss, forward and backward in one pass: count_masked_kernel writes n = sums[2], then one wave per
// token, four tokens per workgroup.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void count_masked_kernel(const int64_t* __restrict__ ids, long B, int T, int S,
                                                            int64_t mask_id, double* __restrict__ sums) {
    __shared__ unsigned long long red[16];
    unsigned long long c = 0;
    const long n = B * T * (long)S;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const int t = (int)((i / S) % T);
        c += (t >= 1 && ids[i] == mask_id) ? 1ull : 0ull;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < 16; ++w) s += red[w];
        sums[2] = (double)s;
    }
}
__global__ __launch_bounds__(256) void ce_fwd_bwd_kernel(float* __restrict__ logits, const int64_t* __restrict__ ids,
                                                         const int64_t* __restrict__ labels, long n_tok, int T, int S,
                                                         int vf, int nfac, int64_t mask_id, double* __restrict__ sums) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long n = (long)blockIdx.x * 4 + wid;
    double ce = 0, hit = 0;
    if (n < n_tok) {
        float* lp = logits + (size_t)n * vf * nfac;
        int t;
        if (token_counted(lp, ids, n, T, S, mask_id, vf * nfac, lane, t)) {
            const float wgt = (float)(1.0 / sums[2]);
            int64_t tgt = labels[n];
            float loss = 0.f;
            bool all_ok = true;
            for (int f = 0; f < nfac; ++f) {
                const int tf = (int)(tgt % vf);
                tgt /= vf;
                float* lf = lp + f * vf;
                const FactorLse s = factor_lse<false>(lf, vf, lane);
                loss += logf(s.se) + s.mx - lf[tf];
                all_ok = all_ok && (s.mi == tf);
                const float inv = 1.0f / s.se;
                for (int k = lane; k < vf; k += 64) {
                    const float p = expf(lf[k] - s.mx) * inv;
                    lf[k] = (p - (k == tf ? 1.0f : 0.0f)) * wgt;
                }
            }
            if (lane == 0) { ce = loss; hit = all_ok ? 1.0 : 0.0; }
        }
    }
    block_add_sums<false, 0, 1>(sums, ce, hit);
}
int launch_ce_fwd_bwd(const genie_cfg& c, float* logits, const int64_t* ids, const int64_t* labels, int B, double* sums,
                      hipStream_t st) {
    const long n_tok = (long)B * c.T * c.S;
    if (n_tok <= 0) return GENIE_OK;
    count_masked_kernel<<<1, 1024, 0, st>>>(ids, B, c.T, c.S, (int64_t)c.image_vocab_size, sums);
    GENIE_LAUNCH_CHECK("count_masked");
    ce_fwd_bwd_kernel<<<(unsigned)((n_tok + 3) / 4), 256, 0, st>>>(logits, ids, labels, n_tok, c.T, c.S, c.factored_vocab,
                                                                  c.num_factored, (int64_t)c.image_vocab_size, sums);
    GENIE_LAUNCH_CHECK("ce_fwd_bwd");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// The general objective: these two run when any knob is set (and behind genie_ce_objective with a struct).
// Same mapping as ce_fwd_bwd_kernel and, lane by lane, the same order of every sum that kernel takes: at eps = zeta = 0 and w = 1 the
// rows are its bits.  REG: vf <= 512, a factor's values stay in registers (eight per lane), so the row comes from memory once; else
// the three passes of the kernel above, sum z riding in the first.
// ------------------------------------------------------------------------------------------------
// the per-frame loss weights as the loss kernels take them: by value in the kernel arguments (64 floats), no copy, no sync
struct FrameWeights {
    float w[64];
    int n;   // frames t >= n weigh 1 (n = 0: every frame)
    __device__ __forceinline__ float at(int t) const { return t < n ? w[t] : 1.0f; }
};
// the counted tokens per frame: sums[2] = W = sum_t w_t c_t, sums[4] = n = sum_t c_t
__global__ __launch_bounds__(1024) void count_frames_kernel(const int64_t* __restrict__ ids, long n_clips, int T, int S,
                                                            int64_t mask_id, FrameWeights fw, double* __restrict__ sums) {
    __shared__ unsigned int cnt[64];            // frames 0 .. 63 one by one: the only ones that can carry a weight
    __shared__ unsigned long long red[16];      // every later frame (all weigh 1), summed
    if (threadIdx.x < 64) cnt[threadIdx.x] = 0u;
    __syncthreads();
    unsigned long long c = 0;
    const long n = n_clips * T * (long)S;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const int t = (int)((i / S) % T);
        if (t >= 1 && ids[i] == mask_id) {
            if (t < 64) atomicAdd(&cnt[t], 1u);   // integers: any order gives the same count
            else c += 1ull;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long late = 0, all = 0;
        for (int w = 0; w < 16; ++w) late += red[w];
        double W = 0.0;
        for (int t = 1; t < 64 && t < T; ++t) {
            W += (double)fw.at(t) * (double)cnt[t];
            all += cnt[t];
        }
        sums[2] = W + (double)late;
        sums[4] = (double)(all + late);
    }
}

template <bool REG>
__global__ __launch_bounds__(256) void ce_objective_kernel(float* __restrict__ logits, const int64_t* __restrict__ ids,
                                                           const int64_t* __restrict__ labels, long n_tok, int T, int S, int vf,
                                                           int nfac, int64_t mask_id, float eps, float zeta, FrameWeights fw,
                                                           double* __restrict__ sums) {
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long n = (long)blockIdx.x * 4 + wid;
    double obj = 0, hit = 0, ce = 0;
    if (n < n_tok) {
        float* lp = logits + (size_t)n * vf * nfac;
        int t;
        if (token_counted(lp, ids, n, T, S, mask_id, vf * nfac, lane, t)) {
            const float wt = fw.at(t);
            const bool live = wt > 0.0f;   // a zero-weight frame: counted in hits and plain nll, a zero row, never times 1 / W
            const float wgt = live ? (float)((double)wt / sums[2]) : 0.0f;
            const float q_off = eps / (float)vf, q_on = (1.0f - eps) + q_off, inv_vf = 1.0f / (float)vf;
            int64_t tgt = labels[n];
            float nll = 0.f, loss = 0.f;
            bool all_ok = true;
            for (int f = 0; f < nfac; ++f) {
                const int tf = (int)(tgt % vf);
                tgt /= vf;
                float* lf = lp + f * vf;
                float v[REG ? 8 : 1];
                FactorLse s{-INFINITY, 0.f, 0.f, 0};
                if constexpr (REG) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int k = lane + 64 * j;
                        v[j] = k < vf ? lf[k] : -INFINITY;
                        if (k < vf) s.sz += v[j];
                        if (v[j] > s.mx) { s.mx = v[j]; s.mi = k; }
                    }
                    wave_argmax(s.mx, s.mi);
                } else {
                    s = factor_lse<true>(lf, vf, lane);
                }
                const float zy = lf[tf];   // read before any lane stores into the row
                if constexpr (REG) {
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (lane + 64 * j < vf) { v[j] = expf(v[j] - s.mx); s.se += v[j]; }
                    s.se = wave_sum(s.se);
                }
                const float lse = logf(s.se) + s.mx;
                const float nll_f = lse - zy;
                nll += nll_f;
                all_ok = all_ok && (s.mi == tf);
                if (!live) {
                    for (int k = lane; k < vf; k += 64) lf[k] = 0.f;
                    continue;
                }
                const float sz = wave_sum(s.sz);
                loss += ((1.0f - eps) * nll_f + eps * (lse - sz * inv_vf)) + zeta * (lse * lse);
                const float inv = 1.0f / s.se, fac = 1.0f + (2.0f * zeta) * lse;
                if constexpr (REG) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int k = lane + 64 * j;
                        if (k < vf) lf[k] = ((v[j] * inv) * fac - (k == tf ? q_on : q_off)) * wgt;
                    }
                } else {
                    for (int k = lane; k < vf; k += 64) {
                        const float p = expf(lf[k] - s.mx) * inv;
                        lf[k] = (p * fac - (k == tf ? q_on : q_off)) * wgt;
                    }
                }
            }
            if (lane == 0) { obj = (double)wt * (double)loss; hit = all_ok ? 1.0 : 0.0; ce = nll; }
        }
    }
    block_add_sums<false, 0, 1, 3>(sums, obj, hit, ce);
}
static FrameWeights frame_weights_of(const genie_objective& obj) {
    FrameWeights fw;
    fw.n = obj.n_frames;
    for (int t = 0; t < 64; ++t) fw.w[t] = t < obj.n_frames ? obj.frame_weight[t] : 1.0f;
    return fw;
}
static int launch_count_frames(const int64_t* ids, long n_clips, int T, int S, int64_t mask_id, const FrameWeights& fw, double* sums,
                               hipStream_t st) {
    ProfScope prof(GENIE_KC_OTHER, 0.0, 8.0 * n_clips * T * S, st, "count_frames_kernel");
    count_frames_kernel<<<1, 1024, 0, st>>>(ids, n_clips, T, S, mask_id, fw, sums);
    GENIE_LAUNCH_CHECK("count_frames");
    return GENIE_OK;
}
int launch_ce_objective(float* logits, const int64_t* ids, const int64_t* labels, long n_clips, int T, int S, int vf, int nfac,
                        int64_t mask_id, const genie_objective& obj, double* sums, hipStream_t st) {
    const long n_tok = n_clips * T * (long)S;
    if (n_tok <= 0) return GENIE_OK;
    const FrameWeights fw = frame_weights_of(obj);
    const double row_bytes = 8.0 * n_tok * vf * nfac;
    GENIE_TRY(launch_count_frames(ids, n_clips, T, S, mask_id, fw, sums, st));
    ProfScope prof(GENIE_KC_OTHER, 0.0, row_bytes, st, "ce_objective_kernel");
    const unsigned grid = (unsigned)((n_tok + 3) / 4);
    if (vf <= 512)
        ce_objective_kernel<true><<<grid, 256, 0, st>>>(logits, ids, labels, n_tok, T, S, vf, nfac, mask_id, obj.label_smoothing,
                                                        obj.z_loss, fw, sums);
    else
        ce_objective_kernel<false><<<grid, 256, 0, st>>>(logits, ids, labels, n_tok, T, S, vf, nfac, mask_id, obj.label_smoothing,
                                                         obj.z_loss, fw, sums);
    GENIE_LAUNCH_CHECK("ce_objective");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// Distillation.  The mapping is ce_objective_kernel's -- but a launch has at most DISTILL_MAX_GRID workgroups, each walking its share
// of the four-token groups and adding its sums up in registers.
// REG (vf <= 512): a factor's eight student and eight teacher values per lane are requested together, before the first use of either,
// and stay in registers: each row comes from memory once, 12 bytes per logit element (student read + write, teacher read).  Else three
// streaming passes (extrema; sums; elements), the teacher row riding in each -- which is why they are not factor_lse: the shared step
// would branch on its caller, and the kernel sits on a tested register budget.  TAU1 (tau == 1): pt = p and the teacher's tempered
// sum is its plain one, so the second exponential of both rows is never computed.
// log r_k and log pt_k are taken in log-softmax form, (u_k - max u) / tau - log sum: a probability that underflowed to 0 multiplies a
// finite number.
// ------------------------------------------------------------------------------------------------
// a value every lane holds alike, moved to a scalar register: the per-token and per-factor constants (a wave is one token) otherwise
// take a vector register each (compiled without it: 104 / 117 / 71 / 79 VGPRs against 102 / 114 / 64 / 71, one wave per SIMD less in
// the streaming kernel at any tau)
__device__ __forceinline__ float uni(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

template <bool REG, bool TAU1>
__global__ __launch_bounds__(256) void ce_distill_kernel(float* __restrict__ logits, const float* __restrict__ teacher,
                                                         const int64_t* __restrict__ ids, const int64_t* __restrict__ labels,
                                                         long n_tok, int T, int S, int vf, int nfac, int64_t mask_id, float eps,
                                                         float zeta, float alpha, float tau, FrameWeights fw,
                                                         double* __restrict__ sums) {
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double obj = 0, hit = 0, ce = 0, kd = 0, tce = 0;
    // a workgroup walks the groups of four tokens blockIdx.x, blockIdx.x + gridDim.x, ... and adds its sums up in registers: the five
    // double atomics at its end all land in one cache line, and with one set per FOUR-token group (the objective kernel's grid) this body
    // took 2.7 times as long at 32,768 tokens (profiles/train_distill.txt)
    for (long n = (long)blockIdx.x * 4 + wid; n < n_tok; n += (long)gridDim.x * 4) {
        float* lp = logits + (size_t)n * vf * nfac;
        const float* tp = teacher + (size_t)n * vf * nfac;
        int t;
        if (token_counted(lp, ids, n, T, S, mask_id, vf * nfac, lane, t)) {
            const float wt = fw.at(t);
            const bool live = wt > 0.0f;   // a zero-weight frame: counted in hits, plain nll, kd and teacher nll; a zero row
            const float wgt = uni(live ? (float)((double)wt / sums[2]) : 0.0f);
            const float q_off = uni(eps / (float)vf), q_on = uni((1.0f - eps) + q_off), inv_vf = uni(1.0f / (float)vf);
            const float oma = uni(1.0f - alpha), at = uni(alpha * tau), inv_tau = uni(1.0f / tau);
            int64_t tgt = labels[n];
            float nll = 0.f, loss = 0.f, kdt = 0.f, tnll = 0.f;
            bool all_ok = true;
            for (int f = 0; f < nfac; ++f) {
                const int tf = (int)(tgt % vf);
                tgt /= vf;
                float* lf = lp + f * vf;
                const float* uf = tp + f * vf;
                // d: z - max, then (TAU1: the same) (z - max) / tau;  e: exp(z - max);  et: exp((z - max) / tau)
                // c: (u - max u) / tau, then c - d;  ru: exp((u - max u) / tau)
                float d[REG ? 8 : 1], e[REG ? 8 : 1], et[(REG && !TAU1) ? 8 : 1], c[REG ? 8 : 1], ru[REG ? 8 : 1];
                float mx = -INFINITY, mu = -INFINITY, sz = 0.f;
                int mi = 0;
                if (REG) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {   // sixteen requests in flight before the first use
                        const int k = lane + 64 * j;
                        d[j] = k < vf ? lf[k] : -INFINITY;
                        c[j] = k < vf ? uf[k] : -INFINITY;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int k = lane + 64 * j;
                        if (k < vf) sz += d[j];
                        if (d[j] > mx) { mx = d[j]; mi = k; }
                        mu = fmaxf(mu, c[j]);
                    }
                } else {
                    for (int k = lane; k < vf; k += 64) {
                        const float x = lf[k];
                        sz += x;
                        if (x > mx) { mx = x; mi = k; }
                        mu = fmaxf(mu, uf[k]);
                    }
                }
                wave_argmax(mx, mi);
                mx = uni(mx);
                mi = __builtin_amdgcn_readfirstlane(mi);
                mu = uni(wave_max(mu));
                const float zy = uni(lf[tf]), uy = uni(uf[tf]);   // z_y is read before any lane stores into the row
                float se = 0.f, st = 0.f, su = 0.f, su1 = 0.f;
                if (REG) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (lane + 64 * j < vf) {
                            d[j] -= mx;
                            e[j] = expf(d[j]);
                            se += e[j];
                            c[j] -= mu;
                            if (!TAU1) {
                                su1 += expf(c[j]);
                                d[j] *= inv_tau;
                                c[j] *= inv_tau;
                                et[j] = expf(d[j]);
                                st += et[j];
                            }
                            ru[j] = expf(c[j]);
                            su += ru[j];
                            c[j] -= d[j];   // the KL term needs the difference alone
                        }
                    }
                } else {
                    for (int k = lane; k < vf; k += 64) {
                        const float dz = lf[k] - mx, du = uf[k] - mu;
                        se += expf(dz);
                        if (!TAU1) {
                            su1 += expf(du);
                            st += expf(dz * inv_tau);
                            su += expf(du * inv_tau);
                        } else {
                            su += expf(du);
                        }
                    }
                }
                se = uni(wave_sum(se));
                su = uni(wave_sum(su));
                if (!TAU1) { st = uni(wave_sum(st)); su1 = uni(wave_sum(su1)); }
                sz = uni(wave_sum(sz));
                const float log_se = uni(logf(se)), log_su = uni(logf(su));
                const float log_st = TAU1 ? log_se : uni(logf(st));
                const float lse = uni(log_se + mx);
                const float nll_f = lse - zy;
                nll += nll_f;
                tnll += ((TAU1 ? log_su : logf(su1)) + mu) - uy;
                all_ok = all_ok && (mi == tf);
                const float inv = uni(1.0f / se), inv_st = TAU1 ? inv : uni(1.0f / st), inv_su = uni(1.0f / su),
                            zl2 = uni((2.0f * zeta) * lse), dlog = uni(log_su - log_st);
                float kl = 0.f;
                if (REG) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int k = lane + 64 * j;
                        if (k < vf) {
                            const float p = e[j] * inv, pt = TAU1 ? p : et[j] * inv_st, r = ru[j] * inv_su;
                            kl += r * (c[j] - dlog);
                            const float g = (oma * (p - (k == tf ? q_on : q_off)) + zl2 * p) + at * (pt - r);
                            lf[k] = live ? g * wgt : 0.f;
                        }
                    }
                } else {
                    for (int k = lane; k < vf; k += 64) {
                        const float dz = lf[k] - mx, du = uf[k] - mu;
                        const float p = expf(dz) * inv;
                        const float dzt = TAU1 ? dz : dz * inv_tau, dut = TAU1 ? du : du * inv_tau;
                        const float pt = TAU1 ? p : expf(dzt) * inv_st, r = expf(dut) * inv_su;
                        kl += r * ((dut - dzt) - dlog);
                        const float g = (oma * (p - (k == tf ? q_on : q_off)) + zl2 * p) + at * (pt - r);
                        lf[k] = live ? g * wgt : 0.f;
                    }
                }
                const float kd_f = uni((tau * tau) * wave_sum(kl));
                kdt += kd_f;
                const float hard_f = (1.0f - eps) * nll_f + eps * (lse - sz * inv_vf);
                loss += (oma * hard_f + alpha * kd_f) + zeta * (lse * lse);
            }
            if (lane == 0) {
                obj += (double)wt * (double)loss;
                hit += all_ok ? 1.0 : 0.0;
                ce += nll;
                kd += kdt;
                tce += tnll;
            }
        }
    }
    block_add_sums<false, 0, 1, 3, 5, 6>(sums, obj, hit, ce, kd, tce);
}

// workgroups of a launch at most: eight per CU of a 256-CU device, each walking its share of the token groups
constexpr long DISTILL_MAX_GRID = 2048;

int launch_ce_distill(float* logits, const float* teacher, const int64_t* ids, const int64_t* labels, long n_clips, int T, int S,
                      int vf, int nfac, int64_t mask_id, const genie_objective& obj, float alpha, float tau, double* sums,
                      hipStream_t st) {
    const long n_tok = n_clips * T * (long)S;
    if (n_tok <= 0) return GENIE_OK;
    const FrameWeights fw = frame_weights_of(obj);
    GENIE_TRY(launch_count_frames(ids, n_clips, T, S, mask_id, fw, sums, st));
    // (an upper bound, as the objective kernel's 8: the host does not know how many tokens are counted, and an uncounted token's row is
    // only written -- 4 bytes per element, not 12)
    ProfScope prof(GENIE_KC_OTHER, 0.0, 12.0 * n_tok * vf * nfac, st, "ce_distill_kernel");
    const unsigned grid = (unsigned)std::min<long>((n_tok + 3) / 4, DISTILL_MAX_GRID);
#define GENIE_DISTILL_LAUNCH(REG, TAU1)                                                                                         \
    ce_distill_kernel<REG, TAU1><<<grid, 256, 0, st>>>(logits, teacher, ids, labels, n_tok, T, S, vf, nfac, mask_id,            \
                                                       obj.label_smoothing, obj.z_loss, alpha, tau, fw, sums)
    if (vf <= 512) {
        if (tau == 1.0f) GENIE_DISTILL_LAUNCH(true, true);
        else GENIE_DISTILL_LAUNCH(true, false);
    } else {
        if (tau == 1.0f) GENIE_DISTILL_LAUNCH(false, true);
        else GENIE_DISTILL_LAUNCH(false, false);
    }
#undef GENIE_DISTILL_LAUNCH
    GENIE_LAUNCH_CHECK("ce_distill");
    return GENIE_OK;
}

// ------------------------------------------------------------------------------------------------
// The loss launch of a training call, for all three losses: zero the 3 / 5 / 7 sums, then the count kernel and the loss kernel of
//   ds (non-neutral distillation, `teacher` its rows): launch_ce_distill;  else obj (a struct, neutral or not): launch_ce_objective;
//   else the neutral step's pair.  `fn` names the entry point in a failed memset's message.  Arguments were checked by the caller.
// ------------------------------------------------------------------------------------------------
int launch_train_loss(const char* fn, float* logits, const int64_t* ids, const int64_t* labels, long n_clips, int T, int S, int vf,
                      int nfac, int64_t mask_id, const genie_objective* obj, const genie_distill* ds, const float* teacher, double* sums,
                      hipStream_t st) {
    if (hipMemsetAsync(sums, 0, (ds ? 7 : obj ? 5 : 3) * sizeof(double), st) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", fn);
        return GENIE_E_LAUNCH;
    }
    if (ds) {
        static const genie_objective neutral = {};   // eps = zeta = 0, n_frames = 0: every frame weighs 1
        return launch_ce_distill(logits, teacher, ids, labels, n_clips, T, S, vf, nfac, mask_id, obj ? *obj : neutral, ds->alpha,
                                 ds->temperature, sums, st);
    }
    if (obj) return launch_ce_objective(logits, ids, labels, n_clips, T, S, vf, nfac, mask_id, *obj, sums, st);
    genie_cfg c{};   // the neutral step's launcher takes its geometry from a genie_cfg (mask_id fits: checked by the caller)
    c.T = T; c.S = S; c.factored_vocab = vf; c.num_factored = nfac; c.image_vocab_size = (int32_t)mask_id;
    return launch_ce_fwd_bwd(c, logits, ids, labels, (int)n_clips, sums, st);
}

}  // namespace genie
