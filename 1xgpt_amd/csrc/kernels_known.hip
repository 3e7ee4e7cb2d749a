// Inpainting (include/genie_hip.h, "known tokens"): the two launches a MaskGIT decode needs when some tokens of the frame are given.
//   * known_begin_kernel lays a frame's start state: the known token where there is one, the mask id elsewhere, into every copy of the
//     clip's row (rows b and b + B under guidance), and the (B, S) `unmasked` flags.  One launch where the all-mask start takes a fill
//     and a memset; with unmasked == NULL and the destination strides of the two-frame buffer it lays the second frame of a merged commit.
//   * mask_step_known_kernel is mask_step_kernel (kernels_exact.hip) with a re-mask count of its own per clip: the block counts the
//     clip's known tokens K_b from its `known` row (per-thread counts, a wave reduction, LDS across the waves), and
//     n_b = ceil(frac * (S - K_b)) in double from the host's `frac`: one IEEE multiply and a ceil, so host and device agree bit for bit.
//     The row is read again every step (8 S bytes per clip) rather than kept: the loops' workspace holds no new buffer.
// A token is known when 0 <= known[b][s] < mask_id.  Both kernels are plain C++: no scratch, no inline assembly.
#include "kernels.hpp"

namespace genie {

__device__ __forceinline__ bool is_known(int64_t v, int64_t mask_id) { return v >= 0 && v < mask_id; }

__global__ __launch_bounds__(256) void known_begin_kernel(const int64_t* __restrict__ known, long known_stride, int64_t mask_id,
                                                          int64_t* __restrict__ frame, long frame_stride, uint8_t* __restrict__ unmasked,
                                                          int B, int S, int copies) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * S) return;
    const long b = i / S, s = i - b * S;
    const int64_t v = known[b * known_stride + s];
    const bool k = is_known(v, mask_id);
    for (int r = 0; r < copies; ++r) frame[((long)r * B + b) * frame_stride + s] = k ? v : mask_id;
    if (unmasked) unmasked[i] = k ? 1 : 0;
}

int launch_known_begin(const int64_t* known, long known_stride, int64_t mask_id, int64_t* frame, long frame_stride, uint8_t* unmasked, int B,
                       int S, int copies, hipStream_t st) {
    known_begin_kernel<<<(unsigned)(((long)B * S + 255) / 256), 256, 0, st>>>(known, known_stride, mask_id, frame, frame_stride, unmasked, B, S,
                                                                              copies);
    GENIE_LAUNCH_CHECK("known_begin");
    return GENIE_OK;
}

// One block per clip, S keys in LDS, stable rank by count: rank_i = #{j : key_j < key_i or (key_j == key_i and j < i)}; rank < n_b ->
// re-mask, else unmasked.  Already-unmasked tokens (the known ones from the start) carry key +inf and keep the frame's value.
__global__ __launch_bounds__(256) void mask_step_known_kernel(const float* __restrict__ keys, double frac, int last_step, int64_t mask_id,
                                                              const int64_t* __restrict__ known, long known_stride,
                                                              uint8_t* __restrict__ unmasked, int64_t* __restrict__ samples,
                                                              int64_t* __restrict__ prompt_frame, long clip_stride, int S) {
    extern __shared__ float skey[];
    __shared__ int wave_known[4];
    const int b = blockIdx.x;
    uint8_t* um = unmasked + (size_t)b * S;
    int64_t* sm = samples + (size_t)b * S;
    int64_t* pf = prompt_frame + (size_t)b * clip_stride;
    int n = 0;
    if (!last_step) {
        int cnt = 0;
        if (known) {
            const int64_t* kn = known + (size_t)b * known_stride;
            for (int i = threadIdx.x; i < S; i += blockDim.x) cnt += is_known(kn[i], mask_id) ? 1 : 0;
        }
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
        if ((threadIdx.x & 63) == 0) wave_known[threadIdx.x >> 6] = cnt;
    }
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        float k = 0.f;
        if (!last_step) k = um[i] ? INFINITY : keys[(size_t)b * S + i];
        skey[i] = k;
    }
    __syncthreads();
    if (!last_step) {
        int K = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) K += wave_known[w];
        n = (int)ceil(frac * (double)(S - K));
    }
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        const bool prev = um[i] != 0;
        int64_t v = sm[i];
        if (!last_step) {
            const float ki = skey[i];
            int rank = 0;
            for (int j = 0; j < S; ++j) {
                const float kj = skey[j];
                rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
            }
            if (rank < n) v = mask_id; else um[i] = 1;
        }
        if (prev) v = pf[i];
        sm[i] = v;
        pf[i] = v;
    }
}

int launch_mask_step_known(const float* keys, double frac, int last_step, int64_t mask_id, const int64_t* known, long known_stride,
                           uint8_t* unmasked, int64_t* samples, int64_t* prompt_frame, long clip_stride, int B, int S, hipStream_t st) {
    GENIE_CHECK_SHAPE(S <= 8192, "mask_step_known: S=%d too large", S);
    const int threads = S >= 256 ? 256 : ((S + 63) / 64) * 64;
    mask_step_known_kernel<<<B, threads, S * sizeof(float), st>>>(keys, frac, last_step, mask_id, known, known_stride, unmasked, samples,
                                                                   prompt_frame, clip_stride, S);
    GENIE_LAUNCH_CHECK("mask_step_known");
    return GENIE_OK;
}

}  // namespace genie
