// Continuous per-frame actions (genie_action_proj in include/genie_hip.h, which states the arithmetic): the projection of a call's
// action vectors (n, A) into the row table (n, d_model) that genie_frame_cond addresses, and the gradients of that projection from
// d loss / d rows.  A is small (tens) and n is a few hundred rows at most, so both kernels are latency-bound: plain f32 loads and
// stores, 64-bit indexing, every operation rounded on its own (__fsub_rn / __fmul_rn / __fadd_rn) so that NumPy f32 restates them.
#include "common.hpp"
#include "kernels.hpp"

namespace genie {

// z_j = (a_j - mean_j) * inv_std_j; a NULL mean / inv_std skips its operation
__device__ __forceinline__ float action_z(float a, const float* mean, const float* inv_std, int j) {
    if (mean) a = __fsub_rn(a, mean[j]);
    if (inv_std) a = __fmul_rn(a, inv_std[j]);
    return a;
}

// One block per (row, chunk of blockDim.x channels): the row's A normalised inputs are staged once in LDS and shared by its channels,
// then thread c walks j = 0 .. A-1 ascending.  blockIdx.x = row * chunks + chunk.
__global__ __launch_bounds__(256) void action_rows_kernel(const float* __restrict__ W, const float* __restrict__ bias,
                                                          const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                          const float* __restrict__ vecs, float* __restrict__ rows, int A, int d,
                                                          int chunks) {
    __shared__ float z[GENIE_ACTION_MAX_DIM];
    const long row = (long)blockIdx.x / chunks;
    const int c = (int)((long)blockIdx.x - row * chunks) * (int)blockDim.x + (int)threadIdx.x;
    for (int j = threadIdx.x; j < A; j += blockDim.x) z[j] = action_z(vecs[row * A + j], mean, inv_std, j);
    __syncthreads();
    if (c >= d) return;
    const float* w = W + (long)c * A;
    float acc = bias ? bias[c] : 0.0f;
    for (int j = 0; j < A; ++j) acc = __fadd_rn(acc, __fmul_rn(w[j], z[j]));
    rows[row * d + c] = acc;
}

// Thread (c, j): d_weight[c, j] = sum over n ascending of d_rows[n, c] * z[n, j]; j == A is the bias column, sum of d_rows[n, c].
// Adjacent lanes hold adjacent channels (coalesced d_rows reads); z[n, j] is one address per wave.  Strictly sequential in n.
__global__ __launch_bounds__(64) void action_rows_bwd_kernel(const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                             const float* __restrict__ vecs, const float* __restrict__ d_rows,
                                                             long n, int A, int d, float* __restrict__ d_weight,
                                                             float* __restrict__ d_bias, int accumulate) {
    const int c = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x;
    const int j = (int)blockIdx.y;
    if (c >= d) return;
    float acc = 0.0f;
    if (j == A) {
        for (long r = 0; r < n; ++r) acc = __fadd_rn(acc, d_rows[r * d + c]);
        d_bias[c] = accumulate ? __fadd_rn(d_bias[c], acc) : acc;
    } else {
        for (long r = 0; r < n; ++r)
            acc = __fadd_rn(acc, __fmul_rn(d_rows[r * d + c], action_z(vecs[r * A + j], mean, inv_std, j)));
        float* o = d_weight + (long)c * A + j;
        *o = accumulate ? __fadd_rn(*o, acc) : acc;
    }
}

int launch_action_rows(const genie_action_proj& p, const float* vecs, float* rows, long n, int d, hipStream_t st) {
    if (n <= 0) return GENIE_OK;
    const int block = d >= 256 ? 256 : (d + 63) / 64 * 64;
    const int chunks = (d + block - 1) / block;
    GENIE_CHECK_ARG(n <= 0x7fffffffL / chunks, "action_rows: n = %ld rows of %d channels exceed one launch", n, d);
    action_rows_kernel<<<(unsigned)(n * chunks), block, 0, st>>>(p.weight, p.bias, p.mean, p.inv_std, vecs, rows, p.action_dim, d, chunks);
    GENIE_LAUNCH_CHECK("action_rows");
    return GENIE_OK;
}

int launch_action_rows_backward(const genie_action_proj& p, const float* vecs, const float* d_rows, long n, int d, float* d_weight,
                                float* d_bias, int accumulate, hipStream_t st) {
    const int A = p.action_dim;
    action_rows_bwd_kernel<<<dim3((unsigned)((d + 63) / 64), (unsigned)(A + (d_bias ? 1 : 0))), 64, 0, st>>>(
        p.mean, p.inv_std, vecs, d_rows, n, A, d, d_weight, d_bias, accumulate);
    GENIE_LAUNCH_CHECK("action_rows_backward");
    return GENIE_OK;
}

}  // namespace genie
