// LoRA adapters (include/genie_hip.h, "LoRA adapters"): the effective weight W = W0 + s B A of an adapted Linear, and the projection
// of the step's own dW onto the adapters, dA = s B^T dW and dB = s dW A^T.  f32 FMA, no MFMA: both kernels move the (out, in) matrix
// once and spend 2 r flops (merge) or 4 r flops (project) on each of its elements.
//   * One launch serves a table of up to 8 Linears, passed by value; a workgroup finds its item and its 64 x 64 tile of the matrix
//     from the table's running tile counts.
//   * No cross-thread sum anywhere: in the merge a thread owns a 4 x 4 patch of the tile; in the projection the tile of dW is staged
//     in LDS once and read twice, by threads that own (k, column) outputs of the dA partial and then (row, k) outputs of the dB
//     partial, each walking its 64 terms in ascending order.
//   * A tile's partials go to slabs (dA: one per row tile, dB: one per column tile); lora_reduce_kernel adds the slabs of an element
//     in a fixed order, applies s and the accumulate flag.  No atomics: the same bytes run to run, and every slab element that is
//     read has been written by the launch before it (poisoned scratch changes nothing).
#include "kernels.hpp"

namespace genie {

constexpr int LT = 64;   // tile edge

__device__ __forceinline__ int lora_find(const int* first, int n, int block) {
    int e = 0;
    while (e + 1 < n && block >= first[e + 1]) ++e;
    return e;
}

// w[i,j] = w0[i,j] + s * sum_k b[i,k] a[k,j], k ascending, one fma per term and one for s; w may be w0 (each element is read and
// written by the same thread)
__global__ __launch_bounds__(256) void lora_merge_kernel(const LoraTable tb) {
    __shared__ float As[LORA_MAX_RANK][LT];       // [k][column]
    __shared__ float Bt[LORA_MAX_RANK][LT + 4];   // [k][row]
    const int e = lora_find(tb.first, tb.n, blockIdx.x);
    const int out = tb.it[e].out, in = tb.it[e].in, r = tb.it[e].rank;
    const float s = tb.it[e].scale;
    const float* a = tb.it[e].a;
    const float* b = tb.it[e].b;
    const float* w0 = tb.it[e].w0;
    float* w = tb.it[e].w;
    const int nct = (in + LT - 1) / LT, tile = blockIdx.x - tb.first[e];
    const int row0 = (tile / nct) * LT, col0 = (tile % nct) * LT, tid = threadIdx.x;
    for (int idx = tid; idx < r * (LT / 4); idx += 256) {
        const int k = idx / (LT / 4), c = (idx % (LT / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col0 + c < in) v = *reinterpret_cast<const float4*>(a + (size_t)k * in + col0 + c);
        *reinterpret_cast<float4*>(&As[k][c]) = v;
    }
    for (int idx = tid; idx < LT * r; idx += 256) {   // the tile's rows of b are one contiguous run
        const int i = idx / r, k = idx % r;
        Bt[k][i] = row0 + i < out ? b[(size_t)(row0 + i) * r + k] : 0.f;
    }
    __syncthreads();
    const int c = (tid & 15) * 4, i0 = (tid >> 4) * 4;
    float4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < r; ++k) {
        const float4 a4 = *reinterpret_cast<const float4*>(&As[k][c]);
        const float4 b4 = *reinterpret_cast<const float4*>(&Bt[k][i0]);
        const float bq[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc[q].x = fmaf(bq[q], a4.x, acc[q].x);
            acc[q].y = fmaf(bq[q], a4.y, acc[q].y);
            acc[q].z = fmaf(bq[q], a4.z, acc[q].z);
            acc[q].w = fmaf(bq[q], a4.w, acc[q].w);
        }
    }
    if (col0 + c >= in) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = row0 + i0 + q;
        if (i >= out) break;
        const size_t at = (size_t)i * in + col0 + c;
        float4 v = *reinterpret_cast<const float4*>(w0 + at);
        v.x = fmaf(s, acc[q].x, v.x);
        v.y = fmaf(s, acc[q].y, v.y);
        v.z = fmaf(s, acc[q].z, v.z);
        v.w = fmaf(s, acc[q].w, v.w);
        *reinterpret_cast<float4*>(w + at) = v;
    }
}

// One 64 x 64 tile of dw -> its dA partial (r, 64 columns) into the row tile's slab and its dB partial (64 rows, r) into the column
// tile's slab.  KP ranks per thread: wave g of the four owns ranks g KP .. g KP + KP - 1 (zero operands beyond r), so the b / a
// operand of an fma is the same LDS word in all 64 lanes (a broadcast) and the dw operand a conflict-free column or padded row.
template <int KP>
__global__ __launch_bounds__(256) void lora_project_kernel(const LoraTable tb) {
    constexpr int K4 = KP * 4;
    __shared__ float Ds[LT][LT + 1];   // [row][column] of dw
    __shared__ float Bs[LT][K4];       // [row][k]
    __shared__ float As[LT][K4];       // [column][k]
    const int e = lora_find(tb.first, tb.n, blockIdx.x);
    const int out = tb.it[e].out, in = tb.it[e].in, r = tb.it[e].rank;
    const float* a = tb.it[e].a;
    const float* b = tb.it[e].b;
    const float* dw = tb.it[e].dw;
    const int nct = (in + LT - 1) / LT, tile = blockIdx.x - tb.first[e];
    const int ti = tile / nct, tj = tile % nct, row0 = ti * LT, col0 = tj * LT, tid = threadIdx.x;
    for (int idx = tid; idx < LT * (LT / 4); idx += 256) {
        const int i = idx / (LT / 4), c = (idx % (LT / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + i < out && col0 + c < in) v = *reinterpret_cast<const float4*>(dw + (size_t)(row0 + i) * in + col0 + c);
        Ds[i][c] = v.x; Ds[i][c + 1] = v.y; Ds[i][c + 2] = v.z; Ds[i][c + 3] = v.w;
    }
    for (int idx = tid; idx < LT * K4; idx += 256) {
        const int i = idx / K4, k = idx % K4;
        Bs[i][k] = (row0 + i < out && k < r) ? b[(size_t)(row0 + i) * r + k] : 0.f;
    }
    for (int idx = tid; idx < K4 * LT; idx += 256) {
        const int k = idx / LT, j = idx % LT;
        As[j][k] = (k < r && col0 + j < in) ? a[(size_t)k * in + col0 + j] : 0.f;
    }
    __syncthreads();
    const int lane = tid & 63, k0 = (tid >> 6) * KP;
    float acc[KP];
    // dA partial: (k, column = lane) = sum over the tile's rows, ascending
#pragma unroll
    for (int u = 0; u < KP; ++u) acc[u] = 0.f;
#pragma unroll 4
    for (int i = 0; i < LT; ++i) {
        const float d = Ds[i][lane];
#pragma unroll
        for (int u = 0; u < KP; ++u) acc[u] = fmaf(Bs[i][k0 + u], d, acc[u]);
    }
    if (col0 + lane < in) {
        float* slab = tb.scratch + tb.da_off[e] + (size_t)ti * r * in;
#pragma unroll
        for (int u = 0; u < KP; ++u)
            if (k0 + u < r) slab[(size_t)(k0 + u) * in + col0 + lane] = acc[u];
    }
    // dB partial: (row = lane, k) = sum over the tile's columns, ascending
#pragma unroll
    for (int u = 0; u < KP; ++u) acc[u] = 0.f;
#pragma unroll 4
    for (int j = 0; j < LT; ++j) {
        const float d = Ds[lane][j];
#pragma unroll
        for (int u = 0; u < KP; ++u) acc[u] = fmaf(As[j][k0 + u], d, acc[u]);
    }
    if (row0 + lane < out) {
        float* slab = tb.scratch + tb.db_off[e] + (size_t)tj * out * r;
#pragma unroll
        for (int u = 0; u < KP; ++u)
            if (k0 + u < r) slab[(size_t)(row0 + lane) * r + k0 + u] = acc[u];
    }
}

// out[i] = (accumulate ? out[i] : 0) + s * sum_{t < ns} part[t n + i]: four chains over slabs t = 0, 4, 8, .. / 1, 5, .. / .., added
// (0 + 1) + (2 + 3).  Segment 2 e is item e's dA, 2 e + 1 its dB.
__global__ __launch_bounds__(256) void lora_reduce_kernel(const LoraTable tb, int accumulate) {
    const int g = lora_find(tb.rfirst, 2 * tb.n, blockIdx.x), e = g >> 1;
    const int out = tb.it[e].out, in = tb.it[e].in, r = tb.it[e].rank;
    const bool is_b = g & 1;
    const size_t n = is_b ? (size_t)out * r : (size_t)r * in;
    const int ns = is_b ? (in + LT - 1) / LT : (out + LT - 1) / LT;
    const float* part = tb.scratch + (is_b ? tb.db_off[e] : tb.da_off[e]);
    float* dst = is_b ? tb.it[e].db : tb.it[e].da;
    const size_t i = (size_t)(blockIdx.x - tb.rfirst[g]) * 256 + threadIdx.x;
    if (i >= n) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int t = 0;
    for (; t + 3 < ns; t += 4) {
        s0 += part[(size_t)t * n + i];
        s1 += part[(size_t)(t + 1) * n + i];
        s2 += part[(size_t)(t + 2) * n + i];
        s3 += part[(size_t)(t + 3) * n + i];
    }
    for (; t < ns; ++t) s0 += part[(size_t)t * n + i];
    const float sum = (s0 + s1) + (s2 + s3);
    dst[i] = fmaf(tb.it[e].scale, sum, accumulate ? dst[i] : 0.f);
}

static long lora_tiles(const genie_lora_item& it) { return (long)((it.out + LT - 1) / LT) * ((it.in + LT - 1) / LT); }

// The table of a launch.  Slabs of item e: dA partials (row tiles, rank, in) at da_off, dB partials (column tiles, out, rank) at db_off,
// each run rounded up to 64 floats.  Returns the floats of scratch the projection needs; false when a count leaves int32.
bool lora_table(const genie_lora_item* items, int n, LoraTable& tb, size_t& scratch_floats) {
    long tiles = 0, blocks = 0;
    size_t off = 0;
    tb.n = n;
    for (int e = 0; e < n; ++e) {
        const genie_lora_item& it = items[e];
        tb.it[e] = it;
        tb.first[e] = (int)tiles;
        tiles += lora_tiles(it);
        const size_t na = (size_t)it.rank * it.in, nb = (size_t)it.out * it.rank;
        tb.rfirst[2 * e] = (int)blocks;
        blocks += (long)((na + 255) / 256);
        tb.rfirst[2 * e + 1] = (int)blocks;
        blocks += (long)((nb + 255) / 256);
        tb.da_off[e] = off;
        off += align_up((size_t)((it.out + LT - 1) / LT) * na, 64);
        tb.db_off[e] = off;
        off += align_up((size_t)((it.in + LT - 1) / LT) * nb, 64);
        if (tiles > INT32_MAX || blocks > INT32_MAX) return false;
    }
    tb.first[n] = (int)tiles;
    tb.rfirst[2 * n] = (int)blocks;
    tb.scratch = nullptr;
    scratch_floats = off;
    return true;
}

int launch_lora_merge(const LoraTable& tb, hipStream_t st) {
    lora_merge_kernel<<<(unsigned)tb.first[tb.n], 256, 0, st>>>(tb);
    GENIE_LAUNCH_CHECK("lora_merge");
    return GENIE_OK;
}

int launch_lora_project(const LoraTable& tb, int accumulate, hipStream_t st) {
    int rmax = 1;
    for (int e = 0; e < tb.n; ++e) rmax = tb.it[e].rank > rmax ? tb.it[e].rank : rmax;
    const unsigned grid = (unsigned)tb.first[tb.n];
    if (rmax <= 4) lora_project_kernel<1><<<grid, 256, 0, st>>>(tb);
    else if (rmax <= 8) lora_project_kernel<2><<<grid, 256, 0, st>>>(tb);
    else if (rmax <= 16) lora_project_kernel<4><<<grid, 256, 0, st>>>(tb);
    else if (rmax <= 32) lora_project_kernel<8><<<grid, 256, 0, st>>>(tb);
    else lora_project_kernel<16><<<grid, 256, 0, st>>>(tb);
    GENIE_LAUNCH_CHECK("lora_project");
    lora_reduce_kernel<<<(unsigned)tb.rfirst[2 * tb.n], 256, 0, st>>>(tb, accumulate);
    GENIE_LAUNCH_CHECK("lora_reduce");
    return GENIE_OK;
}

}  // namespace genie
