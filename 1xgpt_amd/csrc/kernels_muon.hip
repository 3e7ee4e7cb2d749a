// Muon (include/genie_hip.h, "Muon"): momentum, a Newton-Schulz orthogonalisation of each target matrix's update on the f32 matrix
// cores, and the decayed update with the EMA line.  Everything is f32 (the norm's sum f64) and serves all three training precisions.
//   muon_momentum_kernel   steps 1 to 3 of a whole item table and 64 partial sums of squares per item          1 launch per table
//   muon_normalise_kernel  step 5: adds the 64 partials (ascending) and divides, one more elementwise pass       1 launch per table
//   muon_gemm_kernel       C_i = beta R_i + alpha op(A_i) op(B_i), the item index in blockIdx.y, for all items of one shape:
//                          the 128x128x16 tile of gemm_f32_gen_kernel (train_device.hpp), v_mfma_f32_32x32x2_f32  3 per iteration and shape
//   muon_apply_kernel      steps 8 to 10 of the whole table                                                       1 launch per table
// A tall matrix is addressed transposed inside the products (k-major operand tiles), never transposed in memory.  A = X X^T and
// P = b A + c A A are computed in full: every tile runs the same k-ascending chain on commuting products, so they come out
// bit-symmetric and the tall form may read P[n][k] for P[k][n].  No atomics; nothing reads a workspace byte this call did not write.
#include "train_device.hpp"

namespace genie {

constexpr int MUON_PARTS = 64;   // partial sums of squares (and elementwise workgroups) per item

struct MuonMomItem {
    const float* g;   // gradient (or, MOMENTUM = false, the matrix whose norm is wanted)
    float* mom;       // B
    float* u;         // where u goes (workspace X0)
    unsigned n4;      // rows * cols / 4
};
struct MuonMomTable {
    MuonMomItem it[MUON_MAX_ITEMS];
};
struct MuonNormItem {
    const float* src;
    float* dst;
    unsigned n4;
};
struct MuonNormTable {
    MuonNormItem it[MUON_MAX_ITEMS];
};
struct MuonApplyItem {
    float* w;
    float* ema;       // or NULL
    const float* o;   // the orthogonalised update, (rows, cols)
    unsigned n4;
    float decay, s;   // 1 - lr * wd and lr * adj
};
struct MuonApplyTable {
    MuonApplyItem it[MUON_MAX_ITEMS];
};

// the f64 sum of one workgroup's squares: per thread in walk order, xor-shuffle within the wave, the four waves added 0+1+2+3
__device__ __forceinline__ void muon_block_sum(double s, double* __restrict__ out) {
    __shared__ double red[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = ((red[0] + red[1]) + red[2]) + red[3];
}

// steps 1 to 3 of one element: returns u, updates B
__device__ __forceinline__ float muon_momentum_element(float g, float& b, float coef, float mu, int nesterov) {
    const float gi = g * coef;
    b = mu * b + gi;
    return nesterov ? gi + mu * b : b;
}

template <bool MOMENTUM>
__global__ __launch_bounds__(256) void muon_momentum_kernel(MuonMomTable tb, float mu, int nesterov, float grad_mult,
                                                            const double* __restrict__ sumsq, float max_norm,
                                                            double* __restrict__ part) {
    const MuonMomItem it = tb.it[blockIdx.y];
    const float coef = MOMENTUM ? adamw_coef(grad_mult, sumsq, max_norm) : 1.f;
    double s = 0;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < it.n4; i += MUON_PARTS * 256) {
        float4 u = reinterpret_cast<const float4*>(it.g)[i];
        if constexpr (MOMENTUM) {
            float4 b = reinterpret_cast<const float4*>(it.mom)[i];
            u.x = muon_momentum_element(u.x, b.x, coef, mu, nesterov);
            u.y = muon_momentum_element(u.y, b.y, coef, mu, nesterov);
            u.z = muon_momentum_element(u.z, b.z, coef, mu, nesterov);
            u.w = muon_momentum_element(u.w, b.w, coef, mu, nesterov);
            reinterpret_cast<float4*>(it.mom)[i] = b;
            reinterpret_cast<float4*>(it.u)[i] = u;
        }
        s += (double)u.x * u.x;
        s += (double)u.y * u.y;
        s += (double)u.z * u.z;
        s += (double)u.w * u.w;
    }
    muon_block_sum(s, part + (size_t)blockIdx.y * MUON_PARTS + blockIdx.x);
}

__global__ __launch_bounds__(256) void muon_normalise_kernel(MuonNormTable tb, const double* __restrict__ part, float eps) {
    const MuonNormItem it = tb.it[blockIdx.y];
    double ss = 0;
    for (int j = 0; j < MUON_PARTS; ++j) ss += part[(size_t)blockIdx.y * MUON_PARTS + j];
    const float d = fmaxf((float)sqrt(ss), eps);
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < it.n4; i += MUON_PARTS * 256) {
        float4 x = reinterpret_cast<const float4*>(it.src)[i];
        x.x = x.x / d;
        x.y = x.y / d;
        x.z = x.z / d;
        x.w = x.w / d;
        reinterpret_cast<float4*>(it.dst)[i] = x;
    }
}

__global__ __launch_bounds__(256) void muon_apply_kernel(MuonApplyTable tb, float omd) {
    const MuonApplyItem it = tb.it[blockIdx.y];
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < it.n4; i += MUON_PARTS * 256) {
        float4 w = reinterpret_cast<const float4*>(it.w)[i];
        const float4 o = reinterpret_cast<const float4*>(it.o)[i];
        w.x = w.x * it.decay - it.s * o.x;
        w.y = w.y * it.decay - it.s * o.y;
        w.z = w.z * it.decay - it.s * o.z;
        w.w = w.w * it.decay - it.s * o.w;
        reinterpret_cast<float4*>(it.w)[i] = w;
        if (it.ema) {
            float4 e = reinterpret_cast<const float4*>(it.ema)[i];
            e.x = ema_element(e.x, w.x, omd);
            e.y = ema_element(e.y, w.y, omd);
            e.z = ema_element(e.z, w.z, omd);
            e.w = ema_element(e.w, w.w, omd);
            reinterpret_cast<float4*>(it.ema)[i] = e;
        }
    }
}

// C_i[M,N] = beta * R_i + alpha * sum_k A_i(m,k) B_i(n,k), item i = blockIdx.y, every operand of item i at base + i * stride.
//   TA: A(m,k) = A[k*lda + m] else A[m*lda + k];   TB: B(n,k) = B[k*ldb + n] else B[n*ldb + k];   R NULL: alpha * acc alone.
// M, N multiples of 4 and K of 16 (the entry points demand multiples of 16): loads outside a matrix are replaced by zeros, stores
// outside it are skipped.
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void muon_gemm_kernel(const float* __restrict__ A, long lda, size_t sA, const float* __restrict__ B,
                                                        long ldb, size_t sB, const float* __restrict__ R, float beta,
                                                        float* __restrict__ C, long ldc, size_t sC, int M, int N, int K, float alpha) {
    __shared__ __attribute__((aligned(16))) float sAt[2][GG_TILE];
    __shared__ __attribute__((aligned(16))) float sBt[2][GG_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid >> 1, wn = wid & 1;
    const int r = lane & 31, h = lane >> 5;
    const int n_tiles = (N + GG_BM - 1) / GG_BM;
    const int m0 = (blockIdx.x / n_tiles) * GG_BM, n0 = (blockIdx.x % n_tiles) * GG_BM;
    A += (size_t)blockIdx.y * sA;
    B += (size_t)blockIdx.y * sB;
    C += (size_t)blockIdx.y * sC;
    if (R) R += (size_t)blockIdx.y * sC;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    float4 ra[2], rb[2];
    const int nk = K / GG_BK;
    gg_stage_load<TA, true>(A, lda, m0, M, 0, tid, ra);
    gg_stage_load<TB, true>(B, ldb, n0, N, 0, tid, rb);
    gg_stage_store<TA>(sAt[0], tid, ra);
    gg_stage_store<TB>(sBt[0], tid, rb);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) {
            gg_stage_load<TA, true>(A, lda, m0, M, (kt + 1) * GG_BK, tid, ra);
            gg_stage_load<TB, true>(B, ldb, n0, N, (kt + 1) * GG_BK, tid, rb);
        }
#pragma unroll
        for (int kk = 0; kk < GG_BK / 8; ++kk) {
            float4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = gg_frag<TA>(sAt[buf], wm * 64 + i * 32 + r, kk, h);
                b[i] = gg_frag<TB>(sBt[buf], wn * 64 + i * 32 + r, kk, h);
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
            gg_stage_store<TA>(sAt[buf ^ 1], tid, ra);
            gg_stage_store<TB>(sBt[buf ^ 1], tid, rb);
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
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (row >= M) continue;
                const size_t idx = (size_t)row * ldc + col;
                float v = alpha * acc[i][j][e];
                if (R) v = beta * R[idx] + v;
                C[idx] = v;
            }
        }
}

static int muon_gemm(bool ta, bool tb, const float* A, long lda, size_t sA, const float* B, long ldb, size_t sB, const float* R,
                     float beta, float* C, long ldc, size_t sC, int M, int N, int K, float alpha, int items, hipStream_t st) {
    const int mt = (M + GG_BM - 1) / GG_BM, nt = (N + GG_BM - 1) / GG_BM;
    dim3 grid(mt * nt, items);
    const double mn = (double)M * N * items;
    ProfScope prof(GENIE_KC_GEMM, 2.0 * mn * K, 4.0 * (((double)M * K + (double)N * K) * items + mn * (R ? 3 : 1)), st, "muon_gemm_kernel");
#define MUON_GEMM(TA_, TB_) \
    muon_gemm_kernel<TA_, TB_><<<grid, 256, 0, st>>>(A, lda, sA, B, ldb, sB, R, beta, C, ldc, sC, M, N, K, alpha)
    if (!ta && !tb) MUON_GEMM(false, false);
    else if (!ta && tb) MUON_GEMM(false, true);
    else if (ta && tb) MUON_GEMM(true, true);
    else MUON_GEMM(true, false);
#undef MUON_GEMM
    GENIE_LAUNCH_CHECK("muon_gemm");
    return GENIE_OK;
}

// step 6 on `items` contiguous (rows, cols) matrices that start in x0; x1, A and P are scratch of the same item strides.  The last
// iteration writes to `last` when that is given.  *result: where the final X lies.
static int muon_iterate(float* x0, float* x1, float* A, float* P, float* last, int rows, int cols, int items, int steps, float a,
                        float b, float c, hipStream_t st, float** result) {
    const bool tall = rows > cols;
    const int m = tall ? cols : rows, n = tall ? rows : cols;   // X is (m, n); stored (rows, cols), leading dimension cols
    const size_t sx = (size_t)rows * cols, sg = (size_t)m * m;
    float* cur = x0;
    float* nxt = x1;
    for (int t = 0; t < steps; ++t) {
        float* dst = (t == steps - 1 && last) ? last : nxt;
        // A = X X^T: wide, rows of X against rows of X; tall, columns of the stored array against columns (both operands k-major)
        GENIE_TRY(muon_gemm(tall, tall, cur, cols, sx, cur, cols, sx, nullptr, 0.f, A, m, sg, m, m, n, 1.f, items, st));
        // P = b A + c A A (A symmetric: A A = A A^T, both operands row-major)
        GENIE_TRY(muon_gemm(false, false, A, m, sg, A, m, sg, A, b, P, m, sg, m, m, m, c, items, st));
        if (!tall)   // X = a X + P X: B(n, k) = X[k][n]
            GENIE_TRY(muon_gemm(false, true, P, m, sg, cur, cols, sx, cur, a, dst, cols, sx, rows, cols, m, 1.f, items, st));
        else         // stored array = a X + X P: B(n, k) = P[k][n] = P[n][k]
            GENIE_TRY(muon_gemm(false, false, cur, cols, sx, P, m, sg, cur, a, dst, cols, sx, rows, cols, m, 1.f, items, st));
        nxt = cur;
        cur = dst;
    }
    *result = cur;
    return GENIE_OK;
}

static size_t muon_round(size_t floats) { return (floats + 63) / 64 * 64; }

bool muon_plan(const genie_muon_item* items, int n, MuonPlan& pl) {
    pl.n = n;
    pl.ngroups = 0;
    bool seen[MUON_MAX_ITEMS] = {};
    size_t x = 0, gmax = 0;
    int k = 0;
    for (int e = 0; e < n; ++e) {
        if (seen[e]) continue;
        MuonPlan::Group& g = pl.group[pl.ngroups++];
        g.rows = items[e].rows;
        g.cols = items[e].cols;
        g.first = k;
        g.x_off = x;
        for (int f = e; f < n; ++f)
            if (!seen[f] && items[f].rows == g.rows && items[f].cols == g.cols) {
                seen[f] = true;
                pl.order[k++] = f;
                pl.x_of[f] = x;
                x += (size_t)g.rows * g.cols;
            }
        g.count = k - g.first;
        const size_t m = g.rows < g.cols ? g.rows : g.cols;
        const size_t gs = (size_t)g.count * m * m;
        gmax = gs > gmax ? gs : gmax;
    }
    pl.off_x0 = muon_round((size_t)n * MUON_PARTS * 2);   // the partial sums are doubles, counted here in floats
    pl.off_x1 = pl.off_x0 + muon_round(x);
    pl.off_a = pl.off_x1 + muon_round(x);
    pl.off_p = pl.off_a + muon_round(gmax);
    pl.total_floats = pl.off_p + muon_round(gmax);
    return x < ((size_t)1 << 40);
}

int launch_muon_step(const genie_muon_item* items, const MuonPlan& pl, const genie_muon_settings& s, float* ws, hipStream_t st) {
    double* part = reinterpret_cast<double*>(ws);
    float* x0 = ws + pl.off_x0;
    float* x1 = ws + pl.off_x1;
    const dim3 grid(MUON_PARTS, pl.n);
    MuonMomTable mt;
    MuonNormTable nt;
    for (int e = 0; e < pl.n; ++e) {
        const unsigned n4 = (unsigned)((size_t)items[e].rows * items[e].cols / 4);
        mt.it[e] = {items[e].grad, items[e].momentum, x0 + pl.x_of[e], n4};
        nt.it[e] = {x0 + pl.x_of[e], x0 + pl.x_of[e], n4};
    }
    muon_momentum_kernel<true><<<grid, 256, 0, st>>>(mt, s.momentum, s.nesterov ? 1 : 0, s.grad_mult, s.grad_sumsq, s.max_grad_norm, part);
    GENIE_LAUNCH_CHECK("muon_momentum");
    muon_normalise_kernel<<<grid, 256, 0, st>>>(nt, part, s.eps);
    GENIE_LAUNCH_CHECK("muon_normalise");
    MuonApplyTable at;
    for (int gi = 0; gi < pl.ngroups; ++gi) {
        const MuonPlan::Group& g = pl.group[gi];
        float* res = nullptr;
        GENIE_TRY(muon_iterate(x0 + g.x_off, x1 + g.x_off, ws + pl.off_a, ws + pl.off_p, nullptr, g.rows, g.cols, g.count, s.ns_steps, s.a,
                               s.b, s.c, st, &res));
        const double big = g.rows > g.cols ? g.rows : g.cols;
        const double adj = s.adjust == GENIE_MUON_ADJUST_MATCH_RMS_ADAMW ? 0.2 * sqrt(big) : sqrt(fmax(1.0, (double)g.rows / g.cols));
        for (int k = 0; k < g.count; ++k) {
            const genie_muon_item& it = items[pl.order[g.first + k]];
            at.it[pl.order[g.first + k]] = {it.param, it.ema, res + (size_t)k * g.rows * g.cols, (unsigned)((size_t)g.rows * g.cols / 4),
                                            (float)(1.0 - (double)it.lr * it.weight_decay), (float)((double)it.lr * adj)};
        }
    }
    muon_apply_kernel<<<grid, 256, 0, st>>>(at, s.ema_one_minus_decay);
    GENIE_LAUNCH_CHECK("muon_apply");
    return GENIE_OK;
}

int launch_newton_schulz(const float* in, float* out, int rows, int cols, int batch, int steps, float a, float b, float c, float eps,
                         const MuonPlan& pl, float* ws, hipStream_t st) {
    double* part = reinterpret_cast<double*>(ws);
    float* x0 = ws + pl.off_x0;
    const size_t sx = (size_t)rows * cols;
    const dim3 grid(MUON_PARTS, batch);
    MuonMomTable mt;
    MuonNormTable nt;
    for (int e = 0; e < batch; ++e) {
        mt.it[e] = {in + e * sx, nullptr, nullptr, (unsigned)(sx / 4)};
        nt.it[e] = {in + e * sx, (steps ? x0 : out) + e * sx, (unsigned)(sx / 4)};
    }
    muon_momentum_kernel<false><<<grid, 256, 0, st>>>(mt, 0.f, 0, 1.f, nullptr, 0.f, part);
    GENIE_LAUNCH_CHECK("muon_sumsq");
    muon_normalise_kernel<<<grid, 256, 0, st>>>(nt, part, eps);
    GENIE_LAUNCH_CHECK("muon_normalise");
    float* res = nullptr;
    return muon_iterate(x0, ws + pl.off_x1, ws + pl.off_a, ws + pl.off_p, out, rows, cols, batch, steps, a, b, c, st, &res);
}

}  // namespace genie
