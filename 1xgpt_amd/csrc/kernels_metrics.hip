// Image-space metrics of two uint8 frame batches (genie_frame_metrics in include/genie_hip.h, which states the definition): per image
// the exact sums of (a - b)^2 and |a - b| and the sum of the Gaussian-window SSIM index over every valid window position.
//
// frame_metrics_tile_kernel: one workgroup per (image, channel, 32 x 32 tile of window positions).  It stages the tile's 42 x 42 pixels
// (tile + 10-pixel halo) of both images in LDS, runs the 11-tap horizontal pass over the five fields x, y, x^2, y^2, xy into LDS and the
// vertical pass out of it, evaluates SSIM at its window positions and writes ONE record (ssim, sse, sae) to the workspace.
// frame_metrics_finish_kernel: one wave per image adds that image's records in a fixed order and writes the four outputs.
// No atomics, no cross-workgroup traffic inside a launch: results are bit-identical run to run and independent of the batch.
//
// Arithmetic: pixels are pivoted by 128 (the second moments do not see a shift; the means are shifted back) and every moment is
// accumulated in f64, taps ascending: with integer pixels the moments carry ~1e-13 absolute error, so sigma^2 = E[x^2] - mu^2 does not
// cancel even on a flat pair.  sse / sae are integers throughout.
#include "common.hpp"
#include "kernels.hpp"

namespace genie {

constexpr int FM_TILE = 32;                 // window positions per tile edge
constexpr int FM_HALO = 10;                 // 11-tap window: 10 more pixels than positions
constexpr int FM_IN = FM_TILE + FM_HALO;    // 42 staged pixels per tile edge
constexpr int FM_THREADS = 256;
constexpr int FM_HG = 4;                    // horizontal pass: adjacent positions per work item
constexpr int FM_VG = 4;                    // vertical pass: adjacent positions per thread

struct FrameMetricsPartial {
    double ssim;
    unsigned long long sse, sae;
};
static_assert(sizeof(FrameMetricsPartial) == 24, "workspace record");

// exp(-r^2 / 4.5), r = -5..5, over their sum
__device__ constexpr double FM_TAP[11] = {0.00102838008447911, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002,
                                          0.2130055377112537,  0.26601172486179436,  0.2130055377112537,  0.10936068950970002,
                                          0.03600077212843083, 0.007598758135239185, 0.00102838008447911};

__device__ __forceinline__ double fm_ssim(double mx, double my, double xx, double yy, double xy) {
    constexpr double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const double vx = xx - mx * mx, vy = yy - my * my, cxy = xy - mx * my;   // moments of the pivoted values: shift-invariant
    const double ux = mx + 128.0, uy = my + 128.0;
    return ((2.0 * ux * uy + C1) * (2.0 * cxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
}

__global__ __launch_bounds__(FM_THREADS) void frame_metrics_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                        int H, int W, int tiles_x, int tiles_y,
                                                                        FrameMetricsPartial* __restrict__ part) {
    __shared__ int16_t px[2][FM_IN][FM_IN];              // a - 128, b - 128; 0 outside the image
    __shared__ double hz[5][FM_IN][FM_TILE];             // horizontal pass: mu_x, mu_y, xx, yy, xy
    __shared__ double red_f[FM_THREADS / WAVE];
    __shared__ unsigned long long red_u[2][FM_THREADS / WAVE];

    const int tid = (int)threadIdx.x;
    const long tiles = (long)tiles_x * tiles_y;
    const long plane = (long)blockIdx.x / tiles;         // image * C + channel
    const int tile = (int)((long)blockIdx.x - plane * tiles);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int r0 = ty * FM_TILE, c0 = tx * FM_TILE;
    const long base = plane * ((long)H * W);
    // every pixel is owned by exactly one tile for sse / sae: the tile's own 32 x 32, and what lies beyond the last tile's
    const int own_r = (ty == tiles_y - 1) ? FM_IN : FM_TILE, own_c = (tx == tiles_x - 1) ? FM_IN : FM_TILE;

    unsigned int sse = 0, sae = 0;                       // <= 7 pixels per thread
    for (int i = tid; i < FM_IN * FM_IN; i += FM_THREADS) {
        const int r = i / FM_IN, c = i - r * FM_IN;
        int va = 0, vb = 0;
        if (r0 + r < H && c0 + c < W) {
            const long off = base + (long)(r0 + r) * W + (c0 + c);
            va = (int)a[off];
            vb = (int)b[off];
            if (r < own_r && c < own_c) {
                const int d = va - vb;
                sse += (unsigned int)(d * d);
                sae += (unsigned int)(d < 0 ? -d : d);
            }
            va -= 128;
            vb -= 128;
        }
        px[0][r][c] = (int16_t)va;
        px[1][r][c] = (int16_t)vb;
    }
    __syncthreads();

    // horizontal pass: item = (row, 4 adjacent positions); pixel k of its 14 feeds position j with tap k - j
    for (int item = tid; item < FM_IN * (FM_TILE / FM_HG); item += FM_THREADS) {
        const int r = item / (FM_TILE / FM_HG), cg = (item - r * (FM_TILE / FM_HG)) * FM_HG;
        double acc[5][FM_HG] = {};
#pragma unroll
        for (int k = 0; k < FM_HG + FM_HALO; ++k) {
            const double x = (double)px[0][r][cg + k], y = (double)px[1][r][cg + k];
            const double xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
            for (int j = 0; j < FM_HG; ++j) {
                if (k - j >= 0 && k - j <= FM_HALO) {
                    const double w = FM_TAP[k - j];
                    acc[0][j] = fma(w, x, acc[0][j]);
                    acc[1][j] = fma(w, y, acc[1][j]);
                    acc[2][j] = fma(w, xx, acc[2][j]);
                    acc[3][j] = fma(w, yy, acc[3][j]);
                    acc[4][j] = fma(w, xy, acc[4][j]);
                }
            }
        }
#pragma unroll
        for (int f = 0; f < 5; ++f)
#pragma unroll
            for (int j = 0; j < FM_HG; ++j) hz[f][r][cg + j] = acc[f][j];
    }
    __syncthreads();

    // vertical pass: thread = (column, 4 adjacent positions down), then SSIM at its valid positions, rows ascending
    const int col = tid % FM_TILE, rg = (tid / FM_TILE) * FM_VG;
    double acc[5][FM_VG] = {};
#pragma unroll
    for (int f = 0; f < 5; ++f) {
#pragma unroll
        for (int k = 0; k < FM_VG + FM_HALO; ++k) {
            const double v = hz[f][rg + k][col];
#pragma unroll
            for (int j = 0; j < FM_VG; ++j)
                if (k - j >= 0 && k - j <= FM_HALO) acc[f][j] = fma(FM_TAP[k - j], v, acc[f][j]);
        }
    }
    double ssim = 0.0;
#pragma unroll
    for (int j = 0; j < FM_VG; ++j) {
        const double s = fm_ssim(acc[0][j], acc[1][j], acc[2][j], acc[3][j], acc[4][j]);
        const bool valid = (r0 + rg + j < H - FM_HALO) && (c0 + col < W - FM_HALO);
        ssim += valid ? s : 0.0;
    }

    // workgroup sums in a fixed order: butterfly within a wave, then the four wave sums ascending
    unsigned long long sse64 = sse, sae64 = sae;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ssim += __shfl_xor(ssim, o);
        sse64 += __shfl_xor(sse64, o);
        sae64 += __shfl_xor(sae64, o);
    }
    if (tid % WAVE == 0) {
        red_f[tid / WAVE] = ssim;
        red_u[0][tid / WAVE] = sse64;
        red_u[1][tid / WAVE] = sae64;
    }
    __syncthreads();
    if (tid == 0) {
        FrameMetricsPartial p = {0.0, 0, 0};
#pragma unroll
        for (int w = 0; w < FM_THREADS / WAVE; ++w) {
            p.ssim += red_f[w];
            p.sse += red_u[0][w];
            p.sae += red_u[1][w];
        }
        part[blockIdx.x] = p;
    }
}

// One wave per image: lane l adds records l, l + 64, ... ascending, then a butterfly.  out row = (sse, sae, ssim_sum, n_win).
__global__ __launch_bounds__(WAVE) void frame_metrics_finish_kernel(const FrameMetricsPartial* __restrict__ part, long per_image,
                                                                    double n_win, double* __restrict__ out) {
    const FrameMetricsPartial* p = part + (long)blockIdx.x * per_image;
    double ssim = 0.0;
    unsigned long long sse = 0, sae = 0;
    for (long i = threadIdx.x; i < per_image; i += WAVE) {
        ssim += p[i].ssim;
        sse += p[i].sse;
        sae += p[i].sae;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ssim += __shfl_xor(ssim, o);
        sse += __shfl_xor(sse, o);
        sae += __shfl_xor(sae, o);
    }
    if (threadIdx.x == 0) {
        double* o = out + (long)blockIdx.x * 4;
        o[0] = (double)sse;
        o[1] = (double)sae;
        o[2] = ssim;
        o[3] = n_win;
    }
}

long frame_metrics_tiles(int C, int H, int W) {
    return (long)C * ((H - FM_HALO + FM_TILE - 1) / FM_TILE) * ((W - FM_HALO + FM_TILE - 1) / FM_TILE);
}

size_t frame_metrics_workspace_bytes(long n, int C, int H, int W) {
    return (size_t)n * (size_t)frame_metrics_tiles(C, H, W) * sizeof(FrameMetricsPartial);
}

int launch_frame_metrics(const uint8_t* a, const uint8_t* b, long n, int C, int H, int W, double* out, void* workspace, hipStream_t st) {
    const int tiles_x = (W - FM_HALO + FM_TILE - 1) / FM_TILE, tiles_y = (H - FM_HALO + FM_TILE - 1) / FM_TILE;
    const long per_image = frame_metrics_tiles(C, H, W);
    FrameMetricsPartial* part = static_cast<FrameMetricsPartial*>(workspace);
    frame_metrics_tile_kernel<<<(unsigned)(n * per_image), FM_THREADS, 0, st>>>(a, b, H, W, tiles_x, tiles_y, part);
    GENIE_LAUNCH_CHECK("frame_metrics");
    frame_metrics_finish_kernel<<<(unsigned)n, WAVE, 0, st>>>(part, per_image, (double)C * (double)(H - FM_HALO) * (double)(W - FM_HALO), out);
    GENIE_LAUNCH_CHECK("frame_metrics_finish");
    return GENIE_OK;
}

}  // namespace genie
