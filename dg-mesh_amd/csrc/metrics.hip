// Test-view image metrics for gfx950: MSE, PSNR, SSIM (the rgb_ssim definition) and MS-SSIM of B images against one target,
// entirely on the device.
//
// Replaces, for testing() (R/train.py:559-761, R/ = dgmesh/), get_psnr (R/utils/image_utils.py:24-28), rgb_ssim
// (R/utils/metric_utils.py:26-79: numpy + scipy on the host) and pytorch_msssim.ms_ssim (fp64 torch): four device-to-host image
// copies and six host round trips per view.  pytorch_msssim is not vendored: the MS-SSIM here is this project's own statement of
// that package's defaults.
//
//   level kernel : one 32x16 tile of the "valid" map of one channel per workgroup.  The 42x26 input tile of the target goes to LDS
//                  once, then for each of the B images: its tile goes to LDS, the five windowed moments (E[x], E[y], E[x^2], E[y^2],
//                  E[xy]; the target's two are kept from the first image) come from a separable pass through LDS, and the rgb_ssim
//                  value (level 0), the cs value and the ssim_l value are formed per pixel and summed per workgroup.  Level 0 also
//                  sums the squared error over the input pixels the tile owns.
//   pool kernel  : the next level's images, 2x2 average with stride 2, an odd side zero-padded by one on both ends, divisor 4.
//   finish kernel: one workgroup per image adds the per-workgroup partials in a fixed order and combines levels, weights and channels.
//
// Precision.  Inputs are fp32; every product, moment and sum is fp64.  E[x^2] - mu^2 of a flat region cancels to rounding noise that
// the maps divide by C2 = 8.1e-4 L^2, so fp32 moments would put ~1e-4 per pixel on exactly the images testing() scores (white
// backgrounds); fp64 moments cost ~0.9 GFLOP on a 3x800x800 pair, microseconds on this chip.  No atomics: a fixed partition, fixed
// summation orders, so the results are bit-reproducible and independent of B.
#include "dgm_common.hpp"

#include <math.h>

namespace dgm {

static constexpr int MT = 32, MTY = 16;                // tile of the valid map
static constexpr int MR = MT + 10, MRY = MTY + 10;      // its input tile: 42 x 26
static constexpr int MP = 44;                           // LDS row pitch of the input tiles: a multiple of 4 (16-byte reads)
static constexpr int MAX_LEVELS = 5;

struct Taps {
    double w[11];
};
static Taps taps_host() {
    Taps t;
    double s = 0.0;
    for (int k = 0; k < 11; k++) {
        t.w[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
        s += t.w[k];
    }
    for (int k = 0; k < 11; k++) t.w[k] /= s;
    return t;
}

// what the finish kernel needs to know of each level (by value)
struct LevelTable {
    int n;
    int ntiles[MAX_LEVELS];
    long long partial_off[MAX_LEVELS];  // in doubles
    double inv_count[MAX_LEVELS];       // 1 / pixels of the level's valid map
    double weight[MAX_LEVELS];
};

// sum of four doubles per thread over the 256 threads, in a fixed order; the result is valid in thread 0
__device__ __forceinline__ void block_sum4(double (&v)[4], double (*red)[4]) {
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < 4; q++) red[threadIdx.x >> 6][q] = v[q];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) v[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
}

// partial: (B, C, tiles, 4) doubles = {squared error, sum rgb_ssim, sum cs, sum ssim_l}; the first two are zero above level 0
__global__ void __launch_bounds__(256)
metrics_level_kernel(const Taps tp, const float* __restrict__ img, const float* __restrict__ gt, int B, int C, int H, int W, double C1,
                     double C2, int level0, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float sI[MRY * MP], sG[MRY * MP];
    __shared__ double hq[5][MRY * MT];
    __shared__ double red[4][4];
    const double* w = tp.w;
    const int c = blockIdx.z;
    const size_t plane = (size_t)H * W;
    const int x0 = blockIdx.x * MT, y0 = blockIdx.y * MTY;
    const int ntiles = gridDim.x * gridDim.y, tile = blockIdx.y * gridDim.x + blockIdx.x;
    // input pixels whose squared error this tile sums: its 32x16 block; the last column / row of tiles also takes the 10-pixel rim
    const int own_x = blockIdx.x == gridDim.x - 1 ? MR : MT, own_y = blockIdx.y == gridDim.y - 1 ? MRY : MTY;
    const float* Gc = gt + c * plane;
    for (int i = threadIdx.x; i < MRY * MP; i += 256) {  // (the two pad columns too: the 16-byte reads below touch them)
        const int y = i / MP, x = i - y * MP;
        const int gy = y0 + y, gx = x0 + x;
        sG[i] = (x < MR && gy < H && gx < W) ? Gc[(size_t)gy * W + gx] : 0.f;
    }
    for (int b = 0; b < B; b++) {
        const float* Ic = img + ((size_t)b * C + c) * plane;
        for (int i = threadIdx.x; i < MRY * MP; i += 256) {
            const int y = i / MP, x = i - y * MP;
            const int gy = y0 + y, gx = x0 + x;
            sI[i] = (x < MR && gy < H && gx < W) ? Ic[(size_t)gy * W + gx] : 0.f;
        }
        __syncthreads();
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (level0) {
            for (int i = threadIdx.x; i < MRY * MP; i += 256) {  // (pixels outside the image are zero in both tiles)
                const int y = i / MP, x = i - y * MP;
                if (x < own_x && y < own_y) {
                    const double d = (double)sI[i] - (double)sG[i];
                    acc[0] += d * d;
                }
            }
        }
        if (threadIdx.x < MRY * (MT / 4)) {  // horizontal pass: (row, four columns)
            const int y = threadIdx.x >> 3, xg = (threadIdx.x & 7) * 4;
            float a[16], g[16];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 fa = *reinterpret_cast<const float4*>(&sI[y * MP + xg + 4 * q]);
                const float4 fg = *reinterpret_cast<const float4*>(&sG[y * MP + xg + 4 * q]);
                a[4 * q] = fa.x, a[4 * q + 1] = fa.y, a[4 * q + 2] = fa.z, a[4 * q + 3] = fa.w;
                g[4 * q] = fg.x, g[4 * q + 1] = fg.y, g[4 * q + 2] = fg.z, g[4 * q + 3] = fg.w;
            }
#pragma unroll
            for (int f = 0; f < 5; f++) {
                if (b > 0 && (f == 1 || f == 3)) continue;  // the target's moments are kept from the first image
                double v[14];
#pragma unroll
                for (int e = 0; e < 14; e++) {
                    const double xa = (double)a[e], xg_ = (double)g[e];
                    v[e] = f == 0 ? xa : f == 1 ? xg_ : f == 2 ? xa * xa : f == 3 ? xg_ * xg_ : xa * xg_;
                }
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < 11; k++) s += w[k] * v[j + k];
                    hq[f][y * MT + xg + j] = s;
                }
            }
        }
        __syncthreads();
        const int tx = threadIdx.x & 31, ty = (threadIdx.x >> 5) * 2;  // vertical pass: column tx, rows ty, ty + 1
        double m[5][2];
#pragma unroll
        for (int f = 0; f < 5; f++) {
            double v[12];
#pragma unroll
            for (int e = 0; e < 12; e++) v[e] = hq[f][(ty + e) * MT + tx];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 11; k++) s += w[k] * v[j + k];
                m[f][j] = s;
            }
        }
        const int px = x0 + tx;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int py = y0 + ty + j;
            if (px < W - 10 && py < H - 10) {
                const double mu0 = m[0][j], mu1 = m[1][j];
                const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
                const double s00 = m[2][j] - mu00, s11 = m[3][j] - mu11, s01 = m[4][j] - mu01;
                const double lum_n = 2.0 * mu01 + C1, lum_d = mu00 + mu11 + C1;
                const double cs = (2.0 * s01 + C2) / (s00 + s11 + C2);
                acc[2] += cs;
                acc[3] += (lum_n / lum_d) * cs;
                if (level0) {  // rgb_ssim: clipped variances, covariance bounded by their geometric mean
                    const double c00 = fmax(0.0, s00), c11 = fmax(0.0, s11);
                    const double mag = fmin(sqrt(c00 * c11), fabs(s01));
                    const double c01 = s01 > 0.0 ? mag : (s01 < 0.0 ? -mag : 0.0);
                    acc[1] += (lum_n * (2.0 * c01 + C2)) / (lum_d * (c00 + c11 + C2));
                }
            }
        }
        block_sum4(acc, red);
        if (threadIdx.x == 0) {
            double* o = partial + (((size_t)b * C + c) * ntiles + tile) * 4;
            o[0] = acc[0], o[1] = acc[1], o[2] = acc[2], o[3] = acc[3];
        }
        __syncthreads();  // hq, sI and red are rewritten for the next image
    }
}

// dst: (nA + nB, Ho, Wo); the first nA planes are pooled from srcA, the others from srcB, all (Hi, Wi).  pad = 1 for an odd side.
__global__ void __launch_bounds__(256)
metrics_pool_kernel(const float* __restrict__ srcA, int nA, const float* __restrict__ srcB, int Hi, int Wi, int Ho, int Wo,
                    float* __restrict__ dst) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int p = blockIdx.z;
    if (ox >= Wo || oy >= Ho) return;
    const float* s = (p < nA ? srcA + (size_t)p * Hi * Wi : srcB + (size_t)(p - nA) * Hi * Wi);
    const int ix = 2 * ox - (Wi & 1), iy = 2 * oy - (Hi & 1);
    float v[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const int y = iy + dy, x = ix + dx;
            v[dy][dx] = (y >= 0 && y < Hi && x >= 0 && x < Wi) ? s[(size_t)y * Wi + x] : 0.f;
        }
    dst[((size_t)p * Ho + oy) * Wo + ox] = ((v[0][0] + v[0][1]) + (v[1][0] + v[1][1])) * 0.25f;
}

// one workgroup per image; out: (B, 4) doubles {mse, psnr, ssim, ms_ssim (NaN for a single level)}
__global__ void __launch_bounds__(256)
metrics_finish_kernel(const LevelTable lt, const double* __restrict__ partial, int C, double inv_pixels, double* __restrict__ out) {
    __shared__ double red[4][4];
    const int b = blockIdx.x;
    double sq = 0.0, rgb = 0.0, ms = 0.0;
    for (int c = 0; c < C; c++) {
        double prod = 1.0;
        for (int l = 0; l < lt.n; l++) {
            const double* p = partial + lt.partial_off[l] + ((size_t)b * C + c) * lt.ntiles[l] * 4;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = threadIdx.x; i < lt.ntiles[l]; i += 256)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[q] += p[(size_t)i * 4 + q];
            block_sum4(acc, red);
            __syncthreads();
            if (l == 0) sq += acc[0], rgb += acc[1];
            const double v = (l == lt.n - 1 ? acc[3] : acc[2]) * lt.inv_count[l];  // cs below the last level, ssim_l at it
            prod *= pow(fmax(v, 0.0), lt.weight[l]);
        }
        ms += prod;
    }
    if (threadIdx.x == 0) {
        const double mse = sq * inv_pixels;
        out[b * 4 + 0] = mse;
        out[b * 4 + 1] = -10.0 * log10(mse);
        out[b * 4 + 2] = rgb * lt.inv_count[0] / (double)C;
        out[b * 4 + 3] = lt.n > 1 ? ms / (double)C : __longlong_as_double(0x7ff8000000000000ll);
    }
}

struct MetricsPlan {
    int n;
    int H[MAX_LEVELS], W[MAX_LEVELS], tx[MAX_LEVELS], ty[MAX_LEVELS];
    size_t image_off[MAX_LEVELS];    // bytes; level l >= 1: (B + 1) * C pooled planes, the B images first, then the target
    size_t partial_off[MAX_LEVELS];  // bytes
    size_t bytes;
};

static bool metrics_plan(int B, int C, int H, int W, int levels, MetricsPlan* P) {
    if (B <= 0 || C <= 0 || C > 65535 || (levels != 1 && levels != MAX_LEVELS) || H < 11 || W < 11) return false;
    if (levels > 1 && (H <= 160 || W <= 160)) return false;
    P->n = levels;
    size_t o = 0;
    for (int l = 0; l < levels; l++) {
        P->H[l] = l == 0 ? H : P->H[l - 1] / 2 + (P->H[l - 1] & 1);
        P->W[l] = l == 0 ? W : P->W[l - 1] / 2 + (P->W[l - 1] & 1);
        P->tx[l] = (P->W[l] - 10 + MT - 1) / MT;
        P->ty[l] = (P->H[l] - 10 + MTY - 1) / MTY;
        P->image_off[l] = o;
        if (l > 0) o += align_up((size_t)(B + 1) * C * P->H[l] * P->W[l] * 4, 256);
        P->partial_off[l] = o;
        o += align_up((size_t)B * C * P->tx[l] * P->ty[l] * 4 * 8, 256);
    }
    P->bytes = o + 256;
    return true;
}


}  // namespace dgm

using namespace dgm;

extern "C" {

size_t dgm_image_metrics_workspace_bytes(int B, int C, int H, int W, int levels) {
    MetricsPlan P;
    return metrics_plan(B, C, H, W, levels, &P) ? P.bytes : 0;
}

int dgm_image_metrics(const float* images, const float* gt, int B, int C, int H, int W, float data_range, int levels, char* workspace,
                      double* out, void* stream) {
    MetricsPlan P;
    if (!images || !gt || !workspace || !out || !(data_range > 0.f) || !metrics_plan(B, C, H, W, levels, &P)) {
        set_last_error("image_metrics: bad argument (levels is 1 or 5; H, W >= 11, and > 160 for 5 levels)");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    char* p = align_ptr(workspace);
    const double L = (double)data_range, C1 = (0.01 * L) * (0.01 * L), C2 = (0.03 * L) * (0.03 * L);
    const double weights[MAX_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    const Taps tp = taps_host();
    LevelTable lt;
    lt.n = levels;
    const float *img = images, *tgt = gt;
    for (int l = 0; l < levels; l++) {
        if (l > 0) {
            float* dst = (float*)(p + P.image_off[l]);
            dim3 grid((P.W[l] + 63) / 64, (P.H[l] + 3) / 4, (B + 1) * C);
            hipLaunchKernelGGL(metrics_pool_kernel, grid, dim3(256), 0, st, img, B * C, tgt, P.H[l - 1], P.W[l - 1], P.H[l], P.W[l], dst);
            img = dst;
            tgt = dst + (size_t)B * C * P.H[l] * P.W[l];
        }
        double* partial = (double*)(p + P.partial_off[l]);
        hipLaunchKernelGGL(metrics_level_kernel, dim3(P.tx[l], P.ty[l], C), dim3(256), 0, st, tp, img, tgt, B, C, P.H[l], P.W[l], C1, C2,
                           (int)(l == 0), partial);
        lt.ntiles[l] = P.tx[l] * P.ty[l];
        lt.partial_off[l] = (long long)((P.partial_off[l] - P.partial_off[0]) / 8);
        lt.inv_count[l] = 1.0 / ((double)(P.H[l] - 10) * (double)(P.W[l] - 10));
        lt.weight[l] = levels > 1 ? weights[l] : 1.0;
    }
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(B), dim3(256), 0, st, lt, (const double*)(p + P.partial_off[0]), C,
                       1.0 / ((double)C * H * W), out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error(hipGetErrorString(e));
        return 1;
    }
    return 0;
}

}  // extern "C"
