// LPIPS 0.1 (AlexNet and VGG-16 feature stacks) of B images against one target for gfx950, entirely on the device.
//
// Replaces, for testing() (R/train.py:559-761, R/ = dgmesh/), the two lpips.LPIPS networks of R/utils/metric_utils.py:23 (called
// with normalize=True).  Neither the lpips package nor torchvision is a dependency: the network tables below are this project's own
// statement of the two stacks, and tests/_lpips_ref.py restates them with torch.nn.functional in fp64.
//
//   input kernel : (B, 3, H, W) and the target (3, H, W), fp32 in [0, 1] -> channels-last (B + 1, H, W, 3), ((2x - 1) - shift_c) /
//                  scale_c.  The target is image B of every activation buffer: its features are computed once per call.
//   conv kernel  : conv2d + bias + ReLU as an implicit GEMM, M = output pixels of all B + 1 images, N = C_out, K = kh kw C_in with
//                  k = (ky kw + kx) C_in + c.  A 128 x 64 tile of the output per workgroup, four waves of 64 x 32, K in steps of 16
//                  through LDS.  The A tile is gathered from the channels-last input (zero padding and the edge tiles are
//                  predicates of the gather; nothing padded is materialised), the B tile comes from the weights as packed at load
//                  time, (K rounded up to 16, C_out) with zero rows.  The arithmetic is v_mfma_f32_32x32x2_f32: bit for bit a
//                  k-ordered fp32 fma chain per output element, so an output element does not depend on B or on the tile it is in.
//   pool kernel  : max-pool 3/2 (AlexNet) or 2/2 (VGG), floor output size.
//   tap kernel   : per pixel sum_c w_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2 in fp64, sixteen lanes per pixel, summed over a
//                  fixed partition of the pixels in a fixed order into one partial per workgroup.
//   finish kernel: adds the partials in a fixed order, divides by the pixel count and writes the five tap terms and their sum.
//
// No atomics anywhere: the results are bit-reproducible and row b does not depend on B.
#include "dgm_common.hpp"

#include <math.h>

namespace dgm {

static constexpr int LP_MAX_LAYERS = 13, LP_TAPS = 5;
static constexpr int CBM = 128, CBN = 64, CBK = 16;  // the workgroup's tile of the implicit GEMM
static constexpr int CPA = CBM + 32, CPB = CBN + 32;  // LDS row pitches: the two k rows a wave reads at once fall into different banks
static constexpr int TAP_MAX_BLOCKS = 512;

struct LpLayer {
    int cin, cout, k, stride, pad;
    int pool;  // max-pool in front of the convolution: 0 = none, else its window (stride 2)
    int tap;   // the ReLU output is tap number tap - 1; 0 = not a tap
};
struct LpNet {
    int n, min_side;
    LpLayer l[LP_MAX_LAYERS];
};

static const LpNet LP_NETS[2] = {
    {5, 31, {{3, 64, 11, 4, 2, 0, 1}, {64, 192, 5, 1, 2, 3, 2}, {192, 384, 3, 1, 1, 3, 3}, {384, 256, 3, 1, 1, 0, 4},
             {256, 256, 3, 1, 1, 0, 5}}},
    {13, 16, {{3, 64, 3, 1, 1, 0, 0}, {64, 64, 3, 1, 1, 0, 1},
              {64, 128, 3, 1, 1, 2, 0}, {128, 128, 3, 1, 1, 0, 2},
              {128, 256, 3, 1, 1, 2, 0}, {256, 256, 3, 1, 1, 0, 0}, {256, 256, 3, 1, 1, 0, 3},
              {256, 512, 3, 1, 1, 2, 0}, {512, 512, 3, 1, 1, 0, 0}, {512, 512, 3, 1, 1, 0, 4},
              {512, 512, 3, 1, 1, 2, 0}, {512, 512, 3, 1, 1, 0, 0}, {512, 512, 3, 1, 1, 0, 5}}},
};

typedef float lp_f32x16 __attribute__((ext_vector_type(16)));

// images (B, 3, H, W), gt (3, H, W) -> dst (B + 1, H, W, 3)
__global__ void __launch_bounds__(256)
lpips_input_kernel(const float* __restrict__ images, const float* __restrict__ gt, int B, size_t plane, float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)(B + 1) * plane) return;
    const size_t img = i / plane, p = i - img * plane;
    const float* src = img < (size_t)B ? images + img * 3 * plane : gt;
    const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
#pragma unroll
    for (int c = 0; c < 3; c++) dst[i * 3 + c] = ((2.f * src[c * plane + p] - 1.f) - shift[c]) / scale[c];
}

// in (n, H, W, Cin), wp (Kp, Cout) with Kp = K rounded up to CBK, bias (Cout) -> out (n, Ho, Wo, Cout) = relu(conv + bias).
// VEC: Cin is a multiple of CBK, so the 16 k of a step are 16 consecutive channels of one filter position.
template <bool VEC>
__global__ void __launch_bounds__(256)
lpips_conv_kernel(const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ bias, int M, int H, int W,
                  int Cin, int Ho, int Wo, int Cout, int ksz, int stride, int pad, int K, int ntn, float* __restrict__ out) {
    __shared__ float sA[CBK * CPA], sB[CBK * CPB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockIdx.x % ntn, mt = blockIdx.x / ntn;
    const int n0 = nt * CBN;
    // the gather: this thread brings pixel gm's eight k of each step, [kb, kb + 8)
    const int ml = tid & (CBM - 1), kb = (tid >> 7) * 8;
    const long long gm = (long long)mt * CBM + ml;
    const bool live = gm < M;
    int iy0 = 0, ix0 = 0;
    const float* base = in;
    if (live) {
        const int img = (int)(gm / ((long long)Ho * Wo));
        const int rem = (int)(gm - (long long)img * Ho * Wo);
        const int oy = rem / Wo, ox = rem - oy * Wo;
        iy0 = oy * stride - pad, ix0 = ox * stride - pad;
        base = in + (size_t)img * H * W * Cin;
    }
    // the weights: this thread brings four columns of one k row of each step
    const int bk = tid >> 4, bn = (tid & 15) * 4;
    float ra[8];
    float4 rb;
    auto fetch = [&](int k0) {
        if (VEC) {
            const int tap = k0 / Cin, c0 = k0 - tap * Cin;
            const int ky = tap / ksz, kx = tap - ky * ksz;
            const int iy = iy0 + ky, ix = ix0 + kx;
            if (live && iy >= 0 && iy < H && ix >= 0 && ix < W) {
                const float4* p = reinterpret_cast<const float4*>(base + ((size_t)iy * W + ix) * Cin + c0 + kb);
                const float4 u = p[0], v = p[1];
                ra[0] = u.x, ra[1] = u.y, ra[2] = u.z, ra[3] = u.w, ra[4] = v.x, ra[5] = v.y, ra[6] = v.z, ra[7] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) ra[i] = 0.f;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int k = k0 + kb + i;
                const int tap = k / Cin, c = k - tap * Cin;
                const int ky = tap / ksz, kx = tap - ky * ksz;
                const int iy = iy0 + ky, ix = ix0 + kx;
                ra[i] = (live && k < K && iy >= 0 && iy < H && ix >= 0 && ix < W) ? base[((size_t)iy * W + ix) * Cin + c] : 0.f;
            }
        }
        rb = *reinterpret_cast<const float4*>(wp + (size_t)(k0 + bk) * Cout + n0 + bn);  // (rows up to Kp exist and are zero past K)
    };
    lp_f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; i++) acc0[i] = 0.f, acc1[i] = 0.f;
    const int wm = (wave & 1) * 64, wn = (wave >> 1) * 32, r = lane & 31, h = lane >> 5;
    const int Kp = (K + CBK - 1) / CBK * CBK;
    fetch(0);
    for (int k0 = 0; k0 < Kp; k0 += CBK) {
        __syncthreads();  // the previous step's reads are done
#pragma unroll
        for (int i = 0; i < 8; i++) sA[(kb + i) * CPA + ml] = ra[i];
        sB[bk * CPB + bn] = rb.x, sB[bk * CPB + bn + 1] = rb.y, sB[bk * CPB + bn + 2] = rb.z, sB[bk * CPB + bn + 3] = rb.w;
        __syncthreads();
        if (k0 + CBK < Kp) fetch(k0 + CBK);  // in flight during the products
#pragma unroll
        for (int s = 0; s < CBK; s += 2) {  // lane (r, h) holds A[row r][k = s + h] and B[k = s + h][col r]
            const float a0 = sA[(s + h) * CPA + wm + r], a1 = sA[(s + h) * CPA + wm + 32 + r], b = sB[(s + h) * CPB + wn + r];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
        }
    }
    // accumulator register g of lane (r, h): row (g & 3) + 8 (g >> 2) + 4 h, column r
    const int n = n0 + wn + r;
    const float bv = bias[n];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int g = 0; g < 16; g++) {
            const long long m = (long long)mt * CBM + wm + t * 32 + (g & 3) + 8 * (g >> 2) + 4 * h;
            if (m < M) out[(size_t)m * Cout + n] = fmaxf((t == 0 ? acc0[g] : acc1[g]) + bv, 0.f);
        }
}

// in (n, H, W, C) -> out (n, Ho, Wo, C), window win, stride 2, every window inside the image; C is a multiple of 4
__global__ void __launch_bounds__(256)
lpips_pool_kernel(const float* __restrict__ in, size_t total4, int H, int W, int C4, int Ho, int Wo, int win, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int c = (int)(i % C4);
    size_t q = i / C4;
    const int ox = (int)(q % Wo);
    q /= Wo;
    const int oy = (int)(q % Ho);
    const size_t img = q / Ho;
    const float4* src = reinterpret_cast<const float4*>(in) + ((img * H + 2 * oy) * W + 2 * ox) * C4 + c;
    float4 m = src[0];
    for (int dy = 0; dy < win; dy++)
        for (int dx = 0; dx < win; dx++) {
            const float4 v = src[((size_t)dy * W + dx) * C4];
            m.x = fmaxf(m.x, v.x), m.y = fmaxf(m.y, v.y), m.z = fmaxf(m.z, v.z), m.w = fmaxf(m.w, v.w);
        }
    reinterpret_cast<float4*>(out)[i] = m;
}

__device__ __forceinline__ double group16_sum(double v) {
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d, 16);
    return v;
}

// feat (B + 1, hw, C), the target last; lin (C); partial (B, gridDim.x).  C is a multiple of 64.
__global__ void __launch_bounds__(256)
lpips_tap_kernel(const float* __restrict__ feat, int B, int hw, int C, const float* __restrict__ lin, double* __restrict__ partial) {
    __shared__ double red[16];
    const int b = blockIdx.y, g = threadIdx.x >> 4, j = threadIdx.x & 15;
    const float* fa = feat + (size_t)b * hw * C;
    const float* fb = feat + (size_t)B * hw * C;
    double acc = 0.0;
    for (int p = blockIdx.x * 16 + g; p < hw; p += gridDim.x * 16) {
        const float* pa = fa + (size_t)p * C;
        const float* pb = fb + (size_t)p * C;
        double sa = 0.0, sb = 0.0;
        for (int c = 4 * j; c < C; c += 64) {
            const float4 u = *reinterpret_cast<const float4*>(pa + c), v = *reinterpret_cast<const float4*>(pb + c);
            sa += ((double)u.x * u.x + (double)u.y * u.y) + ((double)u.z * u.z + (double)u.w * u.w);
            sb += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
        }
        const double ia = 1.0 / (sqrt(group16_sum(sa)) + 1e-10), ib = 1.0 / (sqrt(group16_sum(sb)) + 1e-10);
        double s = 0.0;
        for (int c = 4 * j; c < C; c += 64) {
            const float4 u = *reinterpret_cast<const float4*>(pa + c), v = *reinterpret_cast<const float4*>(pb + c);
            const float4 w = *reinterpret_cast<const float4*>(lin + c);
            const double d0 = (double)u.x * ia - (double)v.x * ib, d1 = (double)u.y * ia - (double)v.y * ib;
            const double d2 = (double)u.z * ia - (double)v.z * ib, d3 = (double)u.w * ia - (double)v.w * ib;
            s += ((double)w.x * (d0 * d0) + (double)w.y * (d1 * d1)) + ((double)w.z * (d2 * d2) + (double)w.w * (d3 * d3));
        }
        acc += group16_sum(s);
    }
    if (j == 0) red[g] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 16; i++) t += red[i];
        partial[(size_t)b * gridDim.x + blockIdx.x] = t;
    }
}

struct TapTable {
    int nblk[LP_TAPS];
    long long off[LP_TAPS];  // in doubles; tap k's partials are (B, nblk[k])
    double inv_count[LP_TAPS];
};

// one wave per image; out (B, 6): the five tap terms and their sum
__global__ void __launch_bounds__(64)
lpips_finish_kernel(const TapTable tt, const double* __restrict__ partial, double* __restrict__ out) {
    const int b = blockIdx.x;
    double total = 0.0;
    for (int k = 0; k < LP_TAPS; k++) {
        const double* p = partial + tt.off[k] + (size_t)b * tt.nblk[k];
        double v = 0.0;
        for (int i = threadIdx.x; i < tt.nblk[k]; i += 64) v += p[i];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        v *= tt.inv_count[k];
        total += v;
        if (threadIdx.x == 0) out[b * 6 + k] = v;
    }
    if (threadIdx.x == 0) out[b * 6 + 5] = total;
}

struct LpPlan {
    const LpNet* net;
    int inH[LP_MAX_LAYERS], inW[LP_MAX_LAYERS];    // the convolution's input, after the pool in front of it
    int outH[LP_MAX_LAYERS], outW[LP_MAX_LAYERS];
    int tap_blocks[LP_TAPS];
    size_t tap_off[LP_TAPS];  // bytes from partial_off
    size_t act_bytes, partial_off, bytes;  // two activation buffers of act_bytes, then the partials
};

static bool lpips_plan(int net, int B, int H, int W, LpPlan* P) {
    if (net < 0 || net > 1 || B <= 0 || B > 65535 || H <= 0 || W <= 0) return false;
    const LpNet* N = &LP_NETS[net];
    if (H < N->min_side || W < N->min_side) return false;
    const size_t n = (size_t)B + 1;
    if (n * H * W >= ((size_t)1 << 31) / 4) return false;  // pixel and workgroup indices stay in 32 bits
    P->net = N;
    size_t act = n * H * W * 3;
    int h = H, w = W;
    size_t po = 0;
    for (int i = 0; i < N->n; i++) {
        const LpLayer& L = N->l[i];
        if (L.pool) {
            h = (h - L.pool) / 2 + 1, w = (w - L.pool) / 2 + 1;
            if (n * h * w * L.cin > act) act = n * h * w * L.cin;
        }
        P->inH[i] = h, P->inW[i] = w;
        h = (h + 2 * L.pad - L.k) / L.stride + 1, w = (w + 2 * L.pad - L.k) / L.stride + 1;
        if (h < 1 || w < 1) return false;
        P->outH[i] = h, P->outW[i] = w;
        if (n * h * w * L.cout > act) act = n * h * w * L.cout;
        if (L.tap) {
            const int hw = h * w, nb = (hw + 15) / 16;
            P->tap_blocks[L.tap - 1] = nb < TAP_MAX_BLOCKS ? nb : TAP_MAX_BLOCKS;
            P->tap_off[L.tap - 1] = po;
            po += align_up((size_t)B * P->tap_blocks[L.tap - 1] * 8, 256);
        }
    }
    P->act_bytes = align_up(act * 4, 256);
    P->partial_off = 2 * P->act_bytes;
    P->bytes = P->partial_off + po + 256;
    return true;
}


}  // namespace dgm

using namespace dgm;

extern "C" {

size_t dgm_lpips_workspace_bytes(int net, int B, int H, int W) {
    LpPlan P;
    return lpips_plan(net, B, H, W, &P) ? P.bytes : 0;
}

int dgm_lpips(int net, const float* const* conv_w, const float* const* conv_b, const float* const* lin, const float* images,
              const float* gt, int B, int H, int W, char* workspace, double* out, void* stream) {
    LpPlan P;
    if (!conv_w || !conv_b || !lin || !images || !gt || !workspace || !out || !lpips_plan(net, B, H, W, &P)) {
        set_last_error("lpips: bad argument (net is 0 = alex or 1 = vgg; B >= 1; min(H, W) >= 31 for alex, 16 for vgg)");
        return 1;
    }
    const LpNet* N = P.net;
    for (int i = 0; i < N->n; i++)
        if (!conv_w[i] || !conv_b[i]) {
            set_last_error("lpips: a convolution's weight or bias pointer is NULL");
            return 1;
        }
    for (int k = 0; k < LP_TAPS; k++)
        if (!lin[k]) {
            set_last_error("lpips: a linear layer's weight pointer is NULL");
            return 1;
        }
    hipStream_t st = (hipStream_t)stream;
    char* p = align_ptr(workspace);
    float* buf[2] = {(float*)p, (float*)(p + P.act_bytes)};
    double* partial = (double*)(p + P.partial_off);
    const int n = B + 1;
    const size_t plane = (size_t)H * W;
    int cur = 0;
    hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)((n * plane + 255) / 256)), dim3(256), 0, st, images, gt, B, plane, buf[cur]);
    TapTable tt;
    int h = H, w = W;
    for (int i = 0; i < N->n; i++) {
        const LpLayer& L = N->l[i];
        if (L.pool) {
            const int ho = P.inH[i], wo = P.inW[i];
            const size_t total4 = (size_t)n * ho * wo * (L.cin / 4);
            hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, st, buf[cur], total4, h, w,
                               L.cin / 4, ho, wo, L.pool, buf[cur ^ 1]);
            cur ^= 1, h = ho, w = wo;
        }
        const int ho = P.outH[i], wo = P.outW[i];
        const int M = n * ho * wo, K = L.k * L.k * L.cin, ntn = L.cout / CBN;
        const dim3 grid((unsigned)((M + CBM - 1) / CBM) * ntn);
        if (L.cin % CBK == 0)
            hipLaunchKernelGGL(lpips_conv_kernel<true>, grid, dim3(256), 0, st, buf[cur], conv_w[i], conv_b[i], M, h, w, L.cin, ho, wo,
                               L.cout, L.k, L.stride, L.pad, K, ntn, buf[cur ^ 1]);
        else
            hipLaunchKernelGGL(lpips_conv_kernel<false>, grid, dim3(256), 0, st, buf[cur], conv_w[i], conv_b[i], M, h, w, L.cin, ho, wo,
                               L.cout, L.k, L.stride, L.pad, K, ntn, buf[cur ^ 1]);
        cur ^= 1, h = ho, w = wo;
        if (L.tap) {
            const int k = L.tap - 1;
            hipLaunchKernelGGL(lpips_tap_kernel, dim3(P.tap_blocks[k], B), dim3(256), 0, st, buf[cur], B, h * w, L.cout, lin[k],
                               (double*)((char*)partial + P.tap_off[k]));
            tt.nblk[k] = P.tap_blocks[k];
            tt.off[k] = (long long)(P.tap_off[k] / 8);
            tt.inv_count[k] = 1.0 / ((double)h * (double)w);
        }
    }
    hipLaunchKernelGGL(lpips_finish_kernel, dim3(B), dim3(64), 0, st, tt, (const double*)partial, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error(hipGetErrorString(e));
        return 1;
    }
    return 0;
}

}  // extern "C"
