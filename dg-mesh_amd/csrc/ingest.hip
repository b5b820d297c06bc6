// Dataset ingest for gfx950: PNG unfiltering and the reference's compositing of an RGBA frame over the background, on the device.
//
// Replaces, for readCamerasFromTransforms + PILtoTorch (R/scene/dataset_readers.py:288-302, R/utils/general_utils.py:23-29,
// R/ = dgmesh/), PIL's decoder and four numpy passes on the host.  The host inflates the IDAT stream (zlib); everything after is here.
//
//   unfilter kernel: one workgroup of 1024 threads per image, one lane per scanline, rows skewed by ONE pixel: at step s the lane of
//                    row r reconstructs pixel x = s - r.  The row above reconstructed that x one step earlier, so `up` is the upper
//                    lane's previous output (one __shfl_up), `up-left` is the `up` of the step before and `left` the lane's own
//                    previous output: registers only.  Lane 0 of a wave takes `up` from lane 63 of the wave before through a
//                    double-buffered LDS word behind the step's one __syncthreads().  A band of R = min(H - y0, 1024) rows takes
//                    W + R - 1 steps -- the same count for every thread; nothing spins on memory.  A step's filtered bytes are
//                    loaded during the step before.  Images taller than 1024 rows are
//                    walked in bands by the same workgroup: row 0 of a later band reads `up` from the finished row above in `out`.
//   ingest kernel  : four pixels per thread (16 bytes in, 4 x 16 bytes out), fp64 arithmetic in the reference's order.
//   composite kernel: the same bytes before the division, as (R, G, B, file alpha) words: the input of a `resolution` resize.
//   expand kernel  : the packed rows of a 1-, 2-, 4- or 8-bit grey or palette image (unfiltered as bytes: W' = row bytes, CH = 1)
//                    as one byte per pixel, most significant bits first, times Pillow's grey scale (255, 85, 17, 1) or 1 for indices.
//   masked ingest  : the real captures' compositing (readNerfiesCameras, readiPhoneCameras, readNeuralActorCameras,
//                    R/scene/dataset_readers.py:545-865): the frame where channel 0 of the mask is set, the background elsewhere;
//                    planes (byte / 255, mask > 0) or (R, G, B, 255 (mask > 0)) words for a `resolution` resize.
//
// Built with -ffp-contract=off and correctly rounded fp32 division: (n_c n_a + bg (1 - n_a)) 255 truncates to a different byte than
// any contracted or integer form for some (colour, alpha) pairs.
#include "dgm_common.hpp"

#include <stdio.h>

namespace dgm {


static constexpr int UF_ROWS = 1024;  // rows per band = threads per workgroup
static constexpr int UF_WAVES = UF_ROWS / 64;

typedef unsigned dgm_u4u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned dgm_u32b __attribute__((aligned(1)));

__device__ __forceinline__ unsigned paeth(unsigned a, unsigned b, unsigned c) {
    const int pa = abs((int)b - (int)c), pb = abs((int)a - (int)c), pc = abs((int)a + (int)b - 2 * (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// the CH bytes of one pixel as a word.  ALIGNED: p is a multiple of four when CH is 4 (the output); otherwise any address (the
// filtered scanlines start one byte past a multiple of the row length)
template <int CH, bool ALIGNED>
__device__ __forceinline__ unsigned load_pixel(const unsigned char* p) {
    if (CH == 4) return ALIGNED ? *(const unsigned*)p : *(const dgm_u32b*)p;
    if (CH == 1) return (unsigned)p[0];
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

template <int CH>
__global__ __launch_bounds__(UF_ROWS) void png_unfilter_kernel(int W, int H, const unsigned char* __restrict__ in,
                                                               unsigned char* __restrict__ out) {
    __shared__ unsigned edge[2][UF_WAVES];
    const int r = (int)threadIdx.x, lane = r & 63, wave = r >> 6;
    const size_t stride = 1 + (size_t)W * CH;
    const unsigned char* src = in + (size_t)blockIdx.x * H * stride;
    unsigned char* dst = out + (size_t)blockIdx.x * H * W * CH;
    if (r < 2 * UF_WAVES) (&edge[0][0])[r] = 0u;
    __syncthreads();
    for (int y0 = 0; y0 < H; y0 += UF_ROWS) {
        const int rows = H - y0 < UF_ROWS ? H - y0 : UF_ROWS;
        const bool live = r < rows;
        const int y = live ? y0 + r : y0;
        const unsigned char* srow = src + (size_t)y * stride + 1;
        unsigned char* drow = dst + (size_t)y * W * CH;
        unsigned ft = live ? (unsigned)srow[-1] : 0u;
        if (ft > 4u) ft = 0u;  // (the host refuses such files; this keeps the kernel total)
        unsigned prev = 0u, upleft = 0u;  // this lane's previous output (= left) and previous `up` (= up-left)
        const int steps = W + rows - 1;   // uniform over the workgroup
        // the filtered bytes are fetched one step ahead: the load's latency passes under the step's arithmetic and barrier instead of
        // standing at the head of every step
        unsigned fnext = (live && r == 0) ? load_pixel<CH, false>(srow) : 0u;
        for (int s = 0; s < steps; s++) {
            const int x = s - r;
            const bool act = live && x >= 0 && x < W;
            const unsigned fcur = fnext;
            fnext = (live && x + 1 >= 0 && x + 1 < W) ? load_pixel<CH, false>(srow + (size_t)(x + 1) * CH) : 0u;
            unsigned up = (unsigned)__shfl_up((int)prev, 1, 64);
            if (lane == 0) {
                if (wave > 0)
                    up = edge[(s + 1) & 1][wave - 1];  // lane 63 of the wave before, written in step s - 1
                else
                    up = (act && y0 > 0) ? load_pixel<CH, true>(drow - (size_t)W * CH + (size_t)x * CH) : 0u;
            }
            unsigned o = 0u;
            if (act) {
#pragma unroll
                for (int c = 0; c < CH; c++) {
                    const unsigned a = (prev >> (8 * c)) & 255u, b = (up >> (8 * c)) & 255u, cc = (upleft >> (8 * c)) & 255u;
                    const unsigned pred = ft == 1u ? a : ft == 2u ? b : ft == 3u ? ((a + b) >> 1) : ft == 4u ? paeth(a, b, cc) : 0u;
                    o |= ((((fcur >> (8 * c)) & 255u) + pred) & 255u) << (8 * c);
                }
                unsigned char* d = drow + (size_t)x * CH;
                if (CH == 4) {
                    *(unsigned*)d = o;
                } else if (CH == 1) {
                    d[0] = (unsigned char)o;
                } else {
                    d[0] = (unsigned char)(o & 255u);
                    d[1] = (unsigned char)((o >> 8) & 255u);
                    d[2] = (unsigned char)((o >> 16) & 255u);
                }
            }
            upleft = up;
            prev = o;
            if (lane == 63 && wave < UF_WAVES - 1) edge[s & 1][wave] = o;
            __syncthreads();
        }
        __threadfence_block();  // the band's last row is read from `out` by the next band's first lane
        __syncthreads();
    }
}

// (n_c n_a + bg (1 - n_a)) 255 in fp64, truncated to a byte
__device__ __forceinline__ unsigned composite_byte(unsigned c, double na, double bg) {
    const double nc = (double)c / 255.0;
    const double t0 = nc * na;
    const double t1 = bg * (1.0 - na);
    const double v = (t0 + t1) * 255.0;
    return (unsigned)(int)v & 255u;
}

// then byte / 255 in fp32
__device__ __forceinline__ float composite(unsigned c, double na, double bg) {
    return (float)composite_byte(c, na, bg) / 255.0f;
}

// four pixels of a (.., C) byte image as RGBA words (alpha 255 for C = 3); src may start at any byte for C = 3
template <int C>
__device__ __forceinline__ void load4_rgba(const unsigned char* src, unsigned px[4]) {
    if (C == 4) {
        const dgm_u4u v = *(const dgm_u4u*)src;
        px[0] = v.x, px[1] = v.y, px[2] = v.z, px[3] = v.w;
    } else {
        const unsigned w0 = *(const dgm_u32b*)src, w1 = *(const dgm_u32b*)(src + 4), w2 = *(const dgm_u32b*)(src + 8);
        px[0] = (w0 & 0xffffffu) | 0xff000000u;
        px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8) | 0xff000000u;
        px[2] = (w1 >> 16) | ((w2 & 0xffu) << 16) | 0xff000000u;
        px[3] = (w2 >> 8) | 0xff000000u;
    }
}

template <int C>
__global__ __launch_bounds__(256) void image_ingest_kernel(long long HW, const unsigned char* __restrict__ in, double bg0, double bg1,
                                                           double bg2, float* __restrict__ image, float* __restrict__ mask) {
    const long long n0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= HW) return;
    const size_t b = blockIdx.y;
    const unsigned char* src = in + (b * (size_t)HW + (size_t)n0) * C;
    float* img = image + b * 3 * (size_t)HW + (size_t)n0;
    float* msk = mask + b * (size_t)HW + (size_t)n0;
    const double bg[3] = {bg0, bg1, bg2};
    if (n0 + 4 <= HW) {
        unsigned px[4];
        load4_rgba<C>(src, px);
        double na[4];
        dgm_f4u m;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            na[k] = (double)(px[k] >> 24) / 255.0;
            m[k] = (float)na[k];
        }
        *(dgm_f4u*)msk = m;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            dgm_f4u o;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = composite((px[k] >> (8 * c)) & 255u, na[k], bg[c]);
            *(dgm_f4u*)(img + (size_t)c * HW) = o;
        }
    } else {  // the last one to three pixels of an image whose pixel count is no multiple of four
        for (long long k = 0; n0 + k < HW; k++) {
            const unsigned char* p = src + k * C;
            const double na = (double)(C == 4 ? (unsigned)p[3] : 255u) / 255.0;
            msk[k] = (float)na;
            for (int c = 0; c < 3; c++) img[(size_t)c * HW + k] = composite((unsigned)p[c], na, bg[c]);
        }
    }
}

// the composited bytes themselves, with the file's alpha beside them: what the `resolution` resize takes (csrc/resample.hip)
template <int C>
__global__ __launch_bounds__(256) void image_composite_kernel(long long HW, const unsigned char* __restrict__ in, double bg0, double bg1,
                                                              double bg2, unsigned char* __restrict__ out) {
    const long long n0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= HW) return;
    const size_t b = blockIdx.y;
    const unsigned char* src = in + (b * (size_t)HW + (size_t)n0) * C;
    unsigned* dst = (unsigned*)out + b * (size_t)HW + (size_t)n0;
    const double bg[3] = {bg0, bg1, bg2};
    if (n0 + 4 <= HW) {
        unsigned px[4];
        load4_rgba<C>(src, px);
        dgm_u4u o;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double na = (double)(px[k] >> 24) / 255.0;
            unsigned w = px[k] & 0xff000000u;
#pragma unroll
            for (int c = 0; c < 3; c++) w |= composite_byte((px[k] >> (8 * c)) & 255u, na, bg[c]) << (8 * c);
            o[k] = w;
        }
        *(dgm_u4u*)dst = o;
    } else {
        for (long long k = 0; n0 + k < HW; k++) {
            const unsigned char* p = src + k * C;
            const unsigned a = C == 4 ? (unsigned)p[3] : 255u;
            const double na = (double)a / 255.0;
            unsigned w = a << 24;
            for (int c = 0; c < 3; c++) w |= composite_byte((unsigned)p[c], na, bg[c]) << (8 * c);
            dst[k] = w;
        }
    }
}

// one byte per pixel from rows of ceil(W depth / 8) packed bytes; the bits past a row's last pixel are never looked at
__global__ __launch_bounds__(256) void png_expand_kernel(long long HW, int W, int depth, unsigned scale, const unsigned char* __restrict__ in,
                                                         unsigned char* __restrict__ out) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= HW) return;
    const size_t b = blockIdx.y;
    const long long y = n / W;
    const long long bit = (n - y * W) * depth;
    const size_t row_bytes = ((size_t)W * depth + 7) >> 3;
    const size_t H = (size_t)(HW / W);
    const unsigned byte = in[(b * H + (size_t)y) * row_bytes + (size_t)(bit >> 3)];
    const unsigned v = (byte >> (8 - depth - (int)(bit & 7))) & ((1u << depth) - 1u);
    out[b * (size_t)HW + (size_t)n] = (unsigned char)(v * scale);
}

// the frame where the mask's channel 0 is set, the background's byte elsewhere.  BYTES: (R, G, B, 255 (m > 0)) words; otherwise the
// planes image = byte / 255 (the division of image_ingest_kernel) and alpha = m > 0
template <int C, bool BYTES>
__global__ __launch_bounds__(256) void image_ingest_masked_kernel(long long HW, const unsigned char* __restrict__ in, int Cm,
                                                                  const unsigned char* __restrict__ mask, double bg0, double bg1, double bg2,
                                                                  float* __restrict__ image, float* __restrict__ alpha,
                                                                  unsigned char* __restrict__ bytes_out) {
    const long long n0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= HW) return;
    const size_t b = blockIdx.y;
    const size_t at = b * (size_t)HW + (size_t)n0;
    const unsigned char* src = in + at * C;
    const unsigned char* msrc = mask + at * (size_t)Cm;
    const unsigned bgb[3] = {composite_byte(0u, 0.0, bg0), composite_byte(0u, 0.0, bg1), composite_byte(0u, 0.0, bg2)};
    const unsigned bgw = bgb[0] | (bgb[1] << 8) | (bgb[2] << 16);
    if (n0 + 4 <= HW) {
        unsigned px[4];
        load4_rgba<C>(src, px);
        bool on[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            on[k] = msrc[(size_t)k * Cm] != 0;
            px[k] = on[k] ? ((px[k] & 0xffffffu) | 0xff000000u) : bgw;
        }
        if (BYTES) {
            dgm_u4u o;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = px[k];
            *(dgm_u4u*)((unsigned*)bytes_out + at) = o;
        } else {
            dgm_f4u m;
#pragma unroll
            for (int k = 0; k < 4; k++) m[k] = on[k] ? 1.0f : 0.0f;
            *(dgm_f4u*)(alpha + at) = m;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                dgm_f4u o;
#pragma unroll
                for (int k = 0; k < 4; k++) o[k] = (float)((px[k] >> (8 * c)) & 255u) / 255.0f;
                *(dgm_f4u*)(image + b * 3 * (size_t)HW + (size_t)c * HW + (size_t)n0) = o;
            }
        }
    } else {  // the last one to three pixels of an image whose pixel count is no multiple of four
        for (long long k = 0; n0 + k < HW; k++) {
            const unsigned char* p = src + k * C;
            const bool on = msrc[(size_t)k * Cm] != 0;
            const unsigned w = on ? ((unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | 0xff000000u) : bgw;
            if (BYTES) {
                ((unsigned*)bytes_out)[at + k] = w;
            } else {
                alpha[at + k] = on ? 1.0f : 0.0f;
                for (int c = 0; c < 3; c++) image[b * 3 * (size_t)HW + (size_t)c * HW + (size_t)(n0 + k)] = (float)((w >> (8 * c)) & 255u) / 255.0f;
            }
        }
    }
}

static int launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        static thread_local char m[256];
        snprintf(m, sizeof m, "%s: %s", what, hipGetErrorString(e));
        set_last_error(m);
        return 1;
    }
    return 0;
}

}  // namespace dgm

using namespace dgm;

extern "C" {

int dgm_png_unfilter(int B, int W, int H, int channels, const unsigned char* filtered, unsigned char* out, void* stream) {
    if (B < 1 || W < 1 || H < 1 || W > (1 << 24) || H > (1 << 24) || (channels != 1 && channels != 3 && channels != 4) || !filtered || !out ||
        (channels != 1 && ((uintptr_t)out & 3))) {
        set_last_error("png_unfilter: bad argument (B >= 1, 1 <= W, H <= 2^24, channels 1, 3 or 4, no null pointer, out 4-byte aligned "
                       "unless channels is 1)");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    if (channels == 4)
        hipLaunchKernelGGL(png_unfilter_kernel<4>, dim3(B), dim3(UF_ROWS), 0, st, W, H, filtered, out);
    else if (channels == 1)
        hipLaunchKernelGGL(png_unfilter_kernel<1>, dim3(B), dim3(UF_ROWS), 0, st, W, H, filtered, out);
    else
        hipLaunchKernelGGL(png_unfilter_kernel<3>, dim3(B), dim3(UF_ROWS), 0, st, W, H, filtered, out);
    return launch_status("png_unfilter");
}

int dgm_image_ingest(int B, int H, int W, int C, const unsigned char* in, const float* bg3, float* image, float* mask, void* stream) {
    if (B < 1 || B > 65535 || W < 1 || H < 1 || W > (1 << 24) || H > (1 << 24) || (C != 3 && C != 4) || !in || !bg3 || !image || !mask ||
        (C == 4 && ((uintptr_t)in & 3)) || ((uintptr_t)image & 3) || ((uintptr_t)mask & 3)) {
        set_last_error("image_ingest: bad argument (1 <= B <= 65535, 1 <= W, H <= 2^24, C 3 or 4, no null pointer, image and mask 4-byte "
                       "aligned, in 4-byte aligned when C is 4)");
        return 1;
    }
    const long long HW = (long long)H * W;
    const long long blocks = ((HW + 3) / 4 + 255) / 256;
    if (blocks > 0x7fffffffLL) {
        set_last_error("image_ingest: image too large");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks, (unsigned)B);
    if (C == 4)
        hipLaunchKernelGGL(image_ingest_kernel<4>, grid, dim3(256), 0, st, HW, in, (double)bg3[0], (double)bg3[1], (double)bg3[2], image, mask);
    else
        hipLaunchKernelGGL(image_ingest_kernel<3>, grid, dim3(256), 0, st, HW, in, (double)bg3[0], (double)bg3[1], (double)bg3[2], image, mask);
    return launch_status("image_ingest");
}

int dgm_image_composite_bytes(int B, int H, int W, int C, const unsigned char* in, const float* bg3, unsigned char* out, void* stream) {
    if (B < 1 || B > 65535 || W < 1 || H < 1 || W > (1 << 24) || H > (1 << 24) || (C != 3 && C != 4) || !in || !bg3 || !out ||
        (C == 4 && ((uintptr_t)in & 3)) || ((uintptr_t)out & 3)) {
        set_last_error("image_composite_bytes: bad argument (1 <= B <= 65535, 1 <= W, H <= 2^24, C 3 or 4, no null pointer, out 4-byte "
                       "aligned, in 4-byte aligned when C is 4)");
        return 1;
    }
    const long long HW = (long long)H * W;
    const long long blocks = ((HW + 3) / 4 + 255) / 256;
    if (blocks > 0x7fffffffLL) {
        set_last_error("image_composite_bytes: image too large");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks, (unsigned)B);
    if (C == 4)
        hipLaunchKernelGGL(image_composite_kernel<4>, grid, dim3(256), 0, st, HW, in, (double)bg3[0], (double)bg3[1], (double)bg3[2], out);
    else
        hipLaunchKernelGGL(image_composite_kernel<3>, grid, dim3(256), 0, st, HW, in, (double)bg3[0], (double)bg3[1], (double)bg3[2], out);
    return launch_status("image_composite_bytes");
}

int dgm_png_expand(int B, int W, int H, int depth, int scale, const unsigned char* packed, unsigned char* out, void* stream) {
    if (B < 1 || B > 65535 || W < 1 || H < 1 || W > (1 << 24) || H > (1 << 24) || (depth != 1 && depth != 2 && depth != 4 && depth != 8) ||
        scale < 1 || (long long)scale * ((1 << depth) - 1) > 255 || !packed || !out) {
        set_last_error("png_expand: bad argument (1 <= B <= 65535, 1 <= W, H <= 2^24, depth 1, 2, 4 or 8, scale >= 1 with "
                       "scale (2^depth - 1) <= 255, no null pointer)");
        return 1;
    }
    const long long HW = (long long)H * W;
    const long long blocks = (HW + 255) / 256;
    if (blocks > 0x7fffffffLL) {
        set_last_error("png_expand: image too large");
        return 1;
    }
    hipLaunchKernelGGL(png_expand_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, (hipStream_t)stream, HW, W, depth, (unsigned)scale,
                       packed, out);
    return launch_status("png_expand");
}

int dgm_image_ingest_masked(int B, int H, int W, int C, const unsigned char* in, int Cm, const unsigned char* mask, const float* bg3, int flags,
                            float* image, float* alpha, unsigned char* bytes_out, void* stream) {
    const bool bytes = (flags & DGM_INGEST_BYTES) != 0;
    if (B < 1 || B > 65535 || W < 1 || H < 1 || W > (1 << 24) || H > (1 << 24) || (C != 3 && C != 4) || (Cm != 1 && Cm != 3 && Cm != 4) ||
        (flags & ~DGM_INGEST_BYTES) || !in || !mask || !bg3 || (C == 4 && ((uintptr_t)in & 3)) ||
        (bytes ? (!bytes_out || ((uintptr_t)bytes_out & 3)) : (!image || !alpha || ((uintptr_t)image & 3) || ((uintptr_t)alpha & 3)))) {
        set_last_error("image_ingest_masked: bad argument (1 <= B <= 65535, 1 <= W, H <= 2^24, C 3 or 4, Cm 1, 3 or 4, flags 0 or "
                       "DGM_INGEST_BYTES, no null pointer among in, mask, bg3 and the selected output, outputs 4-byte aligned, in 4-byte "
                       "aligned when C is 4)");
        return 1;
    }
    const long long HW = (long long)H * W;
    const long long blocks = ((HW + 3) / 4 + 255) / 256;
    if (blocks > 0x7fffffffLL) {
        set_last_error("image_ingest_masked: image too large");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)blocks, (unsigned)B);
    const double b0 = (double)bg3[0], b1 = (double)bg3[1], b2 = (double)bg3[2];
    if (C == 4 && bytes)
        hipLaunchKernelGGL((image_ingest_masked_kernel<4, true>), grid, dim3(256), 0, st, HW, in, Cm, mask, b0, b1, b2, image, alpha, bytes_out);
    else if (C == 4)
        hipLaunchKernelGGL((image_ingest_masked_kernel<4, false>), grid, dim3(256), 0, st, HW, in, Cm, mask, b0, b1, b2, image, alpha, bytes_out);
    else if (bytes)
        hipLaunchKernelGGL((image_ingest_masked_kernel<3, true>), grid, dim3(256), 0, st, HW, in, Cm, mask, b0, b1, b2, image, alpha, bytes_out);
    else
        hipLaunchKernelGGL((image_ingest_masked_kernel<3, false>), grid, dim3(256), 0, st, HW, in, Cm, mask, b0, b1, b2, image, alpha, bytes_out);
    return launch_status("image_ingest_masked");
}

}  // extern "C"
