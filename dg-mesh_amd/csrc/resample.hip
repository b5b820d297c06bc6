// Image resampling for gfx950: Pillow's 8-bit Image.resize (Lanczos, bicubic; any separable filter the host tabulates) on the device.
//
// Replaces image.resize(..., LANCZOS) of readCamerasFromTransforms (R/scene/dataset_readers.py:289) and the bicubic resize of
// PILtoTorch (R/utils/general_utils.py:23-29), R/ = dgmesh/.  The arithmetic is Pillow's and is all integer: the host turns the filter
// into fixed-point taps (resample.coefficients), an output byte is clamp((2^21 + sum pixel * tap) >> 22, 0, 255) with an int32
// accumulator; a horizontal pass, a byte intermediate, a vertical pass, either skipped when its axis keeps its size.
//
//   both kernels    : a block is 4 waves, one image row each; a lane owns FOUR neighbouring output pixels of its row, so lanes run
//                     along x, a wave stores 64 x 4 C contiguous bytes (16 bytes a lane for RGBA) or, as planes, 16 bytes a lane
//                     per channel.
//   horizontal      : the taps come tap-major, (ksize, ow padded to 4): a lane reads its four pixels' k-th taps as one 16-byte word,
//                     a wave 1 KiB contiguous.  The input is gathered a pixel at a time (the four windows start at different
//                     columns); neighbouring lanes' windows overlap, which the vector L1 absorbs.
//   vertical        : the taps and the window of an output row are the same for the whole wave (scalar loads); a lane reads its
//                     four pixels of every input row of the window as 4 C contiguous bytes.
//   premultiplied   : RGBA colour bytes are multiplied by alpha as the first executed pass loads them and divided out as the last
//                     executed pass stores them -- Pillow's RGBA -> RGBa -> resize -> RGBA without the two sweeps.
//
// Built with correctly rounded fp32 division for the planar output, byte / 255.0f, which must equal dgm_image_ingest's.
#include "dgm_common.hpp"

#include <stdio.h>

namespace dgm {


static constexpr int RS_ROWS = 4;        // rows (= waves) per block
static constexpr int RS_PRECISION = 22;  // Pillow's PRECISION_BITS for 8-bit channels

typedef unsigned rs_u4u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned rs_u32b __attribute__((aligned(1)));
typedef int rs_i4 __attribute__((ext_vector_type(4)));

struct ResampleOut {  // where the LAST executed pass writes: bytes, or planes when image != nullptr
    unsigned char* bytes;
    float* image;
    float* mask;
};

// the C bytes of pixel p as a word
template <int C>
__device__ __forceinline__ unsigned rs_load_pixel(const unsigned char* p) {
    if (C == 4) return *(const unsigned*)p;
    if (C == 3) return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
    return (unsigned)p[0];
}

// n <= 4 neighbouring pixels as words; all four in wide loads when n == 4
template <int C>
__device__ __forceinline__ void rs_load4(const unsigned char* src, int n, unsigned px[4]) {
    if (n == 4) {
        if (C == 4) {
            const rs_u4u v = *(const rs_u4u*)src;
            px[0] = v.x, px[1] = v.y, px[2] = v.z, px[3] = v.w;
        } else if (C == 3) {
            const unsigned w0 = *(const rs_u32b*)src, w1 = *(const rs_u32b*)(src + 4), w2 = *(const rs_u32b*)(src + 8);
            px[0] = w0 & 0xffffffu;
            px[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
            px[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
            px[3] = w2 >> 8;
        } else {
            const unsigned w = *(const rs_u32b*)src;
            px[0] = w & 255u, px[1] = (w >> 8) & 255u, px[2] = (w >> 16) & 255u, px[3] = w >> 24;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) px[j] = j < n ? rs_load_pixel<C>(src + (size_t)j * C) : 0u;
    }
}

// Pillow's RGBA -> RGBa for one pixel word: c' = ((t >> 8) + t) >> 8 with t = c a + 128 (its MULDIV255); alpha stays
__device__ __forceinline__ unsigned rs_premultiply(unsigned px) {
    const unsigned a = px >> 24;
    unsigned o = px & 0xff000000u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const unsigned t = ((px >> (8 * c)) & 255u) * a + 128u;
        o |= (((t >> 8) + t) >> 8) << (8 * c);
    }
    return o;
}

// Pillow's RGBa -> RGBA: a copy for alpha 0 and 255, otherwise min(255, 255 c / a) in integers
__device__ __forceinline__ unsigned rs_unpremultiply(unsigned px) {
    const unsigned a = px >> 24;
    if (a == 0u || a == 255u) return px;
    unsigned o = px & 0xff000000u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const unsigned q = (255u * ((px >> (8 * c)) & 255u)) / a;
        o |= (q < 255u ? q : 255u) << (8 * c);
    }
    return o;
}

template <int C>
__device__ __forceinline__ void rs_accumulate(int acc[C], unsigned px, int k) {
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] += (int)((px >> (8 * c)) & 255u) * k;
}

// clamp(acc >> 22, 0, 255) per channel, packed as a pixel word (the accumulator already holds the rounding term 2^21).  Written as
// max(acc, 0), a logical shift and an unsigned min.  In the form ashr-then-clamp hipcc selects gfx950's v_ashr_pk_u8_i32, and on
// the MI355X that gave wrong bytes exactly where an accumulator was negative (Lanczos overshoot next to transparent pixels).
template <int C>
__device__ __forceinline__ unsigned rs_pack(const int acc[C]) {
    unsigned o = 0u;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const unsigned u = (unsigned)(acc[c] < 0 ? 0 : acc[c]) >> RS_PRECISION;
        o |= (u > 255u ? 255u : u) << (8 * c);
    }
    return o;
}

// n <= 4 finished pixels of image b, the first at pixel index n0 of its HWo pixels
template <int C>
__device__ __forceinline__ void rs_store4(unsigned px[4], int n, bool unpremultiply, const ResampleOut& out, size_t b, size_t HWo,
                                          size_t n0) {
    if (C == 4 && unpremultiply) {
#pragma unroll
        for (int j = 0; j < 4; j++) px[j] = rs_unpremultiply(px[j]);
    }
    if (out.image != nullptr) {  // planes (C is 3 or 4)
        float* img = out.image + b * 3 * HWo + n0;
        float* msk = out.mask + b * HWo + n0;
        dgm_f4u m;
#pragma unroll
        for (int j = 0; j < 4; j++) m[j] = C == 4 ? (float)((double)(px[j] >> 24) / 255.0) : 1.0f;
        if (n == 4) {
            *(dgm_f4u*)msk = m;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (j < n) msk[j] = m[j];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            dgm_f4u o;
#pragma unroll
            for (int j = 0; j < 4; j++) o[j] = (float)((px[j] >> (8 * c)) & 255u) / 255.0f;
            if (n == 4) {
                *(dgm_f4u*)(img + (size_t)c * HWo) = o;
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (j < n) img[(size_t)c * HWo + j] = o[j];
            }
        }
        return;
    }
    unsigned char* dst = out.bytes + (b * HWo + n0) * C;
    if (n == 4) {
        if (C == 4) {
            rs_u4u v;
            v.x = px[0], v.y = px[1], v.z = px[2], v.w = px[3];
            *(rs_u4u*)dst = v;
        } else if (C == 3) {
            *(rs_u32b*)dst = px[0] | (px[1] << 24);
            *(rs_u32b*)(dst + 4) = (px[1] >> 8) | (px[2] << 16);
            *(rs_u32b*)(dst + 8) = (px[2] >> 16) | (px[3] << 8);
        } else {
            *(rs_u32b*)dst = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j < n) {
                if (C == 4) {
                    *(unsigned*)(dst + 4 * j) = px[j];
                } else {
#pragma unroll
                    for (int c = 0; c < C; c++) dst[j * C + c] = (unsigned char)((px[j] >> (8 * c)) & 255u);
                }
            }
        }
    }
}

// in (B, H, W, C) -> (B, H, ow, C) or planes.  grid (ceil(H / 4), ceil(ceil(ow / 4) / 64), B), block (64, 4).
// taps (ksize, owp), bounds (2, owp) with owp = ow rounded up to 4: see include/dgmesh_hip.h
template <int C>
__global__ __launch_bounds__(64 * RS_ROWS) void resample_h_kernel(int H, int W, int ow, int owp, int ksize, const unsigned char* __restrict__ in,
                                                                  const int* __restrict__ taps, const int* __restrict__ bounds,
                                                                  bool premultiply, bool unpremultiply, ResampleOut out) {
    const int x0 = ((int)blockIdx.y * 64 + (int)threadIdx.x) * 4;
    const int y = (int)blockIdx.x * RS_ROWS + (int)threadIdx.y;
    if (x0 >= ow || y >= H) return;
    const size_t b = blockIdx.z;
    const unsigned char* row = in + (b * (size_t)H + (size_t)y) * (size_t)W * C;
    const rs_i4 first = *(const rs_i4*)(bounds + x0);
    int acc[4][C];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int c = 0; c < C; c++) acc[j][c] = 1 << (RS_PRECISION - 1);
    for (int k = 0; k < ksize; k++) {
        const rs_i4 kk = *(const rs_i4*)(taps + (size_t)k * owp + x0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int x = first[j] + k;  // (taps past a window's count are zero: the clamped pixel adds nothing)
            x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
            unsigned px = rs_load_pixel<C>(row + (size_t)x * C);
            if (C == 4 && premultiply) px = rs_premultiply(px);
            rs_accumulate<C>(acc[j], px, kk[j]);
        }
    }
    unsigned px[4];
#pragma unroll
    for (int j = 0; j < 4; j++) px[j] = rs_pack<C>(acc[j]);
    rs_store4<C>(px, ow - x0 < 4 ? ow - x0 : 4, unpremultiply, out, b, (size_t)H * ow, (size_t)y * ow + x0);
}

// in (B, H, W, C) -> (B, oh, W, C) or planes.  grid (ceil(oh / 4), ceil(ceil(W / 4) / 64), B), block (64, 4).
// taps (oh, ksize), bounds (oh, 2) = (first input row, count)
template <int C>
__global__ __launch_bounds__(64 * RS_ROWS) void resample_v_kernel(int H, int W, int oh, int ksize, const unsigned char* __restrict__ in,
                                                                  const int* __restrict__ taps, const int* __restrict__ bounds,
                                                                  bool premultiply, bool unpremultiply, ResampleOut out) {
    const int x0 = ((int)blockIdx.y * 64 + (int)threadIdx.x) * 4;
    const int y = (int)blockIdx.x * RS_ROWS + (int)threadIdx.y;  // the same for a whole wave
    if (x0 >= W || y >= oh) return;
    const size_t b = blockIdx.z;
    const int n = W - x0 < 4 ? W - x0 : 4;
    const int first = bounds[2 * y];
    int count = bounds[2 * y + 1];
    count = count < 0 ? 0 : (count > ksize ? ksize : count);
    const int* kk = taps + (size_t)y * ksize;
    const unsigned char* img = in + b * (size_t)H * W * C + (size_t)x0 * C;
    int acc[4][C];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int c = 0; c < C; c++) acc[j][c] = 1 << (RS_PRECISION - 1);
    for (int k = 0; k < count; k++) {
        int r = first + k;
        r = r < 0 ? 0 : (r > H - 1 ? H - 1 : r);
        const int w = kk[k];
        unsigned px[4];
        rs_load4<C>(img + (size_t)r * W * C, n, px);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (C == 4 && premultiply) px[j] = rs_premultiply(px[j]);
            rs_accumulate<C>(acc[j], px[j], w);
        }
    }
    unsigned px[4];
#pragma unroll
    for (int j = 0; j < 4; j++) px[j] = rs_pack<C>(acc[j]);
    rs_store4<C>(px, n, unpremultiply, out, b, (size_t)oh * W, (size_t)y * W + x0);
}

template <int C>
static void launch_passes(int B, int H, int W, const unsigned char* in, int oh, int ow, const int* kx, const int* bounds_x, int ksize_x,
                          const int* ky, const int* bounds_y, int ksize_y, bool premultiplied, unsigned char* tmp, ResampleOut out,
                          hipStream_t st) {
    const dim3 block(64, RS_ROWS);
    const unsigned xblocks = (unsigned)(((ow + 3) / 4 + 63) / 64);
    const ResampleOut mid = {tmp, nullptr, nullptr};
    if (kx)
        hipLaunchKernelGGL(resample_h_kernel<C>, dim3((unsigned)((H + RS_ROWS - 1) / RS_ROWS), xblocks, (unsigned)B), block, 0, st, H, W, ow,
                           (ow + 3) & ~3, ksize_x, in, kx, bounds_x, premultiplied, premultiplied && !ky, ky ? mid : out);
    if (ky)
        hipLaunchKernelGGL(resample_v_kernel<C>, dim3((unsigned)((oh + RS_ROWS - 1) / RS_ROWS), xblocks, (unsigned)B), block, 0, st, H, ow, oh,
                           ksize_y, kx ? (const unsigned char*)tmp : in, ky, bounds_y, premultiplied && !kx, premultiplied, out);
}

// Pillow's NEAREST (what Image.resize does to modes P and 1 whatever filter is asked for): out[y][x] = in[ys[y]][xs[x]], the index
// tables computed on the host (resample.nearest_indices); indices are clamped into the image
template <int C>
__global__ __launch_bounds__(64 * RS_ROWS) void resample_nearest_kernel(int H, int W, int oh, int ow, const unsigned char* __restrict__ in,
                                                                       const int* __restrict__ xs, const int* __restrict__ ys,
                                                                       unsigned char* __restrict__ out) {
    const int y = (int)blockIdx.x * RS_ROWS + (int)threadIdx.y, x = (int)blockIdx.y * 64 + (int)threadIdx.x;
    if (y >= oh || x >= ow) return;
    const size_t b = blockIdx.z;
    int sx = xs[x], sy = ys[y];
    sx = sx < 0 ? 0 : (sx >= W ? W - 1 : sx);
    sy = sy < 0 ? 0 : (sy >= H ? H - 1 : sy);
    const unsigned char* s = in + ((b * H + (size_t)sy) * W + (size_t)sx) * C;
    unsigned char* d = out + ((b * oh + (size_t)y) * ow + (size_t)x) * C;
#pragma unroll
    for (int c = 0; c < C; c++) d[c] = s[c];
}

}  // namespace dgm

using namespace dgm;

extern "C" int dgm_resample(int B, int H, int W, int C, const unsigned char* in, int oh, int ow, const int* kx, const int* bounds_x,
                            int ksize_x, const int* ky, const int* bounds_y, int ksize_y, int flags, unsigned char* tmp,
                            unsigned char* out_bytes, float* image, float* mask, void* stream) {
    const int LIM = 1 << 20;
    const bool planes = (flags & DGM_RESAMPLE_PLANES) != 0, premultiplied = (flags & DGM_RESAMPLE_PREMULTIPLIED) != 0;
    const char* why = nullptr;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || oh < 1 || ow < 1 || H > LIM || W > LIM || oh > LIM || ow > LIM)
        why = "1 <= B <= 65535 and every size within [1, 2^20]";
    else if (C != 1 && C != 3 && C != 4)
        why = "C is 1, 3 or 4";
    else if (flags & ~(DGM_RESAMPLE_PREMULTIPLIED | DGM_RESAMPLE_PLANES))
        why = "unknown flag";
    else if (premultiplied && C != 4)
        why = "DGM_RESAMPLE_PREMULTIPLIED needs C = 4";
    else if (planes && C == 1)
        why = "DGM_RESAMPLE_PLANES needs C = 3 or 4";
    else if (!in)
        why = "in is null";
    else if (!kx && !ky)
        why = "no pass to run (kx and ky are both null)";
    else if ((!kx && ow != W) || (!ky && oh != H))
        why = "an axis changes its size but has no taps";
    else if ((kx && (!bounds_x || ksize_x < 1 || ksize_x > LIM)) || (ky && (!bounds_y || ksize_y < 1 || ksize_y > LIM)))
        why = "taps without bounds, or a ksize outside [1, 2^20]";
    else if (kx && (((uintptr_t)kx & 15) || ((uintptr_t)bounds_x & 15)))
        why = "kx and bounds_x are 16-byte aligned";
    else if (ky && (((uintptr_t)ky & 3) || ((uintptr_t)bounds_y & 3)))
        why = "ky and bounds_y are 4-byte aligned";
    else if (kx && ky && !tmp)
        why = "both passes run: tmp is needed";
    else if (planes ? (!image || !mask || ((uintptr_t)image & 3) || ((uintptr_t)mask & 3)) : !out_bytes)
        why = planes ? "image and mask are needed, 4-byte aligned" : "out_bytes is null";
    else if (C == 4 && (((uintptr_t)in & 3) || (kx && ky && ((uintptr_t)tmp & 3)) || (!planes && ((uintptr_t)out_bytes & 3))))
        why = "in, tmp and out_bytes are 4-byte aligned when C is 4";
    if (why) {
        static thread_local char m[256];
        snprintf(m, sizeof m, "resample: bad argument (%s)", why);
        set_last_error(m);
        return 1;
    }
    const ResampleOut out = {planes ? nullptr : out_bytes, planes ? image : nullptr, planes ? mask : nullptr};
    hipStream_t st = (hipStream_t)stream;
    if (C == 4)
        launch_passes<4>(B, H, W, in, oh, ow, kx, bounds_x, ksize_x, ky, bounds_y, ksize_y, premultiplied, tmp, out, st);
    else if (C == 3)
        launch_passes<3>(B, H, W, in, oh, ow, kx, bounds_x, ksize_x, ky, bounds_y, ksize_y, false, tmp, out, st);
    else
        launch_passes<1>(B, H, W, in, oh, ow, kx, bounds_x, ksize_x, ky, bounds_y, ksize_y, false, tmp, out, st);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        static thread_local char m[256];
        snprintf(m, sizeof m, "resample: %s", hipGetErrorString(e));
        set_last_error(m);
        return 1;
    }
    return 0;
}

extern "C" int dgm_resample_nearest(int B, int H, int W, int C, const unsigned char* in, int oh, int ow, const int* xs, const int* ys,
                                    unsigned char* out, void* stream) {
    const int LIM = 1 << 20;
    if (B < 1 || B > 65535 || H < 1 || W < 1 || oh < 1 || ow < 1 || H > LIM || W > LIM || oh > LIM || ow > LIM || (C != 1 && C != 3 && C != 4) ||
        !in || !xs || !ys || !out || ((uintptr_t)xs & 3) || ((uintptr_t)ys & 3)) {
        set_last_error("resample_nearest: bad argument (1 <= B <= 65535, every size within [1, 2^20], C 1, 3 or 4, no null pointer, xs and ys "
                       "4-byte aligned)");
        return 1;
    }
    const dim3 grid((unsigned)((oh + RS_ROWS - 1) / RS_ROWS), (unsigned)((ow + 63) / 64), (unsigned)B), block(64, RS_ROWS);
    hipStream_t st = (hipStream_t)stream;
    if (C == 4)
        hipLaunchKernelGGL(resample_nearest_kernel<4>, grid, block, 0, st, H, W, oh, ow, in, xs, ys, out);
    else if (C == 3)
        hipLaunchKernelGGL(resample_nearest_kernel<3>, grid, block, 0, st, H, W, oh, ow, in, xs, ys, out);
    else
        hipLaunchKernelGGL(resample_nearest_kernel<1>, grid, block, 0, st, H, W, oh, ow, in, xs, ys, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        static thread_local char m[256];
        snprintf(m, sizeof m, "resample_nearest: %s", hipGetErrorString(e));
        set_last_error(m);
        return 1;
    }
    return 0;
}
