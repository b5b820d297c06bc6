// Texture sampling and the trivial texture atlas for gfx950 (mesh_raster.texture, mesh_texture.py; DESIGN.md section 4.18;
// include/dgmesh_hip.h states the definitions for the C ABI, tests/_texture_ref.py restates them in numpy).
//
// dgm_tri_texture_forward / _backward: nvdiffrast.torch.texture without mip-maps.  tex (Ht, Wt, C), uv (n, 2), out (n, C), fp32, no FMA
// (this file is built with -ffp-contract=off).  Texel (i, j) is centred at u = (i + .5) / Wt, v = (j + .5) / Ht; row 0 of memory is at
// v = 0.  Per sample and axis (x with Wt, y with Ht alike), W = (float)Wt:
//   wrap     r = u - floorf(u)                 (in [0, 1]: the reduction happens in float, before any conversion to int)
//            linear:  x = r * W - .5f;  x0 = floorf(x);  fx = x - x0;  i0 = (int)x0, i1 = i0 + 1; i0 < 0 -> i0 + Wt; i1 >= Wt -> i1 - Wt
//            nearest: i = (int)floorf(r * W);  i >= Wt -> i - Wt
//   clamp    linear:  x = min(max(u * W - .5f, -1), W);  x0, fx, i0, i1 as above, then both clamped into [0, Wt - 1]
//            nearest: i = (int)floorf(min(max(u * W, -1), W)) clamped into [0, Wt - 1]
//   zero     linear:  x = min(max(u * W - .5f, -2), W + 1);  x0, fx, i0, i1 as above; a texel with an index outside [0, Wt - 1] is not
//            read and counts as 0.   nearest: i = (int)floorf(min(max(u * W, -1), W)); outside -> 0
// so every float that is converted lies within [-2, Wt + 1] and no finite uv of any magnitude can index outside tex.
//   linear, per channel:  gx = 1 - fx, gy = 1 - fy;  w00 = gx * gy, w10 = fx * gy, w01 = gx * fy, w11 = fx * fy   (wIJ: column i_I, row j_J)
//            out = ((w00 * t00 + w10 * t10) + w01 * t01) + w11 * t11          -- the four products and three adds, in this order
//   nearest: out = t(i, j)
// A sample whose u or v is not finite gives 0 in every channel and no gradient.
// Backward: dtex[texel] += wIJ * dout (fp32 atomics on a zeroed dtex: agrees to rounding run to run, as interpolate's dattr; terms that
//   are exactly 0 are skipped, which changes no sum);
//   duv by plain stores:  du = W * sum_c dout_c * (gy * (t10 - t00) + fy * (t11 - t01)),  dv = H * sum_c dout_c * (gx * (t01 - t00) + fx * (t11 - t10)),
//   the sums over c in fp32, from 0, in channel order; texels not read count as 0; zero for nearest and for a non-finite sample.  (clamp:
//   where both indices of an axis clamp to one texel the difference is exactly 0, the derivative of the clamped coordinate.)
// One thread per sample, looping over C; with C == 4 and 16-byte aligned tex and out a texel is one 16-byte access in the forward.  A gather:
// the four texels of neighbouring samples share cache lines when uv is coherent (a rasterized chart); memory-bound otherwise.
//
// dgm_atlas_uv / dgm_atlas_interpolate: the atlas gives every pair of faces one square cell of s = `cell` texels a side, cells_per_row
// = size / s cells a row, L = s - 3.  Faces 2c and 2c + 1 share cell c at cell column c % cells_per_row, cell row c / cells_per_row.  In
// texel-centre index coordinates local to the cell, face 2c has its corners 0, 1, 2 at (0, 0), (L, 0), (0, L) and face 2c + 1 at
// (s - 1, s - 1), (2, s - 1), (s - 1, 2).  A corner at local (i, j) of cell (cx, cy) has u = ((float)(cx * s + i) + .5f) / (float)size, v alike.
// Local texel (i, j) belongs to face 2c when i + j <= s - 2, with b1 = (float)i / (float)L, b2 = (float)j / (float)L; to face 2c + 1 when i + j >= s,
// with b1 = (float)(s - 1 - i) / (float)L, b2 = (float)(s - 1 - j) / (float)L; to nobody on the diagonal i + j = s - 1.  b0 = (1 - b1) - b2.  The
// barycentrics are NOT clamped: the texels of a chart's bilinear footprint that lie outside the triangle hold the affine extrapolation,
// so bilinear sampling inside a chart is exact for anything affine over the face and no dilation pass is needed.
//   out = (b0 * a0 + b1 * a1) + b2 * a2 per channel, face_id = the face;  zeros and -1 on an unowned texel: the diagonal, the margin right of
//   or below the last whole cell, a face >= F, a face with an index outside [0, V) (checked before any use).
// One thread per texel; every texel of out and face_id is written.  No atomics, no scratch, bit-reproducible.
#include <math.h>

#include "dgm_host.hpp"

#pragma clang fp contract(off)

namespace {
using namespace dgm;

constexpr int TX_THREADS = 256;
constexpr int TX_MAX_SIDE = 16384;  // texture and atlas sides: (float)side and every index product below stay exact

enum { TX_WRAP = DGM_TEX_WRAP, TX_CLAMP = DGM_TEX_CLAMP, TX_ZERO = DGM_TEX_ZERO };


__device__ __forceinline__ bool finitef(float x) { return fabsf(x) < INFINITY; }

// One axis of a linear sample (file header): the two texel indices, -1 for "not read, counts as 0", and the weight fx of the second.
__device__ __forceinline__ void axis_linear(float u, int N, int boundary, int& i0, int& i1, float& fx) {
    const float W = (float)N;
    float x;
    if (boundary == TX_WRAP)
        x = (u - floorf(u)) * W - .5f;
    else if (boundary == TX_CLAMP)
        x = fminf(fmaxf(u * W - .5f, -1.f), W);
    else
        x = fminf(fmaxf(u * W - .5f, -2.f), W + 1.f);
    const float x0 = floorf(x);
    fx = x - x0;
    i0 = (int)x0;
    i1 = i0 + 1;
    if (boundary == TX_WRAP) {
        if (i0 < 0) i0 += N;
        if (i1 >= N) i1 -= N;
    } else if (boundary == TX_CLAMP) {
        i0 = min(max(i0, 0), N - 1);
        i1 = min(max(i1, 0), N - 1);
    } else {
        if (i0 < 0 || i0 >= N) i0 = -1;
        if (i1 < 0 || i1 >= N) i1 = -1;
    }
}

// One axis of a nearest sample: the texel index, -1 for "counts as 0".
__device__ __forceinline__ int axis_nearest(float u, int N, int boundary) {
    const float W = (float)N;
    if (boundary == TX_WRAP) {
        int i = (int)floorf((u - floorf(u)) * W);
        return i >= N ? i - N : i;
    }
    const int i = (int)floorf(fminf(fmaxf(u * W, -1.f), W));
    if (boundary == TX_CLAMP) return min(max(i, 0), N - 1);
    return (i < 0 || i >= N) ? -1 : i;
}

struct Taps {
    long long o00, o10, o01, o11;  // texel offsets (in texels), -1: not read
    float fx, fy;
};

__device__ __forceinline__ Taps taps_linear(float u, float v, int Ht, int Wt, int boundary) {
    int i0, i1, j0, j1;
    Taps t;
    axis_linear(u, Wt, boundary, i0, i1, t.fx);
    axis_linear(v, Ht, boundary, j0, j1, t.fy);
    auto at = [&](int i, int j) { return (i < 0 || j < 0) ? -1LL : (long long)j * Wt + i; };
    t.o00 = at(i0, j0);
    t.o10 = at(i1, j0);
    t.o01 = at(i0, j1);
    t.o11 = at(i1, j1);
    return t;
}

__device__ __forceinline__ float blend(float w00, float w10, float w01, float w11, float t00, float t10, float t01, float t11) {
    return ((w00 * t00 + w10 * t10) + w01 * t01) + w11 * t11;
}

// VEC4: C == 4 with 16-byte aligned tex and out
template <bool VEC4>
__global__ void __launch_bounds__(TX_THREADS)
texture_fwd_kernel(int n, int Ht, int Wt, int C, int linear, int boundary, const float* __restrict__ tex, const float* __restrict__ uv,
                   float* __restrict__ out) {
    const long long s = (long long)blockIdx.x * TX_THREADS + threadIdx.x;
    if (s >= n) return;
    const float u = uv[2 * s], v = uv[2 * s + 1];
    float* o = out + s * C;
    const bool ok = finitef(u) && finitef(v);
    if (!linear || !ok) {
        long long at = -1;
        if (ok) {
            const int i = axis_nearest(u, Wt, boundary), j = axis_nearest(v, Ht, boundary);
            if (i >= 0 && j >= 0) at = (long long)j * Wt + i;
        }
        if (VEC4) {
            *(float4*)o = at >= 0 ? *(const float4*)(tex + at * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int c = 0; c < C; c++) o[c] = at >= 0 ? tex[at * C + c] : 0.f;  // ends at the last channel
        }
        return;
    }
    const Taps t = taps_linear(u, v, Ht, Wt, boundary);
    const float gx = 1.f - t.fx, gy = 1.f - t.fy;
    const float w00 = gx * gy, w10 = t.fx * gy, w01 = gx * t.fy, w11 = t.fx * t.fy;
    if (VEC4) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 a = t.o00 >= 0 ? *(const float4*)(tex + t.o00 * 4) : z, b = t.o10 >= 0 ? *(const float4*)(tex + t.o10 * 4) : z;
        const float4 c = t.o01 >= 0 ? *(const float4*)(tex + t.o01 * 4) : z, d = t.o11 >= 0 ? *(const float4*)(tex + t.o11 * 4) : z;
        *(float4*)o = make_float4(blend(w00, w10, w01, w11, a.x, b.x, c.x, d.x), blend(w00, w10, w01, w11, a.y, b.y, c.y, d.y),
                                  blend(w00, w10, w01, w11, a.z, b.z, c.z, d.z), blend(w00, w10, w01, w11, a.w, b.w, c.w, d.w));
    } else {
        for (int c = 0; c < C; c++) {  // ends at the last channel
            const float t00 = t.o00 >= 0 ? tex[t.o00 * C + c] : 0.f, t10 = t.o10 >= 0 ? tex[t.o10 * C + c] : 0.f;
            const float t01 = t.o01 >= 0 ? tex[t.o01 * C + c] : 0.f, t11 = t.o11 >= 0 ? tex[t.o11 * C + c] : 0.f;
            o[c] = blend(w00, w10, w01, w11, t00, t10, t01, t11);
        }
    }
}

// A term that is exactly zero is not added: dtex starts at +0 and x + (+-0) = x, so the sums are the same, and the background pixels of a
// rendered view -- all at uv = (0, 0) with dout = 0 (render_mesh_textured masks them) -- do not queue up on one texel's address.
__device__ __forceinline__ void add_nonzero(float* p, float term) {
    if (term != 0.f) atomicAdd(p, term);  // (NaN != 0: a NaN term is added)
}

// dtex is zero on entry (the launcher's memset); duv is written for every sample
__global__ void __launch_bounds__(TX_THREADS)
texture_bwd_kernel(int n, int Ht, int Wt, int C, int linear, int boundary, const float* __restrict__ tex, const float* __restrict__ uv,
                   const float* __restrict__ dout, float* __restrict__ dtex, float* __restrict__ duv) {
    const long long s = (long long)blockIdx.x * TX_THREADS + threadIdx.x;
    if (s >= n) return;
    const float u = uv[2 * s], v = uv[2 * s + 1];
    const float* g = dout + s * C;
    float du = 0.f, dv = 0.f;
    if (finitef(u) && finitef(v)) {
        if (!linear) {
            const int i = axis_nearest(u, Wt, boundary), j = axis_nearest(v, Ht, boundary);
            if (i >= 0 && j >= 0) {
                float* d = dtex + ((long long)j * Wt + i) * C;
                for (int c = 0; c < C; c++) add_nonzero(d + c, g[c]);  // ends at the last channel
            }
        } else {
            const Taps t = taps_linear(u, v, Ht, Wt, boundary);
            const float gx = 1.f - t.fx, gy = 1.f - t.fy;
            const float w00 = gx * gy, w10 = t.fx * gy, w01 = gx * t.fy, w11 = t.fx * t.fy;
            float su = 0.f, sv = 0.f;
            for (int c = 0; c < C; c++) {  // ends at the last channel
                const float gc = g[c];
                float t00 = 0.f, t10 = 0.f, t01 = 0.f, t11 = 0.f;
                if (t.o00 >= 0) {
                    t00 = tex[t.o00 * C + c];
                    add_nonzero(dtex + t.o00 * C + c, w00 * gc);
                }
                if (t.o10 >= 0) {
                    t10 = tex[t.o10 * C + c];
                    add_nonzero(dtex + t.o10 * C + c, w10 * gc);
                }
                if (t.o01 >= 0) {
                    t01 = tex[t.o01 * C + c];
                    add_nonzero(dtex + t.o01 * C + c, w01 * gc);
                }
                if (t.o11 >= 0) {
                    t11 = tex[t.o11 * C + c];
                    add_nonzero(dtex + t.o11 * C + c, w11 * gc);
                }
                su += gc * (gy * (t10 - t00) + t.fy * (t11 - t01));
                sv += gc * (gx * (t01 - t00) + t.fx * (t11 - t10));
            }
            du = (float)Wt * su;
            dv = (float)Ht * sv;
        }
    }
    duv[2 * s] = du;
    duv[2 * s + 1] = dv;
}

// the corner's texel-centre index along one axis, local to the cell: k = corner 0 / 1 / 2, axis 0 = i, 1 = j (file header)
__device__ __forceinline__ int corner_local(int odd, int k, int axis, int s) {
    const int L = s - 3;
    const int off = (k == 1 + axis) ? L : 0;  // corner 1 moves along i, corner 2 along j
    return odd ? (s - 1) - off : off;
}

__global__ void __launch_bounds__(TX_THREADS) atlas_uv_kernel(int F, int size, int s, int cpr, float* __restrict__ uv) {
    const long long e = (long long)blockIdx.x * TX_THREADS + threadIdx.x;  // (face, corner)
    if (e >= 3LL * F) return;
    const int f = (int)(e / 3), k = (int)(e % 3);
    const int c = f >> 1, odd = f & 1;
    const int cx = c % cpr, cy = c / cpr;
    const float S = (float)size;
    uv[2 * e] = ((float)(cx * s + corner_local(odd, k, 0, s)) + .5f) / S;
    uv[2 * e + 1] = ((float)(cy * s + corner_local(odd, k, 1, s)) + .5f) / S;
}

__global__ void __launch_bounds__(TX_THREADS)
atlas_interp_kernel(int V, int F, int C, int size, int s, int cpr, const float* __restrict__ attr, const int* __restrict__ faces,
                    float* __restrict__ out, int* __restrict__ face_id) {
    const long long p = (long long)blockIdx.x * TX_THREADS + threadIdx.x;
    if (p >= (long long)size * size) return;
    const int x = (int)(p % size), y = (int)(p / size);
    const int cx = x / s, cy = y / s;
    long long f = -1;
    float b1 = 0.f, b2 = 0.f;
    if (cx < cpr && cy < cpr) {
        const int i = x - cx * s, j = y - cy * s;
        const long long c = (long long)cy * cpr + cx;
        const float L = (float)(s - 3);
        if (i + j <= s - 2) {
            f = 2 * c;
            b1 = (float)i / L;
            b2 = (float)j / L;
        } else if (i + j >= s) {
            f = 2 * c + 1;
            b1 = (float)(s - 1 - i) / L;
            b2 = (float)(s - 1 - j) / L;
        }
    }
    int i0 = 0, i1 = 0, i2 = 0;
    if (f >= F) f = -1;
    if (f >= 0) {
        i0 = faces[3 * f];
        i1 = faces[3 * f + 1];
        i2 = faces[3 * f + 2];
        if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) f = -1;
    }
    face_id[p] = (int)f;
    float* o = out + p * C;
    if (f < 0) {
        for (int c = 0; c < C; c++) o[c] = 0.f;  // ends at the last channel
        return;
    }
    const float b0 = (1.f - b1) - b2;
    const float *a0 = attr + (long long)i0 * C, *a1 = attr + (long long)i1 * C, *a2 = attr + (long long)i2 * C;
    for (int c = 0; c < C; c++) o[c] = (b0 * a0[c] + b1 * a1[c]) + b2 * a2[c];  // ends at the last channel
}

const char* texture_args(int n, int Ht, int Wt, int C, int filter, int boundary) {
    if (n < 0 || C < 1) return "tri_texture: need n >= 0 and C >= 1";
    if (Ht < 1 || Wt < 1 || Ht > TX_MAX_SIDE || Wt > TX_MAX_SIDE) return "tri_texture: the texture's sides must be within [1, 16384]";
    if (filter != DGM_TEX_NEAREST && filter != DGM_TEX_LINEAR) return "tri_texture: unknown filter mode";
    if (boundary != TX_WRAP && boundary != TX_CLAMP && boundary != TX_ZERO) return "tri_texture: unknown boundary mode";
    return nullptr;
}

const char* atlas_args(int F, int size, int cell) {
    if (F < 0) return "atlas: need F >= 0";
    if (size < 1 || size > TX_MAX_SIDE) return "atlas: size must be within [1, 16384]";
    if (cell < 4 || cell > size) return "atlas: cell must be within [4, size]";
    const long long cpr = size / cell;
    if (((long long)F + 1) / 2 > cpr * cpr) return "atlas: more face pairs than cells, raise size or lower cell";
    return nullptr;
}

}  // namespace

extern "C" {

int dgm_tri_texture_forward(int n, int Ht, int Wt, int C, int filter, int boundary, const float* tex, const float* uv, float* out, void* stream) {
    if (const char* m = texture_args(n, Ht, Wt, C, filter, boundary)) return fail(m);
    if (n == 0) return 0;  // (before any HIP call)
    if (!tex || !uv || !out) return fail("tri_texture_forward: NULL pointer");
    const unsigned blocks = (unsigned)(((long long)n + TX_THREADS - 1) / TX_THREADS);
    const bool vec4 = C == 4 && !(((uintptr_t)tex | (uintptr_t)out) & 15);
    hipStream_t st = (hipStream_t)stream;
    if (vec4)
        hipLaunchKernelGGL(texture_fwd_kernel<true>, dim3(blocks), dim3(TX_THREADS), 0, st, n, Ht, Wt, C, filter, boundary, tex, uv, out);
    else
        hipLaunchKernelGGL(texture_fwd_kernel<false>, dim3(blocks), dim3(TX_THREADS), 0, st, n, Ht, Wt, C, filter, boundary, tex, uv, out);
    return launch_status();
}

int dgm_tri_texture_backward(int n, int Ht, int Wt, int C, int filter, int boundary, const float* tex, const float* uv, const float* dout,
                             float* dtex, float* duv, void* stream) {
    if (const char* m = texture_args(n, Ht, Wt, C, filter, boundary)) return fail(m);
    if (!dtex) return fail("tri_texture_backward: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(dtex, 0, (size_t)Ht * Wt * C * sizeof(float), st) != hipSuccess) return fail("tri_texture_backward: memset failed");
    if (n == 0) return 0;
    if (!tex || !uv || !dout || !duv) return fail("tri_texture_backward: NULL pointer");
    const unsigned blocks = (unsigned)(((long long)n + TX_THREADS - 1) / TX_THREADS);
    hipLaunchKernelGGL(texture_bwd_kernel, dim3(blocks), dim3(TX_THREADS), 0, st, n, Ht, Wt, C, filter, boundary, tex, uv, dout, dtex, duv);
    return launch_status();
}

int dgm_atlas_uv(int F, int size, int cell, float* uv_out, void* stream) {
    if (const char* m = atlas_args(F, size, cell)) return fail(m);
    if (F == 0) return 0;  // (before any HIP call)
    if (!uv_out) return fail("atlas_uv: NULL pointer");
    const unsigned blocks = (unsigned)((3LL * F + TX_THREADS - 1) / TX_THREADS);
    hipLaunchKernelGGL(atlas_uv_kernel, dim3(blocks), dim3(TX_THREADS), 0, (hipStream_t)stream, F, size, cell, size / cell, uv_out);
    return launch_status();
}

int dgm_atlas_interpolate(int V, int F, int C, int size, int cell, const float* attr, const int* faces, float* out, int* face_id, void* stream) {
    if (const char* m = atlas_args(F, size, cell)) return fail(m);
    if (V < 0 || C < 1) return fail("atlas_interpolate: need V >= 0 and C >= 1");
    if (!out || !face_id || (F > 0 && !faces) || (F > 0 && V > 0 && !attr)) return fail("atlas_interpolate: NULL pointer");
    const unsigned blocks = (unsigned)(((long long)size * size + TX_THREADS - 1) / TX_THREADS);
    hipLaunchKernelGGL(atlas_interp_kernel, dim3(blocks), dim3(TX_THREADS), 0, (hipStream_t)stream, V, F, C, size, cell, size / cell, attr, faces,
                       out, face_id);
    return launch_status();
}

}  // extern "C"
