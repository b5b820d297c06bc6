// Looking at a trained checkpoint on gfx950: the passes behind dg-mesh_amd/visualize.py.  They stand where the reference's
// render_test.py / render_trajectory.py (R/ = dgmesh/) use PyTorch3D's Phong shader (mesh_shape_renderer, R/utils/renderer.py:236-319),
// a matplotlib scatter on the host (pointcloud_renderer, :322-374) and numpy / cv2 frame composition.  Neither package is vendored:
// the conventions are this project's (dg-mesh_amd/visualize.py states them).
//
//   vertex normals : one thread per face adds its unnormalised cross product (v1 - v0) x (v2 - v0) to its three vertices (fp32
//                    atomicAdd: the sums agree to rounding run to run), one thread per vertex normalises (length < 1e-6 -> 0).
//   shade          : one thread per pixel of the rasterizer's rast buffer (u, v, z/w, id + 1): hard Phong with one directional light.
//   point splat    : one thread per point does a 64-bit atomicMin of (ordered z/w bits) << 32 | point id on every pixel of its
//                    size x size square (the triangle rasterizer's visibility scheme: the winner does not depend on arrival order);
//                    one thread per pixel then turns the winning id into a colour.  Bit-reproducible.
//   compose        : one thread per output pixel: up to four fp32 panels side by side, an optional 2 x 2 average, -> uint8.
//
// All four are memory-bound with a few dozen flops per element; nothing is staged in LDS.  Compiled without FMA contraction and
// with correctly rounded / and sqrt (the point splat must land on the pixels mesh_raster.hip's screen mapping gives, and the
// bytes of compose are checked against a numpy restatement).
#include "dgm_host.hpp"

#include <math.h>

using namespace dgm;

namespace {

constexpr int VZ_THREADS = 256;
constexpr int VZ_MAX_DIM = 16384;  // H, W limit, as the mesh rasterizer: H * W and every pixel index stay inside int32
constexpr int VZ_MAX_PANELS = 4;
constexpr unsigned long long KEY_EMPTY = ~0ull;


__device__ __forceinline__ bool face_in_range(const int* __restrict__ tri, int f, int V, int (&v)[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = tri[(size_t)f * 3 + k];
    return (unsigned)v[0] < (unsigned)V && (unsigned)v[1] < (unsigned)V && (unsigned)v[2] < (unsigned)V;
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// ---- vertex normals -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(VZ_THREADS)
normals_scatter_kernel(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, float* __restrict__ normals) {
    const int f = blockIdx.x * VZ_THREADS + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!face_in_range(faces, f, V, v)) return;
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int c = 0; c < 3; c++) p[k][c] = verts[(size_t)v[k] * 3 + c];
    const float ax = p[1][0] - p[0][0], ay = p[1][1] - p[0][1], az = p[1][2] - p[0][2];
    const float bx = p[2][0] - p[0][0], by = p[2][1] - p[0][1], bz = p[2][2] - p[0][2];
    const float n[3] = {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            if (n[c] != 0.f) atomicAdd(normals + (size_t)v[k] * 3 + c, n[c]);
}

__global__ void __launch_bounds__(VZ_THREADS)
normals_normalize_kernel(int V, float* __restrict__ normals) {
    const int i = blockIdx.x * VZ_THREADS + threadIdx.x;
    if (i >= V) return;
    float* n = normals + (size_t)i * 3;
    const float x = n[0], y = n[1], z = n[2];
    const float len = sqrtf(dot3(x, y, z, x, y, z));
    const bool ok = len >= 1e-6f;  // (NaN: not ok)
    n[0] = ok ? x / len : 0.f, n[1] = ok ? y / len : 0.f, n[2] = ok ? z / len : 0.f;
}

// ---- shade ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

__global__ void __launch_bounds__(VZ_THREADS)
shade_kernel(int V, int F, int HW, const float* __restrict__ verts, const float* __restrict__ normals, const int* __restrict__ faces,
             const float4* __restrict__ rast, const dgm_shade_params* __restrict__ params, float* __restrict__ image) {
    const int p = blockIdx.x * VZ_THREADS + threadIdx.x;
    if (p >= HW) return;
    const dgm_shade_params P = *params;  // (uniform: scalar loads)
    const float4 r = rast[p];
    float* o = image + (size_t)p * 3;
    const int id = (int)r.w;
    int v[3];
    if (id < 1 || id > F || !face_in_range(faces, id - 1, V, v)) {
        o[0] = P.background[0], o[1] = P.background[1], o[2] = P.background[2];
        return;
    }
    const float u = r.x, w1 = r.y, w2 = 1.f - r.x - r.y;
    float pos[3], n[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        pos[c] = (u * verts[(size_t)v[0] * 3 + c] + w1 * verts[(size_t)v[1] * 3 + c]) + w2 * verts[(size_t)v[2] * 3 + c];
        n[c] = ((u * normals[(size_t)v[0] * 3 + c] + w1 * normals[(size_t)v[1] * 3 + c]) + w2 * normals[(size_t)v[2] * 3 + c]) * P.normal_sign;
    }
    const float nlen = sqrtf(dot3(n[0], n[1], n[2], n[0], n[1], n[2]));
    const bool nok = nlen >= 1e-6f;
#pragma unroll
    for (int c = 0; c < 3; c++) n[c] = nok ? n[c] / nlen : 0.f;
    const float ndl = dot3(n[0], n[1], n[2], P.light_dir[0], P.light_dir[1], P.light_dir[2]);
    const float diffuse = fmaxf(ndl, 0.f);
    float spec = 0.f;
    if (ndl > 0.f) {
        float view[3], refl[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            view[c] = P.camera_center[c] - pos[c];
            refl[c] = (2.f * ndl) * n[c] - P.light_dir[c];
        }
        const float vlen = sqrtf(dot3(view[0], view[1], view[2], view[0], view[1], view[2]));
        if (vlen > 0.f) {
            const float vdr = fmaxf(dot3(view[0] / vlen, view[1] / vlen, view[2] / vlen, refl[0], refl[1], refl[2]), 0.f);
            spec = powf(vdr, P.shininess);
        }
    }
    const float lit = P.ambient + P.diffuse * diffuse, hl = P.specular * spec;
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = clamp01(lit * P.base_color[c] + hl);
}

// ---- point splat ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long depth_key(float zw, unsigned id) {  // (mesh_raster.hip's key)
    unsigned u = __float_as_uint(zw);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | id;
}

__global__ void __launch_bounds__(VZ_THREADS)
splat_points_kernel(int N, int H, int W, int half, const float4* __restrict__ pos, unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * VZ_THREADS + threadIdx.x;
    if (i >= N) return;
    const float4 p = pos[i];
    if (!(p.w > 0.f) || !isfinite(p.x) || !isfinite(p.y) || !isfinite(p.z) || !isfinite(p.w)) return;
    const float sx = (p.x / p.w + 1.f) * (0.5f * (float)W), sy = (p.y / p.w + 1.f) * (0.5f * (float)H), zw = p.z / p.w;
    if (!isfinite(sx) || !isfinite(sy) || !isfinite(zw)) return;
    const float fx = floorf(sx), fy = floorf(sy);
    // the centre pixel may lie outside the image while its square still reaches in; beyond that the point is dropped (and the
    // conversions below stay inside int)
    if (fx < (float)(-half) || fx > (float)(W - 1 + half) || fy < (float)(-half) || fy > (float)(H - 1 + half)) return;
    const int cx = (int)fx, cy = (int)fy;
    const int x0 = max(cx - half, 0), x1 = min(cx + half, W - 1), y0 = max(cy - half, 0), y1 = min(cy + half, H - 1);
    const unsigned long long key = depth_key(zw, (unsigned)i);
    for (int y = y0; y <= y1; y++)
        for (int x = x0; x <= x1; x++) atomicMin(keys + (size_t)y * W + x, key);
}

struct SplatColors {
    float bg[3], uniform[3];
};

__global__ void __launch_bounds__(VZ_THREADS)
splat_resolve_kernel(int N, int HW, const unsigned long long* __restrict__ keys, const float* __restrict__ colors, const SplatColors sc,
                     float* __restrict__ image) {
    const int p = blockIdx.x * VZ_THREADS + threadIdx.x;
    if (p >= HW) return;
    const unsigned long long key = keys[p];
    float* o = image + (size_t)p * 3;
    const unsigned id = (unsigned)(key & 0xffffffffu);
    if (key == KEY_EMPTY || id >= (unsigned)N) {
        o[0] = sc.bg[0], o[1] = sc.bg[1], o[2] = sc.bg[2];
    } else if (colors) {
        o[0] = colors[(size_t)id * 3], o[1] = colors[(size_t)id * 3 + 1], o[2] = colors[(size_t)id * 3 + 2];
    } else {
        o[0] = sc.uniform[0], o[1] = sc.uniform[1], o[2] = sc.uniform[2];
    }
}

// ---- compose --------------------------------------------------------------------------------------------------------------------
struct Panels {
    const float* ptr[VZ_MAX_PANELS];
    int hwc[VZ_MAX_PANELS];
};

__device__ __forceinline__ float panel_at(const float* __restrict__ s, int hwc, int H, int W, int c, int y, int x) {
    return hwc ? s[((size_t)y * W + x) * 3 + c] : s[((size_t)c * H + y) * W + x];
}

__global__ void __launch_bounds__(VZ_THREADS)
compose_kernel(const Panels pn, int n, int H, int W, int d, unsigned char* __restrict__ out) {
    const int Ho = H / d, Wo = W / d;
    const long long t = (long long)blockIdx.x * VZ_THREADS + threadIdx.x;
    if (t >= (long long)Ho * Wo * n) return;
    const int oy = (int)(t / ((long long)Wo * n)), xx = (int)(t - (long long)oy * Wo * n);
    const int k = xx / Wo, ox = xx - k * Wo;
    const float* s = pn.ptr[k];
    const int hwc = pn.hwc[k];
    unsigned char* o = out + (size_t)t * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float v;
        if (d == 1) {
            v = panel_at(s, hwc, H, W, c, oy, ox);
        } else {
            const float a = panel_at(s, hwc, H, W, c, 2 * oy, 2 * ox), b = panel_at(s, hwc, H, W, c, 2 * oy, 2 * ox + 1);
            const float e = panel_at(s, hwc, H, W, c, 2 * oy + 1, 2 * ox), g = panel_at(s, hwc, H, W, c, 2 * oy + 1, 2 * ox + 1);
            v = ((a + b) + (e + g)) * 0.25f;
        }
        v = clamp01(v) * 255.f;  // (fmaxf(NaN, 0) = 0: NaN writes 0)
        o[c] = (unsigned char)(int)v;
    }
}

bool vz_dims(int H, int W) { return H > 0 && W > 0 && H <= VZ_MAX_DIM && W <= VZ_MAX_DIM; }

}  // namespace

extern "C" {

int dgm_vertex_normals(int V, int F, const float* verts, const int* faces, float* normals, void* stream) {
    if (V < 0 || F < 0) return fail("vertex_normals: need V >= 0 and F >= 0");
    if ((V > 0 && (!verts || !normals)) || (F > 0 && !faces)) return fail("vertex_normals: NULL pointer");
    if (V == 0) return launch_status();
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(normals, 0, (size_t)V * 3 * sizeof(float), st) != hipSuccess) return fail("vertex_normals: memset failed");
    if (F > 0) {
        hipLaunchKernelGGL(normals_scatter_kernel, dim3(blocks(F)), dim3(VZ_THREADS), 0, st, V, F, verts, faces, normals);
        hipLaunchKernelGGL(normals_normalize_kernel, dim3(blocks(V)), dim3(VZ_THREADS), 0, st, V, normals);
    }
    return launch_status();
}

int dgm_mesh_shade(int V, int F, int H, int W, const float* verts, const float* normals, const int* faces, const float* rast,
                   const dgm_shade_params* params, float* image, void* stream) {
    if (V < 0 || F < 0 || !vz_dims(H, W)) return fail("mesh_shade: need V >= 0, F >= 0 and 0 < H, W <= 16384");
    if (!rast || !params || !image || (V > 0 && (!verts || !normals)) || (F > 0 && !faces)) return fail("mesh_shade: NULL pointer");
    hipLaunchKernelGGL(shade_kernel, dim3(blocks((long long)H * W)), dim3(VZ_THREADS), 0, (hipStream_t)stream, V, F, H * W, verts, normals,
                       faces, (const float4*)rast, params, image);
    return launch_status();
}

size_t dgm_point_splat_scratch_bytes(int H, int W) {
    return vz_dims(H, W) ? align_up((size_t)H * W * sizeof(unsigned long long), 256) : 0;
}

int dgm_point_splat(int N, int H, int W, const float* pos_clip, const float* colors, int size, const float* bg_color6, char* scratch,
                    float* image, void* stream) {
    if (N < 0 || !vz_dims(H, W)) return fail("point_splat: need N >= 0 and 0 < H, W <= 16384");
    if (size < 1 || size > 15 || !(size & 1)) return fail("point_splat: size must be odd, 1 to 15");
    if (!bg_color6 || !scratch || !image || (N > 0 && !pos_clip)) return fail("point_splat: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)scratch;
    if (hipMemsetAsync(keys, 0xff, (size_t)H * W * sizeof(unsigned long long), st) != hipSuccess) return fail("point_splat: memset failed");
    if (N > 0)
        hipLaunchKernelGGL(splat_points_kernel, dim3(blocks(N)), dim3(VZ_THREADS), 0, st, N, H, W, size / 2, (const float4*)pos_clip, keys);
    SplatColors sc;
    for (int c = 0; c < 3; c++) sc.bg[c] = bg_color6[c], sc.uniform[c] = bg_color6[3 + c];
    hipLaunchKernelGGL(splat_resolve_kernel, dim3(blocks((long long)H * W)), dim3(VZ_THREADS), 0, st, N, H * W,
                       (const unsigned long long*)keys, colors, sc, image);
    return launch_status();
}

int dgm_compose_frame(int n_panels, const float* const* panels, const int* layouts, int H, int W, int downsample, unsigned char* out_u8,
                      void* stream) {
    if (n_panels < 1 || n_panels > VZ_MAX_PANELS) return fail("compose_frame: 1 to 4 panels");
    if (!vz_dims(H, W) || (downsample != 1 && downsample != 2)) return fail("compose_frame: need 0 < H, W <= 16384 and downsample 1 or 2");
    if (downsample == 2 && ((H | W) & 1)) return fail("compose_frame: downsample 2 needs even H and W");
    if (!panels || !layouts || !out_u8) return fail("compose_frame: NULL pointer");
    Panels pn;
    for (int k = 0; k < VZ_MAX_PANELS; k++) {
        pn.ptr[k] = k < n_panels ? panels[k] : nullptr;
        pn.hwc[k] = k < n_panels ? layouts[k] : 0;
        if (k < n_panels && (!pn.ptr[k] || (pn.hwc[k] != 0 && pn.hwc[k] != 1))) return fail("compose_frame: NULL panel or a layout other than 0 / 1");
    }
    const long long n = (long long)(H / downsample) * (W / downsample) * n_panels;
    hipLaunchKernelGGL(compose_kernel, dim3(blocks(n)), dim3(VZ_THREADS), 0, (hipStream_t)stream, pn, n_panels, H, W, downsample, out_u8);
    return launch_status();
}

}  // extern "C"
