// Ray casting against a triangle mesh for gfx950: the nearest hit of a ray, any hit of a ray (mesh_ray.py; DESIGN.md section 4.19;
// include/dgmesh_hip.h states the definition).  The reference has no counterpart: it renders by rasterisation only.
//
// The pair test is the watertight one of Woop, Benthin and Wald (JCGT 2013) -- fp32, no FMA (this file is built with
// -ffp-contract=off), / correctly rounded.
// Per ray (o, d), once:
//   kz = the axis of largest |d| (ties: the lowest index);  kx = (kz + 1) mod 3, ky = (kx + 1) mod 3, swapped when d[kz] < 0
//   Sx = d[kx] / d[kz],  Sy = d[ky] / d[kz],  Sz = 1 / d[kz]                                    (|Sx|, |Sy| <= 1)
// Per corner v of a face (A, B, C for the three corners):
//   a = v - o (per axis);  Ax = a[kx] - Sx * a[kz],  Ay = a[ky] - Sy * a[kz],  Az = Sz * a[kz]
// Per face:
//   U = Cx * By - Cy * Bx,  V = Ax * Cy - Ay * Cx,  W = Bx * Ay - By * Ax
//   when U, V or W is exactly 0: all three again in fp64 from the fp32 sheared coordinates (the products are exact, so the signs
//       are); the sign test below reads these fp64 values, so that no sign is lost where the rounding to fp32 underflows; then
//       U, V, W = the fp64 values rounded to fp32
//   miss when one of U, V, W is < 0 and one is > 0
//   det = (U + V) + W;  miss when det == 0
//   t = ((U * Az + V * Bz) + W * Cz) / det;  accepted when t_min <= t < t_max and t is finite
//   bary = (U / det, V / det, W / det)
// An edge shared by two faces gives both the same two rounded products, subtracted in the opposite order: one value is the exact
// negation of the other, so a ray can pass between them on neither side; a zero counts for both.
// A face with an index outside [0, V) (checked before any use) or a non-finite corner coordinate is staged as NaN corners: U, V, W
// and t are then NaN, no comparison holds and the face is never accepted.  A ray with a non-finite component or d = 0 tests nothing.
//
// The answer of a ray is the lexicographic minimum of (t, face index) over the accepted faces -- a minimum over a set, so it does
// not depend on the visiting order, on the batch or on the run; none: face -1, t +inf, bary 0.  dgm_ray_occluded: 1 where the set
// is not empty (the ray stops at its first accepted face).
//
// Two paths, one answer.
//   accel == NULL   a tiled brute force: RC_CHUNK = 256 consecutive faces per LDS tile as three float4 each, one ray per lane,
//       every lane reading the same LDS address (a broadcast), the next tile's face fetched into registers before the pair loop.
//   accel           dgm_ray_build sorts the faces by the 30-bit Morton code of their centroid (faces that can never hit last) and
//       stores, per sorted face, the nine corner coordinates and the original index (three float4), padded with NaN faces to whole
//       chunks of 256, and per chunk the box [lo, hi] of its valid faces' corners and their number.  A workgroup of 256 rays walks
//       the chunks; each lane tests its ray against the chunk's box, and the workgroup stages and tests a chunk only if one of its
//       lanes may hit it.  The candidates carry the original index, so the minimum is over the same set with the same keys.
//
// The box test rejects a chunk for a ray only if the pair test accepts none of the chunk's faces for it.  With the box [lo, hi]:
//   zl = lo[kz] - o[kz], zh = hi[kz] - o[kz], and alike xl, xh, yl, yh on kx and ky    (fp32, the pair test's own subtraction)
//   X.  axmin = xl - max(Sx * zl, Sx * zh),  axmax = xh - min(Sx * zl, Sx * zh);  reject when axmin > 0 or axmax < 0; alike on y.
//       Rounding is monotone, so a[kx] >= xl and Sx * a[kz] <= max(Sx * zl, Sx * zh) for every corner in the box, hence every
//       corner's fp32 Ax >= axmin -- no padding is needed.  With all three Ax > 0 the origin of the sheared plane lies strictly
//       outside the triangle (Ax, Ay) of these fp32 numbers, so the exact U, V, W have one value > 0 and one < 0.  A difference of
//       two rounded products has the exact difference's sign or is 0 (monotone again), and any 0 sends all three to fp64 where the
//       signs are exact: the signs stay mixed and the face is rejected.
//   Z.  zmin = min(Sz * zl, Sz * zh), zmax = max(..), pad = 2^-20 max(|zmin|, |zmax|);  reject when zmax + pad < t_min or
//       zmin - pad > min(t_max, the lane's best t so far).  Every corner's fp32 Az lies in [zmin, zmax] (monotone).  An accepted
//       face has U, V, W of one sign, so with e = 2^-24:  the numerator is sum w_i z_i (1 + th_i), |th_i| <= 3 e, det is
//       sum w_i (1 + ph_i), |ph_i| <= 2 e, without cancellation; the quotient is a convex combination of z_i (1 + ps_i),
//       |ps_i| <= 5 e + O(e^2), and the division rounds once more: t lies within 6 e M + O(e^2) of [zmin, zmax], M = max |z_i|.
//       pad = 16 e M leaves 10 e M for the rounding of zmax + pad itself (<= e (M + pad)).  A face whose t exceeds the best so far
//       cannot lower the minimum; one with the same t and a lower index is kept, as the comparison is strict.
//       Premise of Z: the products w_i z_i do not underflow, |det| >= 2^-100 -- twice the area of the sheared triangle; it fails
//       only for a mesh whose extent relative to the ray origin is below ~1e-15, where fp32 has no t to speak of.
//   NaN.  A d component of exactly 0 gives Sx = 0 and Sx * zl = 0: finite, so 0 * inf cannot arise as long as the six differences
//       are finite; when one is not (overflow), or Sz is not finite, the test rejects nothing (every comparison with NaN is false,
//       and min / max are only taken of finite values).  A ray lying in a box plane has axmin = 0 or axmax = 0: not rejected.
//
// Termination.  No workgroup waits for another and nothing spins on a flag; every device loop below names what ends it.  No atomics
// in the cast; the build's sort counts digits with LDS atomics (knn.hip), which changes no result.  Scratch and the structure are
// caller-owned; nothing here allocates device memory or reads anything back to the host.
#include <float.h>
#include <math.h>
#include <stdio.h>

#include "dgm_host.hpp"
#include "mesh_grid.hpp"

#pragma clang fp contract(off)

namespace {
using namespace dgm;

constexpr int RC_THREADS = 256;
constexpr int RC_CHUNK = 256;     // faces per LDS tile = per box of the structure (one face per thread when staging)
constexpr int RC_BOX_PARTS = 128;  // partial boxes of the centroids
constexpr float RC_PAD = 9.5367431640625e-07f;  // 2^-20 (file header, Z)
constexpr int RC_MAX_F = 0x7fffffff - RC_CHUNK;

static_assert(RC_CHUNK == RC_THREADS && RC_THREADS == BOX_THREADS, "one face per thread when staging and in the box reduction");

long long chunks_of(int F) { return ((long long)F + RC_CHUNK - 1) / RC_CHUNK; }

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) < INFINITY; }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return finite1(x) && finite1(y) && finite1(z); }
__device__ __forceinline__ float pick(int k, float x, float y, float z) { return k == 0 ? x : (k == 1 ? y : z); }

// the face's corners; false and nine NaN when it is invalid or beyond F (file header)
__device__ __forceinline__ bool load_face(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, long long f, float c[9]) {
    bool ok = f >= 0 && f < F;
    if (ok) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        ok = i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                c[k] = verts[3 * (long long)i0 + k];
                c[3 + k] = verts[3 * (long long)i1 + k];
                c[6 + k] = verts[3 * (long long)i2 + k];
            }
            ok = finite3(c[0], c[1], c[2]) && finite3(c[3], c[4], c[5]) && finite3(c[6], c[7], c[8]);
        }
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 9; k++) c[k] = NAN;
    }
    return ok;
}

struct Ray {
    float ox, oy, oz;  // o[kx], o[ky], o[kz]
    float Sx, Sy, Sz;
    int kx, ky, kz;
};

// false: the ray tests nothing (a non-finite component, or d = 0)
__device__ __forceinline__ bool ray_setup(const float* __restrict__ origins, const float* __restrict__ dirs, long long i, Ray& r) {
    const float o0 = origins[3 * i], o1 = origins[3 * i + 1], o2 = origins[3 * i + 2];
    const float d0 = dirs[3 * i], d1 = dirs[3 * i + 1], d2 = dirs[3 * i + 2];
    int kz = 0;
    float m = fabsf(d0);
    if (fabsf(d1) > m) {
        kz = 1;
        m = fabsf(d1);
    }
    if (fabsf(d2) > m) {
        kz = 2;
        m = fabsf(d2);
    }
    int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
    const float dz = pick(kz, d0, d1, d2);
    if (dz < 0.f) {
        const int s = kx;
        kx = ky;
        ky = s;
    }
    r.kx = kx;
    r.ky = ky;
    r.kz = kz;
    r.ox = pick(kx, o0, o1, o2);
    r.oy = pick(ky, o0, o1, o2);
    r.oz = pick(kz, o0, o1, o2);
    r.Sx = pick(kx, d0, d1, d2) / dz;
    r.Sy = pick(ky, d0, d1, d2) / dz;
    r.Sz = 1.f / dz;
    return finite3(o0, o1, o2) && finite3(d0, d1, d2) && m > 0.f;
}

struct Hit {
    float t, U, V, W, det;
    int face;
};

// the pair test (file header); corners a = (A.x, A.y, A.z), b = (A.w, B.x, B.y), c = (B.z, B.w, C.x)
__device__ __forceinline__ bool pair_test(const Ray& r, const float4 A, const float4 B, const float4 C, float t_min, float t_max, Hit& h) {
    const float az = pick(r.kz, A.x, A.y, A.z) - r.oz, bz = pick(r.kz, A.w, B.x, B.y) - r.oz, cz = pick(r.kz, B.z, B.w, C.x) - r.oz;
    const float Ax = (pick(r.kx, A.x, A.y, A.z) - r.ox) - r.Sx * az, Ay = (pick(r.ky, A.x, A.y, A.z) - r.oy) - r.Sy * az;
    const float Bx = (pick(r.kx, A.w, B.x, B.y) - r.ox) - r.Sx * bz, By = (pick(r.ky, A.w, B.x, B.y) - r.oy) - r.Sy * bz;
    const float Cx = (pick(r.kx, B.z, B.w, C.x) - r.ox) - r.Sx * cz, Cy = (pick(r.ky, B.z, B.w, C.x) - r.oy) - r.Sy * cz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    bool neg, pos;
    if (U == 0.f || V == 0.f || W == 0.f) {
        const double u = (double)Cx * (double)By - (double)Cy * (double)Bx;
        const double v = (double)Ax * (double)Cy - (double)Ay * (double)Cx;
        const double w = (double)Bx * (double)Ay - (double)By * (double)Ax;
        neg = u < 0.0 || v < 0.0 || w < 0.0;
        pos = u > 0.0 || v > 0.0 || w > 0.0;
        U = (float)u;
        V = (float)v;
        W = (float)w;
    } else {
        neg = U < 0.f || V < 0.f || W < 0.f;
        pos = U > 0.f || V > 0.f || W > 0.f;
    }
    if (neg && pos) return false;
    const float det = (U + V) + W;
    if (det == 0.f) return false;
    const float Az = r.Sz * az, Bz = r.Sz * bz, Cz = r.Sz * cz;
    const float t = ((U * Az + V * Bz) + W * Cz) / det;
    if (!(t >= t_min && t < t_max && finite1(t))) return false;  // (a NaN t fails the first comparison)
    h.t = t;
    h.U = U;
    h.V = V;
    h.W = W;
    h.det = det;
    return true;
}

// true: no face inside the box [lo, hi] can be accepted for the ray with t in [t_min, t_far] (file header: X, Z, NaN)
__device__ __forceinline__ bool box_rejects(const Ray& r, const float4 lo, const float4 hi, float t_min, float t_far) {
    const float zl = pick(r.kz, lo.x, lo.y, lo.z) - r.oz, zh = pick(r.kz, hi.x, hi.y, hi.z) - r.oz;
    const float xl = pick(r.kx, lo.x, lo.y, lo.z) - r.ox, xh = pick(r.kx, hi.x, hi.y, hi.z) - r.ox;
    const float yl = pick(r.ky, lo.x, lo.y, lo.z) - r.oy, yh = pick(r.ky, hi.x, hi.y, hi.z) - r.oy;
    if (!(finite3(zl, xl, yl) && finite3(zh, xh, yh) && finite1(r.Sz))) return false;
    const float sxl = r.Sx * zl, sxh = r.Sx * zh, syl = r.Sy * zl, syh = r.Sy * zh;
    const float axmin = xl - fmaxf(sxl, sxh), axmax = xh - fminf(sxl, sxh);
    const float aymin = yl - fmaxf(syl, syh), aymax = yh - fminf(syl, syh);
    const float z0 = r.Sz * zl, z1 = r.Sz * zh;
    const float zmin = fminf(z0, z1), zmax = fmaxf(z0, z1);
    const float pad = fmaxf(fabsf(zmin), fabsf(zmax)) * RC_PAD;
    return axmin > 0.f || axmax < 0.f || aymin > 0.f || aymax < 0.f || zmax + pad < t_min || zmin - pad > t_far;
}

__device__ __forceinline__ void write_answer(bool any, long long i, bool found, const Hit& best, int* __restrict__ face, float* __restrict__ t,
                                             float* __restrict__ bary, unsigned char* __restrict__ hit) {
    if (any) {
        hit[i] = found ? 1 : 0;
        return;
    }
    face[i] = found ? best.face : -1;
    t[i] = found ? best.t : INFINITY;
    bary[3 * i] = found ? best.U / best.det : 0.f;
    bary[3 * i + 1] = found ? best.V / best.det : 0.f;
    bary[3 * i + 2] = found ? best.W / best.det : 0.f;
}

// (t, face) below the best so far, lexicographically
__device__ __forceinline__ bool better(const Hit& h, int f, bool found, const Hit& best) {
    return !found || h.t < best.t || (h.t == best.t && f < best.face);
}

// brute force: one workgroup per 256 rays, every chunk of 256 faces through the LDS tile.  ANY: dgm_ray_occluded.
template <bool ANY>
__global__ void __launch_bounds__(RC_THREADS)
ray_brute_kernel(int N, int V, int F, const float* __restrict__ origins, const float* __restrict__ dirs, float t_min, float t_max,
                 const float* __restrict__ verts, const int* __restrict__ faces, int* __restrict__ face, float* __restrict__ t,
                 float* __restrict__ bary, unsigned char* __restrict__ hit) {
    __shared__ float4 tile[RC_CHUNK * 3];  // nine floats per face in three float4: 16-byte broadcast reads
    const long long i = (long long)blockIdx.x * RC_THREADS + threadIdx.x;
    const bool act = i < N;
    Ray r = {};
    bool live = act && ray_setup(origins, dirs, i, r);
    Hit best = {}, h = {};
    bool found = false;
    const int nchunks = (F + RC_CHUNK - 1) / RC_CHUNK;  // (F <= RC_MAX_F: checked by the launcher)
    float c[9];
    load_face(V, F, verts, faces, threadIdx.x, c);
    for (int ch = 0; ch < nchunks; ch++) {  // ends at the last chunk (ANY: or when no lane of the workgroup is live)
        tile[threadIdx.x * 3] = make_float4(c[0], c[1], c[2], c[3]);
        tile[threadIdx.x * 3 + 1] = make_float4(c[4], c[5], c[6], c[7]);
        tile[threadIdx.x * 3 + 2] = make_float4(c[8], 0.f, 0.f, 0.f);
        __syncthreads();
        if (ch + 1 < nchunks) load_face(V, F, verts, faces, (long long)(ch + 1) * RC_CHUNK + threadIdx.x, c);  // in flight during the pair loop
        const int m = min(RC_CHUNK, F - ch * RC_CHUNK);
        if (live) {
#pragma unroll 2
            for (int k = 0; k < m; k++) {  // ends at the chunk's last face: at most RC_CHUNK rounds
                if (!pair_test(r, tile[3 * k], tile[3 * k + 1], tile[3 * k + 2], t_min, t_max, h)) continue;
                const int f = ch * RC_CHUNK + k;
                if (better(h, f, found, best)) {
                    best = h;
                    best.face = f;
                    found = true;
                }
                if (ANY) {
                    live = false;
                    break;
                }
            }
        }
        if (ANY) {
            if (__syncthreads_and(!live)) break;  // (the same value in every thread)
        } else {
            __syncthreads();
        }
    }
    if (act) write_answer(ANY, i, found, best, face, t, bary, hit);
}

// accelerated: one workgroup per 256 rays walks the chunk boxes; a chunk is staged when a lane's box test does not reject it
template <bool ANY>
__global__ void __launch_bounds__(RC_THREADS)
ray_accel_kernel(int N, int nchunks, const float* __restrict__ origins, const float* __restrict__ dirs, float t_min, float t_max,
                 const float4* __restrict__ tri, const float4* __restrict__ boxes, int* __restrict__ face, float* __restrict__ t,
                 float* __restrict__ bary, unsigned char* __restrict__ hit) {
    __shared__ float4 tile[RC_CHUNK * 3];
    const long long i = (long long)blockIdx.x * RC_THREADS + threadIdx.x;
    const bool act = i < N;
    Ray r = {};
    bool live = act && ray_setup(origins, dirs, i, r);
    Hit best = {}, h = {};
    bool found = false;
    for (int ch = 0; ch < nchunks; ch++) {  // ends at the last chunk
        const float4 lo = boxes[2 * ch], hi = boxes[2 * ch + 1];  // (uniform: lo.w = the chunk's number of valid faces)
        const float t_far = found ? fminf(t_max, best.t) : t_max;
        const bool want = live && lo.w > 0.f && !box_rejects(r, lo, hi, t_min, t_far);
        if (!__syncthreads_or(want)) continue;  // (the same value in every thread; also the barrier behind the last round's reads)
        const long long at = ((long long)ch * RC_CHUNK + threadIdx.x) * 3;
        tile[threadIdx.x * 3] = tri[at];
        tile[threadIdx.x * 3 + 1] = tri[at + 1];
        tile[threadIdx.x * 3 + 2] = tri[at + 2];
        __syncthreads();
        if (want) {
#pragma unroll 2
            for (int k = 0; k < RC_CHUNK; k++) {  // ends at the chunk's last face (the padding behind F is NaN faces)
                const float4 C = tile[3 * k + 2];
                if (!pair_test(r, tile[3 * k], tile[3 * k + 1], C, t_min, t_max, h)) continue;
                const int f = __float_as_int(C.y);
                if (better(h, f, found, best)) {
                    best = h;
                    best.face = f;
                    found = true;
                }
                if (ANY) {
                    live = false;
                    break;
                }
            }
        }
    }
    if (act) write_answer(ANY, i, found, best, face, t, bary, hit);
}

// V = 0 or F = 0: misses everywhere
__global__ void __launch_bounds__(RC_THREADS)
ray_none_kernel(int N, int* __restrict__ face, float* __restrict__ t, float* __restrict__ bary, unsigned char* __restrict__ hit) {
    const long long i = (long long)blockIdx.x * RC_THREADS + threadIdx.x;
    if (i >= N) return;
    Hit none = {};
    write_answer(hit != nullptr, i, false, none, face, t, bary, hit);
}

// ---- the build -----------------------------------------------------------------------------------------------------------------------
// cen[f] = the face's centroid ((a + b) + c) / 3 per axis and 1, or (0, 0, 0, 0) for a face that can never hit
__global__ void __launch_bounds__(RC_THREADS)
centroid_kernel(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, float4* __restrict__ cen) {
    const long long f = (long long)blockIdx.x * RC_THREADS + threadIdx.x;
    if (f >= F) return;
    float c[9];
    const bool ok = load_face(V, F, verts, faces, f, c);
    cen[f] = ok ? make_float4(((c[0] + c[3]) + c[6]) / 3.f, ((c[1] + c[4]) + c[7]) / 3.f, ((c[2] + c[5]) + c[8]) / 3.f, 1.f)
                : make_float4(0.f, 0.f, 0.f, 0.f);
}

// partial[b] = the box of the valid centroids block b visits (min and max are exact: the order does not matter)
__global__ void __launch_bounds__(RC_THREADS) centroid_box_kernel(int F, const float4* __restrict__ cen, float* __restrict__ partial) {
    float v[6];
    box_start<6>(v);
    for (long long f = (long long)blockIdx.x * RC_THREADS + threadIdx.x; f < F; f += (long long)gridDim.x * RC_THREADS) {  // ends at F
        const float4 c = cen[f];
        if (c.w == 0.f) continue;
        const float p[3] = {c.x, c.y, c.z};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            v[a] = box_join(a, v[a], p[a]);
            v[3 + a] = box_join(3 + a, v[3 + a], p[a]);
        }
    }
    box_reduce_partial<6>(v, partial);
}

__global__ void centroid_box_final_kernel(int nparts, const float* __restrict__ partial, float* __restrict__ bbox) {
    if (threadIdx.x < 6) bbox[threadIdx.x] = box_final_row<6>(nparts, partial, threadIdx.x);  // (at most RC_BOX_PARTS rounds)
}

// key = the 30-bit Morton code of the centroid in the centroids' box, 0xFFFFFFFF for a face that can never hit; value = the face.
// The order only decides which faces share a box: it changes how much is tested, never an answer.
__global__ void __launch_bounds__(RC_THREADS)
morton_kernel(int F, const float4* __restrict__ cen, const float* __restrict__ bbox, unsigned* __restrict__ keys, unsigned* __restrict__ vals) {
    const long long f = (long long)blockIdx.x * RC_THREADS + threadIdx.x;
    if (f >= F) return;
    const float4 c = cen[f];
    const float p[3] = {c.x, c.y, c.z};
    unsigned q[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float lo = bbox[a], hi = bbox[3 + a];
        q[a] = morton_spread10(min(f2u_sat(((p[a] - lo) / (hi - lo)) * 1023.f), 1023u));  // (a flat box: 0 / 0 = NaN -> 0)
    }
    keys[f] = c.w == 0.f ? 0xFFFFFFFFu : (q[0] | (q[1] << 1) | (q[2] << 2));
    vals[f] = (unsigned)f;
}

// the structure: per sorted position three float4 (a, b, c, the original face index, 0, 0), per chunk two float4 (lo, count; hi, 0)
__global__ void __launch_bounds__(RC_THREADS)
chunk_kernel(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, const unsigned* __restrict__ order,
             float4* __restrict__ tri, float4* __restrict__ boxes) {
    __shared__ float red[6][RC_THREADS];
    __shared__ unsigned count[RC_THREADS / 64];
    const long long at = (long long)blockIdx.x * RC_CHUNK + threadIdx.x;
    const int f = at < F ? (int)order[at] : -1;
    float c[9];
    const bool ok = load_face(V, F, verts, faces, f, c);
    tri[3 * at] = make_float4(c[0], c[1], c[2], c[3]);
    tri[3 * at + 1] = make_float4(c[4], c[5], c[6], c[7]);
    tri[3 * at + 2] = make_float4(c[8], __int_as_float(f), 0.f, 0.f);
    float v[6];
    box_start<6>(v);
    if (ok) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            v[a] = fminf(fminf(c[a], c[3 + a]), c[6 + a]);
            v[3 + a] = fmaxf(fmaxf(c[a], c[3 + a]), c[6 + a]);
        }
    }
    const unsigned long long valid = __ballot(ok);
    if (lane_id() == 0) count[threadIdx.x >> 6] = (unsigned)__popcll(valid);
    box_reduce<6>(red, v);  // (its barriers also publish count)
    if (threadIdx.x == 0) {
        const unsigned n = count[0] + count[1] + count[2] + count[3];
        boxes[2 * blockIdx.x] = make_float4(red[0][0], red[1][0], red[2][0], (float)n);
        boxes[2 * blockIdx.x + 1] = make_float4(red[3][0], red[4][0], red[5][0], 0.f);
    }
}

struct BuildLayout {
    size_t partial, bbox, cen, keysA, keysB, valsA, valsB, hist, scanned, total;
};

BuildLayout build_layout(int F) {
    BuildLayout L;
    const size_t n = (size_t)F, words = radix_sort_hist_words(F);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    };
    L.partial = take(RC_BOX_PARTS * 6 * 4);
    L.bbox = take(8 * 4);
    L.cen = take(n * 16);
    L.keysA = take(n * 4);
    L.keysB = take(n * 4);
    L.valsA = take(n * 4);
    L.valsB = take(n * 4);
    L.hist = take(words * 4);
    L.scanned = take(words * 4);
    L.total = o + 256;  // (the launcher aligns the pointer up itself)
    return L;
}

const char* cast_args(const char* name, int N, int V, int F, const void* origins, const void* dirs, const void* verts, const void* faces,
                      const char* accel, bool outputs) {
    static thread_local char msg[160];
    const char* why = nullptr;
    if (N < 0 || V < 0 || F < 0)
        why = "need N >= 0, V >= 0 and F >= 0";
    else if (F > RC_MAX_F)
        why = "too many faces";
    else if (N > 0 && (!origins || !dirs || !outputs || (F > 0 && !faces) || (F > 0 && V > 0 && !verts)))
        why = "NULL pointer";
    else if (N > 0 && ((uintptr_t)accel & 15))
        why = "accel must be 16-byte aligned";
    if (!why) return nullptr;
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return msg;
}

template <bool ANY>
int launch_cast(int N, int V, int F, const float* origins, const float* dirs, float t_min, float t_max, const float* verts, const int* faces,
                const char* accel, int* face, float* t, float* bary, unsigned char* hit, hipStream_t st) {
    const dim3 grid(blocks(N)), block(RC_THREADS);  // (at most 2^23 workgroups: N is an int)
    if (F == 0 || V == 0) {
        hipLaunchKernelGGL(ray_none_kernel, grid, block, 0, st, N, face, t, bary, hit);
    } else if (!accel) {
        hipLaunchKernelGGL(ray_brute_kernel<ANY>, grid, block, 0, st, N, V, F, origins, dirs, t_min, t_max, verts, faces, face, t, bary, hit);
    } else {
        const long long nch = chunks_of(F);
        const float4* tri = (const float4*)accel;
        const float4* boxes = tri + nch * RC_CHUNK * 3;
        hipLaunchKernelGGL(ray_accel_kernel<ANY>, grid, block, 0, st, N, (int)nch, origins, dirs, t_min, t_max, tri, boxes, face, t, bary, hit);
    }
    return launch_status();
}

}  // namespace

extern "C" {

size_t dgm_ray_accel_bytes(int F) {
    if (F < 0 || F > RC_MAX_F) return 0;
    return (size_t)chunks_of(F) * (RC_CHUNK * 48 + 32);
}

size_t dgm_ray_build_scratch_bytes(int F) {
    if (F < 0 || F > RC_MAX_F) return 0;
    return build_layout(F).total;
}

int dgm_ray_build(int V, int F, const float* verts, const int* faces, char* scratch, char* accel, void* stream) {
    if (V < 0 || F < 0) return fail("ray_build: need V >= 0 and F >= 0");
    if (F > RC_MAX_F) return fail("ray_build: too many faces");
    if (F == 0) return 0;  // (before any HIP call: the structure of no face has no byte)
    if (!faces || !scratch || !accel || (V > 0 && !verts)) return fail("ray_build: NULL pointer");
    if ((uintptr_t)accel & 15) return fail("ray_build: accel must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const BuildLayout L = build_layout(F);
    char* base = align_ptr(scratch);
    float* partial = (float*)(base + L.partial);
    float* bbox = (float*)(base + L.bbox);
    float4* cen = (float4*)(base + L.cen);
    unsigned *keysA = (unsigned*)(base + L.keysA), *keysB = (unsigned*)(base + L.keysB);
    unsigned *valsA = (unsigned*)(base + L.valsA), *valsB = (unsigned*)(base + L.valsB);
    const long long nch = chunks_of(F);
    float4* tri = (float4*)accel;
    float4* boxes = tri + nch * RC_CHUNK * 3;
    hipLaunchKernelGGL(centroid_kernel, dim3(blocks(F)), dim3(RC_THREADS), 0, st, V, F, verts, faces, cen);
    const int nparts = (int)(nch < RC_BOX_PARTS ? nch : RC_BOX_PARTS);
    hipLaunchKernelGGL(centroid_box_kernel, dim3(nparts), dim3(RC_THREADS), 0, st, F, (const float4*)cen, partial);
    hipLaunchKernelGGL(centroid_box_final_kernel, dim3(1), dim3(64), 0, st, nparts, (const float*)partial, bbox);
    hipLaunchKernelGGL(morton_kernel, dim3(blocks(F)), dim3(RC_THREADS), 0, st, F, (const float4*)cen, (const float*)bbox, keysA, valsA);
    const unsigned* order = radix_sort_pairs(st, F, 4, keysA, valsA, keysB, valsB, (unsigned*)(base + L.hist), (unsigned*)(base + L.scanned));
    hipLaunchKernelGGL(chunk_kernel, dim3((unsigned)nch), dim3(RC_THREADS), 0, st, V, F, verts, faces, order, tri, boxes);
    return launch_status();
}

int dgm_ray_cast(int N, int V, int F, const float* origins, const float* dirs, float t_min, float t_max, const float* verts, const int* faces,
                 const char* accel, int* face, float* t, float* bary, void* stream) {
    if (const char* m = cast_args("ray_cast", N, V, F, origins, dirs, verts, faces, accel, face && t && bary)) return fail(m);
    if (N == 0) return 0;  // (before any HIP call)
    return launch_cast<false>(N, V, F, origins, dirs, t_min, t_max, verts, faces, accel, face, t, bary, nullptr, (hipStream_t)stream);
}

int dgm_ray_occluded(int N, int V, int F, const float* origins, const float* dirs, float t_min, float t_max, const float* verts,
                     const int* faces, const char* accel, unsigned char* hit, void* stream) {
    if (const char* m = cast_args("ray_occluded", N, V, F, origins, dirs, verts, faces, accel, hit != nullptr)) return fail(m);
    if (N == 0) return 0;  // (before any HIP call)
    return launch_cast<true>(N, V, F, origins, dirs, t_min, t_max, verts, faces, accel, nullptr, nullptr, nullptr, hit, (hipStream_t)stream);
}

}  // extern "C"
