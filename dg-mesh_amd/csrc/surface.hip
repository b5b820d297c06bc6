// Closest point on a triangle mesh for gfx950, with the two small passes that use it: barycentric interpolation of a vertex attribute
// and the colour of a canonical position (correspondence.py).  The reference has no counterpart: its README
// lists "Mesh correspondence visualization" as an open item.
//
// Per (query p, face (a, b, c)) pair -- fp32, no FMA (this file is built with -ffp-contract=off and correctly rounded / and sqrt);
// dot(x, y) = (x0*y0 + x1*y1) + x2*y2; the region test of Ericson, Real-Time Collision Detection, section 5.1.5, in its order:
//   ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c
//   d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp)
//   vc = d1*d4 - d3*d2, vb = d5*d2 - d1*d6, va = d3*d6 - d5*d4
//   1. d1 <= 0 and d2 <= 0                          (vertex A)  v = 0, w = 0
//   2. d3 >= 0 and d4 <= d3                         (vertex B)  v = 1, w = 0
//   3. vc <= 0 and d1 >= 0 and d3 <= 0              (edge AB)   v = d1 / (d1 - d3), w = 0
//   4. d6 >= 0 and d5 <= d6                         (vertex C)  v = 0, w = 1
//   5. vb <= 0 and d2 >= 0 and d6 <= 0              (edge AC)   v = 0, w = d2 / (d2 - d6)
//   6. va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    (edge BC)   w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w
//   7. otherwise                                    (interior)  den = 1 / ((va + vb) + vc), v = vb*den, w = vc*den
//   the first rule that holds decides; q = (a + ab*v) + ac*w per axis, dist2 = dot(p - q, p - q), bary = ((1 - v) - w, v, w).
// A face is a candidate when its three indices lie in [0, V) and the length sqrt((nx*nx + ny*ny) + nz*nz) of n = cross(ab, ac)
// (nx = ab.y*ac.z - ab.z*ac.y, ...) is positive and finite (face_geometry_kernel's len > 0; an infinite or NaN length -- a non-finite
// vertex, an overflow -- is refused with it).  A NaN dist2 never wins a comparison.
// The answer of a query is the lexicographic minimum of (dist2, face index) over the candidates with dist2 < max_d2 (strict); none:
// face = -1, dist2 = +inf, bary = 0.  It is a minimum over a SET, so it does not depend on the order in which the faces are visited
// and is bit-reproducible; a face met twice loses the tie to itself.
//   * finite max_d2: a hashed uniform grid over the FACES.  A face is registered in every cell its box overlaps; the box is the
//     face's AABB widened by 2^-19 of its largest |coordinate| S per axis: q is a rounded combination of the corners and may leave
//     the exact AABB -- ab, ac, their products with v and w, the two sums and v + w <= 1 up to rounding add up to at most 16 * 2^-24 S,
//     half the widening (v and w of a sliver, whose |n|^2 drowns in the rounding of the products, stay within rounding of [0, 1] all
//     the same: measured and asserted by tests/test_surface_host.py).  Cell edge c = max(1.001 sqrt(max_d2), 1.001 E, 2^-20 extent), E = the largest box edge of a
//     candidate face, reduced on the device and read by the later kernels from device memory.  A box then spans at most two cells
//     per axis: at most 8 references per face (the upper cell is clamped to lower + 1, so the bound holds by construction), and the
//     scratch is known on the host.  Cell coordinates are taken in fp64 from fp32 values (mesh_grid.hpp); a face with fp32
//     dist2 < max_d2 has |p - q| < c on every axis, so q's cell -- one the face is registered in -- is among the 27 around p's.
//     Inside a bucket a face whose box lies farther from p than the best so far is skipped: the fp32 gap to the box is a lower bound
//     of the fp32 dist2, rounding included (surf_grid_kernel), so a skipped face can neither win nor tie.
//     Cells hash into 2^k >= F buckets; a collision only adds candidates.  The table is built by count, scan and scatter (atomics:
//     the order inside a bucket varies run to run, the result does not); the queries are visited sorted by their own bucket.
//   * max_d2 = +inf: a tiled brute force, 256 faces of nine floats per LDS tile, one query per lane.
// Scratch is caller-owned and a pure function of (N, F); nothing here allocates device memory or reads anything back to the host.
#include <float.h>
#include <math.h>

#include "dgm_host.hpp"
#include "mesh_grid.hpp"
#include "mesh_scan.hpp"

#pragma clang fp contract(off)

namespace {
using namespace dgm;

constexpr int SF_THREADS = 256;
constexpr int BF_TILE = 256;  // faces per LDS tile of the brute force
constexpr int BOX_PARTS = 128;
constexpr int REFS_PER_FACE = 8;
constexpr unsigned QUERY_MASK = 0xFFFFu;            // buckets of the queries' visiting order (two radix passes)
constexpr float BOX_PAD = 1.9073486328125e-06f;     // 2^-19

// ---- the pair arithmetic (file header) ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float dot3(float x0, float x1, float x2, float y0, float y1, float y2) { return (x0 * y0 + x1 * y1) + x2 * y2; }

__device__ __forceinline__ void closest_vw(const float p[3], const float a[3], const float b[3], const float c[3], float& v, float& w,
                                           float& dist2) {
    const float ab0 = b[0] - a[0], ab1 = b[1] - a[1], ab2 = b[2] - a[2];
    const float ac0 = c[0] - a[0], ac1 = c[1] - a[1], ac2 = c[2] - a[2];
    const float ap0 = p[0] - a[0], ap1 = p[1] - a[1], ap2 = p[2] - a[2];
    const float bp0 = p[0] - b[0], bp1 = p[1] - b[1], bp2 = p[2] - b[2];
    const float cp0 = p[0] - c[0], cp1 = p[1] - c[1], cp2 = p[2] - c[2];
    const float d1 = dot3(ab0, ab1, ab2, ap0, ap1, ap2), d2 = dot3(ac0, ac1, ac2, ap0, ap1, ap2);
    const float d3 = dot3(ab0, ab1, ab2, bp0, bp1, bp2), d4 = dot3(ac0, ac1, ac2, bp0, bp1, bp2);
    const float d5 = dot3(ab0, ab1, ab2, cp0, cp1, cp2), d6 = dot3(ac0, ac1, ac2, cp0, cp1, cp2);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.f && d2 <= 0.f) {
        v = 0.f;
        w = 0.f;
    } else if (d3 >= 0.f && d4 <= d3) {
        v = 1.f;
        w = 0.f;
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        v = d1 / (d1 - d3);
        w = 0.f;
    } else if (d6 >= 0.f && d5 <= d6) {
        v = 0.f;
        w = 1.f;
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
        v = 0.f;
        w = d2 / (d2 - d6);
    } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
        w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        v = 1.f - w;
    } else {
        const float den = 1.f / ((va + vb) + vc);
        v = vb * den;
        w = vc * den;
    }
    const float q0 = (a[0] + ab0 * v) + ac0 * w, q1 = (a[1] + ab1 * v) + ac1 * w, q2 = (a[2] + ab2 * v) + ac2 * w;
    const float e0 = p[0] - q0, e1 = p[1] - q1, e2 = p[2] - q2;
    dist2 = dot3(e0, e1, e2, e0, e1, e2);
}

// the face's corners, or NaN in all nine when it is no candidate (then every dist2 against it is NaN and loses every comparison)
__device__ __forceinline__ void load_face(int V, const float* __restrict__ verts, const int* __restrict__ faces, long long f, float t[9]) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    bool ok = i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
    if (ok) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            t[k] = verts[3 * (long long)i0 + k];
            t[3 + k] = verts[3 * (long long)i1 + k];
            t[6 + k] = verts[3 * (long long)i2 + k];
        }
        const float e1x = t[3] - t[0], e1y = t[4] - t[1], e1z = t[5] - t[2];
        const float e2x = t[6] - t[0], e2y = t[7] - t[1], e2z = t[8] - t[2];
        const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        ok = len > 0.f && len < INFINITY;
    }
    if (!ok) {
        const float nan = __int_as_float(0x7fc00000);
#pragma unroll
        for (int k = 0; k < 9; k++) t[k] = nan;
    }
}

__device__ __forceinline__ void consider(const float p[3], const float t[9], int j, float& best, int& bi) {
    float v, w, d;
    closest_vw(p, t, t + 3, t + 6, v, w, d);
    if (d < best || (d == best && j < bi)) {  // bi == -1: only dist2 < max_d2 admits the first candidate
        best = d;
        bi = j;
    }
}

__device__ __forceinline__ void write_answer(const float p[3], const float t[9], int bi, float best, long long n, int* __restrict__ face,
                                             float* __restrict__ d2out, float* __restrict__ bary) {
    float v = 0.f, w = 0.f, d = INFINITY, u = 0.f;
    if (bi >= 0) {  // the winner once more: the same operations, the same bits
        closest_vw(p, t, t + 3, t + 6, v, w, d);
        u = (1.f - v) - w;
        d = best;
    }
    face[n] = bi;
    d2out[n] = d;
    bary[3 * n] = u;
    bary[3 * n + 1] = v;
    bary[3 * n + 2] = w;
}

// ---- brute force ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SF_THREADS)
surf_brute_kernel(int N, int V, int F, const float* __restrict__ pts, const float* __restrict__ verts, const int* __restrict__ faces,
                  float max_d2, int* __restrict__ face, float* __restrict__ d2out, float* __restrict__ bary) {
    __shared__ float tile[BF_TILE * 9];
    const long long i = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    const bool act = i < N;
    float p[3];
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = act ? pts[3 * i + k] : 0.f;
    float best = max_d2;
    int bi = -1;
    for (int base = 0; base < F; base += BF_TILE) {
        const int j = base + (int)threadIdx.x;
        if (j < F) {
            float t[9];
            load_face(V, verts, faces, j, t);
#pragma unroll
            for (int k = 0; k < 9; k++) tile[threadIdx.x * 9 + k] = t[k];
        }
        __syncthreads();
        const int m = min(BF_TILE, F - base);
        for (int k = 0; k < m; k++) {
            float t[9];
#pragma unroll
            for (int e = 0; e < 9; e++) t[e] = tile[k * 9 + e];
            consider(p, t, base + k, best, bi);
        }
        __syncthreads();
    }
    if (act) {
        float t[9];
        if (bi >= 0) load_face(V, verts, faces, bi, t);
        write_answer(p, t, bi, best, i, face, d2out, bary);
    }
}

__global__ void __launch_bounds__(SF_THREADS)
surf_none_kernel(int N, int* __restrict__ face, float* __restrict__ d2out, float* __restrict__ bary) {
    const long long i = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (i >= N) return;
    face[i] = -1;
    d2out[i] = INFINITY;
    bary[3 * i] = bary[3 * i + 1] = bary[3 * i + 2] = 0.f;
}

// ---- the grid over the faces ------------------------------------------------------------------------------------------------------------
// the widened box of a candidate face (file header)
__device__ __forceinline__ void face_box(const float4 A, const float4 B, const float4 C, float lo[3], float hi[3]) {
    const float a[3] = {A.x, A.y, A.z}, b[3] = {B.x, B.y, B.z}, c[3] = {C.x, C.y, C.z};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float l = fminf(fminf(a[k], b[k]), c[k]), h = fmaxf(fmaxf(a[k], b[k]), c[k]);
        const float pad = BOX_PAD * fmaxf(fabsf(l), fabsf(h));
        lo[k] = l - pad;
        hi[k] = h + pad;
    }
}

// corners as three float4 per face (w of the first: 1 for a candidate, 0 otherwise) and the widened box as two
__global__ void __launch_bounds__(SF_THREADS)
face_prep_kernel(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, float4* __restrict__ tri,
                 float4* __restrict__ box) {
    const long long f = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (f >= F) return;
    float t[9];
    load_face(V, verts, faces, f, t);
    const float4 A = make_float4(t[0], t[1], t[2], t[0] == t[0] ? 1.f : 0.f), B = make_float4(t[3], t[4], t[5], 0.f),
                 C = make_float4(t[6], t[7], t[8], 0.f);
    tri[3 * f] = A;
    tri[3 * f + 1] = B;
    tri[3 * f + 2] = C;
    float lo[3], hi[3];
    face_box(A, B, C, lo, hi);  // (NaN for a refused face: its lower bound below is 0 and the pair test refuses it)
    box[2 * f] = make_float4(lo[0], lo[1], lo[2], 0.f);
    box[2 * f + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
}

// per workgroup: (min lo) x 3, (max hi) x 3, the largest box edge
__global__ void __launch_bounds__(BOX_THREADS) box_partial_kernel(int F, const float4* __restrict__ tri, float* __restrict__ partial) {
    float v[7];
    box_start<7>(v);
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f < F; f += (long long)gridDim.x * 256) {  // ends at F
        const float4 A = tri[3 * f];
        if (A.w == 0.f) continue;
        float lo[3], hi[3];
        face_box(A, tri[3 * f + 1], tri[3 * f + 2], lo, hi);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            v[k] = box_join(k, v[k], lo[k]);
            v[3 + k] = box_join(3 + k, v[3 + k], hi[k]);
            v[6] = box_join(6, v[6], hi[k] - lo[k]);
        }
    }
    box_reduce_partial<7>(v, partial);
}

// every cell the box of face f overlaps -> visit(bucket): at most two cells per axis, REFS_PER_FACE in all
template <class Visit>
__device__ __forceinline__ void for_each_cell(const float4* __restrict__ tri, long long f, const GridParams* __restrict__ gp, unsigned mask,
                                              Visit visit) {
    const float4 A = tri[3 * f];
    if (A.w == 0.f) return;
    float lo[3], hi[3];
    face_box(A, tri[3 * f + 1], tri[3 * f + 2], lo, hi);
    const double inv = gp->inv;
    int c0[3], c1[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        c0[k] = cell_coord(lo[k], gp->origin[k], inv);
        c1[k] = min(cell_coord(hi[k], gp->origin[k], inv), c0[k] + 1);
    }
    for (int z = c0[2]; z <= c1[2]; z++)
        for (int y = c0[1]; y <= c1[1]; y++)
            for (int x = c0[0]; x <= c1[0]; x++) visit(cell_hash(x, y, z, mask));
}

__global__ void __launch_bounds__(SF_THREADS)
face_count_kernel(int F, const float4* __restrict__ tri, const GridParams* __restrict__ gp, unsigned mask, unsigned* __restrict__ cnt) {
    const long long f = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (f >= F) return;
    for_each_cell(tri, f, gp, mask, [&](unsigned b) { atomicAdd(&cnt[b], 1u); });
}

__global__ void __launch_bounds__(SF_THREADS)
face_scatter_kernel(int F, const float4* __restrict__ tri, const GridParams* __restrict__ gp, unsigned mask, unsigned* __restrict__ cursor,
                    unsigned capacity, unsigned* __restrict__ refs) {
    const long long f = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (f >= F) return;
    for_each_cell(tri, f, gp, mask, [&](unsigned b) {
        const unsigned at = atomicAdd(&cursor[b], 1u);
        if (at < capacity) refs[at] = (unsigned)f;  // (always: the count pass walked the same cells)
    });
}

__global__ void __launch_bounds__(SF_THREADS)
query_key_kernel(int N, const float* __restrict__ pts, const GridParams* __restrict__ gp, unsigned* __restrict__ key, unsigned* __restrict__ val) {
    const long long i = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (i >= N) return;
    const double inv = gp->inv;
    key[i] = cell_hash(cell_coord(pts[3 * i], gp->origin[0], inv), cell_coord(pts[3 * i + 1], gp->origin[1], inv),
                       cell_coord(pts[3 * i + 2], gp->origin[2], inv), QUERY_MASK);
    val[i] = (unsigned)i;
}

__global__ void __launch_bounds__(SF_THREADS)
surf_grid_kernel(int N, int F, const float* __restrict__ pts, const unsigned* __restrict__ order, const GridParams* __restrict__ gp,
                 unsigned mask, const unsigned* __restrict__ start, const unsigned* __restrict__ refs, const float4* __restrict__ tri,
                 const float4* __restrict__ box, float max_d2, int* __restrict__ face, float* __restrict__ d2out, float* __restrict__ bary) {
    const long long i = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (i >= N) return;
    const unsigned qi = order[i];
    if (qi >= (unsigned)N) return;
    float p[3];
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = pts[3 * (long long)qi + k];
    const double inv = gp->inv;
    const int cx = cell_coord(p[0], gp->origin[0], inv), cy = cell_coord(p[1], gp->origin[1], inv), cz = cell_coord(p[2], gp->origin[2], inv);
    float best = max_d2;
    int bi = -1;
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const unsigned b = cell_hash(cx + dx, cy + dy, cz + dz, mask);
                const unsigned j1 = start[b + 1];
                for (unsigned j = start[b]; j < j1; j++) {
                    const unsigned f = refs[j];
                    if (f >= (unsigned)F) continue;
                    // a lower bound of this pair's dist2, rounding included: q lies in the face's box, p_k - q_k and the gap to the
                    // box are single roundings of exact differences, and products and sums of non-negative terms round monotonically
                    const float4 lo = box[2 * (long long)f], hi = box[2 * (long long)f + 1];
                    const float g0 = fmaxf(fmaxf(lo.x - p[0], p[0] - hi.x), 0.f), g1 = fmaxf(fmaxf(lo.y - p[1], p[1] - hi.y), 0.f),
                                g2 = fmaxf(fmaxf(lo.z - p[2], p[2] - hi.z), 0.f);
                    if (dot3(g0, g1, g2, g0, g1, g2) > best) continue;  // (cannot win, cannot tie)
                    const float4 A = tri[3 * (long long)f], B = tri[3 * (long long)f + 1], C = tri[3 * (long long)f + 2];
                    const float t[9] = {A.x, A.y, A.z, B.x, B.y, B.z, C.x, C.y, C.z};
                    consider(p, t, (int)f, best, bi);
                }
            }
    float t[9];
    if (bi >= 0) {
        const float4 A = tri[3 * (long long)bi], B = tri[3 * (long long)bi + 1], C = tri[3 * (long long)bi + 2];
        t[0] = A.x, t[1] = A.y, t[2] = A.z, t[3] = B.x, t[4] = B.y, t[5] = B.z, t[6] = C.x, t[7] = C.y, t[8] = C.z;
    }
    write_answer(p, t, bi, best, qi, face, d2out, bary);
}

struct SurfLayout {
    size_t partial, params, tri, box, cnt, start, cursor, refs, tiles, keysA, valsA, keysB, valsB, hist, scanned, total;
    size_t H;
    int nb;
};

SurfLayout surf_layout(int N, int F) {
    SurfLayout L;
    L.H = pow2_at_least((size_t)F);
    L.nb = scan_tiles((long long)L.H);
    const size_t hw = radix_sort_hist_words(N);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    };
    L.partial = take(BOX_PARTS * 7 * 4);
    L.params = take(sizeof(GridParams));
    L.tri = take((size_t)F * 48);
    L.box = take((size_t)F * 32);
    L.cnt = take(L.H * 4);
    L.start = take((L.H + 1) * 4);
    L.cursor = take(L.H * 4);
    L.refs = take((size_t)F * REFS_PER_FACE * 4);
    L.tiles = take((size_t)L.nb * 2 * 4);
    L.keysA = take((size_t)N * 4);
    L.valsA = take((size_t)N * 4);
    L.keysB = take((size_t)N * 4);
    L.valsB = take((size_t)N * 4);
    L.hist = take(hw * 4);
    L.scanned = take(hw * 4);
    L.total = o + 256;  // (+256: the caller's pointer is aligned up)
    return L;
}

// ---- interpolation and palette -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SF_THREADS)
surf_interp_kernel(long long total, int V, int F, int C, const float* __restrict__ attr, const int* __restrict__ faces,
                   const int* __restrict__ face, const float* __restrict__ bary, float fill, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (i >= total) return;
    const long long n = i / C;
    const int c = (int)(i - n * C);
    const int f = face[n];
    float r = fill;
    if (f >= 0 && f < F) {
        const int i0 = faces[3 * (long long)f], i1 = faces[3 * (long long)f + 1], i2 = faces[3 * (long long)f + 2];
        if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V)
            r = (attr[(long long)i0 * C + c] * bary[3 * n] + attr[(long long)i1 * C + c] * bary[3 * n + 1]) +
                attr[(long long)i2 * C + c] * bary[3 * n + 2];
    }
    out[i] = r;
}

__global__ void __launch_bounds__(SF_THREADS)
palette_kernel(int N, const float* __restrict__ xyz, const float* __restrict__ center, const float* __restrict__ scale, int mode, int cells,
               float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * SF_THREADS + threadIdx.x;
    if (i >= N) return;
    const float s = scale[0], fc = (float)cells;
    float u[3];
    bool lost = false;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float t = ((xyz[3 * i + a] - center[a]) / s) * 0.5f + 0.5f;
        lost = lost || t != t;
        u[a] = fminf(fmaxf(t, 0.f), 1.f);
        k += (int)floorf(u[a] * fc);
    }
    const float shade = (mode == 1 && (k & 1)) ? 0.55f : 1.f;
    out[3 * i] = lost ? 1.f : u[0] * shade;
    out[3 * i + 1] = lost ? 0.f : u[1] * shade;
    out[3 * i + 2] = lost ? 1.f : u[2] * shade;
}

}  // namespace

extern "C" {

size_t dgm_surf_closest_scratch_bytes(int N, int F) {
    if (N < 0 || F < 0) return 0;
    return surf_layout(N, F).total;
}

int dgm_surf_closest(int N, int V, int F, const float* points, const float* verts, const int* faces, float max_d2, char* scratch,
                     int* face, float* d2, float* bary, void* stream) {
    if (N < 0 || V < 0 || F < 0) return fail("surf_closest: need N >= 0, V >= 0 and F >= 0");
    if (N == 0) return 0;  // (before any HIP call)
    if (!points || !face || !d2 || !bary || (F > 0 && !faces) || (F > 0 && V > 0 && !verts)) return fail("surf_closest: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (F == 0 || V == 0 || !(max_d2 > 0.f)) {  // nothing can be reported (NaN bound included)
        hipLaunchKernelGGL(surf_none_kernel, dim3(blocks(N)), dim3(SF_THREADS), 0, st, N, face, d2, bary);
        return launch_status();
    }
    if (isinf(max_d2)) {
        hipLaunchKernelGGL(surf_brute_kernel, dim3(blocks(N)), dim3(SF_THREADS), 0, st, N, V, F, points, verts, faces, max_d2, face, d2,
                           bary);
        return launch_status();
    }
    if (!scratch) return fail("surf_closest: NULL scratch");
    if ((long long)F * REFS_PER_FACE > 0x7fffffffLL) return fail("surf_closest: too many faces for the grid (8 F must stay below 2^31)");
    const SurfLayout L = surf_layout(N, F);
    char* base = align_ptr(scratch);
    float* partial = (float*)(base + L.partial);
    GridParams* gp = (GridParams*)(base + L.params);
    float4* tri = (float4*)(base + L.tri);
    float4* box = (float4*)(base + L.box);
    unsigned *cnt = (unsigned*)(base + L.cnt), *start = (unsigned*)(base + L.start), *cursor = (unsigned*)(base + L.cursor);
    unsigned *refs = (unsigned*)(base + L.refs), *tiles = (unsigned*)(base + L.tiles);
    unsigned *keysA = (unsigned*)(base + L.keysA), *valsA = (unsigned*)(base + L.valsA);
    unsigned *keysB = (unsigned*)(base + L.keysB), *valsB = (unsigned*)(base + L.valsB);
    const unsigned mask = (unsigned)(L.H - 1);
    if (hipMemsetAsync(cnt, 0, L.H * 4, st) != hipSuccess) return fail("surf_closest: memset failed");
    hipLaunchKernelGGL(face_prep_kernel, dim3(blocks(F)), dim3(SF_THREADS), 0, st, V, F, verts, faces, tri, box);
    const int nparts = F < BOX_PARTS * 256 ? (F + 255) / 256 : BOX_PARTS;
    hipLaunchKernelGGL(box_partial_kernel, dim3(nparts), dim3(256), 0, st, F, (const float4*)tri, partial);
    hipLaunchKernelGGL(grid_params_kernel<7>, dim3(1), dim3(64), 0, st, nparts, (const float*)partial, max_d2, gp);
    hipLaunchKernelGGL(face_count_kernel, dim3(blocks(F)), dim3(SF_THREADS), 0, st, F, (const float4*)tri, (const GridParams*)gp, mask, cnt);
    scan_exclusive(st, (long long)L.H, cnt, tiles, tiles + L.nb, start, cursor, true, start + L.H);
    hipLaunchKernelGGL(face_scatter_kernel, dim3(blocks(F)), dim3(SF_THREADS), 0, st, F, (const float4*)tri, (const GridParams*)gp, mask,
                       cursor, (unsigned)((size_t)F * REFS_PER_FACE), refs);
    hipLaunchKernelGGL(query_key_kernel, dim3(blocks(N)), dim3(SF_THREADS), 0, st, N, points, (const GridParams*)gp, keysA, valsA);
    const unsigned* order = radix_sort_pairs(st, N, 2, keysA, valsA, keysB, valsB, (unsigned*)(base + L.hist), (unsigned*)(base + L.scanned));
    hipLaunchKernelGGL(surf_grid_kernel, dim3(blocks(N)), dim3(SF_THREADS), 0, st, N, F, points, order, (const GridParams*)gp, mask,
                       (const unsigned*)start, (const unsigned*)refs, (const float4*)tri, (const float4*)box, max_d2, face,
                       d2, bary);
    return launch_status();
}

int dgm_surf_interp(int N, int V, int F, int C, const float* attr, const int* faces, const int* face, const float* bary, float fill,
                    float* out, void* stream) {
    if (N < 0 || V < 0 || F < 0 || C < 1) return fail("surf_interp: need N >= 0, V >= 0, F >= 0 and C >= 1");
    if (N == 0) return 0;  // (before any HIP call)
    if (!face || !bary || !out || (F > 0 && !faces) || (F > 0 && V > 0 && !attr)) return fail("surf_interp: NULL pointer");
    const long long total = (long long)N * C;
    hipLaunchKernelGGL(surf_interp_kernel, dim3(blocks(total)), dim3(SF_THREADS), 0, (hipStream_t)stream, total, V, F, C, attr, faces, face,
                       bary, fill, out);
    return launch_status();
}

int dgm_corr_palette(int N, const float* xyz, const float* center, const float* scale, int mode, int cells, float* out, void* stream) {
    if (N < 0) return fail("corr_palette: need N >= 0");
    if (mode != 0 && mode != 1) return fail("corr_palette: mode must be 0 (rgb) or 1 (checker)");
    if (cells < 1 || cells > 4096) return fail("corr_palette: cells must be within [1, 4096]");
    if (N == 0) return 0;  // (before any HIP call)
    if (!xyz || !center || !scale || !out) return fail("corr_palette: NULL pointer");
    hipLaunchKernelGGL(palette_kernel, dim3(blocks(N)), dim3(SF_THREADS), 0, (hipStream_t)stream, N, xyz, center, scale, mode, cells, out);
    return launch_status();
}

}  // extern "C"
