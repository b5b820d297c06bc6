// Gaussian-mesh anchoring for gfx950: face geometry, an exact bounded nearest-neighbour search and the per-face bookkeeping of
// GaussianModelDPSRDynamicAnchor.anchor_mesh (R/scene/gaussian_model_dpsr_dynamic_anchor.py:745-829; R/ = dgmesh/).  The reference
// copies the mesh to the host for trimesh (triangles_center, face_normals) and matches every Gaussian to its nearest face centroid
// with pytorch3d.knn_points(K=1), a brute force over P x F pairs.
//
// Nearest neighbour (queries -> targets):
//   d2 = (dx*dx + dy*dy) + dz*dz in fp32 without FMA (this file is built with -ffp-contract=off); idx[q] = the target with the least
//   d2, ties to the smallest target index, reported only when d2 < max_d2 (strict), else idx = -1 and d2 = +inf.  The answer is the
//   lexicographic minimum of (d2, index) over a candidate set that contains every target with d2 < max_d2, so it does not depend on
//   the order in which candidates are visited (the grid below is filled with atomics) and is bit-reproducible.
//   * finite max_d2: a hashed uniform grid over the targets with cell edge c = 1.001 sqrt(max_d2) (at least 2^-20 of the targets'
//     bounding-box extent, so that cell coordinates stay below 2^20).  Cell coordinates are taken in fp64 from the fp32 points, so a
//     target with fp32 d2 < max_d2 lies within one cell of the query's cell on every axis: the 27 cells around the query hold it.
//     Cells hash into a table of 2^k >= Nt buckets; a collision only adds candidates.  The table is built by histogram, scan
//     (mesh_scan.hpp) and scatter, its cells are those of mesh_grid.hpp; the queries are visited in the order of their own bucket so that the lanes of a wave mostly scan the same cells.
//   * max_d2 = +inf: a tiled brute force (256 targets per LDS tile, one query per lane) -- the unbounded knn_points(K=1).
// Scratch is caller-owned; nothing here allocates device memory or reads anything back to the host.
#include <float.h>
#include <math.h>

#include "dgm_host.hpp"
#include "mesh_grid.hpp"
#include "mesh_scan.hpp"

#pragma clang fp contract(off)

namespace {
using namespace dgm;

constexpr int AN_THREADS = 256;
constexpr int BF_TILE = 256;  // targets per LDS tile of the brute force
constexpr int BBOX_PARTS = 128;

// ---- face geometry -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AN_THREADS)
face_geometry_kernel(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, float* __restrict__ cent,
                     float* __restrict__ nrm) {
    const long long f = (long long)blockIdx.x * AN_THREADS + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {  // an index out of range: a face that no query can choose
        const float nan = __int_as_float(0x7fc00000);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            cent[3 * f + k] = nan;
            nrm[3 * f + k] = 0.f;
        }
        return;
    }
    float p0[3], p1[3], p2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        p0[k] = verts[3 * (long long)a + k];
        p1[k] = verts[3 * (long long)b + k];
        p2[k] = verts[3 * (long long)c + k];
        cent[3 * f + k] = ((p0[k] + p1[k]) + p2[k]) / 3.0f;
    }
    const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    const bool ok = len > 0.f;
    nrm[3 * f] = ok ? nx / len : 0.f;
    nrm[3 * f + 1] = ok ? ny / len : 0.f;
    nrm[3 * f + 2] = ok ? nz / len : 0.f;
}

// ---- grid helpers --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BOX_THREADS) bbox_partial_kernel(int n, const float* __restrict__ pts, float* __restrict__ partial) {
    float v[6];
    box_start<6>(v);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {  // ends at n
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float x = pts[3 * i + a];
            v[a] = box_join(a, v[a], x);
            v[3 + a] = box_join(3 + a, v[3 + a], x);
        }
    }
    box_reduce_partial<6>(v, partial);
}

// bucket of every point (targets: into `mask + 1` buckets; queries: the same hash into their own table), counted
__global__ void __launch_bounds__(AN_THREADS)
bucket_count_kernel(int n, const float* __restrict__ pts, const GridParams* __restrict__ gp, unsigned mask, unsigned* __restrict__ key,
                    unsigned* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * AN_THREADS + threadIdx.x;
    if (i >= n) return;
    const double inv = gp->inv;
    const unsigned b = cell_hash(cell_coord(pts[3 * i], gp->origin[0], inv), cell_coord(pts[3 * i + 1], gp->origin[1], inv),
                                 cell_coord(pts[3 * i + 2], gp->origin[2], inv), mask);
    key[i] = b;
    atomicAdd(&cnt[b], 1u);
}

__global__ void __launch_bounds__(AN_THREADS)
target_scatter_kernel(int n, const float* __restrict__ pts, const unsigned* __restrict__ key, unsigned* __restrict__ cursor,
                      float4* __restrict__ sorted) {
    const long long i = (long long)blockIdx.x * AN_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned at = atomicAdd(&cursor[key[i]], 1u);
    sorted[at] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], __int_as_float((int)i));
}

__global__ void __launch_bounds__(AN_THREADS)
query_scatter_kernel(int n, const unsigned* __restrict__ key, unsigned* __restrict__ cursor, unsigned* __restrict__ order) {
    const long long i = (long long)blockIdx.x * AN_THREADS + threadIdx.x;
    if (i >= n) return;
    order[atomicAdd(&cursor[key[i]], 1u)] = (unsigned)i;
}

__device__ __forceinline__ void consider(float qx, float qy, float qz, float4 c, float& best, int& bi) {
    const float dx = c.x - qx, dy = c.y - qy, dz = c.z - qz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const int j = __float_as_int(c.w);
    if (d2 < best || (d2 == best && j < bi)) {  // bi == -1: only d2 < max_d2 admits the first candidate
        best = d2;
        bi = j;
    }
}

__global__ void __launch_bounds__(AN_THREADS)
grid_query_kernel(int Nq, const float* __restrict__ q, const unsigned* __restrict__ order, const GridParams* __restrict__ gp,
                  unsigned mask, const unsigned* __restrict__ start, const float4* __restrict__ sorted, float max_d2,
                  int* __restrict__ idx, float* __restrict__ d2out) {
    const long long i = (long long)blockIdx.x * AN_THREADS + threadIdx.x;
    if (i >= Nq) return;
    const unsigned qi = order[i];
    const float qx = q[3 * (long long)qi], qy = q[3 * (long long)qi + 1], qz = q[3 * (long long)qi + 2];
    const double inv = gp->inv;
    const int cx = cell_coord(qx, gp->origin[0], inv), cy = cell_coord(qy, gp->origin[1], inv), cz = cell_coord(qz, gp->origin[2], inv);
    float best = max_d2;
    int bi = -1;
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const unsigned b = cell_hash(cx + dx, cy + dy, cz + dz, mask);
                const unsigned j1 = start[b + 1];
                for (unsigned j = start[b]; j < j1; j++) consider(qx, qy, qz, sorted[j], best, bi);
            }
    idx[qi] = bi;
    d2out[qi] = bi >= 0 ? best : INFINITY;
}

__global__ void __launch_bounds__(AN_THREADS)
brute_query_kernel(int Nq, int Nt, const float* __restrict__ q, const float* __restrict__ t, float max_d2, int* __restrict__ idx,
                   float* __restrict__ d2out) {
    __shared__ float4 tile[BF_TILE];
    const long long i = (long long)blockIdx.x * AN_THREADS + threadIdx.x;
    const bool act = i < Nq;
    const float qx = act ? q[3 * i] : 0.f, qy = act ? q[3 * i + 1] : 0.f, qz = act ? q[3 * i + 2] : 0.f;
    float best = max_d2;
    int bi = -1;
    for (int base = 0; base < Nt; base += BF_TILE) {
        const int j = base + (int)threadIdx.x;
        if (j < Nt) tile[threadIdx.x] = make_float4(t[3 * (long long)j], t[3 * (long long)j + 1], t[3 * (long long)j + 2], __int_as_float(j));
        __syncthreads();
        const int m = min(BF_TILE, Nt - base);
        for (int k = 0; k < m; k++) consider(qx, qy, qz, tile[k], best, bi);
        __syncthreads();
    }
    if (act) {
        idx[i] = bi;
        d2out[i] = bi >= 0 ? best : INFINITY;
    }
}

__global__ void __launch_bounds__(AN_THREADS) nn_none_kernel(int Nq, int* __restrict__ idx, float* __restrict__ d2out) {
    const long long i = (long long)blockIdx.x * AN_THREADS + threadIdx.x;
    if (i >= Nq) return;
    idx[i] = -1;
    d2out[i] = INFINITY;
}

struct NnLayout {
    size_t partial, params, cnt_t, start_t, cursor_t, key_t, sorted, cnt_q, start_q, key_q, order, tiles, total;
    size_t Ht, Hq;
};

NnLayout nn_layout(int Nq, int Nt) {
    NnLayout L;
    L.Ht = pow2_at_least((size_t)Nt);
    L.Hq = pow2_at_least((size_t)Nq);
    const size_t nb = (size_t)scan_tiles((long long)(L.Ht > L.Hq ? L.Ht : L.Hq));
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    };
    L.partial = take(BBOX_PARTS * 6 * 4);
    L.params = take(sizeof(GridParams));
    L.cnt_t = take(L.Ht * 4);
    L.start_t = take((L.Ht + 1) * 4);
    L.cursor_t = take((L.Ht > L.Hq ? L.Ht : L.Hq) * 4);  // (the targets' cursors, then the queries')
    L.key_t = take((size_t)Nt * 4);
    L.sorted = take((size_t)Nt * 16);
    L.cnt_q = take(L.Hq * 4);
    L.start_q = take((L.Hq + 1) * 4);
    L.key_q = take((size_t)Nq * 4);
    L.order = take((size_t)Nq * 4);
    L.tiles = take(2 * nb * 4);
    L.total = o + 256;  // (+256: the caller's pointer is aligned up)
    return L;
}

// exclusive scan of cnt[0, H) into start[0, H] (start[H] = the total) and cursor[0, H)
void scan_counts(hipStream_t st, size_t H, const unsigned* cnt, unsigned* start, unsigned* cursor, unsigned* tiles) {
    scan_exclusive(st, (long long)H, cnt, tiles, tiles + scan_tiles((long long)H), start, cursor, true, start + H);
}

// ---- classification ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AN_THREADS)
face_count_kernel(int P, int F, const int* __restrict__ face_of, unsigned* __restrict__ counts, unsigned* __restrict__ key,
                  unsigned* __restrict__ val) {
    const long long g = (long long)blockIdx.x * AN_THREADS + threadIdx.x;
    if (g >= P) return;
    const int f = face_of[g];
    const bool ok = f >= 0 && f < F;
    if (ok) atomicAdd(&counts[f], 1u);
    key[g] = ok ? (unsigned)f : (unsigned)F;  // (invalid Gaussians sort behind every face)
    val[g] = (unsigned)g;
}

struct FaceClass {  // (count, is 1-1, is n-1) of a face
    const unsigned* counts;
    __device__ void operator()(long long f, unsigned* x) const {
        const unsigned c = counts[f];
        x[0] = c;
        x[1] = c == 1u ? 1u : 0u;
        x[2] = c > 1u ? 1u : 0u;
    }
};
struct FaceEmit {
    int* offsets;
    int* lists;
    const unsigned* totals;  // (n11, nn1) after the tile scan
    __device__ void operator()(long long f, const unsigned* v, const unsigned* pre) const {
        offsets[f] = (int)pre[0];
        const unsigned n11 = totals[1], nn1 = totals[2];
        long long at;
        if (v[1])
            at = pre[1];
        else if (v[2])
            at = (long long)n11 + pre[2];
        else
            at = (long long)n11 + nn1 + (f - pre[1] - pre[2]);
        lists[at] = (int)f;
    }
};

// totals: [0] valid Gaussians, [1] 1-1 faces, [2] n-1 faces (written by the tile scans); the caller's int4 from them
__global__ void totals_kernel(int F, const unsigned* __restrict__ t, int* __restrict__ out) {
    if (threadIdx.x != 0) return;
    out[0] = (int)t[1];
    out[1] = (int)t[2];
    out[2] = F - (int)t[1] - (int)t[2];
    out[3] = (int)t[0];
}

__global__ void __launch_bounds__(AN_THREADS)
rank_kernel(int P, int F, const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, const int* __restrict__ offsets,
            int* __restrict__ members, int* __restrict__ rank) {
    const long long j = (long long)blockIdx.x * AN_THREADS + threadIdx.x;
    if (j >= P) return;
    const unsigned f = keys[j], g = vals[j];
    const bool ok = f < (unsigned)F;
    members[j] = ok ? (int)g : -1;
    rank[g] = ok ? (int)(j - offsets[f]) : -1;
}

struct ClassifyLayout {
    size_t keysA, valsA, keysB, valsB, hist, scanned, tiles, tot, total;
    int nb;
};

ClassifyLayout classify_layout(int P, int F) {
    ClassifyLayout L;
    L.nb = scan_tiles(F);
    const size_t n = (size_t)P, hw = radix_sort_hist_words(P);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t at = o;
        o = align_up(o + bytes, 256);
        return at;
    };
    L.keysA = take(n * 4);
    L.valsA = take(n * 4);
    L.keysB = take(n * 4);
    L.valsB = take(n * 4);
    L.hist = take(hw * 4);
    L.scanned = take(hw * 4);
    L.tiles = take((size_t)(L.nb > 0 ? L.nb : 1) * 6 * 4);
    L.tot = take(4 * 4);
    L.total = o + 256;
    return L;
}

}  // namespace

extern "C" {

int dgm_anchor_face_geometry(int V, int F, const float* verts, const int* faces, float* centroids, float* normals, void* stream) {
    if (V < 0 || F < 0) return fail("anchor_face_geometry: need V >= 0 and F >= 0");
    if (F == 0) return launch_status();
    if (!faces || !centroids || !normals || (V > 0 && !verts)) return fail("anchor_face_geometry: NULL pointer");
    hipLaunchKernelGGL(face_geometry_kernel, dim3(blocks(F)), dim3(AN_THREADS), 0, (hipStream_t)stream, V, F, verts, faces, centroids,
                       normals);
    return launch_status();
}

size_t dgm_anchor_nn_scratch_bytes(int Nq, int Nt) {
    if (Nq < 0 || Nt < 0) return 0;
    return nn_layout(Nq, Nt).total;
}

int dgm_anchor_nn(int Nq, int Nt, const float* queries, const float* targets, float max_d2, char* scratch, int* idx, float* d2,
                  void* stream) {
    if (Nq < 0 || Nt < 0) return fail("anchor_nn: need Nq >= 0 and Nt >= 0");
    if (Nq == 0) return launch_status();
    if (!queries || !idx || !d2 || (Nt > 0 && !targets)) return fail("anchor_nn: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (Nt == 0 || !(max_d2 > 0.f)) {  // nothing can be reported (NaN bound included)
        hipLaunchKernelGGL(nn_none_kernel, dim3(blocks(Nq)), dim3(AN_THREADS), 0, st, Nq, idx, d2);
        return launch_status();
    }
    if (isinf(max_d2)) {
        hipLaunchKernelGGL(brute_query_kernel, dim3(blocks(Nq)), dim3(AN_THREADS), 0, st, Nq, Nt, queries, targets, max_d2, idx, d2);
        return launch_status();
    }
    if (!scratch) return fail("anchor_nn: NULL scratch");
    const NnLayout L = nn_layout(Nq, Nt);
    char* base = align_ptr(scratch);
    float* partial = (float*)(base + L.partial);
    GridParams* gp = (GridParams*)(base + L.params);
    unsigned *cnt_t = (unsigned*)(base + L.cnt_t), *start_t = (unsigned*)(base + L.start_t), *cursor_t = (unsigned*)(base + L.cursor_t);
    unsigned *key_t = (unsigned*)(base + L.key_t), *cnt_q = (unsigned*)(base + L.cnt_q), *start_q = (unsigned*)(base + L.start_q);
    unsigned *key_q = (unsigned*)(base + L.key_q), *order = (unsigned*)(base + L.order), *tiles = (unsigned*)(base + L.tiles);
    float4* sorted = (float4*)(base + L.sorted);
    const unsigned mask_t = (unsigned)(L.Ht - 1), mask_q = (unsigned)(L.Hq - 1);
    if (hipMemsetAsync(cnt_t, 0, L.Ht * 4, st) != hipSuccess || hipMemsetAsync(cnt_q, 0, L.Hq * 4, st) != hipSuccess)
        return fail("anchor_nn: memset failed");
    const int nparts = Nt < BBOX_PARTS * 256 ? (Nt + 255) / 256 : BBOX_PARTS;
    hipLaunchKernelGGL(bbox_partial_kernel, dim3(nparts), dim3(256), 0, st, Nt, targets, partial);
    hipLaunchKernelGGL(grid_params_kernel<6>, dim3(1), dim3(64), 0, st, nparts, (const float*)partial, max_d2, gp);
    hipLaunchKernelGGL(bucket_count_kernel, dim3(blocks(Nt)), dim3(AN_THREADS), 0, st, Nt, targets, (const GridParams*)gp, mask_t, key_t,
                       cnt_t);
    hipLaunchKernelGGL(bucket_count_kernel, dim3(blocks(Nq)), dim3(AN_THREADS), 0, st, Nq, queries, (const GridParams*)gp, mask_q, key_q,
                       cnt_q);
    scan_counts(st, L.Ht, cnt_t, start_t, cursor_t, tiles);
    hipLaunchKernelGGL(target_scatter_kernel, dim3(blocks(Nt)), dim3(AN_THREADS), 0, st, Nt, targets, (const unsigned*)key_t, cursor_t,
                       sorted);
    scan_counts(st, L.Hq, cnt_q, start_q, cursor_t, tiles);  // (the targets' cursors are spent: reused for the queries)
    hipLaunchKernelGGL(query_scatter_kernel, dim3(blocks(Nq)), dim3(AN_THREADS), 0, st, Nq, (const unsigned*)key_q, cursor_t, order);
    hipLaunchKernelGGL(grid_query_kernel, dim3(blocks(Nq)), dim3(AN_THREADS), 0, st, Nq, queries, (const unsigned*)order,
                       (const GridParams*)gp, mask_t, (const unsigned*)start_t, (const float4*)sorted, max_d2, idx, d2);
    return launch_status();
}

size_t dgm_anchor_classify_scratch_bytes(int P, int F) {
    if (P < 0 || F < 0) return 0;
    return classify_layout(P, F).total;
}

int dgm_anchor_classify(int P, int F, const int* face_of, char* scratch, int* counts, int* offsets, int* lists, int* members, int* rank,
                        int* totals, void* stream) {
    if (P < 0 || F < 0) return fail("anchor_classify: need P >= 0 and F >= 0");
    if (!scratch || !totals || (P > 0 && (!face_of || !members || !rank)) || (F > 0 && (!counts || !offsets || !lists)))
        return fail("anchor_classify: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const ClassifyLayout L = classify_layout(P, F);
    char* base = align_ptr(scratch);
    unsigned *keysA = (unsigned*)(base + L.keysA), *valsA = (unsigned*)(base + L.valsA);
    unsigned *keysB = (unsigned*)(base + L.keysB), *valsB = (unsigned*)(base + L.valsB);
    unsigned *tiles = (unsigned*)(base + L.tiles), *tot = (unsigned*)(base + L.tot);
    if (hipMemsetAsync(tot, 0, 16, st) != hipSuccess || (F > 0 && hipMemsetAsync(counts, 0, (size_t)F * 4, st) != hipSuccess))
        return fail("anchor_classify: memset failed");
    if (P > 0)
        hipLaunchKernelGGL(face_count_kernel, dim3(blocks(P)), dim3(AN_THREADS), 0, st, P, F, face_of, (unsigned*)counts, keysA, valsA);
    if (F > 0) {
        scan_exclusive<3>(st, (long long)F, FaceClass{(const unsigned*)counts}, FaceEmit{offsets, lists, (const unsigned*)tot}, tiles,
                          tiles + 3 * L.nb, tot);
    }
    hipLaunchKernelGGL(totals_kernel, dim3(1), dim3(64), 0, st, F, (const unsigned*)tot, totals);
    if (P > 0) {
        int bits = 0;
        while (bits < 32 && ((unsigned)F >> bits) != 0u) bits++;  // keys are <= F
        const int passes = bits > 0 ? (bits + 7) / 8 : 1;
        const unsigned* vals = radix_sort_pairs(st, P, passes, keysA, valsA, keysB, valsB, (unsigned*)(base + L.hist),
                                                (unsigned*)(base + L.scanned));
        const unsigned* keys = vals == valsA ? keysA : keysB;
        hipLaunchKernelGGL(rank_kernel, dim3(blocks(P)), dim3(AN_THREADS), 0, st, P, F, keys, vals, (const int*)offsets, members, rank);
    }
    return launch_status();
}

}  // extern "C"
