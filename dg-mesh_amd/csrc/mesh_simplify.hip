// Simplifying an extracted triangle mesh for gfx950: uniform-grid vertex clustering with quadric-error placement (Lindstrom,
// "Out-of-core simplification of large polygonal models", SIGGRAPH 2000), which with a tiny cell is also pymeshlab's
// meshing_merge_close_vertices + meshing_remove_duplicate_faces + meshing_remove_null_faces of the reference's clean_mesh
// (R/scene/gaussian_model.py:603-697; R/ = dgmesh/).  DESIGN.md section 4.15; include/dgmesh_hip.h states the definitions.
//
//   box       a face is VALID iff its indices are in [0, V) and pairwise different and its nine coordinates are finite.  The box is
//             the min / max over the corners of the valid faces, on the order-preserving integer encoding of mesh_clean.hip: merged
//             per workgroup into a box of its own, the boxes by one more workgroup.  No atomics, no float arithmetic.
//   cluster   every used vertex gets its 64-bit cell key (fp32, correctly rounded subtract and divide, no contraction); an open-addressing
//             table maps key -> the smallest vertex index of the cell (64-bit CAS on the key, atomicMin on the index: the slot a key
//             lands in depends on arrival order, the index it ends with does not).  rep[v] = that index, -1 for an unused vertex.
//   remap     every valid face through rep; NULL when two corners share a cluster.  The others go into a second table whose slots are
//             claimed with the face's own index (CAS) and compared through the owner's remapped triple, written by the launch
//             before; atomicMin keeps the smallest face index of every unordered triple, and a face that is not that one is a
//             DUPLICATE.  No packing of the triple: no limit on the number of clusters.
//   compact   dgm_mesh_compact_count / dgm_mesh_compact_emit of mesh_clean.hip, unchanged, on (placed vertices, remapped faces in OLD
//             vertex indices, keep): the survivors in the order of their representatives, clusters without a face dropped.
//   place     an inverted index cluster -> its valid faces (each once): int32 atomic counts, an exclusive scan over fixed tiles, an
//             atomic fill, then every list put into ascending face order by ranking (an entry's place is the number of smaller
//             entries of its list: any length, no workgroup-sized limit).  One thread per cluster then adds the quadric in fp64 in
//             that order and solves the regularised 3x3 system by Cholesky.  No float is ever added by an atomic.
//
// Termination.  No workgroup waits for another and nothing spins on a flag.  Every device loop below names what ends it.
// Visibility.  Inside a launch the two tables are read and written with agent-scope atomics only; everything else a kernel reads was
// written by an earlier launch on the same stream.
// Scratch is caller-owned; nothing here allocates device memory or reads anything back to the host.
#include <float.h>
#include <math.h>
#include <stdio.h>

#include "dgm_host.hpp"
#include "mesh_scan.hpp"

#pragma clang fp contract(off)

namespace {
using namespace dgm;

constexpr int SP_THREADS = 256;
constexpr int SP_ITEMS = 16;
constexpr int SP_TILE = SP_THREADS * SP_ITEMS;  // integers per workgroup of the offset scan: its fixed partition
static_assert(SP_TILE == SCAN_TILE, "the scratch layout counts the tiles of mesh_scan.hpp");
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_MAX_DIM = 1 << 20;
constexpr unsigned long long KEY_EMPTY = ~0ull;
constexpr int SLOT_EMPTY = -1;

int tiles(long long n) { return (int)((n + SP_TILE - 1) / SP_TILE); }


#define AGENT __HIP_MEMORY_SCOPE_AGENT

// order-preserving float <-> unsigned, as mesh_clean.hip (-0 < +0)
__device__ __forceinline__ unsigned f2key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {  // (splitmix64's finaliser)
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

struct Grid {
    float ox, oy, oz, h;
    int nx, ny, nz;
};

// ---- box -------------------------------------------------------------------------------------------------------------------------
// every workgroup stores its own encoded box (6 words; the empty box where it has no valid face): no word is shared between workgroups
__global__ void __launch_bounds__(SP_THREADS)
sp_box_kernel(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, unsigned char* __restrict__ fvalid,
              int* __restrict__ used, unsigned* __restrict__ partial) {
    __shared__ unsigned lds[SP_WAVES][6];
    const long long f = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    if (f < F) {
        const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        // checked before anything is dereferenced with them
        bool ok = idx[0] >= 0 && idx[0] < V && idx[1] >= 0 && idx[1] < V && idx[2] >= 0 && idx[2] < V && idx[0] != idx[1] &&
                  idx[1] != idx[2] && idx[0] != idx[2];
        if (ok) {
            float p[9];
#pragma unroll
            for (int c = 0; c < 3; c++)
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    p[3 * c + a] = verts[3 * (long long)idx[c] + a];
                    ok = ok && finite_f(p[3 * c + a]);
                }
            if (ok) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    used[idx[c]] = 1;  // (racing stores of one value)
#pragma unroll
                    for (int a = 0; a < 3; a++) {
                        const unsigned k = f2key(p[3 * c + a]);
                        mn[a] = k < mn[a] ? k : mn[a];
                        mx[a] = k > mx[a] ? k : mx[a];
                    }
                }
            }
        }
        fvalid[f] = ok ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const unsigned on = __shfl_xor(mn[a], off), ox = __shfl_xor(mx[a], off);
            mn[a] = on < mn[a] ? on : mn[a];
            mx[a] = ox > mx[a] ? ox : mx[a];
        }
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) lds[threadIdx.x >> 6][a] = mn[a], lds[threadIdx.x >> 6][3 + a] = mx[a];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned r = lds[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < SP_WAVES; w++) {
            const unsigned o = lds[w][threadIdx.x];
            r = threadIdx.x < 3 ? (o < r ? o : r) : (o > r ? o : r);
        }
        partial[6 * (long long)blockIdx.x + threadIdx.x] = r;
    }
}

// one workgroup: min / max over the workgroups' boxes (any order: integers), encoded into box[0..5] for the later calls and decoded
// into `out`; no valid face: (+inf, -inf)
__global__ void __launch_bounds__(SP_THREADS)
sp_box_reduce_kernel(int nb, const unsigned* __restrict__ partial, unsigned* __restrict__ box, float* __restrict__ out) {
    __shared__ unsigned lds[SP_WAVES][6];
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    for (int b = threadIdx.x; b < nb; b += SP_THREADS) {  // (ends: b grows by a constant)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const unsigned kn = partial[6 * (long long)b + a], kx = partial[6 * (long long)b + 3 + a];
            mn[a] = kn < mn[a] ? kn : mn[a];
            mx[a] = kx > mx[a] ? kx : mx[a];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const unsigned on = __shfl_xor(mn[a], off), ox = __shfl_xor(mx[a], off);
            mn[a] = on < mn[a] ? on : mn[a];
            mx[a] = ox > mx[a] ? ox : mx[a];
        }
    }
    if (lane_id() == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) lds[threadIdx.x >> 6][a] = mn[a], lds[threadIdx.x >> 6][3 + a] = mx[a];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned r = lds[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < SP_WAVES; w++) {
            const unsigned o = lds[w][threadIdx.x];
            r = threadIdx.x < 3 ? (o < r ? o : r) : (o > r ? o : r);
        }
        box[threadIdx.x] = r;
        lds[0][threadIdx.x] = r;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const bool empty = lds[0][0] == 0xffffffffu && lds[0][3] == 0u;
        out[threadIdx.x] = empty ? (threadIdx.x < 3 ? INFINITY : -INFINITY) : key2f(lds[0][threadIdx.x]);
    }
}

// ---- cells and clusters ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_THREADS)
sp_table_init_kernel(long long cap, unsigned long long* __restrict__ tkey, int* __restrict__ trep) {
    const long long i = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= cap) return;
    tkey[i] = KEY_EMPTY;
    trep[i] = 0x7fffffff;
}

// idx = min(n - 1, floor((x - o) / h)), fp32, in this order
__device__ __forceinline__ int cell_axis(float x, float o, float h, int n) {
    const float d = x - o;
    const float q = floorf(d / h);
    const float top = (float)(n - 1);  // (n <= 2^20: exact)
    return q >= top ? n - 1 : (q > 0.f ? (int)q : 0);
}

__device__ __forceinline__ unsigned long long cell_key(const Grid& g, const float* __restrict__ p) {
    const int ix = cell_axis(p[0], g.ox, g.h, g.nx), iy = cell_axis(p[1], g.oy, g.h, g.ny), iz = cell_axis(p[2], g.oz, g.h, g.nz);
    return ((unsigned long long)iz * (unsigned long long)g.ny + (unsigned long long)iy) * (unsigned long long)g.nx + (unsigned long long)ix;
}

__global__ void __launch_bounds__(SP_THREADS)
sp_cell_insert_kernel(int V, const float* __restrict__ verts, const int* __restrict__ used, Grid g, long long cap,
                      unsigned long long* tkey, int* trep, unsigned long long* __restrict__ vkey) {
    const long long v = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V || !used[v]) return;
    const unsigned long long key = cell_key(g, verts + 3 * v);
    vkey[v] = key;
    long long slot = (long long)(mix64(key) & (unsigned long long)(cap - 1));
    // ends: `step` grows by one, cap steps at the most; cap > the number of keys, so an empty slot or the key's own is met before
    for (long long step = 0; step < cap; step++) {
        unsigned long long cur = __hip_atomic_load(tkey + slot, __ATOMIC_RELAXED, AGENT);
        if (cur == KEY_EMPTY) {
            unsigned long long expected = KEY_EMPTY;
            cur = __hip_atomic_compare_exchange_strong(tkey + slot, &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, AGENT) ? key : expected;
        }
        if (cur == key) {
            __hip_atomic_fetch_min(trep + slot, (int)v, __ATOMIC_RELAXED, AGENT);
            return;
        }
        slot = (slot + 1) & (cap - 1);
    }
}

__global__ void __launch_bounds__(SP_THREADS)
sp_cell_lookup_kernel(int V, const int* __restrict__ used, const unsigned long long* __restrict__ vkey, long long cap,
                      const unsigned long long* __restrict__ tkey, const int* __restrict__ trep, int* __restrict__ rep) {
    const long long v = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V) return;
    int r = -1;
    if (used[v]) {
        const unsigned long long key = vkey[v];
        long long slot = (long long)(mix64(key) & (unsigned long long)(cap - 1));
        r = (int)v;  // (never kept: the key was inserted by the launch before)
        // ends: cap steps at the most; the table no longer changes
        for (long long step = 0; step < cap; step++) {
            const unsigned long long cur = tkey[slot];
            if (cur == key) {
                r = trep[slot];
                break;
            }
            if (cur == KEY_EMPTY) break;
            slot = (slot + 1) & (cap - 1);
        }
        if (r < 0 || r >= V) r = (int)v;
    }
    rep[v] = r;
}

// ---- faces -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_THREADS)
sp_remap_kernel(int V, int F, const int* __restrict__ faces, const unsigned char* __restrict__ fvalid, const int* __restrict__ rep,
                int* __restrict__ rep_faces, unsigned char* __restrict__ keep) {
    const long long f = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (f >= F) return;
    int a = -1, b = -1, c = -1;
    if (fvalid[f]) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        // (a valid face's indices are inside rep; checked again, should the caller hand other faces than the box call saw)
        if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) a = rep[i0], b = rep[i1], c = rep[i2];
        if (a < 0 || b < 0 || c < 0) a = b = c = -1;
    }
    rep_faces[3 * f] = a;
    rep_faces[3 * f + 1] = b;
    rep_faces[3 * f + 2] = c;
    keep[f] = (a >= 0 && a != b && b != c && a != c) ? 1 : 0;  // not invalid, not null; duplicates leave in sp_dup_flag_kernel
}

__global__ void __launch_bounds__(SP_THREADS) sp_dup_init_kernel(long long cap, int* __restrict__ owner, int* __restrict__ first) {
    const long long i = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= cap) return;
    owner[i] = SLOT_EMPTY;
    first[i] = 0x7fffffff;
}

struct Tri {
    int a, b, c;  // ascending
};
__device__ __forceinline__ Tri sorted_tri(const int* __restrict__ t) {
    int a = t[0], b = t[1], c = t[2], s;
    if (a > b) s = a, a = b, b = s;
    if (b > c) s = b, b = c, c = s;
    if (a > b) s = a, a = b, b = s;
    return {a, b, c};
}
__device__ __forceinline__ unsigned long long tri_hash(const Tri& t) {
    return mix64(mix64(((unsigned long long)(unsigned)t.a << 32) | (unsigned)t.b) ^ (unsigned long long)(unsigned)t.c);
}

// INSERT: claim the triple's slot with this face's index and lower first[slot] to it; otherwise only find the slot.
template <bool INSERT>
__device__ __forceinline__ long long dup_slot(int f, const int* __restrict__ rep_faces, long long cap, int* owner) {
    const Tri me = sorted_tri(rep_faces + 3 * (long long)f);
    long long slot = (long long)(tri_hash(me) & (unsigned long long)(cap - 1));
    // ends: cap steps at the most; cap > the number of faces, and a face claims one slot at the most, so an empty slot or the
    // triple's own is met before
    for (long long step = 0; step < cap; step++) {
        int cur = INSERT ? __hip_atomic_load(owner + slot, __ATOMIC_RELAXED, AGENT) : owner[slot];
        if (INSERT && cur == SLOT_EMPTY) {
            int expected = SLOT_EMPTY;
            cur = __hip_atomic_compare_exchange_strong(owner + slot, &expected, f, __ATOMIC_RELAXED, __ATOMIC_RELAXED, AGENT) ? f : expected;
        }
        if (cur == SLOT_EMPTY) return -1;
        if (cur == f) return slot;
        const Tri o = sorted_tri(rep_faces + 3 * (long long)cur);  // (the owner's triple: written by the launch before)
        if (o.a == me.a && o.b == me.b && o.c == me.c) return slot;
        slot = (slot + 1) & (cap - 1);
    }
    return -1;
}

__global__ void __launch_bounds__(SP_THREADS)
sp_dup_insert_kernel(int F, const int* __restrict__ rep_faces, const unsigned char* __restrict__ keep, long long cap, int* owner, int* first) {
    const long long f = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (f >= F || !keep[f]) return;
    const long long slot = dup_slot<true>((int)f, rep_faces, cap, owner);
    if (slot >= 0) __hip_atomic_fetch_min(first + slot, (int)f, __ATOMIC_RELAXED, AGENT);
}

__global__ void __launch_bounds__(SP_THREADS)
sp_dup_flag_kernel(int F, const int* __restrict__ rep_faces, long long cap, int* owner, const int* __restrict__ first,
                   unsigned char* __restrict__ keep) {
    const long long f = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (f >= F || !keep[f]) return;
    const long long slot = dup_slot<false>((int)f, rep_faces, cap, owner);
    if (slot >= 0 && first[slot] != (int)f) keep[f] = 0;
}

// ---- the inverted index cluster -> faces -----------------------------------------------------------------------------------------
// the distinct clusters of a valid face: 1 to 3
__device__ __forceinline__ int face_clusters(const int* __restrict__ t, int* r) {
    int n = 0;
    r[n++] = t[0];
    if (t[1] != t[0]) r[n++] = t[1];
    if (t[2] != t[0] && t[2] != t[1]) r[n++] = t[2];
    return n;
}

__global__ void __launch_bounds__(SP_THREADS)
sp_inst_count_kernel(int V, int F, const int* __restrict__ rep_faces, unsigned* __restrict__ count) {
    const long long f = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (f >= F || rep_faces[3 * f] < 0) return;
    int r[3];
    const int n = face_clusters(rep_faces + 3 * f, r);
    for (int k = 0; k < n; k++)
        if (r[k] >= 0 && r[k] < V) atomicAdd(count + r[k], 1u);
}

__global__ void __launch_bounds__(SP_THREADS)
sp_inst_fill_kernel(int V, int F, const int* __restrict__ rep_faces, const unsigned* __restrict__ offset, unsigned* __restrict__ cursor,
                    unsigned long long cap, int* __restrict__ inst_face, int* __restrict__ inst_rep) {
    const long long f = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (f >= F || rep_faces[3 * f] < 0) return;
    int r[3];
    const int n = face_clusters(rep_faces + 3 * f, r);
    for (int k = 0; k < n; k++) {
        if (r[k] < 0 || r[k] >= V) continue;
        const unsigned long long at = (unsigned long long)offset[r[k]] + atomicAdd(cursor + r[k], 1u);
        if (at < cap) {  // (cap = 3 F: the room of the two arrays)
            inst_face[at] = (int)f;
            inst_rep[at] = r[k];
        }
    }
}

// the place of an entry in its list = the number of smaller entries (the entries of one list are different faces)
__global__ void __launch_bounds__(SP_THREADS)
sp_inst_rank_kernel(int V, const unsigned* __restrict__ total, const int* __restrict__ inst_face, const int* __restrict__ inst_rep,
                    const unsigned* __restrict__ offset, const unsigned* __restrict__ count, int* __restrict__ sorted) {
    const unsigned long long i = (unsigned long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= total[0]) return;
    const int r = inst_rep[i];
    if (r < 0 || r >= V) return;
    const unsigned start = offset[r], len = count[r];
    const int mine = inst_face[i];
    unsigned rank = 0;
    for (unsigned j = 0; j < len; j++) rank += inst_face[(unsigned long long)start + j] < mine ? 1u : 0u;  // (ends: j grows to len)
    sorted[(unsigned long long)start + rank] = mine;  // (rank < len: `mine` is not smaller than itself)
}

// ---- placement -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_THREADS)
sp_place_kernel(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ rep,
                const unsigned long long* __restrict__ vkey, const unsigned* __restrict__ offset, const unsigned* __restrict__ count,
                const int* __restrict__ sorted, Grid g, double eps, float* __restrict__ placed) {
    const long long v = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V) return;
    if (rep[v] != (int)v) {  // not a representative: its row is never emitted
#pragma unroll
        for (int a = 0; a < 3; a++) placed[3 * v + a] = verts[3 * v + a];
        return;
    }
    const unsigned long long key = vkey[v];
    const unsigned long long nx = (unsigned long long)g.nx, ny = (unsigned long long)g.ny;
    const double h = (double)g.h;
    const double idx[3] = {(double)(key % nx), (double)((key / nx) % ny), (double)(key / (nx * ny))};
    const double o[3] = {(double)g.ox, (double)g.oy, (double)g.oz};
    double c[3];
#pragma unroll
    for (int a = 0; a < 3; a++) c[a] = o[a] + (idx[a] + 0.5) * h;

    double Axx = 0, Axy = 0, Axz = 0, Ayy = 0, Ayz = 0, Azz = 0, bx = 0, by = 0, bz = 0, gx = 0, gy = 0, gz = 0;
    const unsigned start = offset[v], len = count[v];
    for (unsigned j = 0; j < len; j++) {  // (ends: j grows to len)
        const int f = sorted[(unsigned long long)start + j];
        if (f < 0 || f >= F) continue;
        double p[3][3];
        bool inside = true;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const long long vi = faces[3 * (long long)f + k];  // (a listed face is valid: its indices are in range)
            inside = inside && vi >= 0 && vi < V;
#pragma unroll
            for (int a = 0; a < 3; a++) p[k][a] = inside ? (double)verts[3 * vi + a] : 0.0;
        }
        if (!inside) continue;
        const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        const double n0 = e1[1] * e2[2] - e1[2] * e2[1], n1 = e1[2] * e2[0] - e1[0] * e2[2], n2 = e1[0] * e2[1] - e1[1] * e2[0];
        const double d = -((n0 * (p[0][0] - c[0]) + n1 * (p[0][1] - c[1])) + n2 * (p[0][2] - c[2]));
        Axx += n0 * n0, Axy += n0 * n1, Axz += n0 * n2, Ayy += n1 * n1, Ayz += n1 * n2, Azz += n2 * n2;
        bx += n0 * d, by += n1 * d, bz += n2 * d;
        gx += ((p[0][0] + p[1][0]) + p[2][0]) / 3.0 - c[0];
        gy += ((p[0][1] + p[1][1]) + p[2][1]) / 3.0 - c[1];
        gz += ((p[0][2] + p[1][2]) + p[2][2]) / 3.0 - c[2];
    }
    double x[3] = {0, 0, 0};
    if (len > 0) {
        const double xh[3] = {gx / (double)len, gy / (double)len, gz / (double)len};
        const double mu = eps * ((Axx + Ayy) + Azz);
        if (!(mu > 0.0)) {  // (mu == 0; a NaN trace also lands here and places the centroid)
            x[0] = xh[0], x[1] = xh[1], x[2] = xh[2];
        } else {
            // (A + mu I) x = mu xh - b by Cholesky: the matrix is symmetric positive definite, condition <= 3 / eps
            const double m00 = Axx + mu, m11 = Ayy + mu, m22 = Azz + mu;
            const double r0 = mu * xh[0] - bx, r1 = mu * xh[1] - by, r2 = mu * xh[2] - bz;
            const double l00 = sqrt(m00);
            const double l10 = Axy / l00, l20 = Axz / l00;
            const double l11 = sqrt(m11 - l10 * l10);
            const double l21 = (Ayz - l20 * l10) / l11;
            const double l22 = sqrt(m22 - (l20 * l20 + l21 * l21));
            const double y0 = r0 / l00;
            const double y1 = (r1 - l10 * y0) / l11;
            const double y2 = (r2 - (l20 * y0 + l21 * y1)) / l22;
            x[2] = y2 / l22;
            x[1] = (y1 - l21 * x[2]) / l11;
            x[0] = (y0 - (l10 * x[1] + l20 * x[2])) / l00;
        }
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!(x[a] == x[a])) x[a] = xh[a];  // (an overflowed sum: the centroid)
            x[a] = x[a] < -h ? -h : (x[a] > h ? h : x[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) placed[3 * v + a] = (float)(c[a] + x[a]);
}

// ---- vert_map --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SP_THREADS) sp_newidx_kernel(int V, int Vn, const int* __restrict__ vert_index, int* __restrict__ newidx) {
    const long long i = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= Vn) return;
    const int r = vert_index[i];
    if (r >= 0 && r < V) newidx[r] = (int)i;
}

__global__ void __launch_bounds__(SP_THREADS)
sp_vert_map_kernel(int V, const int* __restrict__ rep, const int* __restrict__ newidx, int* __restrict__ vert_map) {
    const long long v = (long long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (v >= V) return;
    const int r = rep[v];
    vert_map[v] = (r >= 0 && r < V) ? newidx[r] : -1;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
long long pow2_at_least(long long n) {
    long long c = 64;
    while (c < n) c <<= 1;
    return c;
}

struct SimplifyScratch {
    unsigned* box;  // 6 encoded words, then total[0] at word 8
    unsigned char* fvalid;
    int *used, *rep, *trep, *owner, *first, *inst_face, *inst_rep, *sorted, *newidx;
    unsigned long long *vkey, *tkey;
    unsigned *count, *offset, *cursor, *tile_total, *tile_off, *partial;
    long long cap_v, cap_f;
    size_t bytes;
};

SimplifyScratch simplify_layout(char* scratch, int V, int F) {
    SimplifyScratch s;
    char* base = align_ptr(scratch);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char* at = base + o;
        o = align_up(o + bytes, 256);
        return at;
    };
    s.cap_v = pow2_at_least(2 * (long long)V);
    s.cap_f = pow2_at_least(2 * (long long)F);
    const size_t nb = (size_t)tiles(V) + 1;
    s.box = (unsigned*)take(64);
    s.fvalid = (unsigned char*)take((size_t)F);
    s.used = (int*)take((size_t)V * 4);
    s.rep = (int*)take((size_t)V * 4);
    s.vkey = (unsigned long long*)take((size_t)V * 8);
    s.tkey = (unsigned long long*)take((size_t)s.cap_v * 8);
    s.trep = (int*)take((size_t)s.cap_v * 4);
    s.owner = (int*)take((size_t)s.cap_f * 4);
    s.first = (int*)take((size_t)s.cap_f * 4);
    s.count = (unsigned*)take((size_t)V * 4);
    s.offset = (unsigned*)take((size_t)V * 4);
    s.cursor = (unsigned*)take((size_t)V * 4);
    s.tile_total = (unsigned*)take(nb * 4);
    s.tile_off = (unsigned*)take(nb * 4);
    s.inst_face = (int*)take((size_t)F * 12);
    s.inst_rep = (int*)take((size_t)F * 12);
    s.sorted = (int*)take((size_t)F * 12);
    s.newidx = (int*)take((size_t)V * 4);
    s.partial = (unsigned*)take(((size_t)blocks(F) + 1) * 24);
    s.bytes = o + 256;
    return s;
}

constexpr int SP_MAX_FACES = 1 << 29;  // 3 F instances are counted in 32-bit words

int check_sizes(const char* who, int V, int F) {
    static thread_local char msg[160];
    if (V < 0 || F < 0) {
        snprintf(msg, sizeof msg, "%s: need V >= 0 and F >= 0", who);
        return fail(msg);
    }
    if (F > SP_MAX_FACES) {
        snprintf(msg, sizeof msg, "%s: F = %d is over the supported %d faces", who, F, SP_MAX_FACES);
        return fail(msg);
    }
    return 0;
}

int check_grid(const char* who, float ox, float oy, float oz, int nx, int ny, int nz, float h) {
    static thread_local char msg[256];
    if (!(h > 0.f) || !(h <= FLT_MAX)) {
        snprintf(msg, sizeof msg, "%s: need a finite cell size h > 0, got %g", who, (double)h);
        return fail(msg);
    }
    if (nx < 1 || ny < 1 || nz < 1) {
        snprintf(msg, sizeof msg, "%s: need grid dimensions >= 1, got %d x %d x %d", who, nx, ny, nz);
        return fail(msg);
    }
    if (nx > SP_MAX_DIM || ny > SP_MAX_DIM || nz > SP_MAX_DIM) {
        snprintf(msg, sizeof msg, "%s: a grid of %d x %d x %d cells of size %g is over the limit of 2^20 cells per axis", who, nx, ny, nz,
                 (double)h);
        return fail(msg);
    }
    if (!(ox == ox) || !(oy == oy) || !(oz == oz) || fabsf(ox) > FLT_MAX || fabsf(oy) > FLT_MAX || fabsf(oz) > FLT_MAX) {
        snprintf(msg, sizeof msg, "%s: need a finite box origin", who);
        return fail(msg);
    }
    return 0;
}

}  // namespace

extern "C" {

size_t dgm_mesh_simplify_scratch_bytes(int V, int F) {
    if (V < 0 || F < 0 || F > SP_MAX_FACES) return 0;
    return simplify_layout(nullptr, V, F).bytes;
}

int dgm_mesh_simplify_box(int V, int F, const float* verts, const int* faces, char* scratch, float* box, void* stream) {
    if (check_sizes("mesh_simplify_box", V, F)) return 1;
    if (!scratch || !box || (V > 0 && !verts) || (F > 0 && !faces)) return fail("mesh_simplify_box: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const SimplifyScratch s = simplify_layout(scratch, V, F);
    if (V > 0 && hipMemsetAsync(s.used, 0, (size_t)V * 4, st) != hipSuccess) return launch_status();
    if (F > 0) hipLaunchKernelGGL(sp_box_kernel, dim3(blocks(F)), dim3(SP_THREADS), 0, st, V, F, verts, faces, s.fvalid, s.used, s.partial);
    hipLaunchKernelGGL(sp_box_reduce_kernel, dim3(1), dim3(SP_THREADS), 0, st, (int)blocks(F), (const unsigned*)s.partial, s.box, box);
    return launch_status();
}

int dgm_mesh_simplify_count(int V, int F, const float* verts, const int* faces, float ox, float oy, float oz, int nx, int ny, int nz,
                            float h, char* scratch, char* compact_scratch, int* rep_faces, unsigned char* keep, int* counts,
                            void* stream) {
    if (check_sizes("mesh_simplify_count", V, F)) return 1;
    if (check_grid("mesh_simplify_count", ox, oy, oz, nx, ny, nz, h)) return 1;
    if (!scratch || !compact_scratch || !counts || (V > 0 && !verts) || (F > 0 && (!faces || !rep_faces || !keep)))
        return fail("mesh_simplify_count: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const SimplifyScratch s = simplify_layout(scratch, V, F);
    const Grid g = {ox, oy, oz, h, nx, ny, nz};
    if (V > 0) {
        hipLaunchKernelGGL(sp_table_init_kernel, dim3(blocks(s.cap_v)), dim3(SP_THREADS), 0, st, s.cap_v, s.tkey, s.trep);
        hipLaunchKernelGGL(sp_cell_insert_kernel, dim3(blocks(V)), dim3(SP_THREADS), 0, st, V, verts, (const int*)s.used, g, s.cap_v, s.tkey,
                           s.trep, s.vkey);
        hipLaunchKernelGGL(sp_cell_lookup_kernel, dim3(blocks(V)), dim3(SP_THREADS), 0, st, V, (const int*)s.used,
                           (const unsigned long long*)s.vkey, s.cap_v, (const unsigned long long*)s.tkey, (const int*)s.trep, s.rep);
    }
    if (F > 0) {
        hipLaunchKernelGGL(sp_remap_kernel, dim3(blocks(F)), dim3(SP_THREADS), 0, st, V, F, faces, (const unsigned char*)s.fvalid,
                           (const int*)s.rep, rep_faces, keep);
        hipLaunchKernelGGL(sp_dup_init_kernel, dim3(blocks(s.cap_f)), dim3(SP_THREADS), 0, st, s.cap_f, s.owner, s.first);
        hipLaunchKernelGGL(sp_dup_insert_kernel, dim3(blocks(F)), dim3(SP_THREADS), 0, st, F, (const int*)rep_faces,
                           (const unsigned char*)keep, s.cap_f, s.owner, s.first);
        hipLaunchKernelGGL(sp_dup_flag_kernel, dim3(blocks(F)), dim3(SP_THREADS), 0, st, F, (const int*)rep_faces, s.cap_f, s.owner,
                           (const int*)s.first, keep);
    }
    if (launch_status()) return 1;
    return dgm_mesh_compact_count(V, F, rep_faces, keep, compact_scratch, counts, stream);
}

int dgm_mesh_simplify_place(int V, int F, const float* verts, const int* faces, const int* rep_faces, float ox, float oy, float oz, int nx,
                            int ny, int nz, float h, double regularization, char* scratch, float* placed, void* stream) {
    if (check_sizes("mesh_simplify_place", V, F)) return 1;
    if (check_grid("mesh_simplify_place", ox, oy, oz, nx, ny, nz, h)) return 1;
    if (!(regularization >= 0.0) || !(regularization <= DBL_MAX)) return fail("mesh_simplify_place: need a finite regularization >= 0");
    if (!scratch || (V > 0 && (!verts || !placed)) || (F > 0 && (!faces || !rep_faces))) return fail("mesh_simplify_place: NULL pointer");
    if (V == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const SimplifyScratch s = simplify_layout(scratch, V, F);
    const Grid g = {ox, oy, oz, h, nx, ny, nz};
    unsigned* total = s.box + 8;
    if (hipMemsetAsync(s.count, 0, (size_t)V * 4, st) != hipSuccess) return launch_status();
    if (F > 0) hipLaunchKernelGGL(sp_inst_count_kernel, dim3(blocks(F)), dim3(SP_THREADS), 0, st, V, F, rep_faces, s.count);
    scan_exclusive(st, (long long)V, (const unsigned*)s.count, s.tile_total, s.tile_off, s.offset, s.cursor, false, total);
    if (F > 0) {
        hipLaunchKernelGGL(sp_inst_fill_kernel, dim3(blocks(F)), dim3(SP_THREADS), 0, st, V, F, rep_faces, (const unsigned*)s.offset, s.cursor,
                           3ull * (unsigned long long)F, s.inst_face, s.inst_rep);
        hipLaunchKernelGGL(sp_inst_rank_kernel, dim3(blocks(3ll * F)), dim3(SP_THREADS), 0, st, V, (const unsigned*)total,
                           (const int*)s.inst_face, (const int*)s.inst_rep, (const unsigned*)s.offset, (const unsigned*)s.count, s.sorted);
    }
    hipLaunchKernelGGL(sp_place_kernel, dim3(blocks(V)), dim3(SP_THREADS), 0, st, V, F, verts, faces, (const int*)s.rep,
                       (const unsigned long long*)s.vkey, (const unsigned*)s.offset, (const unsigned*)s.count, (const int*)s.sorted, g,
                       regularization, placed);
    return launch_status();
}

int dgm_mesh_simplify_vert_map(int V, int F, int Vn, const int* vert_index, char* scratch, int* vert_map, void* stream) {
    if (check_sizes("mesh_simplify_vert_map", V, F)) return 1;
    if (Vn < 0 || Vn > V) return fail("mesh_simplify_vert_map: need 0 <= Vn <= V");
    if (!scratch || (V > 0 && !vert_map) || (Vn > 0 && !vert_index)) return fail("mesh_simplify_vert_map: NULL pointer");
    if (V == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const SimplifyScratch s = simplify_layout(scratch, V, F);
    if (hipMemsetAsync(s.newidx, 0xff, (size_t)V * 4, st) != hipSuccess) return launch_status();  // (-1)
    if (Vn > 0) hipLaunchKernelGGL(sp_newidx_kernel, dim3(blocks(Vn)), dim3(SP_THREADS), 0, st, V, Vn, vert_index, s.newidx);
    hipLaunchKernelGGL(sp_vert_map_kernel, dim3(blocks(V)), dim3(SP_THREADS), 0, st, V, (const int*)s.rep, (const int*)s.newidx, vert_map);
    return launch_status();
}

}  // extern "C"
