// Cleaning an extracted triangle mesh for gfx950: connected components, per-component statistics, selection and order-preserving
// compaction -- the device side of verts_on_largest_mesh (R/nvdiffrast_utils/dpsr_utils.py:345-368; R/ = dgmesh/), which the
// reference runs on the host with igl, and of its pymeshlab meshing_remove_connected_component_by_* calls
// (R/scene/gaussian_model.py:633-650).  DESIGN.md section 4.13.  Everything is integer or min / max work: bit-reproducible.
//
//   label     union-find by minimum over the vertices: parent[v] <= v always, parent[v] only ever decreases, and a root (parent[r] == r)
//             is only ever changed by a compare-and-swap that expects r.  One hooking launch over the faces (the lock-free single-pass
//             form of ECL-CC, Jaiganesh & Burtscher, HPDC 2018: a link is made root to root by CAS, so no link is ever lost and no
//             second round is needed), then one launch that chases every vertex to its root and writes labels[v] = the smallest vertex
//             index of v's component.  Two vertices are connected when a valid face uses both (igl's adjacency_matrix +
//             connected_components: connectivity through shared VERTICES, not through shared edges).  A face is valid iff its three
//             indices are in [0, V) and pairwise different; every other face connects nothing.
//   stats     per root: valid faces, vertices, bounding box.  int32 atomic adds and atomic min / max on an order-preserving integer
//             encoding of the floats, merged per lane and per workgroup (a table in LDS) first: a mesh is mostly a few large components,
//             which would otherwise meet on one or two lines of memory.  No float is ever added.
//   select    keep[f] = face f is valid and its component passes every criterion: the component with the most valid faces (ties: the
//             smaller label; one 64-bit atomic max on (faces << 32 | ~label)), at least min_faces valid faces, a box diagonal of at
//             least min_diameter_frac of the whole mesh's.  The whole mesh's box is the min / max over the roots' boxes.
//   compact   flags -> exclusive prefix sums over FIXED tiles of 4096 integers (16 consecutive per thread) -> the survivors in their
//             old order, the faces re-indexed, and the old index of every surviving vertex and face.
//
// Termination.  No workgroup waits for another and nothing spins on a flag.  Every device loop below names, in a comment, the
// monotone quantity that ends it.
// Visibility.  The per-XCD L2s are not coherent and a CU's L1 is never refreshed by another CU's stores, so inside the hooking launch
// `parent` is read with agent-scope atomic loads and written with agent-scope atomics only.  Were a read stale all the same, it
// would return an older, larger ancestor of the same vertex: the chase still descends strictly, a CAS on a vertex that is no longer
// a root fails against the true value and the link is retried from the value it returned.  The label launch starts after the
// hooking launch has ended and writes `labels`, never `parent`: it reads a table that no longer changes.
// Scratch is caller-owned; nothing here allocates device memory or reads anything back to the host.
#include <float.h>
#include <math.h>

#include "dgm_host.hpp"
#include "mesh_scan.hpp"
#include "mesh_unionfind.hpp"  // ld_parent, find_root, unite (shared with mesh_repair.hip)

#pragma clang fp contract(off)

namespace {
using namespace dgm;

constexpr int MC_THREADS = 256;
constexpr int MC_ITEMS = 16;                        // consecutive integers per thread
constexpr int MC_TILE = MC_THREADS * MC_ITEMS;      // integers per workgroup: the fixed partition of every scan here
constexpr int MC_WAVES = MC_THREADS / 64;
static_assert(MC_ITEMS == SCAN_ITEMS && MC_WAVES == SCAN_WAVES, "the compaction kernels use the tile prefix of mesh_scan.hpp");
constexpr int SEL_MAX_BLOCKS = 1024;

int tiles(long long n) { return (int)((n + MC_TILE - 1) / MC_TILE); }


// order-preserving float <-> unsigned (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN: a NaN orders by its bits)
__device__ __forceinline__ unsigned f2key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ bool face_valid(int V, int a, int b, int c) {
    return a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V && a != b && b != c && a != c;
}

// ---- labelling -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MC_THREADS) cc_init_kernel(int V, int* __restrict__ parent, int* __restrict__ info) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v < 2) info[v] = 0;
    if (v < V) parent[v] = (int)v;
}

// (find_root and unite: mesh_unionfind.hpp)

// info[0]: faces with an index outside [0, V); info[1]: faces with all indices in range and two of them equal
__global__ void __launch_bounds__(MC_THREADS) cc_hook_kernel(int V, int F, const int* __restrict__ faces, int* parent, int* info) {
    const long long f = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {  // checked before anything is dereferenced with them
        atomicAdd(info, 1);
        return;
    }
    if (a == b || b == c || a == c) {
        atomicAdd(info + 1, 1);
        return;
    }
    unite(parent, a, b);
    unite(parent, b, c);
}

__global__ void __launch_bounds__(MC_THREADS) cc_label_kernel(int V, const int* __restrict__ parent, int* __restrict__ labels) {
    const long long i = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= V) return;
    int v = (int)i, p = parent[v];
    // ends: p = parent[v] < v strictly until the root (the table no longer changes in this launch)
    while (p != v) {
        v = p;
        p = parent[v];
    }
    labels[i] = v;
}

// ---- statistics ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MC_THREADS)
stats_init_kernel(int V, int* __restrict__ comp_faces, int* __restrict__ comp_verts, unsigned* __restrict__ box) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= V) return;
    comp_faces[v] = 0;
    comp_verts[v] = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        box[6 * v + a] = 0xffffffffu;
        box[6 * v + 3 + a] = 0u;
    }
}

struct Acc {
    int lab, cnt;
    unsigned mn[3], mx[3];
};

template <bool BOX>
__device__ __forceinline__ void acc_reset(Acc& s, int lab) {
    s.lab = lab;
    s.cnt = 0;
    if (BOX) {
#pragma unroll
        for (int a = 0; a < 3; a++) s.mn[a] = 0xffffffffu, s.mx[a] = 0u;
    }
}

template <bool BOX>
__device__ __forceinline__ void acc_commit(const Acc& s, int* __restrict__ count, unsigned* __restrict__ box) {
    __hip_atomic_fetch_add(count + s.lab, s.cnt, __ATOMIC_RELAXED, AGENT);
    if (BOX) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            __hip_atomic_fetch_min(box + 6 * (long long)s.lab + a, s.mn[a], __ATOMIC_RELAXED, AGENT);
            __hip_atomic_fetch_max(box + 6 * (long long)s.lab + 3 + a, s.mx[a], __ATOMIC_RELAXED, AGENT);
        }
    }
}

// The workgroup's table in LDS: the first ST_SLOTS labels its lanes meet get a slot each, and a lane's run is merged there with LDS
// atomics; a label that finds the table full goes to memory directly.  (A mesh is mostly a few large components whose vertices
// interleave in index order, and many tiny ones: the large ones would otherwise meet on one or two lines of memory.)
constexpr int ST_SLOTS = 16;
struct StatTable {
    int lab[ST_SLOTS], cnt[ST_SLOTS];
    unsigned mn[ST_SLOTS][3], mx[ST_SLOTS][3];
};
#define WGRP __HIP_MEMORY_SCOPE_WORKGROUP

__device__ __forceinline__ void table_init(StatTable& t) {
    if (threadIdx.x < ST_SLOTS) {
        t.lab[threadIdx.x] = -1;
        t.cnt[threadIdx.x] = 0;
#pragma unroll
        for (int a = 0; a < 3; a++) t.mn[threadIdx.x][a] = 0xffffffffu, t.mx[threadIdx.x][a] = 0u;
    }
    __syncthreads();
}

template <bool BOX>
__device__ __forceinline__ void acc_flush(const Acc& s, StatTable& t, int* __restrict__ count, unsigned* __restrict__ box) {
    // ends: i grows by one per pass, ST_SLOTS passes at the most (a slot's label is written once, -1 -> label, and never again)
    for (int i = 0; i < ST_SLOTS; i++) {
        int cur = __hip_atomic_load(&t.lab[i], __ATOMIC_RELAXED, WGRP);
        if (cur == -1) {
            int expected = -1;
            cur = __hip_atomic_compare_exchange_strong(&t.lab[i], &expected, s.lab, __ATOMIC_RELAXED, __ATOMIC_RELAXED, WGRP) ? s.lab : expected;
        }
        if (cur == s.lab) {
            __hip_atomic_fetch_add(&t.cnt[i], s.cnt, __ATOMIC_RELAXED, WGRP);
            if (BOX) {
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    __hip_atomic_fetch_min(&t.mn[i][a], s.mn[a], __ATOMIC_RELAXED, WGRP);
                    __hip_atomic_fetch_max(&t.mx[i][a], s.mx[a], __ATOMIC_RELAXED, WGRP);
                }
            }
            return;
        }
    }
    acc_commit<BOX>(s, count, box);
}

// every thread of the workgroup calls this, after its last acc_flush
template <bool BOX>
__device__ __forceinline__ void table_commit(StatTable& t, int* __restrict__ count, unsigned* __restrict__ box) {
    __syncthreads();
    if (threadIdx.x < ST_SLOTS && t.lab[threadIdx.x] >= 0 && t.cnt[threadIdx.x] > 0) {
        Acc s;
        s.lab = t.lab[threadIdx.x];
        s.cnt = t.cnt[threadIdx.x];
#pragma unroll
        for (int a = 0; a < 3; a++) s.mn[a] = t.mn[threadIdx.x][a], s.mx[a] = t.mx[threadIdx.x][a];
        acc_commit<BOX>(s, count, box);
    }
}

__global__ void __launch_bounds__(MC_THREADS)
stats_vert_kernel(int V, const float* __restrict__ verts, const int* __restrict__ labels, int* __restrict__ comp_verts,
                  unsigned* __restrict__ box) {
    __shared__ StatTable table;
    table_init(table);
    Acc s;
    acc_reset<true>(s, -1);
    const long long base = (long long)blockIdx.x * MC_TILE + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < MC_ITEMS; k++) {
        const long long v = base + (long long)k * MC_THREADS;
        if (v >= V) break;
        const int lab = labels[v];
        if (lab < 0 || lab >= V) continue;  // (a label table that is not one: nothing is written outside the arrays)
        if (lab != s.lab) {
            if (s.cnt > 0) acc_flush<true>(s, table, comp_verts, box);
            acc_reset<true>(s, lab);
        }
        s.cnt++;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const unsigned key = f2key(verts[3 * v + a]);
            s.mn[a] = key < s.mn[a] ? key : s.mn[a];
            s.mx[a] = key > s.mx[a] ? key : s.mx[a];
        }
    }
    if (s.cnt > 0) acc_flush<true>(s, table, comp_verts, box);
    table_commit<true>(table, comp_verts, box);
}

__global__ void __launch_bounds__(MC_THREADS)
stats_face_kernel(int V, int F, const int* __restrict__ faces, const int* __restrict__ labels, int* __restrict__ comp_faces) {
    __shared__ StatTable table;
    table_init(table);
    Acc s;
    acc_reset<false>(s, -1);
    const long long base = (long long)blockIdx.x * MC_TILE + threadIdx.x;
#pragma unroll 4
    for (int k = 0; k < MC_ITEMS; k++) {
        const long long f = base + (long long)k * MC_THREADS;
        if (f >= F) break;
        const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        if (!face_valid(V, a, b, c)) continue;
        const int lab = labels[a];
        if (lab < 0 || lab >= V) continue;
        if (lab != s.lab) {
            if (s.cnt > 0) acc_flush<false>(s, table, comp_faces, nullptr);
            acc_reset<false>(s, lab);
        }
        s.cnt++;
    }
    if (s.cnt > 0) acc_flush<false>(s, table, comp_faces, nullptr);
    table_commit<false>(table, comp_faces, nullptr);
}

// the encoded boxes become floats in place; an index that is no root gets the empty box (+inf, -inf)
__global__ void __launch_bounds__(MC_THREADS) stats_decode_kernel(int V, const int* __restrict__ comp_verts, unsigned* box) {
    const long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= V) return;
    const bool root = comp_verts[v] > 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float mn = root ? key2f(box[6 * v + a]) : INFINITY, mx = root ? key2f(box[6 * v + 3 + a]) : -INFINITY;
        box[6 * v + a] = __float_as_uint(mn);
        box[6 * v + 3 + a] = __float_as_uint(mx);
    }
}

// ---- selection -------------------------------------------------------------------------------------------------------------------
// scratch words: [0, 1] the 64-bit key of the largest component, [2..4] / [5..7] the whole mesh's encoded box
__global__ void sel_init_kernel(unsigned* __restrict__ sel) {
    if (threadIdx.x < 8) sel[threadIdx.x] = threadIdx.x >= 2 && threadIdx.x < 5 ? 0xffffffffu : 0u;
}

__global__ void __launch_bounds__(MC_THREADS)
sel_reduce_kernel(int V, const int* __restrict__ comp_faces, const int* __restrict__ comp_verts, const float* __restrict__ box,
                  unsigned* __restrict__ sel) {
    unsigned long long best = 0ull;
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    const long long stride = (long long)gridDim.x * MC_THREADS;
    for (long long v = (long long)blockIdx.x * MC_THREADS + threadIdx.x; v < V; v += stride) {
        if (comp_verts[v] <= 0) continue;  // not a root
        const int nf = comp_faces[v];
        const unsigned long long key = ((unsigned long long)(unsigned)(nf > 0 ? nf : 0) << 32) | (0xffffffffu - (unsigned)v);
        best = key > best ? key : best;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const unsigned kn = f2key(box[6 * v + a]), kx = f2key(box[6 * v + 3 + a]);
            mn[a] = kn < mn[a] ? kn : mn[a];
            mx[a] = kx > mx[a] ? kx : mx[a];
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long ob = __shfl_xor(best, off);
        best = ob > best ? ob : best;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const unsigned on = __shfl_xor(mn[a], off), ox = __shfl_xor(mx[a], off);
            mn[a] = on < mn[a] ? on : mn[a];
            mx[a] = ox > mx[a] ? ox : mx[a];
        }
    }
    if (lane_id() == 0 && best != 0ull) {  // (a wave that saw a root: its key is not 0, its box not empty)
        __hip_atomic_fetch_max((unsigned long long*)sel, best, __ATOMIC_RELAXED, AGENT);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            __hip_atomic_fetch_min(sel + 2 + a, mn[a], __ATOMIC_RELAXED, AGENT);
            __hip_atomic_fetch_max(sel + 5 + a, mx[a], __ATOMIC_RELAXED, AGENT);
        }
    }
}

// squared diagonal of a box, fp32, in this order, without contraction
__device__ __forceinline__ float diag2(float x0, float y0, float z0, float x1, float y1, float z1) {
    const float dx = x1 - x0, dy = y1 - y0, dz = z1 - z0;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ void __launch_bounds__(MC_THREADS)
sel_keep_kernel(int V, int F, const int* __restrict__ faces, const int* __restrict__ labels, const int* __restrict__ comp_faces,
                const float* __restrict__ box, int largest, int min_faces, float frac, const unsigned* __restrict__ sel,
                unsigned char* __restrict__ keep) {
    const long long f = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    bool k = face_valid(V, a, b, c);
    int lab = 0;
    if (k) {
        lab = labels[a];
        k = lab >= 0 && lab < V;
    }
    if (k && largest) k = (unsigned)lab == 0xffffffffu - sel[0];  // (little endian: word 0 is the key's low half)
    if (k && min_faces > 0) k = comp_faces[lab] >= min_faces;
    if (k && frac > 0.f) {
        const float whole = diag2(key2f(sel[2]), key2f(sel[3]), key2f(sel[4]), key2f(sel[5]), key2f(sel[6]), key2f(sel[7]));
        const float* bx = box + 6 * (long long)lab;
        const float mine = diag2(bx[0], bx[1], bx[2], bx[3], bx[4], bx[5]);
        k = mine >= (frac * frac) * whole;
    }
    keep[f] = k ? 1 : 0;
}

// ---- compaction ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MC_THREADS)
compact_mark_kernel(int V, int F, const int* __restrict__ faces, const unsigned char* __restrict__ keep, int* __restrict__ vert_flag,
                    int* __restrict__ face_flag) {
    const long long f = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    // (a kept face with an index out of range is dropped here whatever `keep` says: the emit pass indexes with a, b, c)
    const bool k = keep[f] != 0 && a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
    face_flag[f] = k ? 1 : 0;
    if (k) vert_flag[a] = 1, vert_flag[b] = 1, vert_flag[c] = 1;  // (racing stores of one value)
}

// a set flag counts 1 in the shared tile prefix (mesh_scan.hpp)
struct FlagLoad {
    const int* flag;
    __device__ void operator()(long long i, unsigned* x) const { x[0] = flag[i] != 0 ? 1u : 0u; }
};

// blocks [0, nbV) take the vertex flags, the others the face flags
__global__ void __launch_bounds__(MC_THREADS)
scan_totals_kernel(long long nV, const int* __restrict__ vflag, int nbV, long long nF, const int* __restrict__ fflag,
                   unsigned* __restrict__ tile_total) {
    __shared__ unsigned lds[MC_WAVES][1];
    const bool isV = (int)blockIdx.x < nbV;
    const long long tile = isV ? blockIdx.x : blockIdx.x - nbV;
    unsigned fl[MC_ITEMS][1], pre, total;
    scan_tile_prefix<1>(isV ? nV : nF, FlagLoad{isV ? vflag : fflag}, tile * MC_TILE + (long long)threadIdx.x * MC_ITEMS, fl, lds, &pre, &total);
    if (threadIdx.x == 0) tile_total[blockIdx.x] = total;
}

// two workgroups: exclusive offsets of the vertex tiles (block 0) and of the face tiles (block 1), added in tile order; counts[block]
__global__ void __launch_bounds__(MC_THREADS)
scan_offsets_kernel(int nbV, int nbF, const unsigned* __restrict__ tile_total, unsigned* __restrict__ tile_off, int* __restrict__ counts) {
    __shared__ unsigned lds[MC_THREADS];
    __shared__ unsigned carry;
    const int first = blockIdx.x == 0 ? 0 : nbV, nb = blockIdx.x == 0 ? nbV : nbF;
    if (threadIdx.x == 0) carry = 0;
    for (int base = 0; base < nb; base += MC_THREADS) {  // (ends: base grows by a constant)
        const int i = base + (int)threadIdx.x;
        lds[threadIdx.x] = i < nb ? tile_total[first + i] : 0u;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned run = carry;
            for (int t = 0; t < MC_THREADS; t++) {
                const unsigned v = lds[t];
                lds[t] = run;
                run += v;
            }
            carry = run;
        }
        __syncthreads();
        if (i < nb) tile_off[first + i] = lds[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = (int)carry;
}

__global__ void __launch_bounds__(MC_THREADS)
emit_verts_kernel(long long V, int Vn, const float* __restrict__ verts, const int* __restrict__ vflag, const unsigned* __restrict__ tile_off,
                  int* __restrict__ vert_new, float* __restrict__ verts_out, int* __restrict__ vert_index) {
    __shared__ unsigned lds[MC_WAVES][1];
    unsigned fl[MC_ITEMS][1], at, total;
    const long long base = (long long)blockIdx.x * MC_TILE + (long long)threadIdx.x * MC_ITEMS;
    scan_tile_prefix<1>(V, FlagLoad{vflag}, base, fl, lds, &at, &total);
    at += tile_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < MC_ITEMS; k++) {
        const long long v = base + k;
        if (v >= V) break;
        vert_new[v] = (int)at;
        if (fl[k][0]) {
            if (at < (unsigned)Vn) {  // (Vn is the count this scan produced; the test keeps a wrong Vn inside the outputs)
#pragma unroll
                for (int a = 0; a < 3; a++) verts_out[3 * (long long)at + a] = verts[3 * v + a];
                vert_index[at] = (int)v;
            }
            at++;
        }
    }
}

__global__ void __launch_bounds__(MC_THREADS)
emit_faces_kernel(long long F, int Fn, const int* __restrict__ faces, const int* __restrict__ fflag, const unsigned* __restrict__ tile_off,
                  const int* __restrict__ vert_new, int* __restrict__ faces_out, int* __restrict__ face_index) {
    __shared__ unsigned lds[MC_WAVES][1];
    unsigned fl[MC_ITEMS][1], at, total;
    const long long base = (long long)blockIdx.x * MC_TILE + (long long)threadIdx.x * MC_ITEMS;
    scan_tile_prefix<1>(F, FlagLoad{fflag}, base, fl, lds, &at, &total);
    at += tile_off[blockIdx.x];
#pragma unroll
    for (int k = 0; k < MC_ITEMS; k++) {
        const long long f = base + k;
        if (f >= F) break;
        if (fl[k][0]) {
            if (at < (unsigned)Fn) {  // (a set flag says that the three indices are inside vert_new)
#pragma unroll
                for (int a = 0; a < 3; a++) faces_out[3 * (long long)at + a] = vert_new[faces[3 * f + a]];
                face_index[at] = (int)f;
            }
            at++;
        }
    }
}

struct CompactScratch {
    int *vert_flag, *vert_new, *face_flag;
    unsigned *tile_total, *tile_off;
    size_t bytes;
};

CompactScratch compact_layout(char* scratch, int V, int F) {
    CompactScratch s;
    char* base = align_ptr(scratch);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char* at = base + o;
        o = align_up(o + bytes, 256);
        return at;
    };
    const size_t nb = (size_t)tiles(V) + (size_t)tiles(F) + 1;
    s.vert_flag = (int*)take((size_t)V * 4);
    s.vert_new = (int*)take((size_t)V * 4);
    s.face_flag = (int*)take((size_t)F * 4);
    s.tile_total = (unsigned*)take(nb * 4);
    s.tile_off = (unsigned*)take(nb * 4);
    s.bytes = o + 256;
    return s;
}

}  // namespace

extern "C" {

int dgm_mesh_clean_tile(void) { return MC_TILE; }

size_t dgm_mesh_cc_scratch_bytes(int V, int F) {
    if (V < 0 || F < 0) return 0;
    return align_up((size_t)V * 4, 256) + 256;
}

int dgm_mesh_cc_label(int V, int F, const int* faces, char* scratch, int* labels, int* info, void* stream) {
    if (V < 0 || F < 0) return fail("mesh_cc_label: need V >= 0 and F >= 0");
    if (!info || !scratch || (V > 0 && !labels) || (F > 0 && !faces)) return fail("mesh_cc_label: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    int* parent = (int*)align_ptr(scratch);
    hipLaunchKernelGGL(cc_init_kernel, dim3(blocks(V > 2 ? V : 2)), dim3(MC_THREADS), 0, st, V, parent, info);
    if (F > 0) hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks(F)), dim3(MC_THREADS), 0, st, V, F, faces, parent, info);
    if (V > 0) hipLaunchKernelGGL(cc_label_kernel, dim3(blocks(V)), dim3(MC_THREADS), 0, st, V, (const int*)parent, labels);
    return launch_status();
}

int dgm_mesh_cc_stats(int V, int F, const float* verts, const int* faces, const int* labels, int* comp_faces, int* comp_verts,
                      float* comp_bbox, void* stream) {
    if (V < 0 || F < 0) return fail("mesh_cc_stats: need V >= 0 and F >= 0");
    if (V == 0) return 0;
    if (!verts || !labels || !comp_faces || !comp_verts || !comp_bbox || (F > 0 && !faces)) return fail("mesh_cc_stats: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    unsigned* box = (unsigned*)comp_bbox;
    hipLaunchKernelGGL(stats_init_kernel, dim3(blocks(V)), dim3(MC_THREADS), 0, st, V, comp_faces, comp_verts, box);
    hipLaunchKernelGGL(stats_vert_kernel, dim3(tiles(V)), dim3(MC_THREADS), 0, st, V, verts, labels, comp_verts, box);
    if (F > 0) hipLaunchKernelGGL(stats_face_kernel, dim3(tiles(F)), dim3(MC_THREADS), 0, st, V, F, faces, labels, comp_faces);
    hipLaunchKernelGGL(stats_decode_kernel, dim3(blocks(V)), dim3(MC_THREADS), 0, st, V, (const int*)comp_verts, box);
    return launch_status();
}

size_t dgm_mesh_cc_select_scratch_bytes(void) { return 256 + 64; }

int dgm_mesh_cc_select(int V, int F, const int* faces, const int* labels, const int* comp_faces, const int* comp_verts,
                       const float* comp_bbox, int largest, int min_faces, float min_diameter_frac, char* scratch, unsigned char* keep,
                       void* stream) {
    if (V < 0 || F < 0) return fail("mesh_cc_select: need V >= 0 and F >= 0");
    if (!(min_diameter_frac >= 0.f) || min_faces < 0) return fail("mesh_cc_select: need min_faces >= 0 and min_diameter_frac >= 0");
    if (F == 0) return 0;
    if (!faces || !keep || !scratch || (V > 0 && (!labels || !comp_faces || !comp_verts || !comp_bbox)))
        return fail("mesh_cc_select: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    unsigned* sel = (unsigned*)align_ptr(scratch);
    hipLaunchKernelGGL(sel_init_kernel, dim3(1), dim3(64), 0, st, sel);
    if (V > 0) {
        unsigned nb = blocks(V);
        if (nb > SEL_MAX_BLOCKS) nb = SEL_MAX_BLOCKS;
        hipLaunchKernelGGL(sel_reduce_kernel, dim3(nb), dim3(MC_THREADS), 0, st, V, comp_faces, comp_verts, comp_bbox, sel);
    }
    hipLaunchKernelGGL(sel_keep_kernel, dim3(blocks(F)), dim3(MC_THREADS), 0, st, V, F, faces, labels, comp_faces, comp_bbox,
                       largest ? 1 : 0, min_faces, min_diameter_frac, (const unsigned*)sel, keep);
    return launch_status();
}

size_t dgm_mesh_compact_scratch_bytes(int V, int F) {
    if (V < 0 || F < 0) return 0;
    return compact_layout(nullptr, V, F).bytes;
}

int dgm_mesh_compact_count(int V, int F, const int* faces, const unsigned char* keep, char* scratch, int* counts, void* stream) {
    if (V < 0 || F < 0) return fail("mesh_compact_count: need V >= 0 and F >= 0");
    if (!scratch || !counts || (F > 0 && (!faces || !keep))) return fail("mesh_compact_count: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const CompactScratch s = compact_layout(scratch, V, F);
    const int nbV = tiles(V), nbF = tiles(F);
    if (V > 0 && hipMemsetAsync(s.vert_flag, 0, (size_t)V * 4, st) != hipSuccess) return launch_status();
    if (F > 0) hipLaunchKernelGGL(compact_mark_kernel, dim3(blocks(F)), dim3(MC_THREADS), 0, st, V, F, faces, keep, s.vert_flag, s.face_flag);
    if (nbV + nbF > 0)
        hipLaunchKernelGGL(scan_totals_kernel, dim3(nbV + nbF), dim3(MC_THREADS), 0, st, (long long)V, (const int*)s.vert_flag, nbV,
                           (long long)F, (const int*)s.face_flag, s.tile_total);
    hipLaunchKernelGGL(scan_offsets_kernel, dim3(2), dim3(MC_THREADS), 0, st, nbV, nbF, (const unsigned*)s.tile_total, s.tile_off, counts);
    return launch_status();
}

int dgm_mesh_compact_emit(int V, int F, const float* verts, const int* faces, char* scratch, int Vn, int Fn, float* verts_out,
                          int* faces_out, int* vert_index, int* face_index, void* stream) {
    if (V < 0 || F < 0 || Vn < 0 || Fn < 0 || Vn > V || Fn > F) return fail("mesh_compact_emit: need 0 <= Vn <= V and 0 <= Fn <= F");
    if (!scratch || (V > 0 && !verts) || (F > 0 && !faces) || (Vn > 0 && (!verts_out || !vert_index)) ||
        (Fn > 0 && (!faces_out || !face_index)))
        return fail("mesh_compact_emit: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const CompactScratch s = compact_layout(scratch, V, F);
    const int nbV = tiles(V), nbF = tiles(F);
    if (nbV > 0)
        hipLaunchKernelGGL(emit_verts_kernel, dim3(nbV), dim3(MC_THREADS), 0, st, (long long)V, Vn, verts, (const int*)s.vert_flag,
                           (const unsigned*)s.tile_off, s.vert_new, verts_out, vert_index);
    if (nbF > 0)
        hipLaunchKernelGGL(emit_faces_kernel, dim3(nbF), dim3(MC_THREADS), 0, st, (long long)F, Fn, faces, (const int*)s.face_flag,
                           (const unsigned*)s.tile_off + nbV, (const int*)s.vert_new, faces_out, face_index);
    return launch_status();
}

}  // extern "C"
