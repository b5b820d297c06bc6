// The edge table of a triangle mesh and Taubin / Laplacian smoothing on it, for gfx950: per-vertex sorted adjacency, the unique
// edges with their faces and counts per direction, the classification of every edge and vertex, and one smoothing step.  The
// reference builds the edge list and the edge -> face map with torch.unique on the host side of its regulariser
// (R/nvdiffrast_utils/mesh.py:97-149, used in R/nvdiffrast_utils/regularizer.py:31-34, 64-82; R/ = dgmesh/).  DESIGN.md section
// 4.16; include/dgmesh_hip.h states the definitions.
//
//   half-edges  a face is VALID iff its indices are in [0, V) and pairwise different (mesh_clean.hip's definition; coordinates play no
//               part).  A valid face (a, b, c) has the directed half-edges a->b, b->c, c->a.  Every corner gets two entries in its own
//               list: (next corner, direction 0 = leaving this vertex, face) and (previous corner, direction 1 = arriving, face).
//   lists       int32 atomic counts per vertex, an exclusive scan over fixed tiles (mesh_scan.hpp), an atomic fill, then every list
//               put into ascending (neighbour, direction, face) order by ranking: an entry's place is the number of smaller entries
//               of its list (the entries of one list are pairwise different: any length, no workgroup-sized limit).  The atomics
//               hand out counts and places only; what ends up where does not depend on arrival order.
//   degrees     one thread per vertex walks its sorted list: the distinct neighbours (deg), those above the vertex itself (updeg = the
//               edges the vertex owns as their smaller end), the class of every incident edge -> vert_flag, and the class counts of
//               the owned edges, summed per workgroup and then by one more workgroup (integers: any order gives the same sums).
//   offsets     the scans of deg (adj_offset, 2E at its end) and of updeg (the first edge of every vertex, E at its end).
//   emit        one thread per vertex walks its list again and writes its neighbours, their edges' classes, and its owned edges: u < v,
//               ordered by u and then v, which is the lexicographic order of torch.unique(dim=0).
//   smoothing   one thread per vertex: the gather of its neighbours is the whole cost, a vertex of an extracted mesh has about six of
//               them (72 bytes), and neighbouring threads read neighbouring pieces of adj; a wave per vertex would leave 58 lanes idle.
//               The sum runs in fp64 in ascending neighbour order, is divided once and rounded to fp32 once.
//
// Termination.  No workgroup waits for another and nothing spins on a flag.  Every device loop below names what ends it.
// Visibility.  Everything a kernel reads was written by an earlier launch on the same stream; inside a launch only the counts and
// cursors are shared, through atomic adds.  No float is ever added by an atomic.
// Scratch is caller-owned; nothing here allocates device memory or reads anything back to the host.
#include <float.h>
#include <math.h>
#include <stdio.h>

#include "mesh_edge_lists.hpp"  // the keys, the list walk and the scratch layout, shared with mesh_repair.hip

#pragma clang fp contract(off)

namespace {
using namespace dgm;

constexpr int ME_THREADS = 256;
constexpr int ME_WAVES = ME_THREADS / 64;
constexpr int ME_INFO = 8;             // words of `info`

// ---- the lists -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ME_THREADS) me_count_kernel(int V, int F, const int* __restrict__ faces, unsigned* __restrict__ count) {
    const long long f = (long long)blockIdx.x * ME_THREADS + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!valid_face(V, a, b, c)) return;  // (checked before anything is indexed with them)
    atomicAdd(count + a, 2u);
    atomicAdd(count + b, 2u);
    atomicAdd(count + c, 2u);
}

__global__ void __launch_bounds__(ME_THREADS)
me_fill_kernel(int V, int F, const int* __restrict__ faces, const unsigned* __restrict__ offset, unsigned* __restrict__ cursor,
               unsigned long long cap, unsigned long long* __restrict__ raw, int* __restrict__ owner) {
    const long long f = (long long)blockIdx.x * ME_THREADS + threadIdx.x;
    if (f >= F) return;
    const int idx[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    if (!valid_face(V, idx[0], idx[1], idx[2])) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int cur = idx[k], next = idx[(k + 1) % 3], prev = idx[(k + 2) % 3];
        const unsigned long long at = (unsigned long long)offset[cur] + atomicAdd(cursor + cur, 2u);
        if (at + 1 < cap) {  // (cap = 6 F: the room of the two arrays)
            raw[at] = make_key(next, 0, (int)f);
            raw[at + 1] = make_key(prev, 1, (int)f);
            owner[at] = cur;
            owner[at + 1] = cur;
        }
    }
}

// the place of an entry in its list = the number of smaller entries (the entries of one list are pairwise different)
__global__ void __launch_bounds__(ME_THREADS)
me_rank_kernel(int V, const unsigned* __restrict__ total, const unsigned long long* __restrict__ raw, const int* __restrict__ owner,
               const unsigned* __restrict__ offset, const unsigned* __restrict__ count, unsigned long long* __restrict__ sorted) {
    const unsigned long long i = (unsigned long long)blockIdx.x * ME_THREADS + threadIdx.x;
    if (i >= total[0]) return;
    const int r = owner[i];
    if (r < 0 || r >= V) return;
    const unsigned start = offset[r], len = count[r];
    const unsigned long long mine = raw[i];
    unsigned rank = 0;
    for (unsigned j = 0; j < len; j++) rank += raw[(unsigned long long)start + j] < mine ? 1u : 0u;  // (ends: j grows to len)
    sorted[(unsigned long long)start + rank] = mine;  // (rank < len: `mine` is not smaller than itself)
}

// ---- degrees, classes, flags -----------------------------------------------------------------------------------------------------
// every workgroup stores its own sums (ME_SUMS words): no word is shared between workgroups
__global__ void __launch_bounds__(ME_THREADS)
me_degree_kernel(int V, const unsigned long long* __restrict__ sorted, const unsigned* __restrict__ offset, const unsigned* __restrict__ count,
                 unsigned* __restrict__ deg, unsigned* __restrict__ updeg, unsigned char* __restrict__ vert_flag, unsigned* __restrict__ partial) {
    __shared__ unsigned lds[ME_WAVES][ME_SUMS];
    const long long v = (long long)blockIdx.x * ME_THREADS + threadIdx.x;
    unsigned sums[ME_SUMS] = {0u, 0u, 0u, 0u, 0u};
    if (v < V) {
        unsigned d = 0, up = 0, flag = 0;
        const unsigned len = count[v];
        for_each_neighbour(sorted, offset[v], len, [&](int nbr, int c0, int c1, int, int) {
            const int kind = edge_kind(c0, c1);
            d++;
            flag |= kind == KIND_BOUNDARY ? 2u : (kind == KIND_REGULAR ? 0u : 4u);
            if (nbr > (int)v) {
                up++;
                sums[kind == KIND_BOUNDARY ? 0 : (kind == KIND_NONMANIFOLD ? 1 : (kind == KIND_MISORIENTED ? 2 : 3))]++;
            }
        });
        if (len > 0) flag |= 1u, sums[4] = 1u;
        deg[v] = d;
        updeg[v] = up;
        vert_flag[v] = (unsigned char)flag;
    }
#pragma unroll
    for (int k = 0; k < ME_SUMS; k++) {  // (every lane takes part: the returns above are inside the `if`)
        const unsigned s = wave_sum_u32(sums[k]);
        if (lane_id() == 0) lds[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < ME_SUMS) {
        unsigned r = 0;
#pragma unroll
        for (int w = 0; w < ME_WAVES; w++) r += lds[w][threadIdx.x];
        partial[ME_SUMS * (long long)blockIdx.x + threadIdx.x] = r;
    }
}

// one workgroup: the workgroups' sums and the scans' totals -> info
__global__ void __launch_bounds__(ME_THREADS)
me_info_kernel(int nb, const unsigned* __restrict__ partial, const unsigned* __restrict__ ctl, const int* __restrict__ adj_total,
               int* __restrict__ info) {
    __shared__ unsigned lds[ME_WAVES][ME_SUMS];
    unsigned sums[ME_SUMS] = {0u, 0u, 0u, 0u, 0u};
    for (int b = threadIdx.x; b < nb; b += ME_THREADS) {  // (ends: b grows by a constant)
#pragma unroll
        for (int k = 0; k < ME_SUMS; k++) sums[k] += partial[ME_SUMS * (long long)b + k];
    }
#pragma unroll
    for (int k = 0; k < ME_SUMS; k++) {
        const unsigned s = wave_sum_u32(sums[k]);
        if (lane_id() == 0) lds[threadIdx.x >> 6][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned r[ME_SUMS];
#pragma unroll
        for (int k = 0; k < ME_SUMS; k++) {
            r[k] = 0;
#pragma unroll
            for (int w = 0; w < ME_WAVES; w++) r[k] += lds[w][k];
        }
        info[0] = (int)ctl[1];      // E
        info[1] = (int)r[0];        // boundary edges
        info[2] = (int)r[1];        // non-manifold edges
        info[3] = (int)r[2];        // misoriented edges
        info[4] = (int)r[3];        // regular edges
        info[5] = (int)r[4];        // used vertices
        info[6] = (int)(ctl[0] / 6u);  // valid faces: six list entries each
        info[7] = adj_total[0];     // 2 E
    }
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ME_THREADS)
me_emit_kernel(int V, int E, const unsigned long long* __restrict__ sorted, const unsigned* __restrict__ offset, const unsigned* __restrict__ count,
               const int* __restrict__ adj_offset, const unsigned* __restrict__ edge_offset, int* __restrict__ adj,
               unsigned char* __restrict__ adj_kind, int* __restrict__ edges, int* __restrict__ edge_faces, int* __restrict__ edge_count) {
    const long long v = (long long)blockIdx.x * ME_THREADS + threadIdx.x;
    if (v >= V) return;
    const long long room = 2ll * E;
    long long at = adj_offset[v];
    long long e = edge_offset[v];
    for_each_neighbour(sorted, offset[v], count[v], [&](int nbr, int c0, int c1, int f0, int f1) {
        if (at >= 0 && at < room) {  // (nothing is written at or behind 2 E and E)
            if (adj) adj[at] = nbr;
            if (adj_kind) adj_kind[at] = (unsigned char)edge_kind(c0, c1);
        }
        at++;
        if (nbr > (int)v) {
            if (e >= 0 && e < E) {
                if (edges) edges[2 * e] = (int)v, edges[2 * e + 1] = nbr;
                if (edge_faces) edge_faces[2 * e] = f0, edge_faces[2 * e + 1] = f1;
                if (edge_count) edge_count[2 * e] = c0, edge_count[2 * e + 1] = c1;
            }
            e++;
        }
    });
}

// ---- smoothing -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// boundary: 0 fixed, 1 curve, 2 free
__global__ void __launch_bounds__(ME_THREADS)
me_smooth_kernel(int V, int A, const float* __restrict__ in, const int* __restrict__ adj_offset, const int* __restrict__ adj,
                 const unsigned char* __restrict__ adj_kind, const unsigned char* __restrict__ vert_flag, double factor, int boundary,
                 float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * ME_THREADS + threadIdx.x;
    if (i >= V) return;
    const float xf[3] = {in[3 * i], in[3 * i + 1], in[3 * i + 2]};
    const bool rim = (vert_flag[i] & 2u) != 0u;
    const long long start = adj_offset[i], end = adj_offset[i + 1];
    bool move = finite_f(xf[0]) && finite_f(xf[1]) && finite_f(xf[2]) && !(boundary == 0 && rim) && start >= 0 && start < end && end <= A;
    const bool along = boundary == 1 && rim;  // the rim is smoothed along itself
    double s[3] = {0.0, 0.0, 0.0};
    int n = 0;
    if (move) {
        for (long long j = start; j < end; j++) {  // (ends: j grows to end)
            if (along && adj_kind[j] != KIND_BOUNDARY) continue;
            const int k = adj[j];
            if (k < 0 || k >= V) {  // (checked before it is used; such a list moves nothing)
                move = false;
                break;
            }
#pragma unroll
            for (int a = 0; a < 3; a++) s[a] += (double)in[3 * (long long)k + a];
            n++;
        }
    }
    if (!move || n == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) out[3 * i + a] = xf[a];
        return;
    }
    const double cnt = (double)n;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double x = (double)xf[a];
        const double m = s[a] / cnt;
        out[3 * i + a] = (float)(x + factor * (m - x));
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int check_sizes(const char* who, int V, int F) {
    static thread_local char msg[160];
    if (V < 0 || F < 0) {
        snprintf(msg, sizeof msg, "%s: need V >= 0 and F >= 0", who);
        return fail(msg);
    }
    if (F > ME_MAX_FACES) {
        snprintf(msg, sizeof msg, "%s: F = %d is over the supported %d faces", who, F, ME_MAX_FACES);
        return fail(msg);
    }
    return 0;
}

}  // namespace

extern "C" {

size_t dgm_mesh_edges_scratch_bytes(int V, int F) {
    if (V < 0 || F < 0 || F > ME_MAX_FACES) return 0;
    return edges_layout(nullptr, V, F).bytes;
}

int dgm_mesh_edges_count(int V, int F, const int* faces, char* scratch, int* adj_offset, unsigned char* vert_flag, int* info, void* stream) {
    if (check_sizes("mesh_edges_count", V, F)) return 1;
    if (!scratch || !adj_offset || !info || (V > 0 && !vert_flag) || (F > 0 && !faces)) return fail("mesh_edges_count: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (V == 0) {  // no vertex: no valid face
        if (hipMemsetAsync(info, 0, ME_INFO * 4, st) != hipSuccess || hipMemsetAsync(adj_offset, 0, 4, st) != hipSuccess) return launch_status();
        return launch_status();
    }
    const EdgesScratch s = edges_layout(scratch, V, F);
    if (hipMemsetAsync(s.count, 0, (size_t)V * 4, st) != hipSuccess) return launch_status();
    if (F > 0) hipLaunchKernelGGL(me_count_kernel, dim3(blocks(F)), dim3(ME_THREADS), 0, st, V, F, faces, s.count);
    scan_exclusive(st, (long long)V, (const unsigned*)s.count, s.tile_total, s.tile_off, s.offset, s.cursor, false, s.ctl);
    if (F > 0) {
        hipLaunchKernelGGL(me_fill_kernel, dim3(blocks(F)), dim3(ME_THREADS), 0, st, V, F, faces, (const unsigned*)s.offset, s.cursor,
                           6ull * (unsigned long long)F, s.raw, s.owner);
        hipLaunchKernelGGL(me_rank_kernel, dim3(blocks(6ll * F)), dim3(ME_THREADS), 0, st, V, (const unsigned*)s.ctl,
                           (const unsigned long long*)s.raw, (const int*)s.owner, (const unsigned*)s.offset, (const unsigned*)s.count, s.sorted);
    }
    hipLaunchKernelGGL(me_degree_kernel, dim3(blocks(V)), dim3(ME_THREADS), 0, st, V, (const unsigned long long*)s.sorted,
                       (const unsigned*)s.offset, (const unsigned*)s.count, s.deg, s.updeg, vert_flag, s.partial);
    // (2 E <= 6 F < 2^31: the offsets are the same numbers as int32)
    scan_exclusive(st, (long long)V, (const unsigned*)s.deg, s.tile_total, s.tile_off, (unsigned*)adj_offset, nullptr, false, (unsigned*)adj_offset + V);
    scan_exclusive(st, (long long)V, (const unsigned*)s.updeg, s.tile_total, s.tile_off, s.edge_offset, nullptr, false, s.ctl + 1);
    hipLaunchKernelGGL(me_info_kernel, dim3(1), dim3(ME_THREADS), 0, st, (int)blocks(V), (const unsigned*)s.partial, (const unsigned*)s.ctl,
                       (const int*)adj_offset + V, info);
    return launch_status();
}

int dgm_mesh_edges_emit(int V, int F, char* scratch, int E, const int* adj_offset, int* adj, unsigned char* adj_kind, int* edges,
                        int* edge_faces, int* edge_count, void* stream) {
    if (check_sizes("mesh_edges_emit", V, F)) return 1;
    if (E < 0 || (long long)E > 3ll * F) return fail("mesh_edges_emit: need 0 <= E <= 3 F");
    if (!scratch || !adj_offset) return fail("mesh_edges_emit: NULL pointer");
    if (V == 0 || E == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const EdgesScratch s = edges_layout(scratch, V, F);
    hipLaunchKernelGGL(me_emit_kernel, dim3(blocks(V)), dim3(ME_THREADS), 0, st, V, E, (const unsigned long long*)s.sorted,
                       (const unsigned*)s.offset, (const unsigned*)s.count, adj_offset, (const unsigned*)s.edge_offset, adj, adj_kind, edges,
                       edge_faces, edge_count);
    return launch_status();
}

int dgm_mesh_smooth_step(int V, int A, const float* verts_in, const int* adj_offset, const int* adj, const unsigned char* adj_kind,
                         const unsigned char* vert_flag, double factor, int boundary, float* verts_out, void* stream) {
    if (V < 0 || A < 0) return fail("mesh_smooth_step: need V >= 0 and A >= 0");
    if (boundary < 0 || boundary > 2) return fail("mesh_smooth_step: boundary must be 0 (fixed), 1 (curve) or 2 (free)");
    if (!(factor == factor) || fabs(factor) > DBL_MAX) return fail("mesh_smooth_step: need a finite factor");
    if (V == 0) return 0;
    if (!verts_in || !verts_out || !adj_offset || !vert_flag || (A > 0 && (!adj || (boundary == 1 && !adj_kind))))
        return fail("mesh_smooth_step: NULL pointer");
    if (verts_in == verts_out) return fail("mesh_smooth_step: verts_out must not be verts_in (every vertex reads its neighbours' old positions)");
    hipLaunchKernelGGL(me_smooth_kernel, dim3(blocks(V)), dim3(ME_THREADS), 0, (hipStream_t)stream, V, A, verts_in, adj_offset, adj, adj_kind,
                       vert_flag, factor, boundary, verts_out);
    return launch_status();
}

}  // extern "C"
