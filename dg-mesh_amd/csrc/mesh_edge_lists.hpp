// The per-vertex sorted half-edge lists of the edge table and the walk over them, shared by mesh_edges.hip,
// which builds the lists in its scratch and emits the public tables from them, and mesh_repair.hip, which needs BOTH faces of a
// two-face edge (the public edge_faces keeps the smallest face per direction only) and therefore walks the lists themselves.
//   list of vertex v   sorted[offset[v] .. offset[v] + count[v]): for every corner of a valid face at v the entries (next corner,
//                      direction 0 = leaving v, face) and (previous corner, direction 1 = arriving at v, face), ascending as triples.
// Included by one translation unit each: everything is local to it.  Every loop names what ends it.
#pragma once
#include "dgm_host.hpp"
#include "mesh_scan.hpp"

namespace {

constexpr int ME_MAX_FACES = 1 << 28;  // 6 F list entries and 2 E <= 6 F adjacency entries are counted in int32
constexpr int ME_SUMS = 5;             // sums per workgroup: boundary, non-manifold, misoriented and regular edges, used vertices

// the class of an edge from its faces per direction
constexpr int KIND_REGULAR = 0, KIND_BOUNDARY = 1, KIND_NONMANIFOLD = 2, KIND_MISORIENTED = 3;

__device__ __forceinline__ bool valid_face(int V, int a, int b, int c) {
    return a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V && a != b && b != c && a != c;
}

// (neighbour, direction, face) in one word that orders like the triple; face < 2^31
__device__ __forceinline__ unsigned long long make_key(int nbr, int dir, int face) {
    return ((unsigned long long)(unsigned)nbr << 32) | ((unsigned long long)dir << 31) | (unsigned long long)(unsigned)face;
}
__device__ __forceinline__ int key_nbr(unsigned long long k) { return (int)(k >> 32); }
__device__ __forceinline__ int key_dir(unsigned long long k) { return (int)((k >> 31) & 1ull); }
__device__ __forceinline__ int key_face(unsigned long long k) { return (int)(k & 0x7fffffffull); }

__device__ __forceinline__ int edge_kind(int c0, int c1) {
    const int s = c0 + c1;
    return s == 1 ? KIND_BOUNDARY : (s >= 3 ? KIND_NONMANIFOLD : (c0 == 1 && c1 == 1 ? KIND_REGULAR : KIND_MISORIENTED));
}

// group(neighbour, faces leaving, faces arriving, the two smallest faces leaving, the two smallest faces arriving; -1 for none) for
// every distinct neighbour of one sorted list, ascending
template <class G>
__device__ __forceinline__ void for_each_neighbour2(const unsigned long long* __restrict__ sorted, unsigned start, unsigned len, G&& group) {
    unsigned j = 0;
    while (j < len) {  // (ends: the inner loop moves j on by one at least, its first entry being the group's own)
        const int nbr = key_nbr(sorted[(unsigned long long)start + j]);
        int c[2] = {0, 0}, first[2][2] = {{-1, -1}, {-1, -1}};
        for (; j < len; j++) {  // (ends: j grows to len)
            const unsigned long long k = sorted[(unsigned long long)start + j];
            if (key_nbr(k) != nbr) break;
            const int d = key_dir(k);
            if (c[d] < 2) first[d][c[d]] = key_face(k);  // (ascending faces inside a direction: the first are the smallest)
            c[d]++;
        }
        group(nbr, c[0], c[1], first[0], first[1]);
    }
}

// group(neighbour, faces leaving, faces arriving, smallest face leaving or -1, smallest face arriving or -1)
template <class G>
__device__ __forceinline__ void for_each_neighbour(const unsigned long long* __restrict__ sorted, unsigned start, unsigned len, G&& group) {
    for_each_neighbour2(sorted, start, len, [&](int nbr, int c0, int c1, const int* f0, const int* f1) { group(nbr, c0, c1, f0[0], f1[0]); });
}

// the scratch of dgm_mesh_edges_count: dgm_mesh_edges_scratch_bytes(V, F) bytes
struct EdgesScratch {
    unsigned* ctl;  // [0] the list entries (6 per valid face), [1] E
    unsigned *count, *offset, *cursor, *deg, *updeg, *edge_offset, *tile_total, *tile_off, *partial;
    unsigned long long *raw, *sorted;
    int* owner;
    size_t bytes;
};

inline EdgesScratch edges_layout(char* scratch, int V, int F) {
    EdgesScratch s;
    char* base = dgm::align_ptr(scratch);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char* at = base + o;
        o = dgm::align_up(o + bytes, 256);
        return at;
    };
    const size_t nt = (size_t)scan_tiles(V) + 1;
    s.ctl = (unsigned*)take(64);
    s.count = (unsigned*)take((size_t)V * 4);
    s.offset = (unsigned*)take((size_t)V * 4);
    s.cursor = (unsigned*)take((size_t)V * 4);
    s.deg = (unsigned*)take((size_t)V * 4);
    s.updeg = (unsigned*)take((size_t)V * 4);
    s.edge_offset = (unsigned*)take((size_t)V * 4);
    s.tile_total = (unsigned*)take(nt * 4);
    s.tile_off = (unsigned*)take(nt * 4);
    s.partial = (unsigned*)take(((size_t)dgm::blocks(V) + 1) * ME_SUMS * 4);
    s.raw = (unsigned long long*)take((size_t)F * 48);
    s.sorted = (unsigned long long*)take((size_t)F * 48);
    s.owner = (int*)take((size_t)F * 24);
    s.bytes = o + 256;
    return s;
}

}  // namespace
