// Repairing an extracted triangle mesh for gfx950: a consistent, outward orientation per body and the filling of small holes -- the
// device side of the last stage of the reference's mesh clean-up (pymeshlab meshing_close_holes, then trimesh fill_holes,
// fix_inversion and fix_normals; R/scene/gaussian_model.py:652-691; R/ = dgmesh/).  Both work on the sorted half-edge lists that
// dgm_mesh_edges_count leaves in its scratch (mesh_edge_lists.hpp).  DESIGN.md section 4.20; include/dgmesh_hip.h states the
// definitions.
//
//   orient    union-find by minimum (mesh_unionfind.hpp) on the DOUBLE COVER of the face adjacency: node 2 f + s is face f kept (s = 0)
//             or turned (s = 1).  An edge that exactly two valid faces traverse links them: in opposite directions (counts (1, 1)) they
//             agree, (f, s) - (g, s); in the same direction ((2, 0) or (0, 2)) they disagree, (f, s) - (g, 1 - s).  One hooking launch
//             over the vertices (every vertex owns the edges to its larger neighbours), then with l0 = root(2 f), l1 = root(2 f + 1):
//             the component of f is l0 >> 1 = its smallest face; it cannot be oriented iff l0 == l1; f disagrees with the smallest
//             face iff l1 < l0.  Faces, disagreeing faces, open half-edges and the signed volume are summed per component with integer
//             atomics; a last launch decides every face from its component's sums.
//   volume    term(f) = llrint(det(p, q, r) 2^(30 - 3 e)) of the corners minus the box' lower corner in fp64, 2^e >= the longest box side:
//             |term| <= 6 2^30, so 2^28 faces stay below 2^61 in the int64 sum, and integer sums do not depend on their order.
//   holes     the boundary half-edges in the edge table's order (a scan over the vertices' owned boundary edges), in- and out-degrees
//             on the boundary by integer atomics, next(i) where the head is a simple vertex, then (min, jump) pointer doubling over two
//             buffers for ceil(log2(B + 1)) launches, a number the host fixes before it launches: afterwards jump < 0 marks a chain
//             that ends (the mark is absorbing) and min is the smallest half-edge of a cycle, its leader.  One thread per leader walks
//             its cycle, at most max_hole_edges + 1 steps, takes the length and forms the fp64 centroid.  Output offsets come from
//             the two-component scan of mesh_scan.hpp; the emit call writes the fans.
//
// Termination.  No workgroup waits for another and nothing spins on a flag.  Every device loop below names what ends it.
// Visibility.  Inside the hooking launch `parent` is touched by agent-scope atomics only (mesh_unionfind.hpp); everything else a
// kernel reads was written by an earlier launch on the same stream, and inside a launch only counts are shared, through integer
// atomics.  No float is ever added by an atomic.
// Scratch is caller-owned; nothing here allocates device memory or reads anything back to the host.
#include <float.h>
#include <math.h>
#include <stdio.h>

#include "mesh_edge_lists.hpp"
#include "mesh_unionfind.hpp"

#pragma clang fp contract(off)

namespace {
using namespace dgm;

constexpr int MR_THREADS = 256;
constexpr int MR_INFO = 8;  // words of either `info`

// per-face state after labelling
constexpr unsigned char ST_INVALID = 0, ST_AGREES = 1, ST_DISAGREES = 2, ST_UNORIENTABLE = 3;

// order-preserving float <-> unsigned (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN: a NaN orders by its bits)
__device__ __forceinline__ unsigned f2key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ bool finite_f(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// ---- orientation -----------------------------------------------------------------------------------------------------------------
struct OrientScratch {
    unsigned* box;  // the keys of the lower corner [0..3) and of the upper corner [3..6)
    int *parent, *conn, *comp, *nfaces, *flips, *open;
    long long* vol;
    unsigned char* state;
    size_t bytes;
};

OrientScratch orient_layout(char* scratch, int F) {
    OrientScratch s;
    char* base = align_ptr(scratch);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char* at = base + o;
        o = align_up(o + bytes, 256);
        return at;
    };
    s.box = (unsigned*)take(64);
    s.parent = (int*)take((size_t)F * 8);
    s.conn = (int*)take((size_t)F * 4);
    s.comp = (int*)take((size_t)F * 4);
    s.nfaces = (int*)take((size_t)F * 4);
    s.flips = (int*)take((size_t)F * 4);
    s.open = (int*)take((size_t)F * 4);
    s.vol = (long long*)take((size_t)F * 8);
    s.state = (unsigned char*)take((size_t)F);
    s.bytes = o + 256;
    return s;
}

__global__ void __launch_bounds__(MR_THREADS) or_init_kernel(int F, OrientScratch s, int* __restrict__ info) {
    const long long i = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    if (i < MR_INFO) info[i] = 0;
    if (i < 6) s.box[i] = i < 3 ? 0xffffffffu : 0u;
    if (i < 2ll * F) s.parent[i] = (int)i;
    if (i < F) {
        s.conn[i] = 0;
        s.nfaces[i] = 0;
        s.flips[i] = 0;
        s.open[i] = 0;
        s.vol[i] = 0ll;
    }
}

// the box of the used vertices (a vertex is used iff its list is not empty): min / max of the keys, per workgroup in LDS first
__global__ void __launch_bounds__(MR_THREADS)
or_box_kernel(int V, const float* __restrict__ verts, const unsigned* __restrict__ count, unsigned* __restrict__ box) {
    __shared__ unsigned lds[6];
    if (threadIdx.x < 6) lds[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
    __syncthreads();
    const long long v = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    if (v < V && count[v] > 0u) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const unsigned k = f2key(verts[3 * v + a]);
            atomicMin(lds + a, k);
            atomicMax(lds + 3 + a, k);
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(box + threadIdx.x, lds[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(box + threadIdx.x, lds[threadIdx.x]);
}

// every vertex links the faces across the edges to its larger neighbours
__global__ void __launch_bounds__(MR_THREADS)
or_hook_kernel(int V, int F, const unsigned long long* __restrict__ sorted, const unsigned* __restrict__ offset, const unsigned* __restrict__ count,
               int* parent, int* conn) {
    const long long v = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    if (v >= V) return;
    for_each_neighbour2(sorted, offset[v], count[v], [&](int nbr, int c0, int c1, const int* f0, const int* f1) {
        if (nbr <= (int)v || c0 + c1 != 2) return;  // boundary and non-manifold edges connect nothing
        const bool agree = c0 == 1;                 // (1, 1); otherwise (2, 0) or (0, 2)
        const int f = c0 >= 1 ? f0[0] : f1[0];
        const int g = c0 == 2 ? f0[1] : (c0 == 1 ? f1[0] : f1[1]);
        if (f < 0 || f >= F || g < 0 || g >= F) return;  // (checked before they index anything)
        unite(parent, 2 * f, agree ? 2 * g : 2 * g + 1);
        unite(parent, 2 * f + 1, agree ? 2 * g + 1 : 2 * g);
        atomicAdd(conn + f, 1);
        atomicAdd(conn + g, 1);
    });
}

struct Box {
    double lo[3];
    int shift;  // 30 - 3 e
    bool ok;    // finite and with an extent
};

__device__ __forceinline__ Box decode_box(const unsigned* __restrict__ box) {
    Box b;
    b.ok = true;
    double longest = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float lo = key2f(box[a]), hi = key2f(box[3 + a]);
        b.ok = b.ok && finite_f(lo) && finite_f(hi);
        b.lo[a] = (double)lo;
        const double side = (double)hi - (double)lo;
        longest = side > longest ? side : longest;
    }
    b.ok = b.ok && longest > 0.0;
    int x = 0;
    const double m = b.ok ? frexp(longest, &x) : 0.5;  // longest = m 2^x, 0.5 <= m < 1
    b.shift = 30 - 3 * (m == 0.5 ? x - 1 : x);         // the smallest e with 2^e >= longest
    return b;
}

__global__ void __launch_bounds__(MR_THREADS)
or_label_kernel(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, int use_volume, OrientScratch s) {
    const long long f = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    int comp = -1, open = 0, dis = 0;  // what this face adds to its component
    long long term = 0ll;
    if (f < F) {
        const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        unsigned char st = ST_INVALID;
        if (valid_face(V, a, b, c)) {
            const int l0 = settled_root(s.parent, 2 * (int)f), l1 = settled_root(s.parent, 2 * (int)f + 1);
            comp = l0 >> 1;
            st = l0 == l1 ? ST_UNORIENTABLE : (l1 < l0 ? ST_DISAGREES : ST_AGREES);
            open = 3 - s.conn[f];
            open = open > 0 ? open : 0;
            dis = st == ST_DISAGREES ? 1 : 0;
            const Box box = decode_box(s.box);
            if (st != ST_UNORIENTABLE && use_volume && box.ok) {
                const int i1 = dis ? c : b, i2 = dis ? b : c;  // after the winding fix
                double p[3], q[3], r[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    p[k] = (double)verts[3 * (long long)a + k] - box.lo[k];
                    q[k] = (double)verts[3 * (long long)i1 + k] - box.lo[k];
                    r[k] = (double)verts[3 * (long long)i2 + k] - box.lo[k];
                }
                const double det = p[0] * (q[1] * r[2] - q[2] * r[1]) - p[1] * (q[0] * r[2] - q[2] * r[0]) + p[2] * (q[0] * r[1] - q[1] * r[0]);
                if (fabs(det) <= DBL_MAX) term = llrint(ldexp(det, box.shift));  // (a non-finite determinant adds nothing)
            }
        }
        s.comp[f] = comp;
        s.state[f] = st;
    }
    // The faces of a wave mostly belong to one component, and a mesh is mostly a few large components, which would otherwise meet on
    // one line of memory: where the wave's valid faces agree on the component, its sums are formed first and one lane adds them.
    // Integer sums: the grouping changes nothing.  term = hi 2^16 + lo, |hi| <= 6 2^14 + 1, 0 <= lo < 2^16: 64 of each fit 32 bits.
    // (Every lane takes part in the wave sums: nothing returns above.)
    const bool live = comp >= 0;
    const unsigned n_sum = wave_sum_u32(live ? 1u : 0u), open_sum = wave_sum_u32((unsigned)open), dis_sum = wave_sum_u32((unsigned)dis);
    const unsigned lo_sum = wave_sum_u32((unsigned)(term & 0xffffll));
    const int hi_sum = (int)wave_sum_u32((unsigned)(int)(term >> 16));
    const unsigned long long lanes = __ballot(live);
    if (lanes == 0ull) return;
    const int leader = __ffsll((long long)lanes) - 1;
    const int first = __shfl(comp, leader, 64);
    if (__ballot(live && comp != first) == 0ull) {
        if (lane_id() == leader) {
            atomicAdd(s.nfaces + comp, (int)n_sum);
            if (open_sum > 0u) atomicAdd(s.open + comp, (int)open_sum);
            if (dis_sum > 0u) atomicAdd(s.flips + comp, (int)dis_sum);
            const long long sum = (long long)hi_sum * 65536ll + (long long)lo_sum;
            if (sum != 0ll) atomicAdd((unsigned long long*)s.vol + comp, (unsigned long long)sum);  // (two's complement: the signed sum)
        }
        return;
    }
    if (!live) return;
    atomicAdd(s.nfaces + comp, 1);
    if (open > 0) atomicAdd(s.open + comp, open);
    if (dis) atomicAdd(s.flips + comp, 1);
    if (term != 0ll) atomicAdd((unsigned long long*)s.vol + comp, (unsigned long long)term);
}

// info: components, closed components, unorientable components, faces flipped, components inverted, outward skipped
__global__ void __launch_bounds__(MR_THREADS)
or_decide_kernel(int F, const int* __restrict__ faces, int outward, OrientScratch s, int* __restrict__ faces_out,
                 unsigned char* __restrict__ flipped, int* __restrict__ info) {
    const long long f = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    bool flip = false;
    if (f < F) {
        const unsigned char st = s.state[f];
        const int comp = s.comp[f];
        if (st != ST_INVALID && comp >= 0 && comp < F) {
            const bool closed = s.open[comp] == 0;
            const bool root = comp == (int)f;
            if (root) {
                atomicAdd(info + 0, 1);
                if (closed) atomicAdd(info + 1, 1);
                if (st == ST_UNORIENTABLE) atomicAdd(info + 2, 1);
            }
            if (st != ST_UNORIENTABLE) {
                const int n = s.nfaces[comp], k = s.flips[comp];
                bool invert = n - k < k;  // the orientation that flips fewer faces; a tie keeps the smallest face
                const long long vol = s.vol[comp];
                if (outward && closed && vol != 0ll && decode_box(s.box).ok) {
                    invert = vol < 0ll;
                    if (root && invert) atomicAdd(info + 4, 1);
                }
                flip = (st == ST_DISAGREES) != invert;
            }
        }
        const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
        faces_out[3 * f] = a;
        faces_out[3 * f + 1] = flip ? c : b;
        faces_out[3 * f + 2] = flip ? b : c;
        flipped[f] = flip ? 1 : 0;
        if (f == 0) info[5] = outward && !decode_box(s.box).ok ? 1 : 0;
    }
    const unsigned flips = wave_sum_u32(flip ? 1u : 0u);  // (every lane takes part: nothing returns above)
    if (lane_id() == 0 && flips > 0u) atomicAdd(info + 3, (int)flips);
}

// ---- holes -----------------------------------------------------------------------------------------------------------------------
struct FillScratch {
    unsigned* ctl;  // [0] the boundary half-edges found
    unsigned *bcount, *boff, *indeg, *outdeg, *outhe, *tile_total, *tile_off, *foff, *voff;
    int *tail, *head, *next, *len;
    int2 *pd[2];
    float* cent;
    size_t bytes;
};

FillScratch fill_layout(char* scratch, int V, int B) {
    FillScratch s;
    char* base = align_ptr(scratch);
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char* at = base + o;
        o = align_up(o + bytes, 256);
        return at;
    };
    const int tv = scan_tiles(V), tb = scan_tiles(B);
    const size_t nt = 2 * (size_t)(tv > tb ? tv : tb) + 2;  // two components side by side
    s.ctl = (unsigned*)take(64);
    s.bcount = (unsigned*)take((size_t)V * 4);
    s.boff = (unsigned*)take((size_t)V * 4);
    s.indeg = (unsigned*)take((size_t)V * 4);
    s.outdeg = (unsigned*)take((size_t)V * 4);
    s.outhe = (unsigned*)take((size_t)V * 4);
    s.tile_total = (unsigned*)take(nt * 4);
    s.tile_off = (unsigned*)take(nt * 4);
    s.foff = (unsigned*)take((size_t)B * 4);
    s.voff = (unsigned*)take((size_t)B * 4);
    s.tail = (int*)take((size_t)B * 4);
    s.head = (int*)take((size_t)B * 4);
    s.next = (int*)take((size_t)B * 4);
    s.len = (int*)take((size_t)B * 4);
    s.pd[0] = (int2*)take((size_t)B * 8);
    s.pd[1] = (int2*)take((size_t)B * 8);
    s.cent = (float*)take((size_t)B * 12);
    s.bytes = o + 256;
    return s;
}

// the launches of the pointer doubling: the smallest K with 2^K >= B + 1 (no cycle and no chain has more than B half-edges)
int doubling_rounds(int B) {
    int k = 0;
    while ((1ll << k) < (long long)B + 1) k++;  // (ends: k grows, at 32 at the latest)
    return k;
}

__global__ void __launch_bounds__(MR_THREADS)
fh_count_kernel(int V, const unsigned long long* __restrict__ sorted, const unsigned* __restrict__ offset, const unsigned* __restrict__ count,
                unsigned* __restrict__ bcount) {
    const long long v = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    if (v >= V) return;
    unsigned n = 0;
    for_each_neighbour2(sorted, offset[v], count[v], [&](int nbr, int c0, int c1, const int*, const int*) {
        if (nbr > (int)v && c0 + c1 == 1) n++;
    });
    bcount[v] = n;
}

// the half-edges of the owned boundary edges of every vertex, in its list's (ascending neighbour) order; the degrees on the boundary
__global__ void __launch_bounds__(MR_THREADS)
fh_fill_kernel(int V, int F, int B, const unsigned long long* __restrict__ sorted, const unsigned* __restrict__ offset,
               const unsigned* __restrict__ count, const unsigned char* __restrict__ flipped, FillScratch s) {
    const long long v = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    if (v >= V) return;
    long long at = s.boff[v];
    for_each_neighbour2(sorted, offset[v], count[v], [&](int nbr, int c0, int c1, const int* f0, const int* f1) {
        if (nbr <= (int)v || c0 + c1 != 1) return;
        const int f = c0 == 1 ? f0[0] : f1[0];
        bool leaving = c0 == 1;  // the face traverses v -> nbr
        if (flipped && f >= 0 && f < F && flipped[f]) leaving = !leaving;
        const int a = leaving ? (int)v : nbr, b = leaving ? nbr : (int)v;
        if (at < B && nbr < V) {  // (nothing is written at or behind B; nbr indexes the degrees)
            s.tail[at] = a;
            s.head[at] = b;
            atomicAdd(s.outdeg + a, 1u);
            atomicAdd(s.indeg + b, 1u);
            atomicMin(s.outhe + a, (unsigned)at);  // (read for simple vertices only, where this is the single writer)
        }
        at++;
    });
}

__global__ void __launch_bounds__(MR_THREADS) fh_next_kernel(int V, int B, FillScratch s) {
    const long long i = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    if (i >= B || i >= s.ctl[0]) return;
    const int b = s.head[i];
    int nx = -1;
    if (b >= 0 && b < V && s.outdeg[b] == 1u && s.indeg[b] == 1u) nx = (int)s.outhe[b];  // (b is simple)
    if (nx >= B) nx = -1;
    s.next[i] = nx;
    s.pd[0][i] = make_int2((int)i, nx);
}

// (min, jump)[i] <- (min(min[i], min[jump[i]]), jump[jump[i]]); jump < 0, "the chain ends", is absorbing
__global__ void __launch_bounds__(MR_THREADS) fh_double_kernel(int B, const unsigned* __restrict__ total, const int2* __restrict__ in, int2* __restrict__ out) {
    const long long i = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    if (i >= B || i >= total[0]) return;
    int2 me = in[i];
    if (me.y >= 0) {
        const int2 other = in[me.y];
        me.x = other.x < me.x ? other.x : me.x;
        me.y = other.y;
    }
    out[i] = me;
}

// info: boundary edges, holes filled, holes too long, edges on open chains (verts added and faces added come from the scan)
__global__ void __launch_bounds__(MR_THREADS)
fh_leader_kernel(int B, int max_hole_edges, const float* __restrict__ verts, const int2* __restrict__ pd, FillScratch s, int* __restrict__ info) {
    const long long i = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    const bool live = i < B && i < s.ctl[0];
    bool chain = false;
    if (live) {
        const int2 me = pd[i];
        chain = me.y < 0;
        int len = 0;
        if (!chain && me.x == (int)i) {  // the leader of a cycle
            int n = 1, j = s.next[i];
            while (j != (int)i && j >= 0 && n <= max_hole_edges) {  // (ends: n grows to max_hole_edges + 1)
                j = s.next[j];
                n++;
            }
            if (j == (int)i && n <= max_hole_edges) {
                len = n;
                atomicAdd(info + 1, 1);
                if (n >= 4) {  // the centroid: the tails in loop order from the leader's, in fp64, divided once, rounded once
                    double sum[3] = {0.0, 0.0, 0.0};
                    j = (int)i;
                    for (int k = 0; k < n; k++) {  // (ends: k grows to n)
                        const long long t = s.tail[j];
#pragma unroll
                        for (int a = 0; a < 3; a++) sum[a] += (double)verts[3 * t + a];
                        j = s.next[j];
                    }
#pragma unroll
                    for (int a = 0; a < 3; a++) s.cent[3 * i + a] = (float)(sum[a] / (double)n);
                }
            } else {
                atomicAdd(info + 2, 1);
            }
        }
        s.len[i] = len;
        if (i == 0) info[0] = (int)s.ctl[0];
    }
    const unsigned chains = wave_sum_u32(chain ? 1u : 0u);  // (every lane takes part: nothing returns above)
    if (lane_id() == 0 && chains > 0u) atomicAdd(info + 3, (int)chains);
}

// what half-edge i adds: x[0] new vertices (the leader of a hole of 4 or more), x[1] new faces (one per half-edge; one per triangular hole)
struct FillLoad {
    const unsigned* total;
    const int2* pd;
    const int* len;
    __device__ void operator()(long long i, unsigned* x) const {
        x[0] = x[1] = 0u;
        if (i >= total[0]) return;
        const int2 me = pd[i];
        if (me.y < 0) return;
        const int n = len[me.x];
        if (n == 0) return;
        const bool leader = me.x == (int)i;
        x[0] = n >= 4 && leader ? 1u : 0u;
        x[1] = n >= 4 || leader ? 1u : 0u;
    }
};
struct FillStore {
    unsigned *voff, *foff;
    __device__ void operator()(long long i, const unsigned*, const unsigned* pre) const {
        voff[i] = pre[0];
        foff[i] = pre[1];
    }
};

__global__ void __launch_bounds__(MR_THREADS)
fh_emit_kernel(int V, int F, int B, int nv, int nf, const int2* __restrict__ pd, FillScratch s, float* __restrict__ verts_out,
               int* __restrict__ faces_out) {
    const long long i = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    if (i >= B || i >= s.ctl[0]) return;
    const int2 me = pd[i];
    if (me.y < 0) return;
    const int n = s.len[me.x];
    if (n == 0) return;
    const bool leader = me.x == (int)i;
    const int a = s.tail[i], b = s.head[i];
    const long long at = s.foff[i];
    if (n == 3) {
        if (leader && at < nf) {
            faces_out[3 * ((long long)F + at)] = b;
            faces_out[3 * ((long long)F + at) + 1] = a;
            faces_out[3 * ((long long)F + at) + 2] = s.head[s.next[i]];
        }
        return;
    }
    const long long nw = s.voff[me.x];
    if (nw >= nv) return;  // (nothing is written at or behind V + nv rows and F + nf rows)
    if (leader) {
#pragma unroll
        for (int k = 0; k < 3; k++) verts_out[3 * ((long long)V + nw) + k] = s.cent[3 * i + k];
    }
    if (at < nf) {
        faces_out[3 * ((long long)F + at)] = b;
        faces_out[3 * ((long long)F + at) + 1] = a;
        faces_out[3 * ((long long)F + at) + 2] = (int)((long long)V + nw);
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

size_t dgm_mesh_orient_scratch_bytes(int V, int F) {
    if (V < 0 || F < 0 || F > ME_MAX_FACES) return 0;
    return orient_layout(nullptr, F).bytes;
}

int dgm_mesh_orient(int V, int F, const float* verts, const int* faces, char* edges_scratch, char* scratch, int outward, int* faces_out,
                    unsigned char* flipped, int* info, void* stream) {
    if (check_sizes("mesh_orient", V, F)) return 1;
    if (!info) return fail("mesh_orient: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (V == 0 || F == 0) {  // no valid face: nothing to orient, and no box for the volume rule
        if (hipMemsetAsync(info, 0, MR_INFO * 4, st) != hipSuccess) return launch_status();
        if (outward && hipMemsetAsync(info + 5, 1, 1, st) != hipSuccess) return launch_status();  // (the low byte: outward skipped = 1)
        if (F > 0) {
            if (!faces || !faces_out || !flipped) return fail("mesh_orient: NULL pointer");
            if (hipMemcpyAsync(faces_out, faces, (size_t)F * 12, hipMemcpyDeviceToDevice, st) != hipSuccess) return launch_status();
            if (hipMemsetAsync(flipped, 0, (size_t)F, st) != hipSuccess) return launch_status();
        }
        return launch_status();
    }
    if (!verts || !faces || !edges_scratch || !scratch || !faces_out || !flipped) return fail("mesh_orient: NULL pointer");
    if (faces_out == faces) return fail("mesh_orient: faces_out must not be faces");
    const EdgesScratch e = edges_layout(edges_scratch, V, F);
    const OrientScratch s = orient_layout(scratch, F);
    hipLaunchKernelGGL(or_init_kernel, dim3(blocks(2ll * F)), dim3(MR_THREADS), 0, st, F, s, info);
    if (outward) hipLaunchKernelGGL(or_box_kernel, dim3(blocks(V)), dim3(MR_THREADS), 0, st, V, verts, (const unsigned*)e.count, s.box);
    hipLaunchKernelGGL(or_hook_kernel, dim3(blocks(V)), dim3(MR_THREADS), 0, st, V, F, (const unsigned long long*)e.sorted, (const unsigned*)e.offset,
                       (const unsigned*)e.count, s.parent, s.conn);
    hipLaunchKernelGGL(or_label_kernel, dim3(blocks(F)), dim3(MR_THREADS), 0, st, V, F, verts, faces, outward ? 1 : 0, s);
    hipLaunchKernelGGL(or_decide_kernel, dim3(blocks(F)), dim3(MR_THREADS), 0, st, F, faces, outward ? 1 : 0, s, faces_out, flipped, info);
    return launch_status();
}

size_t dgm_mesh_fill_scratch_bytes(int V, int B) {
    if (V < 0 || B < 0 || B > 3 * (long long)ME_MAX_FACES) return 0;
    return fill_layout(nullptr, V, B).bytes;
}

int dgm_mesh_fill_count(int V, int F, int B, const float* verts, char* edges_scratch, const unsigned char* flipped, int max_hole_edges,
                        char* scratch, int* info, void* stream) {
    if (check_sizes("mesh_fill_count", V, F)) return 1;
    if (B < 0 || (long long)B > 3ll * F) return fail("mesh_fill_count: need 0 <= B <= 3 F");
    if (max_hole_edges < 0) return fail("mesh_fill_count: need max_hole_edges >= 0");
    if (!info || (V > 0 && B > 0 && (!verts || !edges_scratch || !scratch))) return fail("mesh_fill_count: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(info, 0, MR_INFO * 4, st) != hipSuccess) return launch_status();
    if (V == 0 || B == 0) return launch_status();
    const EdgesScratch e = edges_layout(edges_scratch, V, F);
    const FillScratch s = fill_layout(scratch, V, B);
    const unsigned long long* sorted = e.sorted;
    const unsigned *offset = e.offset, *count = e.count;
    if (hipMemsetAsync(s.indeg, 0, (size_t)V * 4, st) != hipSuccess || hipMemsetAsync(s.outdeg, 0, (size_t)V * 4, st) != hipSuccess ||
        hipMemsetAsync(s.outhe, 0xff, (size_t)V * 4, st) != hipSuccess)
        return launch_status();
    hipLaunchKernelGGL(fh_count_kernel, dim3(blocks(V)), dim3(MR_THREADS), 0, st, V, sorted, offset, count, s.bcount);
    scan_exclusive(st, (long long)V, (const unsigned*)s.bcount, s.tile_total, s.tile_off, s.boff, nullptr, false, s.ctl);
    hipLaunchKernelGGL(fh_fill_kernel, dim3(blocks(V)), dim3(MR_THREADS), 0, st, V, F, B, sorted, offset, count, flipped, s);
    hipLaunchKernelGGL(fh_next_kernel, dim3(blocks(B)), dim3(MR_THREADS), 0, st, V, B, s);
    const int rounds = doubling_rounds(B);  // fixed before anything is launched: it depends on B alone
    for (int k = 0; k < rounds; k++)
        hipLaunchKernelGGL(fh_double_kernel, dim3(blocks(B)), dim3(MR_THREADS), 0, st, B, (const unsigned*)s.ctl, (const int2*)s.pd[k & 1], s.pd[(k + 1) & 1]);
    const int2* pd = s.pd[rounds & 1];
    hipLaunchKernelGGL(fh_leader_kernel, dim3(blocks(B)), dim3(MR_THREADS), 0, st, B, max_hole_edges, verts, pd, s, info);
    scan_exclusive<2>(st, (long long)B, FillLoad{s.ctl, pd, s.len}, FillStore{s.voff, s.foff}, s.tile_total, s.tile_off, (unsigned*)info + 4);
    return launch_status();
}

int dgm_mesh_fill_emit(int V, int F, int B, const float* verts, const int* faces, char* scratch, int nv, int nf, float* verts_out,
                       int* faces_out, void* stream) {
    if (check_sizes("mesh_fill_emit", V, F)) return 1;
    if (B < 0 || (long long)B > 3ll * F) return fail("mesh_fill_emit: need 0 <= B <= 3 F");
    if (nv < 0 || nf < 0 || nv > B || nf > B) return fail("mesh_fill_emit: need 0 <= nv <= B and 0 <= nf <= B");
    if ((long long)V + nv > 0x7fffffffll) return fail("mesh_fill_emit: V + nv is over the int32 range of a face index");
    if ((V + nv > 0 && !verts_out) || (F + nf > 0 && !faces_out) || (V > 0 && !verts) || (F > 0 && !faces) || (nf > 0 && !scratch))
        return fail("mesh_fill_emit: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (V > 0 && hipMemcpyAsync(verts_out, verts, (size_t)V * 12, hipMemcpyDeviceToDevice, st) != hipSuccess) return launch_status();
    if (F > 0 && hipMemcpyAsync(faces_out, faces, (size_t)F * 12, hipMemcpyDeviceToDevice, st) != hipSuccess) return launch_status();
    if (nf == 0) return launch_status();
    const FillScratch s = fill_layout(scratch, V, B);
    hipLaunchKernelGGL(fh_emit_kernel, dim3(blocks(B)), dim3(MR_THREADS), 0, st, V, F, B, nv, nf, (const int2*)s.pd[doubling_rounds(B) & 1], s, verts_out,
                       faces_out);
    return launch_status();
}

}  // extern "C"
