// Differentiable triangle rasterizer for gfx950: rasterize -> interpolate -> antialias with the call shapes of nvdiffrast.torch,
// and their adjoints.  Stands where nvdiffrast stands in the reference's mesh branch (R/utils/renderer.py:33-121).
//
// Conventions (include/dgmesh_hip.h, section "mesh rasterizer"; dg-mesh_amd/mesh_raster.py): pos (V, 4) clip space, tri (F, 3)
// int32, screen s = ((x/w + 1) W/2, (y/w + 1) H/2), pixel (px, py) centred at (px + .5, py + .5), row 0 at NDC y = -1.
//
// Forward raster: one thread per triangle sets it up (culled when a vertex has w <= 0, an index is outside [0, V), or the fp64
// signed area of the fp32 screen triangle is zero or not finite) and walks the pixel centres of its bounding box; a triangle
// whose box holds more than RAST_LARGE centres is appended to a list (wave-aggregated counter) that a second kernel walks with a
// workgroup per triangle.  A covered centre does one 64-bit atomicMin of (ordered bits of z/w) << 32 | face id, so the winner --
// smallest z/w, ties to the lower id -- does not depend on arrival order, and neither on the split.  A resolve pass turns each
// winning key into (u, v, z/w, id + 1), recomputed from the face with the same expressions: the forward is bit-reproducible.
//
// Coverage: the edge function of edge k (opposite vertex k) is evaluated with its endpoints in ascending vertex-id order and
// negated when that reverses the triangle's order, so the two faces of a shared edge see exactly negated values; a centre is
// covered when all three oriented values are >= 0 (inclusive edges: a closed mesh has no cracks).
//
// Antialias: per pair of horizontal / vertical neighbours with different ids, the front pixel's face T (smaller z/w; background
// farthest) and the first silhouette edge of T (one face, two faces whose third vertices lie on the same screen side, or more than
// two faces; horizontal pairs consider only edges with |ds_y| >= |ds_x|, vertical pairs the others) whose line crosses the
// segment between the centres at distance t from the front centre: t > .5 blends (t - .5) of the front colour into the other
// pixel, t < .5 blends (.5 - t) of the other colour into the front pixel.  Edge topology: an open-addressing hash of the
// undirected edges built per call (face count and xor of the third vertices), reused by the backward.
#include "dgm_host.hpp"

using namespace dgm;

namespace {

constexpr int TR_THREADS = 256;
constexpr int RAST_LARGE = 64;           // bounding-box pixel centres above which a triangle goes to the workgroup path
constexpr int RAST_LARGE_BLOCKS = 1024;  // workgroups of the large-triangle pass (they stride over the list)
constexpr int TR_MAX_DIM = 16384;        // H, W limit: H * W and every pixel index stay far inside int32
constexpr unsigned long long KEY_EMPTY = ~0ull;

struct RastLayout {
    size_t keys, list, counter, total;
};

// scratch: keys[H W] (u64 depth | id) | list[F] (int, large triangles) | counter (uint)
RastLayout rast_layout(int F, int H, int W) {
    RastLayout L;
    L.keys = 0;
    L.list = align_up(L.keys + (size_t)H * W * sizeof(unsigned long long), 256);
    L.counter = align_up(L.list + (size_t)F * sizeof(int), 256);
    L.total = align_up(L.counter + sizeof(unsigned), 256);
    return L;
}

struct AaLayout {
    size_t keys, vals, total;
    unsigned cap;
};

// scratch: keys[cap] (u64 min id << 32 | max id, KEY_EMPTY when free) | vals[cap] (uint2: face count, xor of third vertices)
AaLayout aa_layout(int F) {
    AaLayout L;
    L.cap = (unsigned)(4 * (size_t)F + 64);  // load factor <= 3/4 even when no edge is shared
    L.keys = 0;
    L.vals = align_up(L.keys + (size_t)L.cap * sizeof(unsigned long long), 256);
    L.total = align_up(L.vals + (size_t)L.cap * sizeof(uint2), 256);
    return L;
}

struct Tri {
    float sx[3], sy[3], zw[3], w[3];
    int vid[3];
    bool ok;
    float o;  // +1 / -1: orientation of the screen triangle
};

__device__ __forceinline__ int edge_a(int k) { return k == 2 ? 0 : k + 1; }  // edge k: vertices ((k+1)%3, (k+2)%3)
__device__ __forceinline__ int edge_b(int k) { return k == 0 ? 2 : k - 1; }

__device__ __forceinline__ void screen(float4 p, int H, int W, float& sx, float& sy, float& zw) {
    sx = (p.x / p.w + 1.f) * (0.5f * (float)W);
    sy = (p.y / p.w + 1.f) * (0.5f * (float)H);
    zw = p.z / p.w;
}

__device__ __forceinline__ Tri tri_setup(const float4* __restrict__ pos, const int* __restrict__ tri, int f, int V, int H, int W) {
    Tri t;
    t.ok = false;
    t.o = 1.f;
#pragma unroll
    for (int k = 0; k < 3; k++) t.vid[k] = tri[(size_t)f * 3 + k];
    if ((unsigned)t.vid[0] >= (unsigned)V || (unsigned)t.vid[1] >= (unsigned)V || (unsigned)t.vid[2] >= (unsigned)V) return t;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float4 p = pos[t.vid[k]];
        if (!(p.w > 0.f)) return t;  // (NaN w: culled too)
        screen(p, H, W, t.sx[k], t.sy[k], t.zw[k]);
        t.w[k] = p.w;
        fin = fin && isfinite(t.sx[k]) && isfinite(t.sy[k]) && isfinite(t.zw[k]);
    }
    if (!fin) return t;
    // orientation from the exact sign of the fp32 screen triangle's area (differences and products of fp32 are exact in fp64)
    const double ax = (double)t.sx[1] - (double)t.sx[0], ay = (double)t.sy[1] - (double)t.sy[0];
    const double bx = (double)t.sx[2] - (double)t.sx[0], by = (double)t.sy[2] - (double)t.sy[0];
    const double a2 = ax * by - ay * bx;
    if (!(a2 != 0.0)) return t;
    t.o = a2 > 0.0 ? 1.f : -1.f;
    t.ok = true;
    return t;
}

__device__ __forceinline__ float edge_fn(float ax, float ay, float bx, float by, float px, float py) {
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

// E_k(p): edge k with its endpoints in ascending vertex-id order, signed as in the triangle's cyclic order
__device__ __forceinline__ float edge_canon(const Tri& t, int k, float px, float py) {
    const int a = edge_a(k), b = edge_b(k);
    if (t.vid[a] <= t.vid[b]) return edge_fn(t.sx[a], t.sy[a], t.sx[b], t.sy[b], px, py);
    return -edge_fn(t.sx[b], t.sy[b], t.sx[a], t.sy[a], px, py);
}

struct Sample {
    float E[3];
    bool covered;
};

__device__ __forceinline__ Sample sample(const Tri& t, float px, float py) {
    Sample s;
#pragma unroll
    for (int k = 0; k < 3; k++) s.E[k] = edge_canon(t, k, px, py);
    const float D = s.E[0] + s.E[1] + s.E[2];
    s.covered = t.o * s.E[0] >= 0.f && t.o * s.E[1] >= 0.f && t.o * s.E[2] >= 0.f && D != 0.f;
    return s;
}

__device__ __forceinline__ float sample_depth(const Tri& t, const Sample& s) {
    const float D = s.E[0] + s.E[1] + s.E[2];
    return (s.E[0] * t.zw[0] + s.E[1] * t.zw[1] + s.E[2] * t.zw[2]) / D;
}

__device__ __forceinline__ unsigned long long depth_key(float zw, int f) {
    unsigned u = __float_as_uint(zw);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned)f;
}

// bounding box of the pixel centres of a set-up triangle (empty: x1 < x0 or y1 < y0)
__device__ __forceinline__ void tri_bbox(const Tri& t, int H, int W, int& x0, int& x1, int& y0, int& y1) {
    const float mnx = fminf(t.sx[0], fminf(t.sx[1], t.sx[2])), mxx = fmaxf(t.sx[0], fmaxf(t.sx[1], t.sx[2]));
    const float mny = fminf(t.sy[0], fminf(t.sy[1], t.sy[2])), mxy = fmaxf(t.sy[0], fmaxf(t.sy[1], t.sy[2]));
    x0 = (int)ceilf(fminf(fmaxf(mnx - 0.5f, -1.f), (float)W));
    x1 = (int)floorf(fminf(fmaxf(mxx - 0.5f, -1.f), (float)W));
    y0 = (int)ceilf(fminf(fmaxf(mny - 0.5f, -1.f), (float)H));
    y1 = (int)floorf(fminf(fmaxf(mxy - 0.5f, -1.f), (float)H));
    x0 = max(x0, 0), y0 = max(y0, 0), x1 = min(x1, W - 1), y1 = min(y1, H - 1);
}

__device__ __forceinline__ void raster_pixel(const Tri& t, int f, int px, int py, int W, unsigned long long* __restrict__ keys) {
    const Sample s = sample(t, (float)px + 0.5f, (float)py + 0.5f);
    if (!s.covered) return;
    atomicMin(keys + (size_t)py * W + px, depth_key(sample_depth(t, s), f));
}

// ---- forward raster: one thread per triangle; large ones go to the list -------------------------------------------------------
__global__ void __launch_bounds__(TR_THREADS)
raster_small_kernel(int V, int F, int H, int W, const float4* __restrict__ pos, const int* __restrict__ tri,
                    unsigned long long* __restrict__ keys, int* __restrict__ list, unsigned* __restrict__ counter) {
    const int f = blockIdx.x * TR_THREADS + threadIdx.x;
    Tri t;
    t.ok = false;
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    if (f < F) {
        t = tri_setup(pos, tri, f, V, H, W);
        if (t.ok) tri_bbox(t, H, W, x0, x1, y0, y1);
    }
    const long long n = (x1 >= x0 && y1 >= y0) ? (long long)(x1 - x0 + 1) * (y1 - y0 + 1) : 0;
    const bool big = n > RAST_LARGE;
    const unsigned long long m = __ballot(big);
    if (big) {  // wave-aggregated append: one atomic per wave
        const int lane = lane_id(), leader = __ffsll((unsigned long long)m) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(m));
        base = __shfl(base, leader);
        list[base + __popcll(m & ((1ull << lane) - 1ull))] = f;
        return;
    }
    for (int py = y0; py <= y1; py++)
        for (int px = x0; px <= x1; px++) raster_pixel(t, f, px, py, W, keys);
}

__global__ void __launch_bounds__(TR_THREADS)
raster_large_kernel(int V, int H, int W, const float4* __restrict__ pos, const int* __restrict__ tri, unsigned long long* __restrict__ keys,
                    const int* __restrict__ list, const unsigned* __restrict__ counter) {
    const unsigned n = *counter;
    for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
        const int f = list[i];
        const Tri t = tri_setup(pos, tri, f, V, H, W);
        int x0, x1, y0, y1;
        tri_bbox(t, H, W, x0, x1, y0, y1);
        const int bw = x1 - x0 + 1;
        const int cnt = bw * (y1 - y0 + 1);  // (<= H W < 2^28)
        for (int j = threadIdx.x; j < cnt; j += TR_THREADS) raster_pixel(t, f, x0 + j % bw, y0 + j / bw, W, keys);
    }
}

struct Bary {
    float e[3], S, u, v;
};

// perspective-correct barycentrics: e_k = E_k / w_k, u = e_0 / S, v = e_1 / S (S = e_0 + e_1 + e_2)
__device__ __forceinline__ Bary bary(const Tri& t, const Sample& s) {
    Bary b;
#pragma unroll
    for (int k = 0; k < 3; k++) b.e[k] = s.E[k] / t.w[k];
    b.S = b.e[0] + b.e[1] + b.e[2];
    b.u = b.e[0] / b.S, b.v = b.e[1] / b.S;
    return b;
}

__global__ void __launch_bounds__(TR_THREADS)
raster_resolve_kernel(int V, int H, int W, const float4* __restrict__ pos, const int* __restrict__ tri,
                      const unsigned long long* __restrict__ keys, float4* __restrict__ rast) {
    const int p = blockIdx.x * TR_THREADS + threadIdx.x;
    if (p >= H * W) return;
    const unsigned long long key = keys[p];
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (key != KEY_EMPTY) {
        const int f = (int)(unsigned)(key & 0xffffffffu);
        const Tri t = tri_setup(pos, tri, f, V, H, W);
        const Sample s = sample(t, (float)(p % W) + 0.5f, (float)(p / W) + 0.5f);
        const Bary b = bary(t, s);
        r = make_float4(b.u, b.v, sample_depth(t, s), (float)(f + 1));
    }
    rast[p] = r;
}

// d(screen x, y) (+ a direct w term) of one vertex -> d(clip x, y, w), scattered
__device__ __forceinline__ void scatter_screen_grad(float* __restrict__ dpos, int vid, float4 p, int H, int W, float gsx, float gsy,
                                                    float gw) {
    const float iw = 1.f / p.w;
    const float dx = gsx * (0.5f * (float)W) * iw, dy = gsy * (0.5f * (float)H) * iw;
    const float dw = gw - (dx * p.x + dy * p.y) * iw;
    atomicAdd(dpos + (size_t)vid * 4 + 0, dx);
    atomicAdd(dpos + (size_t)vid * 4 + 1, dy);
    atomicAdd(dpos + (size_t)vid * 4 + 3, dw);
}

// accumulates g x the gradients of E(a, b, x) = (b - a) x (x - a) w.r.t. a and b
__device__ __forceinline__ void edge_grad(float ax, float ay, float bx, float by, float px, float py, float g, float& gax, float& gay,
                                          float& gbx, float& gby) {
    gax += g * (by - py), gay += g * (px - bx);
    gbx += g * (py - ay), gby += g * (ax - px);
}

// ---- rasterize backward: drast (u, v) -> dpos (x, y, w) of the winning face's vertices -----------------------------------------
__global__ void __launch_bounds__(TR_THREADS)
raster_backward_kernel(int V, int F, int H, int W, const float4* __restrict__ pos, const int* __restrict__ tri,
                       const float4* __restrict__ rast, const float4* __restrict__ drast, float* __restrict__ dpos) {
    const int p = blockIdx.x * TR_THREADS + threadIdx.x;
    if (p >= H * W) return;
    const int id = (int)rast[p].w;
    if (id <= 0 || id > F) return;
    const float4 d = drast[p];
    if (d.x == 0.f && d.y == 0.f) return;
    const Tri t = tri_setup(pos, tri, id - 1, V, H, W);
    if (!t.ok) return;
    const float px = (float)(p % W) + 0.5f, py = (float)(p / W) + 0.5f;
    const Sample s = sample(t, px, py);
    const Bary b = bary(t, s);
    float gsx[3] = {0.f, 0.f, 0.f}, gsy[3] = {0.f, 0.f, 0.f}, gw[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float ge = (d.x * ((k == 0 ? 1.f : 0.f) - b.u) + d.y * ((k == 1 ? 1.f : 0.f) - b.v)) / b.S;  // dL/de_k
        gw[k] = -ge * b.e[k] / t.w[k];
        const int a = edge_a(k), c = edge_b(k);
        edge_grad(t.sx[a], t.sy[a], t.sx[c], t.sy[c], px, py, ge / t.w[k], gsx[a], gsy[a], gsx[c], gsy[c]);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) scatter_screen_grad(dpos, t.vid[k], pos[t.vid[k]], H, W, gsx[k], gsy[k], gw[k]);
}

// ---- interpolate -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool face_verts(const int* __restrict__ tri, int id, int V, int F, int v[3]) {
    if (id <= 0 || id > F) return false;
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = tri[(size_t)(id - 1) * 3 + k];
    return (unsigned)v[0] < (unsigned)V && (unsigned)v[1] < (unsigned)V && (unsigned)v[2] < (unsigned)V;
}

__global__ void __launch_bounds__(TR_THREADS)
interp_forward_kernel(int V, int F, int HW, int C, const float* __restrict__ attr, const float4* __restrict__ rast,
                      const int* __restrict__ tri, float* __restrict__ out) {
    const int p = blockIdx.x * TR_THREADS + threadIdx.x;
    if (p >= HW) return;
    const float4 r = rast[p];
    int v[3];
    float* o = out + (size_t)p * C;
    if (!face_verts(tri, (int)r.w, V, F, v)) {
        for (int c = 0; c < C; c++) o[c] = 0.f;
        return;
    }
    const float w2 = 1.f - r.x - r.y;
    for (int c = 0; c < C; c++)
        o[c] = r.x * attr[(size_t)v[0] * C + c] + r.y * attr[(size_t)v[1] * C + c] + w2 * attr[(size_t)v[2] * C + c];
}

__global__ void __launch_bounds__(TR_THREADS)
interp_backward_kernel(int V, int F, int HW, int C, const float* __restrict__ attr, const float4* __restrict__ rast,
                       const int* __restrict__ tri, const float* __restrict__ dout, float* __restrict__ dattr, float4* __restrict__ drast) {
    const int p = blockIdx.x * TR_THREADS + threadIdx.x;
    if (p >= HW) return;
    const float4 r = rast[p];
    int v[3];
    float du = 0.f, dv = 0.f;
    if (face_verts(tri, (int)r.w, V, F, v)) {
        const float w2 = 1.f - r.x - r.y;
        const float* g = dout + (size_t)p * C;
        for (int c = 0; c < C; c++) {
            const float gc = g[c];
            const float a2 = attr[(size_t)v[2] * C + c];
            du += gc * (attr[(size_t)v[0] * C + c] - a2);
            dv += gc * (attr[(size_t)v[1] * C + c] - a2);
            if (gc != 0.f) {
                atomicAdd(dattr + (size_t)v[0] * C + c, r.x * gc);
                atomicAdd(dattr + (size_t)v[1] * C + c, r.y * gc);
                atomicAdd(dattr + (size_t)v[2] * C + c, w2 * gc);
            }
        }
    }
    drast[p] = make_float4(du, dv, 0.f, 0.f);
}

// ---- antialias: edge topology --------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long edge_key(int a, int b) {
    const unsigned lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
    return ((unsigned long long)lo << 32) | hi;
}

__device__ __forceinline__ unsigned hash_slot(unsigned long long key, unsigned cap) {
    const unsigned long long h = key * 0x9E3779B97F4A7C15ull;
    return (unsigned)(((h >> 32) * (unsigned long long)cap) >> 32);
}

__global__ void __launch_bounds__(TR_THREADS)
topo_build_kernel(int V, int F, const int* __restrict__ tri, unsigned cap, unsigned long long* __restrict__ keys, uint2* __restrict__ vals) {
    const int f = blockIdx.x * TR_THREADS + threadIdx.x;
    if (f >= F) return;
    int v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = tri[(size_t)f * 3 + k];
    if ((unsigned)v[0] >= (unsigned)V || (unsigned)v[1] >= (unsigned)V || (unsigned)v[2] >= (unsigned)V) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const unsigned long long key = edge_key(v[edge_a(k)], v[edge_b(k)]);
        unsigned s = hash_slot(key, cap);
        for (;;) {  // (load factor <= 3/4: a free slot always exists)
            const unsigned long long old = atomicCAS(keys + s, KEY_EMPTY, key);
            if (old == KEY_EMPTY || old == key) break;
            s = s + 1 == cap ? 0 : s + 1;
        }
        atomicAdd(&vals[s].x, 1u);
        atomicXor(&vals[s].y, (unsigned)v[k]);
    }
}

__device__ __forceinline__ uint2 topo_find(unsigned long long key, unsigned cap, const unsigned long long* __restrict__ keys,
                                           const uint2* __restrict__ vals) {
    unsigned s = hash_slot(key, cap);
    for (unsigned n = 0; n < cap; n++) {
        const unsigned long long k = keys[s];
        if (k == key) return vals[s];
        if (k == KEY_EMPTY) break;
        s = s + 1 == cap ? 0 : s + 1;
    }
    return make_uint2(0u, 0u);
}

struct AaCtx {
    int V, F, H, W;
    const float4* pos;
    const int* tri;
    const float4* rast;
    unsigned cap;
    const unsigned long long* keys;
    const uint2* vals;
};

struct AaHit {
    bool hit;
    bool q_front;  // the front pixel is q (else p)
    float t;       // crossing distance from the front centre, in pixels
    int k;         // the edge of the front face
    float ff, fo;  // E of that edge at the front / the other centre
    Tri tr;
};

// edge k of T is a silhouette: one face, more than two, or two whose third vertices lie on the same screen side (or on the line)
__device__ __forceinline__ bool silhouette(const AaCtx& c, const Tri& T, int k) {
    const int a = edge_a(k), b = edge_b(k);
    const uint2 e = topo_find(edge_key(T.vid[a], T.vid[b]), c.cap, c.keys, c.vals);
    if (e.x != 2u) return true;
    const int other = (int)(e.y ^ (unsigned)T.vid[k]);
    if ((unsigned)other >= (unsigned)c.V) return true;
    float ox, oy, oz;
    screen(c.pos[other], c.H, c.W, ox, oy, oz);
    const float Ec = edge_fn(T.sx[a], T.sy[a], T.sx[b], T.sy[b], T.sx[k], T.sy[k]);
    const float Eo = edge_fn(T.sx[a], T.sy[a], T.sx[b], T.sy[b], ox, oy);
    return !((Ec > 0.f && Eo < 0.f) || (Ec < 0.f && Eo > 0.f));
}

// the pair (p, q), q = p + 1 (horizontal) or p + W (vertical)
__device__ __forceinline__ AaHit aa_pair(const AaCtx& c, int p, int q, bool vertical) {
    AaHit h;
    h.hit = false;
    const float4 rp = c.rast[p], rq = c.rast[q];
    const int ip = (int)rp.w, iq = (int)rq.w;
    if (ip == iq) return h;
    bool qf;  // front: the smaller (z/w, id); background farthest
    if (ip == 0) qf = true;
    else if (iq == 0) qf = false;
    else qf = rq.z < rp.z || (rq.z == rp.z && iq < ip);
    const int idf = qf ? iq : ip;
    if (idf <= 0 || idf > c.F) return h;
    h.tr = tri_setup(c.pos, c.tri, idf - 1, c.V, c.H, c.W);
    if (!h.tr.ok) return h;
    const int pf = qf ? q : p, po = qf ? p : q;
    const float fx = (float)(pf % c.W) + 0.5f, fy = (float)(pf / c.W) + 0.5f;
    const float ox = (float)(po % c.W) + 0.5f, oy = (float)(po / c.W) + 0.5f;
    const Tri& T = h.tr;
    for (int k = 0; k < 3; k++) {
        const int a = edge_a(k), b = edge_b(k);
        const float dx = T.sx[b] - T.sx[a], dy = T.sy[b] - T.sy[a];
        const bool steep = fabsf(dy) >= fabsf(dx);
        if (steep == vertical) continue;
        const float ff = edge_fn(T.sx[a], T.sy[a], T.sx[b], T.sy[b], fx, fy);
        const float fo = edge_fn(T.sx[a], T.sy[a], T.sx[b], T.sy[b], ox, oy);
        if (!((ff > 0.f && fo < 0.f) || (ff < 0.f && fo > 0.f))) continue;
        if (!silhouette(c, T, k)) continue;
        h.hit = true, h.q_front = qf, h.k = k, h.ff = ff, h.fo = fo, h.t = ff / (ff - fo);
        return h;
    }
    return h;
}

// the pixel that receives the blend, the one whose colour is blended in, and the weight (0 when t == .5)
__device__ __forceinline__ void aa_target(const AaHit& h, int p, int q, int& tgt, int& src, float& alpha) {
    const int pf = h.q_front ? q : p, po = h.q_front ? p : q;
    if (h.t > 0.5f) tgt = po, src = pf, alpha = h.t - 0.5f;
    else tgt = pf, src = po, alpha = 0.5f - h.t;
}

// the pairs of pixel p in a fixed order (left, right, up, down), each as its (first pixel, vertical)
__device__ __forceinline__ int aa_pairs_of(int p, int W, int H, int first[4], bool vert[4]) {
    const int x = p % W, y = p / W;
    int n = 0;
    if (x > 0) first[n] = p - 1, vert[n] = false, n++;
    if (x < W - 1) first[n] = p, vert[n] = false, n++;
    if (y > 0) first[n] = p - W, vert[n] = true, n++;
    if (y < H - 1) first[n] = p, vert[n] = true, n++;
    return n;
}

__global__ void __launch_bounds__(TR_THREADS)
aa_forward_kernel(AaCtx c, int C, const float* __restrict__ color, float* __restrict__ out) {
    const int p = blockIdx.x * TR_THREADS + threadIdx.x;
    if (p >= c.H * c.W) return;
    int first[4];
    bool vert[4];
    const int n = aa_pairs_of(p, c.W, c.H, first, vert);
    const float* cp = color + (size_t)p * C;
    float* o = out + (size_t)p * C;
    for (int ch = 0; ch < C; ch++) o[ch] = cp[ch];
    for (int i = 0; i < n; i++) {
        const int a = first[i], b = vert[i] ? a + c.W : a + 1;
        const AaHit h = aa_pair(c, a, b, vert[i]);
        if (!h.hit) continue;
        int tgt, src;
        float al;
        aa_target(h, a, b, tgt, src, al);
        if (tgt != p || al == 0.f) continue;
        const float* cs = color + (size_t)src * C;
        for (int ch = 0; ch < C; ch++) o[ch] += al * (cs[ch] - cp[ch]);
    }
}

__global__ void __launch_bounds__(TR_THREADS)
aa_backward_kernel(AaCtx c, int C, const float* __restrict__ color, const float* __restrict__ dout, float* __restrict__ dcolor,
                   float* __restrict__ dpos) {
    const int p = blockIdx.x * TR_THREADS + threadIdx.x;
    if (p >= c.H * c.W) return;
    int first[4];
    bool vert[4];
    const int n = aa_pairs_of(p, c.W, c.H, first, vert);
    float* dc = dcolor + (size_t)p * C;
    const float* gp = dout + (size_t)p * C;
    for (int ch = 0; ch < C; ch++) dc[ch] = gp[ch];
    for (int i = 0; i < n; i++) {
        const int a = first[i], b = vert[i] ? a + c.W : a + 1;
        const AaHit h = aa_pair(c, a, b, vert[i]);
        if (!h.hit) continue;
        int tgt, src;
        float al;
        aa_target(h, a, b, tgt, src, al);
        // colour (a gather): out[tgt] += al (color[src] - color[tgt])
        const float* gt = dout + (size_t)tgt * C;
        if (tgt == p) {
            for (int ch = 0; ch < C; ch++) dc[ch] -= al * gp[ch];
        } else {
            for (int ch = 0; ch < C; ch++) dc[ch] += al * gt[ch];
        }
        // positions (a scatter): once per pair, by its first pixel; dL/dt = +-sum_c (color[src] - color[tgt]) dout[tgt]
        if (a != p) continue;
        const float* cs = color + (size_t)src * C;
        const float* ct = color + (size_t)tgt * C;
        float G = 0.f;
        for (int ch = 0; ch < C; ch++) G += (cs[ch] - ct[ch]) * gt[ch];
        if (G == 0.f || al == 0.f) continue;
        const float gtt = h.t > 0.5f ? G : -G;
        const float den = h.ff - h.fo;
        const float gff = gtt * (-h.fo) / (den * den), gfo = gtt * h.ff / (den * den);
        const int pf = h.q_front ? b : a, po = h.q_front ? a : b;
        const float fx = (float)(pf % c.W) + 0.5f, fy = (float)(pf / c.W) + 0.5f;
        const float ox = (float)(po % c.W) + 0.5f, oy = (float)(po / c.W) + 0.5f;
        const Tri& T = h.tr;
        const int ea = edge_a(h.k), eb = edge_b(h.k);
        float gax = 0.f, gay = 0.f, gbx = 0.f, gby = 0.f;
        edge_grad(T.sx[ea], T.sy[ea], T.sx[eb], T.sy[eb], fx, fy, gff, gax, gay, gbx, gby);
        edge_grad(T.sx[ea], T.sy[ea], T.sx[eb], T.sy[eb], ox, oy, gfo, gax, gay, gbx, gby);
        scatter_screen_grad(dpos, T.vid[ea], c.pos[T.vid[ea]], c.H, c.W, gax, gay, 0.f);
        scatter_screen_grad(dpos, T.vid[eb], c.pos[T.vid[eb]], c.H, c.W, gbx, gby, 0.f);
    }
}


bool tr_dims(int V, int F, int H, int W) {
    return V >= 0 && F >= 0 && F < (1 << 24) && H > 0 && W > 0 && H <= TR_MAX_DIM && W <= TR_MAX_DIM;
}


}  // namespace

extern "C" {

size_t dgm_tri_raster_scratch_bytes(int F, int H, int W) {
    return tr_dims(0, F, H, W) ? rast_layout(F, H, W).total : 0;
}

int dgm_tri_rasterize_forward(int V, int F, int H, int W, const float* pos, const int* tri, char* scratch, float* rast, void* stream) {
    if (!tr_dims(V, F, H, W)) return fail("tri_rasterize: need V >= 0, 0 <= F < 2^24 and 0 < H, W <= 16384");
    if (!scratch || !rast || (F > 0 && (!tri || (V > 0 && !pos)))) return fail("tri_rasterize: NULL pointer");
    const RastLayout L = rast_layout(F, H, W);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)(scratch + L.keys);
    unsigned* counter = (unsigned*)(scratch + L.counter);
    if (hipMemsetAsync(keys, 0xff, (size_t)H * W * sizeof(unsigned long long), st) != hipSuccess ||
        hipMemsetAsync(counter, 0, sizeof(unsigned), st) != hipSuccess)
        return fail("tri_rasterize: memset failed");
    if (F > 0 && V > 0) {
        hipLaunchKernelGGL(raster_small_kernel, dim3(blocks(F)), dim3(TR_THREADS), 0, st, V, F, H, W, (const float4*)pos, tri, keys,
                           (int*)(scratch + L.list), counter);
        hipLaunchKernelGGL(raster_large_kernel, dim3((unsigned)min(F, RAST_LARGE_BLOCKS)), dim3(TR_THREADS), 0, st, V, H, W,
                           (const float4*)pos, tri, keys, (const int*)(scratch + L.list), (const unsigned*)counter);
    }
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(blocks((long long)H * W)), dim3(TR_THREADS), 0, st, V, H, W, (const float4*)pos, tri,
                       (const unsigned long long*)keys, (float4*)rast);
    return launch_status();
}

int dgm_tri_rasterize_backward(int V, int F, int H, int W, const float* pos, const int* tri, const float* rast, const float* drast,
                               float* dpos, void* stream) {
    if (!tr_dims(V, F, H, W)) return fail("tri_rasterize_backward: need V >= 0, 0 <= F < 2^24 and 0 < H, W <= 16384");
    if (!rast || !drast || (V > 0 && (!pos || !dpos)) || (F > 0 && !tri)) return fail("tri_rasterize_backward: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (V == 0) return launch_status();
    if (hipMemsetAsync(dpos, 0, (size_t)V * 4 * sizeof(float), st) != hipSuccess) return fail("tri_rasterize_backward: memset failed");
    if (F > 0)
        hipLaunchKernelGGL(raster_backward_kernel, dim3(blocks((long long)H * W)), dim3(TR_THREADS), 0, st, V, F, H, W, (const float4*)pos,
                           tri, (const float4*)rast, (const float4*)drast, dpos);
    return launch_status();
}

int dgm_tri_interpolate_forward(int V, int F, int H, int W, int C, const float* attr, const float* rast, const int* tri, float* out,
                                void* stream) {
    if (!tr_dims(V, F, H, W) || C <= 0) return fail("tri_interpolate: need V >= 0, 0 <= F < 2^24, 0 < H, W <= 16384 and C > 0");
    if (!rast || !out || (V > 0 && !attr) || (F > 0 && !tri)) return fail("tri_interpolate: NULL pointer");
    hipLaunchKernelGGL(interp_forward_kernel, dim3(blocks((long long)H * W)), dim3(TR_THREADS), 0, (hipStream_t)stream, V, F, H * W, C,
                       attr, (const float4*)rast, tri, out);
    return launch_status();
}

int dgm_tri_interpolate_backward(int V, int F, int H, int W, int C, const float* attr, const float* rast, const int* tri,
                                 const float* dout, float* dattr, float* drast, void* stream) {
    if (!tr_dims(V, F, H, W) || C <= 0) return fail("tri_interpolate_backward: need V >= 0, 0 <= F < 2^24, 0 < H, W <= 16384 and C > 0");
    if (!rast || !dout || !drast || (V > 0 && (!attr || !dattr)) || (F > 0 && !tri)) return fail("tri_interpolate_backward: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (V > 0 && hipMemsetAsync(dattr, 0, (size_t)V * C * sizeof(float), st) != hipSuccess)
        return fail("tri_interpolate_backward: memset failed");
    hipLaunchKernelGGL(interp_backward_kernel, dim3(blocks((long long)H * W)), dim3(TR_THREADS), 0, st, V, F, H * W, C, attr,
                       (const float4*)rast, tri, dout, dattr, (float4*)drast);
    return launch_status();
}

size_t dgm_tri_aa_scratch_bytes(int F) {
    return tr_dims(0, F, 1, 1) ? aa_layout(F).total : 0;
}

int dgm_tri_antialias_forward(int V, int F, int H, int W, int C, const float* color, const float* rast, const float* pos, const int* tri,
                              char* scratch, float* out, void* stream) {
    if (!tr_dims(V, F, H, W) || C <= 0) return fail("tri_antialias: need V >= 0, 0 <= F < 2^24, 0 < H, W <= 16384 and C > 0");
    if (!color || !rast || !scratch || !out || (V > 0 && !pos) || (F > 0 && !tri)) return fail("tri_antialias: NULL pointer");
    const AaLayout L = aa_layout(F);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* keys = (unsigned long long*)(scratch + L.keys);
    uint2* vals = (uint2*)(scratch + L.vals);
    if (hipMemsetAsync(keys, 0xff, (size_t)L.cap * sizeof(unsigned long long), st) != hipSuccess ||
        hipMemsetAsync(vals, 0, (size_t)L.cap * sizeof(uint2), st) != hipSuccess)
        return fail("tri_antialias: memset failed");
    if (F > 0) hipLaunchKernelGGL(topo_build_kernel, dim3(blocks(F)), dim3(TR_THREADS), 0, st, V, F, tri, L.cap, keys, vals);
    const AaCtx c{V, F, H, W, (const float4*)pos, tri, (const float4*)rast, L.cap, keys, vals};
    hipLaunchKernelGGL(aa_forward_kernel, dim3(blocks((long long)H * W)), dim3(TR_THREADS), 0, st, c, C, color, out);
    return launch_status();
}

int dgm_tri_antialias_backward(int V, int F, int H, int W, int C, const float* color, const float* rast, const float* pos, const int* tri,
                               const char* scratch, const float* dout, float* dcolor, float* dpos, void* stream) {
    if (!tr_dims(V, F, H, W) || C <= 0) return fail("tri_antialias_backward: need V >= 0, 0 <= F < 2^24, 0 < H, W <= 16384 and C > 0");
    if (!color || !rast || !scratch || !dout || !dcolor || (V > 0 && (!pos || !dpos)) || (F > 0 && !tri))
        return fail("tri_antialias_backward: NULL pointer");
    const AaLayout L = aa_layout(F);
    hipStream_t st = (hipStream_t)stream;
    if (V > 0 && hipMemsetAsync(dpos, 0, (size_t)V * 4 * sizeof(float), st) != hipSuccess)
        return fail("tri_antialias_backward: memset failed");
    const AaCtx c{V, F, H, W, (const float4*)pos, tri, (const float4*)rast, L.cap, (const unsigned long long*)(scratch + L.keys),
                  (const uint2*)(scratch + L.vals)};
    hipLaunchKernelGGL(aa_backward_kernel, dim3(blocks((long long)H * W)), dim3(TR_THREADS), 0, st, c, C, color, dout, dcolor, dpos);
    return launch_status();
}

}  // extern "C"
