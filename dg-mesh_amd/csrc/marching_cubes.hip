// Differentiable marching cubes for gfx950: scalar grid -> triangle mesh, and the adjoint back to the grid (and a per-point
// deformation).  Stands where diso.DiffMC stands in the reference's mesh branch (R/utils/renderer.py:171).
//
// Conventions (include/dgmesh_hip.h, section "marching cubes"): grid (X, Y, Z) fp32 row-major, point (i, j, k) at (i, j, k);
// inside iff f < iso (NaN: outside); edge a->b crossed iff inside(a) != inside(b); vertex p_a + t (p_b - p_a),
// t = (iso - fa) / (fb - fa), p = index (+ deform[point]); optional division by (dim - 1) per axis.  Case table:
// mc_tables.hpp (tools/gen_mc_tables.py).
//
// Ordering without atomics: every grid point owns its +x, +y, +z edges, so a vertex is (point, axis) and needs no dedup.  The
// count pass packs, per 64 consecutive points (a "word", one wave), four 64-bit ballots -- inside, x-, y-, z-crossed -- plus the
// word's vertex / triangle counts; one workgroup scans the per-block totals; the emit pass turns them into per-word offsets and
// writes the vertices; the face pass reads the offsets of any word to name the vertices of a cell's edges:
//     vid(q, axis) = voff[q / 64] + popcount of the crossed bits of the word's lanes below q + crossed lower axes of q itself.
// Those 0.5 B of ballots + 8 B of offsets per 64 points are the edge-to-vertex map the backward gathers through: each point sums
// the terms of its <= 6 incident crossed edges in a fixed order (own x, y, z, then incoming x, y, z), so dgrid is bit-reproducible.
#include "dgm_host.hpp"
#include "mc_tables.hpp"

using namespace dgm;

namespace {

constexpr int MC_THREADS = 256;           // count / emit: 4 waves, each takes 4 words (4 points per thread)
constexpr int MC_PTS = 1024;              // points per count / emit workgroup
constexpr int MC_WORDS = MC_PTS / 64;     // words per count / emit workgroup
constexpr int MC_SCAN_THREADS = 1024;     // the single workgroup of the block scan

struct McWord {
    unsigned long long in, ex, ey, ez;  // lane l <-> point 64 w + l: inside, +x / +y / +z edge crossed
};

struct McLayout {
    size_t words, wcnt, voff, foff, blk, total;
};

// scratch: words[W] (32 B) | wcnt[W] (uint2: vertices, triangles of the word) | voff[W] | foff[W] | blk[NB] (uint2: block totals,
// then their exclusive prefix)
McLayout mc_layout(long long N) {
    const size_t W = (size_t)((N + 63) / 64), NB = (size_t)((N + MC_PTS - 1) / MC_PTS);
    McLayout L;
    L.words = 0;
    L.wcnt = align_up(L.words + W * sizeof(McWord), 256);
    L.voff = align_up(L.wcnt + W * sizeof(uint2), 256);
    L.foff = align_up(L.voff + W * sizeof(unsigned), 256);
    L.blk = align_up(L.foff + W * sizeof(unsigned), 256);
    L.total = align_up(L.blk + NB * sizeof(uint2), 256);
    return L;
}

struct McDims {
    int X, Y, Z;
    long long YZ, N;
};

__device__ __forceinline__ bool mc_inside(float f, float iso) { return f < iso; }  // (NaN < iso is false: outside)

__device__ __forceinline__ unsigned mc_bit(unsigned long long m, int l) { return (unsigned)(m >> l) & 1u; }

__device__ __forceinline__ bool mc_in(const McWord* __restrict__ W, long long q) { return mc_bit(W[q >> 6].in, (int)(q & 63)) != 0; }

// case of the cell whose origin is point p (corner c at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1))
__device__ __forceinline__ unsigned mc_case(const McWord* __restrict__ W, long long p, const McDims& d) {
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const long long q = p + (k & 1) * d.YZ + ((k >> 1) & 1) * (long long)d.Z + (k >> 2);
        c |= (unsigned)mc_in(W, q) << k;
    }
    return c;
}

__device__ __forceinline__ int mc_vid(const McWord* __restrict__ W, const unsigned* __restrict__ voff, long long q, int axis) {
    const long long w = q >> 6;
    const int l = (int)(q & 63);
    const unsigned long long low = (1ull << l) - 1ull;
    const McWord m = W[w];
    unsigned v = voff[w] + __popcll(m.ex & low) + __popcll(m.ey & low) + __popcll(m.ez & low);
    if (axis > 0) v += mc_bit(m.ex, l);
    if (axis > 1) v += mc_bit(m.ey, l);
    return (int)v;
}

// (32-bit division: every point index is < 2^31 (mc_dims); a 64-bit division is a long software sequence on the GPU)
__device__ __forceinline__ void mc_decode(long long p, const McDims& d, int& i, int& j, int& k) {
    const unsigned u = (unsigned)p, yz = (unsigned)d.YZ, z = (unsigned)d.Z;
    const unsigned ii = u / yz, r = u - ii * yz, jj = r / z;
    i = (int)ii, j = (int)jj, k = (int)(r - jj * z);
}

// ---- count: ballots, per-word and per-block vertex / triangle counts -------------------------------------------------------------
__global__ void __launch_bounds__(MC_THREADS)
mc_count_kernel(McDims d, const float* __restrict__ g, float iso, McWord* __restrict__ words, uint2* __restrict__ wcnt,
                uint2* __restrict__ blk) {
    __shared__ unsigned s_v[MC_THREADS / 64], s_f[MC_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const long long nW = (d.N + 63) >> 6;
    unsigned tv = 0, tf = 0;
    for (int r = 0; r < MC_PTS / MC_THREADS; r++) {
        const long long p = (long long)blockIdx.x * MC_PTS + r * MC_THREADS + threadIdx.x;
        bool in = false, cx = false, cy = false, cz = false;
        unsigned nt = 0;
        if (p < d.N) {
            int i, j, k;
            mc_decode(p, d, i, j, k);
            const float f0 = g[p];
            in = mc_inside(f0, iso);
            bool ix = false, iy = false, iz = false;
            if (i < d.X - 1) ix = mc_inside(g[p + d.YZ], iso), cx = in != ix;
            if (j < d.Y - 1) iy = mc_inside(g[p + d.Z], iso), cy = in != iy;
            if (k < d.Z - 1) iz = mc_inside(g[p + 1], iso), cz = in != iz;
            if (i < d.X - 1 && j < d.Y - 1 && k < d.Z - 1) {
                const bool ixy = mc_inside(g[p + d.YZ + d.Z], iso), ixz = mc_inside(g[p + d.YZ + 1], iso);
                const bool iyz = mc_inside(g[p + d.Z + 1], iso), ixyz = mc_inside(g[p + d.YZ + d.Z + 1], iso);
                const unsigned c = (unsigned)in | ((unsigned)ix << 1) | ((unsigned)iy << 2) | ((unsigned)ixy << 3) |
                                   ((unsigned)iz << 4) | ((unsigned)ixz << 5) | ((unsigned)iyz << 6) | ((unsigned)ixyz << 7);
                nt = dgm_mc_tri_count[c];
            }
        }
        McWord m;
        m.in = __ballot(in), m.ex = __ballot(cx), m.ey = __ballot(cy), m.ez = __ballot(cz);
        const unsigned nv = __popcll(m.ex) + __popcll(m.ey) + __popcll(m.ez);
        const unsigned nf = wave_sum_u32(nt);
        const long long w = (long long)blockIdx.x * MC_WORDS + r * (MC_THREADS / 64) + wave;
        if (lane == 0 && w < nW) {
            words[w] = m;
            wcnt[w] = make_uint2(nv, nf);
        }
        tv += nv, tf += nf;
    }
    if (lane == 0) s_v[wave] = tv, s_f[wave] = tf;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned v = 0, f = 0;
        for (int w = 0; w < MC_THREADS / 64; w++) v += s_v[w], f += s_f[w];
        blk[blockIdx.x] = make_uint2(v, f);
    }
}

// ---- scan: block totals -> exclusive block offsets (in place) and {V, F} ----------------------------------------------------------
__device__ __forceinline__ unsigned mc_block_exclusive(unsigned v, unsigned* s_tot, unsigned& total) {
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const unsigned inc = wave_inclusive_scan_u32(v);
    if (lane == 63) s_tot[wave] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int w = 0; w < MC_SCAN_THREADS / 64; w++) {
        before += w < wave ? s_tot[w] : 0u;
        all += s_tot[w];
    }
    __syncthreads();
    total = all;
    return before + inc - v;
}

__global__ void __launch_bounds__(MC_SCAN_THREADS)
mc_scan_kernel(int NB, uint2* __restrict__ blk, int* __restrict__ counts) {
    __shared__ unsigned s_tot[2][MC_SCAN_THREADS / 64];
    const int seg = (NB + MC_SCAN_THREADS - 1) / MC_SCAN_THREADS;
    const int lo = min(NB, (int)threadIdx.x * seg), hi = min(NB, lo + seg);
    unsigned sv = 0, sf = 0;
#pragma unroll 8
    for (int b = lo; b < hi; b++) {  // (unrolled: the loads go out together instead of one latency each)
        const uint2 t = blk[b];
        sv += t.x, sf += t.y;
    }
    unsigned V, F;
    unsigned ov = mc_block_exclusive(sv, s_tot[0], V);
    unsigned of = mc_block_exclusive(sf, s_tot[1], F);
    for (int b = lo; b < hi; b++) {
        const uint2 t = blk[b];
        blk[b] = make_uint2(ov, of);
        ov += t.x, of += t.y;
    }
    if (threadIdx.x == 0) counts[0] = (int)V, counts[1] = (int)F;
}

// ---- emit: per-word offsets and the vertices (one thread per point; the vertices of a word are consecutive) -----------------------
__global__ void __launch_bounds__(MC_THREADS)
mc_emit_verts_kernel(McDims d, const float* __restrict__ g, const float* __restrict__ deform, float iso, int normalize,
                     const McWord* __restrict__ words, const uint2* __restrict__ wcnt, const uint2* __restrict__ blk,
                     unsigned* __restrict__ voff, unsigned* __restrict__ foff, int V, float* __restrict__ verts) {
    __shared__ uint2 s_off[MC_WORDS];
    const long long nW = (d.N + 63) >> 6;
    if (threadIdx.x == 0) {
        uint2 o = blk[blockIdx.x];
        for (int w = 0; w < MC_WORDS; w++) {  // word order inside the block = point order
            s_off[w] = o;
            const long long gw = (long long)blockIdx.x * MC_WORDS + w;
            if (gw < nW) {
                const uint2 c = wcnt[gw];
                o.x += c.x, o.y += c.y;
            }
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const float sx = normalize ? (float)(d.X - 1) : 1.f, sy = normalize ? (float)(d.Y - 1) : 1.f, sz = normalize ? (float)(d.Z - 1) : 1.f;
    for (int r = 0; r < MC_PTS / MC_THREADS; r++) {
        const int lw = r * (MC_THREADS / 64) + wave;
        const long long w = (long long)blockIdx.x * MC_WORDS + lw;
        if (w >= nW) break;  // (whole waves: w is uniform across the wave)
        if (lane == 0) voff[w] = s_off[lw].x, foff[w] = s_off[lw].y;
        const McWord m = words[w];
        const unsigned long long low = (1ull << lane) - 1ull;
        const unsigned crossed = mc_bit(m.ex, lane) | (mc_bit(m.ey, lane) << 1) | (mc_bit(m.ez, lane) << 2);
        if (!crossed) continue;
        unsigned v = s_off[lw].x + __popcll(m.ex & low) + __popcll(m.ey & low) + __popcll(m.ez & low);
        const long long p = w * 64 + lane;
        int idx[3];
        mc_decode(p, d, idx[0], idx[1], idx[2]);
        const float fa = g[p];
        float pa[3];
#pragma unroll
        for (int c = 0; c < 3; c++) pa[c] = deform ? (float)idx[c] + deform[p * 3 + c] : (float)idx[c];
        const long long stride[3] = {d.YZ, (long long)d.Z, 1};
        const float scale[3] = {sx, sy, sz};
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            if (!((crossed >> ax) & 1)) continue;
            const long long b = p + stride[ax];
            const float fb = g[b];
            const float t = (iso - fa) / (fb - fa);
            if ((int)v < V) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float ib = (float)(idx[c] + (c == ax));
                    const float pb = deform ? ib + deform[b * 3 + c] : ib;
                    float x = pa[c] + t * (pb - pa[c]);
                    if (normalize) x = x / scale[c];
                    verts[(size_t)v * 3 + c] = x;
                }
            }
            v++;
        }
    }
}

// ---- faces: one thread per cell origin; a wave scans its word's triangle counts -----------------------------------------------------
__global__ void __launch_bounds__(MC_THREADS)
mc_emit_faces_kernel(McDims d, const McWord* __restrict__ words, const unsigned* __restrict__ voff, const unsigned* __restrict__ foff,
                     int F, int* __restrict__ faces) {
    const long long p = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    unsigned c = 0, nt = 0;
    if (p < d.N) {
        int i, j, k;
        mc_decode(p, d, i, j, k);
        if (i < d.X - 1 && j < d.Y - 1 && k < d.Z - 1) {
            c = mc_case(words, p, d);
            nt = dgm_mc_tri_count[c];
        }
    }
    const unsigned excl = wave_inclusive_scan_u32(nt) - nt;
    if (!nt) return;
    const unsigned f0 = foff[p >> 6] + excl;
    for (unsigned s = 0; s < nt; s++) {
        if ((int)(f0 + s) >= F) break;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const int e = dgm_mc_tri_table[c][3 * s + r];
            const int a = dgm_mc_edge_corner_a[e];
            const long long q = p + (a & 1) * d.YZ + ((a >> 1) & 1) * (long long)d.Z + (a >> 2);
            faces[(size_t)(f0 + s) * 3 + r] = mc_vid(words, voff, q, e >> 2);
        }
    }
}

// ---- backward: gather over the <= 6 incident crossed edges of every point -----------------------------------------------------------
__global__ void __launch_bounds__(MC_THREADS)
mc_backward_kernel(McDims d, const float* __restrict__ g, const float* __restrict__ deform, float iso, int normalize,
                   const McWord* __restrict__ words, const unsigned* __restrict__ voff, int V, const float* __restrict__ dverts,
                   float* __restrict__ dgrid, float* __restrict__ ddeform) {
    const long long p = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (p >= d.N) return;
    int idx[3];
    mc_decode(p, d, idx[0], idx[1], idx[2]);
    const long long stride[3] = {d.YZ, (long long)d.Z, 1};
    const float scale[3] = {normalize ? (float)(d.X - 1) : 1.f, normalize ? (float)(d.Y - 1) : 1.f, normalize ? (float)(d.Z - 1) : 1.f};
    const McWord m = words[p >> 6];
    const int l = (int)(p & 63);
    unsigned own = mc_bit(m.ex, l) | (mc_bit(m.ey, l) << 1) | (mc_bit(m.ez, l) << 2), inc = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        if (idx[ax] > 0) {
            const long long q = p - stride[ax];
            const McWord mq = words[q >> 6];
            const unsigned long long bits = ax == 0 ? mq.ex : (ax == 1 ? mq.ey : mq.ez);
            inc |= mc_bit(bits, (int)(q & 63)) << ax;
        }
    }
    float gs = 0.f, dd[3] = {0.f, 0.f, 0.f};
    if (own | inc) {
        const float fp = g[p];
        float pp[3];
#pragma unroll
        for (int c = 0; c < 3; c++) pp[c] = deform ? (float)idx[c] + deform[p * 3 + c] : (float)idx[c];
        for (int dir = 0; dir < 2; dir++) {  // 0: p is a (own edges), 1: p is b (incoming edges)
            const unsigned set = dir ? inc : own;
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                if (!((set >> ax) & 1)) continue;
                const long long o = dir ? p - stride[ax] : p + stride[ax];
                const int vid = mc_vid(words, voff, dir ? o : p, ax);
                if (vid >= V) continue;
                const float fo = g[o];
                const float fa = dir ? fo : fp, fb = dir ? fp : fo;
                const float t = (iso - fa) / (fb - fa);
                float po[3], du[3], dt = 0.f;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const float io = (float)(idx[c] + (c == ax ? (dir ? -1 : 1) : 0));
                    po[c] = deform ? io + deform[o * 3 + c] : io;
                    du[c] = dverts[(size_t)vid * 3 + c] / scale[c];
                    const float pa = dir ? po[c] : pp[c], pb = dir ? pp[c] : po[c];
                    dt += du[c] * (pb - pa);
                }
                const float den = fb - fa;
                gs += dir ? dt * (-(iso - fa) / (den * den)) : dt * ((iso - fb) / (den * den));
                const float w = dir ? t : 1.f - t;
#pragma unroll
                for (int c = 0; c < 3; c++) dd[c] += w * du[c];
            }
        }
    }
    dgrid[p] = gs;
    if (ddeform) {
#pragma unroll
        for (int c = 0; c < 3; c++) ddeform[p * 3 + c] = dd[c];
    }
}


// dims >= 2 and every vertex id / triangle count within int32 (at most 3 vertices per point, 5 triangles per cell)
bool mc_dims(int X, int Y, int Z, McDims& d) {
    if (X < 2 || Y < 2 || Z < 2) return false;
    const long long N = (long long)X * Y * Z;
    if (N * (long long)DGM_MC_MAX_TRIS > 0x7fffffffLL) return false;
    d.X = X, d.Y = Y, d.Z = Z, d.YZ = (long long)Y * Z, d.N = N;
    return true;
}

}  // namespace

extern "C" {

size_t dgm_mc_scratch_bytes(int X, int Y, int Z) {
    McDims d;
    return mc_dims(X, Y, Z, d) ? mc_layout(d.N).total : 0;
}

int dgm_mc_count(int X, int Y, int Z, const float* grid, float iso, char* scratch, int* counts, void* stream) {
    McDims d;
    if (!mc_dims(X, Y, Z, d)) return fail("mc_count: every dimension must be >= 2 and 5 * X * Y * Z must fit in int32");
    if (!grid || !scratch || !counts) return fail("mc_count: NULL pointer");
    const McLayout L = mc_layout(d.N);
    hipStream_t st = (hipStream_t)stream;
    const int NB = (int)((d.N + MC_PTS - 1) / MC_PTS);
    hipLaunchKernelGGL(mc_count_kernel, dim3(NB), dim3(MC_THREADS), 0, st, d, grid, iso, (McWord*)(scratch + L.words),
                       (uint2*)(scratch + L.wcnt), (uint2*)(scratch + L.blk));
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(MC_SCAN_THREADS), 0, st, NB, (uint2*)(scratch + L.blk), counts);
    return launch_status();
}

int dgm_mc_emit(int X, int Y, int Z, const float* grid, const float* deform, float iso, int normalize, char* scratch, int V, int F,
                float* verts, int* faces, void* stream) {
    McDims d;
    if (!mc_dims(X, Y, Z, d)) return fail("mc_emit: every dimension must be >= 2 and 5 * X * Y * Z must fit in int32");
    if (!grid || !scratch || V < 0 || F < 0 || (V > 0 && !verts) || (F > 0 && !faces)) return fail("mc_emit: NULL pointer or bad count");
    const McLayout L = mc_layout(d.N);
    hipStream_t st = (hipStream_t)stream;
    const int NB = (int)((d.N + MC_PTS - 1) / MC_PTS);
    const McWord* words = (const McWord*)(scratch + L.words);
    unsigned* voff = (unsigned*)(scratch + L.voff);
    unsigned* foff = (unsigned*)(scratch + L.foff);
    hipLaunchKernelGGL(mc_emit_verts_kernel, dim3(NB), dim3(MC_THREADS), 0, st, d, grid, deform, iso, normalize, words,
                       (const uint2*)(scratch + L.wcnt), (const uint2*)(scratch + L.blk), voff, foff, V, verts);
    if (F > 0)
        hipLaunchKernelGGL(mc_emit_faces_kernel, dim3((unsigned)((d.N + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, st, d,
                           words, voff, foff, F, faces);
    return launch_status();
}

int dgm_mc_backward(int X, int Y, int Z, const float* grid, const float* deform, float iso, int normalize, const char* scratch, int V,
                    const float* dverts, float* dgrid, float* ddeform, void* stream) {
    McDims d;
    if (!mc_dims(X, Y, Z, d)) return fail("mc_backward: every dimension must be >= 2 and 5 * X * Y * Z must fit in int32");
    if (!grid || !scratch || !dgrid || V < 0 || (V > 0 && !dverts) || (!deform != !ddeform))
        return fail("mc_backward: NULL pointer or bad count");
    const McLayout L = mc_layout(d.N);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_backward_kernel, dim3((unsigned)((d.N + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0, st, d, grid,
                       deform, iso, normalize, (const McWord*)(scratch + L.words), (const unsigned*)(scratch + L.voff), V, dverts,
                       dgrid, ddeform);
    return launch_status();
}

}  // extern "C"
