// Entering the mesh phase for gfx950: the device side of GaussianModelDPSRDynamicAnchor.update_scale_center and normal_initialization
// (R/scene/gaussian_model_dpsr_dynamic_anchor.py:93-120, 684-734; R/ = dgmesh/).  The reference takes 50 torch.max / torch.min pairs
// for the bounding boxes and copies the mesh to the host for trimesh.sample.sample_surface (numpy cumsum / searchsorted).  Here
// (DESIGN.md section 4.7):
//   bbox        the six extrema of xyz + d_xyz (one fp32 addition per coordinate, as the reference) in ONE launch: 16-byte loads of
//               four 12-byte rows per thread, a wave / workgroup reduction, per-workgroup partials and a last-arriver finish.  Min and
//               max are exact (and -0 < +0 here), so the result does not depend on the reduction tree.  A NaN coordinate makes both extrema of its axis
//               NaN (torch.max / torch.min propagate NaN).
//   face_areas  area[f] = 0.5 |cross(v1 - v0, v2 - v0)| in fp32 without FMA; 0 for an index outside [0, V) and for a non-finite result.
//   area_scan   inclusive cumulative areas in fp64 over a FIXED partition (tiles of 4096 faces, 16 consecutive faces per thread):
//               per-thread running sums, the thread totals of a tile added up in thread order, the tile totals in tile order.  Every
//               level hands its exact partial sum to the next (the last value of a thread IS the prefix of the next thread), so cum is
//               non-decreasing exactly, independent of scheduling, and bit-reproducible.
//   sample      pick = double(u0) * cum[F - 1]; face = the smallest i with cum[i] >= pick (numpy searchsorted side="left") among the
//               faces with cum[i] > 0, so a face of area 0 is never chosen; trimesh's fold (u1 + u2 > 1: both become 1 - u);
//               point = v0 + (u1 (v1 - v0) + u2 (v2 - v0)) in fp32 without FMA.  cum[F - 1] == 0: face -1 and NaN points.
// Scratch is caller-owned; nothing here allocates device memory or reads anything back to the host.
#include <float.h>
#include <math.h>

#include "dgm_host.hpp"

#pragma clang fp contract(off)

namespace {
using namespace dgm;

constexpr int NI_THREADS = 256;
constexpr int NI_WAVES = NI_THREADS / 64;
constexpr int BBOX_MAX_BLOCKS = 256;                     // partial rows; the finishing workgroup reads one per thread
constexpr int BBOX_GROUP = 4;                            // rows per thread and pass: 48 bytes = three 16-byte loads
constexpr int SCAN_ITEMS = 16;                           // consecutive faces per thread
constexpr int SCAN_TILE = NI_THREADS * SCAN_ITEMS;       // faces per workgroup



// ---- bounding box --------------------------------------------------------------------------------------------------------------
// (the comparisons are false for a NaN `a`, so a NaN that got in stays; a NaN `b` always gets in.  -0 counts as less than +0, so
// that the sign of a zero extremum does not depend on the reduction tree either; torch.aminmax may report the other zero)
__device__ __forceinline__ float nan_min(float a, float b) { return (b < a || b != b || (b == a && signbit(b))) ? b : a; }
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b || (b == a && !signbit(b))) ? b : a; }

struct Box {
    float mn[3], mx[3];
};

__device__ __forceinline__ void box_add(Box& bx, int axis, float v) {
    bx.mn[axis] = nan_min(bx.mn[axis], v);
    bx.mx[axis] = nan_max(bx.mx[axis], v);
}

// reduction over the workgroup; the result is valid in thread 0
__device__ __forceinline__ Box box_reduce(Box bx, float (*red)[6]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            bx.mn[a] = nan_min(bx.mn[a], __shfl_xor(bx.mn[a], off));
            bx.mx[a] = nan_max(bx.mx[a], __shfl_xor(bx.mx[a], off));
        }
    }
    const int wv = threadIdx.x >> 6;
    if (lane_id() == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            red[wv][a] = bx.mn[a];
            red[wv][3 + a] = bx.mx[a];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NI_WAVES; w++) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                bx.mn[a] = nan_min(bx.mn[a], red[w][a]);
                bx.mx[a] = nan_max(bx.mx[a], red[w][3 + a]);
            }
        }
    }
    __syncthreads();
    return bx;
}

// partial: (gridDim.x, 6) floats; arrive: one counter, zero on entry and zero again on exit
template <bool VEC>
__global__ void __launch_bounds__(NI_THREADS)
bbox_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ dxyz, float* partial, unsigned* __restrict__ arrive,
            float* __restrict__ out) {
    __shared__ float red[NI_WAVES + 1][6];  // (row NI_WAVES, word 0: "this workgroup arrived last")
    Box bx;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        bx.mn[a] = INFINITY;
        bx.mx[a] = -INFINITY;
    }
    const long long tid = (long long)blockIdx.x * NI_THREADS + threadIdx.x, nthreads = (long long)gridDim.x * NI_THREADS;
    if (VEC) {
        const long long groups = P / BBOX_GROUP;
        const float4* x4 = (const float4*)xyz;
        const float4* d4 = (const float4*)dxyz;
        for (long long g = tid; g < groups; g += nthreads) {
            float v[12];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float4 p = x4[3 * g + k];
                v[4 * k] = p.x, v[4 * k + 1] = p.y, v[4 * k + 2] = p.z, v[4 * k + 3] = p.w;
            }
            if (dxyz) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float4 d = d4[3 * g + k];
                    v[4 * k] += d.x, v[4 * k + 1] += d.y, v[4 * k + 2] += d.z, v[4 * k + 3] += d.w;
                }
            }
#pragma unroll
            for (int k = 0; k < 12; k++) box_add(bx, k % 3, v[k]);
        }
        for (long long i = groups * BBOX_GROUP + tid; i < P; i += nthreads) {  // the P % 4 last rows
#pragma unroll
            for (int a = 0; a < 3; a++) box_add(bx, a, dxyz ? xyz[3 * i + a] + dxyz[3 * i + a] : xyz[3 * i + a]);
        }
    } else {
        for (long long i = tid; i < P; i += nthreads) {
#pragma unroll
            for (int a = 0; a < 3; a++) box_add(bx, a, dxyz ? xyz[3 * i + a] + dxyz[3 * i + a] : xyz[3 * i + a]);
        }
    }
    bx = box_reduce(bx, red);
    // hand the partial to whichever workgroup arrives last: plain stores, an agent-scope release before the ticket, and an
    // agent-scope acquire by every thread of the finisher before it reads the partials (the per-XCD L2s are not coherent with each
    // other; `partial` is written by other workgroups, hence not __restrict__).  The explicit waits around the release stay: the
    // ticket must not be drawn before the stores have left, whatever the compiler makes of the fence's own wait.
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            partial[blockIdx.x * 6 + a] = bx.mn[a];
            partial[blockIdx.x * 6 + 3 + a] = bx.mx[a];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        red[NI_WAVES][0] = ticket == gridDim.x - 1 ? 1.f : 0.f;
    }
    __syncthreads();
    if (red[NI_WAVES][0] == 0.f) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
    for (int a = 0; a < 3; a++) {
        bx.mn[a] = INFINITY;
        bx.mx[a] = -INFINITY;
    }
    if (threadIdx.x < gridDim.x) {  // gridDim.x <= BBOX_MAX_BLOCKS == NI_THREADS
#pragma unroll
        for (int a = 0; a < 3; a++) {
            bx.mn[a] = partial[threadIdx.x * 6 + a];
            bx.mx[a] = partial[threadIdx.x * 6 + 3 + a];
        }
    }
    bx = box_reduce(bx, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            out[a] = bx.mn[a];
            out[3 + a] = bx.mx[a];
        }
        __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next frame's launch
    }
}

// ---- face areas ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NI_THREADS)
face_area_kernel(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, float* __restrict__ area) {
    const long long f = (long long)blockIdx.x * NI_THREADS + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {
        area[f] = 0.f;
        return;
    }
    float p0[3], p1[3], p2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        p0[k] = verts[3 * (long long)a + k];
        p1[k] = verts[3 * (long long)b + k];
        p2[k] = verts[3 * (long long)c + k];
    }
    const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const float ar = 0.5f * sqrtf((nx * nx + ny * ny) + nz * nz);
    area[f] = ar < INFINITY ? ar : 0.f;  // (NaN and +inf: a face that is never chosen)
}

// ---- fp64 cumulative areas -----------------------------------------------------------------------------------------------------
// The 16 areas of this thread (0 behind F), its exclusive prefix inside the tile (thread totals added in thread order by thread 0)
// and the tile's total.
__device__ __forceinline__ double tile_prefix(long long F, const float* __restrict__ area, long long base, double* a, double* lds,
                                              double& total) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        a[k] = base + k < F ? (double)area[base + k] : 0.0;
        s += a[k];
    }
    lds[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double run = 0.0;
        for (int t = 0; t < NI_THREADS; t++) {
            const double v = lds[t];
            lds[t] = run;
            run += v;
        }
        lds[NI_THREADS] = run;
    }
    __syncthreads();
    total = lds[NI_THREADS];
    return lds[threadIdx.x];
}

__global__ void __launch_bounds__(NI_THREADS) scan_totals_kernel(long long F, const float* __restrict__ area, double* __restrict__ tile_total) {
    __shared__ double lds[NI_THREADS + 1];
    double a[SCAN_ITEMS], total;
    tile_prefix(F, area, (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS, a, lds, total);
    if (threadIdx.x == 0) tile_total[blockIdx.x] = total;
}

// one workgroup: exclusive offsets of the tiles, added in tile order
__global__ void __launch_bounds__(NI_THREADS) scan_offsets_kernel(int nb, const double* __restrict__ tile_total, double* __restrict__ tile_off) {
    __shared__ double lds[NI_THREADS];
    __shared__ double carry;
    if (threadIdx.x == 0) carry = 0.0;
    for (int base = 0; base < nb; base += NI_THREADS) {
        const int i = base + (int)threadIdx.x;
        lds[threadIdx.x] = i < nb ? tile_total[i] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            double run = carry;
            for (int t = 0; t < NI_THREADS; t++) {
                const double v = lds[t];
                lds[t] = run;
                run += v;
            }
            carry = run;
        }
        __syncthreads();
        if (i < nb) tile_off[i] = lds[threadIdx.x];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(NI_THREADS)
scan_emit_kernel(long long F, const float* __restrict__ area, const double* __restrict__ tile_off, double* __restrict__ cum) {
    __shared__ double lds[NI_THREADS + 1];
    double a[SCAN_ITEMS], total;
    const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
    const double pre = tile_prefix(F, area, base, a, lds, total);
    const double off = tile_off[blockIdx.x];
    double run = 0.0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        run += a[k];
        if (base + k < F) cum[base + k] = off + (pre + run);
    }
}

// ---- sampling ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NI_THREADS)
sample_kernel(int V, int F, int count, const float* __restrict__ verts, const int* __restrict__ faces, const double* __restrict__ cum,
              const float* __restrict__ u, float* __restrict__ points, int* __restrict__ face_index) {
    const long long s = (long long)blockIdx.x * NI_THREADS + threadIdx.x;
    if (s >= count) return;
    const float nan = __int_as_float(0x7fc00000);
    const double total = cum[F - 1];
    int f = -1;
    if (total > 0.0) {
        const double pick = (double)u[3 * s] * total;
        int lo = 0, hi = F - 1;  // (cum[F - 1] = total >= pick and > 0: the answer exists)
        while (lo < hi) {
            const int mid = (int)(((long long)lo + hi) >> 1);
            const double c = cum[mid];
            if (c >= pick && c > 0.0)
                hi = mid;
            else
                lo = mid + 1;
        }
        f = lo;
    }
    int a = 0, b = 0, c = 0;
    if (f >= 0) a = faces[3 * (long long)f], b = faces[3 * (long long)f + 1], c = faces[3 * (long long)f + 2];
    // (a chosen face has a positive area, hence indices in range; the test keeps a corrupted table from reading outside verts)
    if (f < 0 || a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) {
        face_index[s] = -1;
        points[3 * s] = points[3 * s + 1] = points[3 * s + 2] = nan;
        return;
    }
    float u1 = u[3 * s + 1], u2 = u[3 * s + 2];
    if (u1 + u2 > 1.0f) {
        u1 = 1.0f - u1;
        u2 = 1.0f - u2;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float p0 = verts[3 * (long long)a + k], p1 = verts[3 * (long long)b + k], p2 = verts[3 * (long long)c + k];
        points[3 * s + k] = p0 + (u1 * (p1 - p0) + u2 * (p2 - p0));
    }
    face_index[s] = f;
}

int scan_blocks(long long n) { return (int)((n + SCAN_TILE - 1) / SCAN_TILE); }

}  // namespace

extern "C" {

size_t dgm_ninit_bbox_scratch_bytes(void) { return 256 + (size_t)BBOX_MAX_BLOCKS * 6 * 4 + 256; }

int dgm_ninit_bbox(int P, const float* xyz, const float* d_xyz, char* scratch, float* out6, void* stream) {
    if (P <= 0) return fail("ninit_bbox: need P >= 1 (the extrema of an empty set do not exist)");
    if (!xyz || !scratch || !out6) return fail("ninit_bbox: NULL pointer");
    char* base = align_ptr(scratch);
    unsigned* arrive = (unsigned*)base;
    float* partial = (float*)(base + 256);
    long long nb = ((long long)P + NI_THREADS * BBOX_GROUP - 1) / (NI_THREADS * BBOX_GROUP);
    if (nb > BBOX_MAX_BLOCKS) nb = BBOX_MAX_BLOCKS;
    const bool vec = (((uintptr_t)xyz | (uintptr_t)d_xyz) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(bbox_kernel<true>, dim3((unsigned)nb), dim3(NI_THREADS), 0, (hipStream_t)stream, P, xyz, d_xyz, partial, arrive,
                           out6);
    else
        hipLaunchKernelGGL(bbox_kernel<false>, dim3((unsigned)nb), dim3(NI_THREADS), 0, (hipStream_t)stream, P, xyz, d_xyz, partial, arrive,
                           out6);
    return launch_status();
}

int dgm_ninit_face_areas(int V, int F, const float* verts, const int* faces, float* area, void* stream) {
    if (V < 0 || F < 0) return fail("ninit_face_areas: need V >= 0 and F >= 0");
    if (F == 0) return 0;
    if (!faces || !area || (V > 0 && !verts)) return fail("ninit_face_areas: NULL pointer");
    hipLaunchKernelGGL(face_area_kernel, dim3(blocks(F)), dim3(NI_THREADS), 0, (hipStream_t)stream, V, F, verts, faces, area);
    return launch_status();
}

size_t dgm_ninit_scan_scratch_bytes(int F) {
    if (F < 0) return 0;
    const size_t nb = (size_t)scan_blocks(F) + 1;
    return 2 * align_up(nb * 8, 256) + 256;
}

int dgm_ninit_area_scan(int F, const float* area, char* scratch, double* cum, void* stream) {
    if (F < 0) return fail("ninit_area_scan: need F >= 0");
    if (F == 0) return 0;
    if (!area || !scratch || !cum) return fail("ninit_area_scan: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    const int nb = scan_blocks(F);
    char* base = align_ptr(scratch);
    double* tile_total = (double*)base;
    double* tile_off = (double*)(base + align_up(((size_t)nb + 1) * 8, 256));
    hipLaunchKernelGGL(scan_totals_kernel, dim3(nb), dim3(NI_THREADS), 0, st, (long long)F, area, tile_total);
    hipLaunchKernelGGL(scan_offsets_kernel, dim3(1), dim3(NI_THREADS), 0, st, nb, (const double*)tile_total, tile_off);
    hipLaunchKernelGGL(scan_emit_kernel, dim3(nb), dim3(NI_THREADS), 0, st, (long long)F, area, (const double*)tile_off, cum);
    return launch_status();
}

int dgm_ninit_sample(int V, int F, int count, const float* verts, const int* faces, const double* cum, const float* u, float* points,
                     int* face_index, void* stream) {
    if (V < 0 || F < 1 || count < 0) return fail("ninit_sample: need V >= 0, F >= 1 and count >= 0");
    if (count == 0) return 0;
    if (!faces || !cum || !u || !points || !face_index || (V > 0 && !verts)) return fail("ninit_sample: NULL pointer");
    hipLaunchKernelGGL(sample_kernel, dim3(blocks(count)), dim3(NI_THREADS), 0, (hipStream_t)stream, V, F, count, verts, faces, cum, u,
                       points, face_index);
    return launch_status();
}

}  // extern "C"
