// Inside / outside queries on a triangle mesh for gfx950: the generalised winding number of query points (mesh_inside.py; DESIGN.md
// section 4.17; include/dgmesh_hip.h states the definition).  The reference has no counterpart: it scores surfaces only.
//
// Per (query p, face (v0, v1, v2)) pair -- fp32, no FMA (this file is built with -ffp-contract=off); sqrt is the hardware's, within 1 ulp:
//   a = v0 - p, b = v1 - p, c = v2 - p                                        (per axis)
//   n = b x c:  n0 = b1*c2 - b2*c1, n1 = b2*c0 - b0*c2, n2 = b0*c1 - b1*c0
//   det = (a0*n0 + a1*n1) + a2*n2
//   la = sqrt((a0*a0 + a1*a1) + a2*a2), lb, lc alike;  ab = (a0*b0 + a1*b1) + a2*b2, bc, ca alike
//   den = (((la*lb)*lc + ab*lc) + bc*la) + ca*lb
//   omega = 2 atan2f(det, den), or exactly 0 when det is 0 or not finite          (van Oosterom and Strackee)
// A face with an index outside [0, V) (checked before any use) or a non-finite corner coordinate is staged as three equal corners:
// then b x c is exactly 0 without contraction (x*y - y*x), det is 0 and the face adds nothing.
//
// Summation order -- a function of F alone, so a query's bits do not depend on N, on the batch or on the run:
//   chunk   WN_CHUNK = 256 consecutive faces, the LDS tile: omega added in fp32, from 0, in face order
//   slice   WN_SLICE_CHUNKS = 64 consecutive chunks (16384 faces): the chunk sums added in fp64, from 0, in order
//   total   the slice sums added in fp64, from 0, in order;  w = (float)(total / (4 pi)), one rounding
// One workgroup takes 256 queries (one per lane) and one slice; it stages a chunk's faces into LDS as three float4 each, and every
// lane then reads the same face: an identical LDS address across the wave is a broadcast.  The next chunk's face is fetched into
// registers before the pair loop of the current one.  With more than one slice the slice sums go to scratch[slice * N + n] and a
// second launch adds them; with one slice the first launch writes w.  A query with a non-finite coordinate gets NaN.
//
// Termination.  No workgroup waits for another and nothing spins on a flag.  Every device loop below names what ends it.
// No atomics.  Scratch is caller-owned; nothing here allocates device memory or reads anything back to the host.
#include <float.h>
#include <math.h>

#include "dgm_host.hpp"

#pragma clang fp contract(off)

namespace {
using namespace dgm;

constexpr int WN_THREADS = 256;
constexpr int WN_CHUNK = 256;         // faces per LDS tile = per fp32 chunk sum (one face per thread when staging)
constexpr int WN_SLICE_CHUNKS = 64;   // chunks per workgroup = per fp64 slice sum
constexpr int WN_SLICE = WN_CHUNK * WN_SLICE_CHUNKS;
constexpr double WN_FOUR_PI = 12.566370614359172;  // 4 * M_PI

static_assert(WN_CHUNK == WN_THREADS, "one face per thread when staging");


long long slices_of(int F) { return ((long long)F + WN_SLICE - 1) / WN_SLICE; }

__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; }

// the face's corners; three equal corners (zeros) when it is invalid or beyond F (file header)
__device__ __forceinline__ void load_face(int V, int F, const float* __restrict__ verts, const int* __restrict__ faces, long long f, float t[9]) {
    bool ok = f < F;
    if (ok) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        ok = i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
        if (ok) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                t[k] = verts[3 * (long long)i0 + k];
                t[3 + k] = verts[3 * (long long)i1 + k];
                t[6 + k] = verts[3 * (long long)i2 + k];
            }
            ok = finite3(t[0], t[1], t[2]) && finite3(t[3], t[4], t[5]) && finite3(t[6], t[7], t[8]);
        }
    }
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 9; k++) t[k] = 0.f;
    }
}

__device__ __forceinline__ float dot3(float x0, float x1, float x2, float y0, float y1, float y2) { return (x0 * y0 + x1 * y1) + x2 * y2; }

// |x| by the hardware's square root (v_sqrt_f32, within 1 ulp): the correctly rounded sqrtf costs 12 more instructions, three times per
// pair, a quarter of the pair loop, and buys nothing the sum can show.  A squared length below the normal
// range (|x| < 1e-19) may come out as 0: the query then sits on a corner, where the value is unspecified but finite.
__device__ __forceinline__ float len3(float x0, float x1, float x2) { return __builtin_amdgcn_sqrtf(dot3(x0, x1, x2, x0, x1, x2)); }

// omega of one pair (file header)
__device__ __forceinline__ float solid_angle(float p0, float p1, float p2, const float4 A, const float4 B, const float4 C) {
    const float a0 = A.x - p0, a1 = A.y - p1, a2 = A.z - p2;
    const float b0 = A.w - p0, b1 = B.x - p1, b2 = B.y - p2;
    const float c0 = B.z - p0, c1 = B.w - p1, c2 = C.x - p2;
    const float n0 = b1 * c2 - b2 * c1, n1 = b2 * c0 - b0 * c2, n2 = b0 * c1 - b1 * c0;
    const float det = dot3(a0, a1, a2, n0, n1, n2);
    const float la = len3(a0, a1, a2), lb = len3(b0, b1, b2), lc = len3(c0, c1, c2);
    const float ab = dot3(a0, a1, a2, b0, b1, b2), bc = dot3(b0, b1, b2, c0, c1, c2), ca = dot3(c0, c1, c2, a0, a1, a2);
    const float den = (((la * lb) * lc + ab * lc) + bc * la) + ca * lb;
    const float omega = 2.f * atan2f(det, den);
    return (det != 0.f && fabsf(det) < INFINITY) ? omega : 0.f;  // (a NaN det fails the second test)
}

// grid: nqb * S workgroups, workgroup g takes query block g / S and slice g % S.  DIRECT (S == 1): writes w; otherwise the slice sums.
template <bool DIRECT>
__global__ void __launch_bounds__(WN_THREADS)
wind_kernel(int N, int V, int F, int S, const float* __restrict__ pts, const float* __restrict__ verts, const int* __restrict__ faces,
            double* __restrict__ sums, float* __restrict__ w) {
    __shared__ float4 tile[WN_CHUNK * 3];  // nine floats per face in three float4 (three pad floats): 16-byte broadcast reads
    const unsigned qb = blockIdx.x / (unsigned)S, s = blockIdx.x % (unsigned)S;
    const long long i = (long long)qb * WN_THREADS + threadIdx.x;
    const bool act = i < N;
    float p0 = 0.f, p1 = 0.f, p2 = 0.f;
    if (act) {
        p0 = pts[3 * i];
        p1 = pts[3 * i + 1];
        p2 = pts[3 * i + 2];
    }
    const int nchunks = (F + WN_CHUNK - 1) / WN_CHUNK;  // (F < 2^31 - 255: checked by the launcher)
    const int first = (int)s * WN_SLICE_CHUNKS;
    const int last = min(first + WN_SLICE_CHUNKS, nchunks);
    double slice = 0.0;
    float t[9];
    load_face(V, F, verts, faces, (long long)first * WN_CHUNK + threadIdx.x, t);
    for (int ch = first; ch < last; ch++) {  // ends at the slice's last chunk: at most WN_SLICE_CHUNKS rounds
        tile[threadIdx.x * 3] = make_float4(t[0], t[1], t[2], t[3]);
        tile[threadIdx.x * 3 + 1] = make_float4(t[4], t[5], t[6], t[7]);
        tile[threadIdx.x * 3 + 2] = make_float4(t[8], 0.f, 0.f, 0.f);
        __syncthreads();
        if (ch + 1 < last) load_face(V, F, verts, faces, (long long)(ch + 1) * WN_CHUNK + threadIdx.x, t);  // in flight during the pair loop
        const int m = min(WN_CHUNK, F - ch * WN_CHUNK);
        float sum = 0.f;
#pragma unroll 4
        for (int k = 0; k < m; k++)  // ends at the chunk's last face: at most WN_CHUNK rounds
            sum += solid_angle(p0, p1, p2, tile[3 * k], tile[3 * k + 1], tile[3 * k + 2]);
        slice += (double)sum;
        __syncthreads();
    }
    if (!act) return;
    if (!finite3(p0, p1, p2)) slice = (double)NAN;
    if (DIRECT)
        w[i] = (float)(slice / WN_FOUR_PI);  // (0.0 + slice == slice: what the second launch would give)
    else
        sums[(long long)s * N + i] = slice;
}

__global__ void __launch_bounds__(WN_THREADS) wind_total_kernel(int N, int S, const double* __restrict__ sums, float* __restrict__ w) {
    const long long i = (long long)blockIdx.x * WN_THREADS + threadIdx.x;
    if (i >= N) return;
    double total = 0.0;
    for (int s = 0; s < S; s++) total += sums[(long long)s * N + i];  // ends at the last slice
    w[i] = (float)(total / WN_FOUR_PI);
}

// V = 0 or F = 0: no face, w = 0 (NaN for a query with a non-finite coordinate)
__global__ void __launch_bounds__(WN_THREADS) wind_none_kernel(int N, const float* __restrict__ pts, float* __restrict__ w) {
    const long long i = (long long)blockIdx.x * WN_THREADS + threadIdx.x;
    if (i >= N) return;
    w[i] = finite3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]) ? 0.f : NAN;
}

}  // namespace

extern "C" {

size_t dgm_wind_scratch_bytes(int N, int F) {
    if (N < 0 || F < 0) return 0;
    return (size_t)N * (size_t)slices_of(F) * sizeof(double);
}

int dgm_wind_number(int N, int V, int F, const float* points, const float* verts, const int* faces, char* scratch, float* w, void* stream) {
    if (N < 0 || V < 0 || F < 0) return fail("wind_number: need N >= 0, V >= 0 and F >= 0");
    if (F > 0x7fffffff - WN_CHUNK) return fail("wind_number: too many faces");
    if (N == 0) return 0;  // (before any HIP call)
    if (!points || !w || (F > 0 && !faces) || (F > 0 && V > 0 && !verts)) return fail("wind_number: NULL pointer");
    const long long S = slices_of(F), nqb = ((long long)N + WN_THREADS - 1) / WN_THREADS;
    if (S > 1 && !scratch) return fail("wind_number: NULL scratch");
    if (S > 1 && ((uintptr_t)scratch & 7)) return fail("wind_number: scratch must be 8-byte aligned");
    if (nqb * (S > 0 ? S : 1) > 0x7fffffffLL) return fail("wind_number: N x slices over the supported grid, split N");
    hipStream_t st = (hipStream_t)stream;
    if (F == 0 || V == 0) {
        hipLaunchKernelGGL(wind_none_kernel, dim3((unsigned)nqb), dim3(WN_THREADS), 0, st, N, points, w);
        return launch_status();
    }
    if (S == 1) {
        hipLaunchKernelGGL(wind_kernel<true>, dim3((unsigned)nqb), dim3(WN_THREADS), 0, st, N, V, F, 1, points, verts, faces, (double*)nullptr, w);
        return launch_status();
    }
    double* sums = (double*)scratch;
    hipLaunchKernelGGL(wind_kernel<false>, dim3((unsigned)(nqb * S)), dim3(WN_THREADS), 0, st, N, V, F, (int)S, points, verts, faces, sums, w);
    hipLaunchKernelGGL(wind_total_kernel, dim3((unsigned)nqb), dim3(WN_THREADS), 0, st, N, (int)S, (const double*)sums, w);
    return launch_status();
}

}  // extern "C"
