// The hashed uniform grid of the bounded searches (anchor.hip over points, surface.hip over face boxes; DESIGN.md sections 4.6 and
// 4.14) and the 256-thread bounding-box reduction that sizes it (also mesh_ray.hip's centroid and chunk boxes).
// Cell coordinates are taken in fp64 from fp32 values and clamped to [-2, CELL_CLAMP]; cells hash into a power-of-two table.
// min and max are exact, so a box does not depend on the order of the reduction.  No workgroup waits for another.
// Included by one translation unit each: everything here is local to it.
#pragma once
#include <float.h>
#include <math.h>

#include "dgm_common.hpp"

namespace {

constexpr double CELL_LIMIT = 1048576.0;  // cells per axis at most (2^20)
constexpr int CELL_CLAMP = (1 << 20) + 3;
constexpr int BOX_THREADS = 256;

struct GridParams {
    double origin[3];
    double inv;  // 1 / cell edge
};

inline size_t pow2_at_least(size_t n) {
    size_t h = 64;
    while (h < n) h <<= 1;  // (ends: h doubles)
    return h;
}

__device__ __forceinline__ int cell_coord(float p, double o, double inv) {
#pragma clang fp contract(off)
    double u = floor(((double)p - o) * inv);
    if (!(u >= -2.0)) u = -2.0;  // (NaN included)
    if (u > (double)CELL_CLAMP) u = (double)CELL_CLAMP;
    return (int)u;
}

__device__ __forceinline__ unsigned cell_hash(int ix, int iy, int iz, unsigned mask) {
    return (((unsigned)ix * 73856093u) ^ ((unsigned)iy * 19349663u) ^ ((unsigned)iz * 83492791u)) & mask;
}

// The grid over the box [lo, hi] (lo > hi on an axis: nothing finite there, any origin will do): cell edge
// max(1.001 sqrt(max_d2), 1.001 edge, 2^-20 extent).  `edge` is the largest box edge of surface.hip's faces; anchor.hip passes 0,
// and the `cell < inf` guard then changes nothing for it: its max_d2 is finite on this path and so is the extent.
__device__ __forceinline__ GridParams grid_params(const float lo[3], const float hi[3], float max_d2, float edge) {
#pragma clang fp contract(off)
    GridParams g;
    double ext = 0.0;
    for (int a = 0; a < 3; a++) {
        const bool some = lo[a] <= hi[a];
        g.origin[a] = some ? (double)lo[a] : 0.0;
        if (some) ext = fmax(ext, (double)hi[a] - (double)lo[a]);
    }
    double cell = 1.001 * sqrt((double)max_d2);
    cell = fmax(cell, 1.001 * (double)edge);
    cell = fmax(cell, ext / CELL_LIMIT);
    g.inv = cell > 0.0 && cell < (double)INFINITY ? 1.0 / cell : 1.0;
    return g;
}

// ---- box reduction: rows 0-2 are minima, rows 3-5 maxima, a 7th row (surface.hip's largest edge) a maximum from 0 -------------------
template <int ROWS>
__device__ __forceinline__ void box_start(float* v) {
#pragma unroll
    for (int r = 0; r < ROWS; r++) v[r] = r < 3 ? FLT_MAX : (r < 6 ? -FLT_MAX : 0.f);
}

// (fminf / fmaxf drop NaN)
__device__ __forceinline__ float box_join(int r, float a, float b) { return r < 3 ? fminf(a, b) : fmaxf(a, b); }

// v: this thread's ROWS values; afterwards red[r][0] = row r over the workgroup's BOX_THREADS threads
template <int ROWS>
__device__ __forceinline__ void box_reduce(float (*red)[BOX_THREADS], const float* v) {
#pragma unroll
    for (int r = 0; r < ROWS; r++) red[r][threadIdx.x] = v[r];
    __syncthreads();
    for (int off = BOX_THREADS / 2; off >= 1; off >>= 1) {  // ends after log2(256) rounds
        if ((int)threadIdx.x < off) {
#pragma unroll
            for (int r = 0; r < ROWS; r++) red[r][threadIdx.x] = box_join(r, red[r][threadIdx.x], red[r][threadIdx.x + off]);
        }
        __syncthreads();
    }
}

// ... and written as this workgroup's partial box: ROWS floats
template <int ROWS>
__device__ __forceinline__ void box_reduce_partial(const float* v, float* __restrict__ partial) {
    __shared__ float red[ROWS][BOX_THREADS];
    box_reduce<ROWS>(red, v);
    if (threadIdx.x < ROWS) partial[blockIdx.x * ROWS + threadIdx.x] = red[threadIdx.x][0];
}

// row r over the partial boxes
template <int ROWS>
__device__ __forceinline__ float box_final_row(int nparts, const float* __restrict__ partial, int r) {
    float v = r < 3 ? FLT_MAX : (r < 6 ? -FLT_MAX : 0.f);
    for (int b = 0; b < nparts; b++) v = box_join(r, v, partial[b * ROWS + r]);  // ends at the last partial box
    return v;
}

// one workgroup of at least ROWS threads: the partial boxes -> the grid
template <int ROWS>
__global__ void grid_params_kernel(int nparts, const float* __restrict__ partial, float max_d2, GridParams* __restrict__ gp) {
    __shared__ float row[ROWS];
    if (threadIdx.x < ROWS) row[threadIdx.x] = box_final_row<ROWS>(nparts, partial, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) *gp = grid_params(row, row + 3, max_d2, ROWS > 6 ? row[ROWS - 1] : 0.f);
}

}  // namespace
