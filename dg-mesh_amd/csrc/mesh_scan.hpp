// The exclusive scan of 32-bit counts that the mesh kernels' inverted indices are built on (mesh_simplify.hip "place",
// mesh_edges.hip): three launches over a fixed partition into tiles, so the offsets do not depend on how workgroups are scheduled.
//   scan_totals_kernel    one workgroup per tile: the tile's sum
//   scan_offsets_kernel   one workgroup: the tiles' exclusive offsets, added in tile order; total[0] = the sum of everything
//   scan_apply_kernel     one workgroup per tile: offset[i] = the sum of val[0 .. i); cursor[i] = 0 where `cursor` is given
// No workgroup waits for another; every loop names what ends it.  Included by one translation unit each: the kernels are local to it.
#pragma once
#include "dgm_common.hpp"

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;  // integers per workgroup: the fixed partition
constexpr int SCAN_WAVES = SCAN_THREADS / 64;

inline int scan_tiles(long long n) { return (int)((n + SCAN_TILE - 1) / SCAN_TILE); }

__device__ __forceinline__ unsigned scan_tile_prefix(long long n, const unsigned* __restrict__ val, long long base, unsigned* x, unsigned* lds,
                                                     unsigned& total) {
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        x[k] = base + k < n ? val[base + k] : 0u;
        s += x[k];
    }
    const unsigned inc = dgm::wave_inclusive_scan_u32(s);
    const int wv = threadIdx.x >> 6;
    if (dgm::lane_id() == 63) lds[wv] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; w++) {
        const unsigned t = lds[w];
        if (w < wv) before += t;
        all += t;
    }
    __syncthreads();
    total = all;
    return before + inc - s;
}

__global__ void __launch_bounds__(SCAN_THREADS)
scan_totals_kernel(long long n, const unsigned* __restrict__ val, unsigned* __restrict__ tile_total) {
    __shared__ unsigned lds[SCAN_WAVES];
    unsigned x[SCAN_ITEMS], total;
    scan_tile_prefix(n, val, (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS, x, lds, total);
    if (threadIdx.x == 0) tile_total[blockIdx.x] = total;
}

// one workgroup: exclusive offsets of the tiles, added in tile order; total[0] = the sum
__global__ void __launch_bounds__(SCAN_THREADS)
scan_offsets_kernel(int nb, const unsigned* __restrict__ tile_total, unsigned* __restrict__ tile_off, unsigned* __restrict__ total) {
    __shared__ unsigned lds[SCAN_THREADS];
    __shared__ unsigned carry;
    if (threadIdx.x == 0) carry = 0;
    for (int base = 0; base < nb; base += SCAN_THREADS) {  // (ends: base grows by a constant)
        const int i = base + (int)threadIdx.x;
        lds[threadIdx.x] = i < nb ? tile_total[i] : 0u;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned run = carry;
            for (int t = 0; t < SCAN_THREADS; t++) {
                const unsigned v = lds[t];
                lds[t] = run;
                run += v;
            }
            carry = run;
        }
        __syncthreads();
        if (i < nb) tile_off[i] = lds[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = carry;
}

__global__ void __launch_bounds__(SCAN_THREADS)
scan_apply_kernel(long long n, const unsigned* __restrict__ val, const unsigned* __restrict__ tile_off, unsigned* __restrict__ offset,
                  unsigned* __restrict__ cursor) {
    __shared__ unsigned lds[SCAN_WAVES];
    unsigned x[SCAN_ITEMS], total;
    const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
    unsigned at = tile_off[blockIdx.x] + scan_tile_prefix(n, val, base, x, lds, total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        if (base + k >= n) break;
        offset[base + k] = at;
        if (cursor) cursor[base + k] = 0u;
        at += x[k];
    }
}

// offset[i] = the sum of val[0 .. i) for i < n (n >= 1), total[0] = the sum of all; tile_total and tile_off: scan_tiles(n) words each
inline void scan_exclusive(hipStream_t st, long long n, const unsigned* val, unsigned* tile_total, unsigned* tile_off, unsigned* offset,
                           unsigned* cursor, unsigned* total) {
    const int nb = scan_tiles(n);
    hipLaunchKernelGGL(scan_totals_kernel, dim3(nb), dim3(SCAN_THREADS), 0, st, n, val, tile_total);
    hipLaunchKernelGGL(scan_offsets_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, nb, (const unsigned*)tile_total, tile_off, total);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(SCAN_THREADS), 0, st, n, val, (const unsigned*)tile_off, offset, cursor);
}

}  // namespace
