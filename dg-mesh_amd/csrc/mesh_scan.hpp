// The exclusive scan of 32-bit counts that the mesh kernels' inverted indices and hash grids are built on (anchor.hip, surface.hip,
// mesh_simplify.hip "place", mesh_edges.hip; mesh_clean.hip uses the tile prefix inside its paired kernels): three phases over a fixed
// partition into tiles, so the offsets do not depend on how workgroups are scheduled.
//   scan_tile_totals_kernel   one workgroup per tile: the tile's sum, per component
//   dgm::launch_scan_blocks   one workgroup (binning.hip): the tiles' exclusive offsets, added in tile order; total = the sum
//   scan_tile_emit_kernel     one workgroup per tile: emit(i, value, the sum of the values before i) for every i < n
// C components (1, or 3 for anchor.hip's classification) are scanned side by side.  val(i, x) loads the C values of element i into
// x; emit(i, x, pre) receives them again with their exclusive prefixes.  Component c of tile t lives at [c * tiles + t].
// No workgroup waits for another; every loop names what ends it.  Included by one translation unit each: the kernels are local to it.
#pragma once
#include "dgm_common.hpp"

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_TILE = SCAN_THREADS * SCAN_ITEMS;  // integers per workgroup: the fixed partition
constexpr int SCAN_WAVES = SCAN_THREADS / 64;

inline int scan_tiles(long long n) { return (int)((n + SCAN_TILE - 1) / SCAN_TILE); }

// The SCAN_ITEMS values of this thread from `base` on (0 behind n), their exclusive prefix inside the tile and the tile's total.
template <int C, class Val>
__device__ __forceinline__ void scan_tile_prefix(long long n, Val val, long long base, unsigned (*x)[C], unsigned (*lds)[C], unsigned* pre,
                                                 unsigned* total) {
    unsigned s[C], inc[C];
#pragma unroll
    for (int c = 0; c < C; c++) s[c] = 0u;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {  // (ends: a constant count)
#pragma unroll
        for (int c = 0; c < C; c++) x[k][c] = 0u;
        if (base + k < n) val(base + k, x[k]);
#pragma unroll
        for (int c = 0; c < C; c++) s[c] += x[k][c];
    }
    const int wv = threadIdx.x >> 6;
    const bool last = dgm::lane_id() == 63;
#pragma unroll
    for (int c = 0; c < C; c++) {
        inc[c] = dgm::wave_inclusive_scan_u32(s[c]);
        if (last) lds[wv][c] = inc[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; c++) {
        unsigned before = 0u, all = 0u;
#pragma unroll
        for (int w = 0; w < SCAN_WAVES; w++) {
            const unsigned t = lds[w][c];
            if (w < wv) before += t;
            all += t;
        }
        pre[c] = before + inc[c] - s[c];
        total[c] = all;
    }
    __syncthreads();
}

template <int C, class Val>
__global__ void __launch_bounds__(SCAN_THREADS) scan_tile_totals_kernel(long long n, Val val, unsigned* __restrict__ tile_total) {
    __shared__ unsigned lds[SCAN_WAVES][C];
    unsigned x[SCAN_ITEMS][C], pre[C], total[C];
    scan_tile_prefix<C>(n, val, (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS, x, lds, pre, total);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < C; c++) tile_total[c * gridDim.x + blockIdx.x] = total[c];
    }
}

template <int C, class Val, class Emit>
__global__ void __launch_bounds__(SCAN_THREADS) scan_tile_emit_kernel(long long n, Val val, Emit emit, const unsigned* __restrict__ tile_off) {
    __shared__ unsigned lds[SCAN_WAVES][C];
    unsigned x[SCAN_ITEMS][C], pre[C], total[C];
    const long long base = (long long)blockIdx.x * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
    scan_tile_prefix<C>(n, val, base, x, lds, pre, total);
#pragma unroll
    for (int c = 0; c < C; c++) pre[c] += tile_off[c * gridDim.x + blockIdx.x];
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {  // (ends: a constant count, or at n)
        if (base + k >= n) break;
        emit(base + k, x[k], pre);
#pragma unroll
        for (int c = 0; c < C; c++) pre[c] += x[k][c];
    }
}

// scan<C>: the sums of val over [0, i) to emit for i < n (n >= 1), total[c] = the sum of all; tile_total and tile_off: C * scan_tiles(n)
// words each
template <int C, class Val, class Emit>
inline void scan_exclusive(hipStream_t st, long long n, Val val, Emit emit, unsigned* tile_total, unsigned* tile_off, unsigned* total) {
    const int nb = scan_tiles(n);
    hipLaunchKernelGGL((scan_tile_totals_kernel<C, Val>), dim3(nb), dim3(SCAN_THREADS), 0, st, n, val, tile_total);
    for (int c = 0; c < C; c++) dgm::launch_scan_blocks(st, nb, tile_total + c * nb, tile_off + c * nb, total + c);
    hipLaunchKernelGGL((scan_tile_emit_kernel<C, Val, Emit>), dim3(nb), dim3(SCAN_THREADS), 0, st, n, val, emit, (const unsigned*)tile_off);
}

// the plain case: u32 counts in, offset[i] = the sum before i; cursor[i] (where given) = the same offset, or 0 with `absolute` unset
struct ScanLoad {
    const unsigned* v;
    __device__ void operator()(long long i, unsigned* x) const { x[0] = v[i]; }
};
struct ScanStore {
    unsigned *offset, *cursor;
    bool absolute;
    __device__ void operator()(long long i, const unsigned*, const unsigned* pre) const {
        offset[i] = pre[0];
        if (cursor) cursor[i] = absolute ? pre[0] : 0u;
    }
};
inline void scan_exclusive(hipStream_t st, long long n, const unsigned* val, unsigned* tile_total, unsigned* tile_off, unsigned* offset,
                           unsigned* cursor, bool absolute, unsigned* total) {
    scan_exclusive<1>(st, n, ScanLoad{val}, ScanStore{offset, cursor, absolute}, tile_total, tile_off, total);
}

}  // namespace
