// Approximate earth mover's distance of two point clouds for gfx950: the match cost of the mesh evaluation, entirely on the device.
//
// Replaces approxmatchkernel + matchcostkernel (R/metrics/pytorch_structural_losses/src/approxmatch.cu:3-182, 184-224, R/ = dgmesh/),
// which the evaluation (R/mesh_evaluation.py:90-93 through R/metrics/evaluation_metrics.py:18-24) runs, for its batch of one, as ONE
// workgroup of 512 threads over 8192 x 8192 pairs, three sweeps per level over nine levels, writing a 256 MB `match` matrix that a
// second kernel reads back once.  Here no n x m array exists: the cost sum(match * dist) is accumulated in the sweep that would have
// written `match`, and every sweep is spread over the chip.
//
// The iteration (per batch element; k = a point of xyz1, l = a point of xyz2, d2 = (dx*dx + dy*dy) + dz*dz, W = exp(level * d2)):
//   remainL[k] = multiL, remainR[l] = multiR, (multiL, multiR) = (1, n / m) if n >= m else (m / n, 1) -- INTEGER division, as
//   approxmatch.cu:6-12 has it; then for level = -4^7, -4^6, ..., -4^-1 (nine levels; the reference's level-0 branch is dead code):
//     1. ratioL[k] = remainL[k] / (1e-9 + sum_l W[k,l] remainR[l])
//     2. sumr[l]   = remainR[l] * sum_k W[k,l] ratioL[k];  ratioR[l] = min(remainR[l] / (sumr[l] + 1e-9), 1) * remainR[l];
//        remainR[l] = max(0, remainR[l] - sumr[l])
//     3. w[k,l] = (W[k,l] * ratioL[k]) * ratioR[l];  cost += sum w[k,l] * sqrt(d2[k,l]);  remainL[k] = max(0, remainL[k] - sum_l w[k,l])
//
// Launch structure.  The three steps depend on each other across the whole grid, so each is a launch of one sweep kernel -- "row sums
// of a kernel matrix against a vector": one row per lane (a workgroup = EMD_R rows), the other cloud staged through LDS in tiles of
// EMD_C points as float4 (x, y, z, weight), read back as wave-uniform ds_read_b128 broadcasts.  With one row per lane 8192 rows are
// only 128 waves, so the column range is split as well: grid = (row tiles, column parts, batch), the number of parts chosen so that
// the grid reaches EMD_TARGET_BLOCKS workgroups (four per CU) where the columns allow it -- a function of (rows, columns) alone, so a
// batch computes exactly what its elements compute alone.  Every (part, row) partial sum goes to scratch; a small finishing launch
// adds a row's partials in part order and applies the step's update.  1 + 9 * 6 + 1 launches per call.
// No atomics anywhere: fixed partition, fixed summation orders, so cost and residual are bit-reproducible.  Scratch is
// O(b (n + m) parts) floats, caller-owned; nothing is allocated and nothing is read back.
//
// Precision.  fp32 throughout the sweeps, no FMA contraction; exp is the fast one (v_exp_f32 on level * d2 * log2 e, as the reference's
// __expf) and the square root is v_sqrt_f32 (1 ulp).  A lane adds a tile's 256 terms in four interleaved chains and the tiles'
// totals after that, which bounds the summation error by (EMD_C / 4 + tiles) ulp instead of one ulp per column.  The partials of a row
// and the final sums over rows are added in fp64.
#include "dgm_common.hpp"

#include <math.h>

namespace dgm {

static constexpr int EMD_R = 256;               // rows per workgroup: one per lane
static constexpr int EMD_C = 256;               // columns per LDS tile
static constexpr int EMD_TARGET_BLOCKS = 1024;  // workgroups a sweep's grid aims for per batch element: 4 per CU on 256 CUs
static constexpr int EMD_LEVELS = 9;
static constexpr int EMD_MAX_POINTS = 1 << 28;  // per cloud: keeps every int tile / column index far from overflow

// column parts of a sweep with `rows` rows and `cols` columns, and the column tiles each part takes
static inline void emd_split(int rows, int cols, int* parts, int* tiles_per_part) {
    const int rt = (rows + EMD_R - 1) / EMD_R, ct = (cols + EMD_C - 1) / EMD_C;
    int want = (EMD_TARGET_BLOCKS + rt - 1) / rt;
    if (want > ct) want = ct;
    *tiles_per_part = (ct + want - 1) / want;
    *parts = (ct + *tiles_per_part - 1) / *tiles_per_part;
}

struct EmdPlan {
    int partsL, tppL;  // rows = xyz1 (steps 1 and 3)
    int partsR, tppR;  // rows = xyz2 (step 2)
    size_t remainL, ratioL, rowcost, remainR, ratioR, partial, partial_per_batch, floats;  // offsets and sizes in floats
};

static bool emd_plan(int b, int n, int m, EmdPlan* P) {
    if (b < 1 || b > 65535 || n < 1 || m < 1 || n > EMD_MAX_POINTS || m > EMD_MAX_POINTS) return false;
    emd_split(n, m, &P->partsL, &P->tppL);
    emd_split(m, n, &P->partsR, &P->tppR);
    size_t o = 0;
    auto take = [&](size_t count) {
        size_t at = o;
        o = align_up(o + count, 64);
        return at;
    };
    const size_t B = (size_t)b;
    P->remainL = take(B * n);
    P->ratioL = take(B * n);
    P->rowcost = take(B * n);
    P->remainR = take(B * m);
    P->ratioR = take(B * m);
    const size_t pl = 2 * (size_t)P->partsL * n, pr = (size_t)P->partsR * m;  // step 3 keeps two sums per (part, row)
    P->partial_per_batch = pl > pr ? pl : pr;
    P->partial = take(B * P->partial_per_batch);
    P->floats = o;
    return true;
}

__global__ void __launch_bounds__(256)
emd_init_kernel(int n, int m, float multiL, float multiR, float* __restrict__ remainL, float* __restrict__ remainR,
                float* __restrict__ rowcost) {
    const size_t bi = blockIdx.z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) remainL[bi * n + i] = multiL, rowcost[bi * n + i] = 0.f;
    if (i < m) remainR[bi * m + i] = multiR;
}

// partial (batch, MODE + 1, parts, rows).  MODE 0: sum over the part's columns of W * colv[col].  MODE 1 (step 3): with
// w = (W * rowv[row]) * colv[col], the sums of w and of w * sqrt(d2).
template <int MODE>
__global__ void __launch_bounds__(EMD_R)
emd_sweep_kernel(int rows, int cols, const float* __restrict__ rxyz, const float* __restrict__ cxyz, const float* __restrict__ colv,
                 const float* __restrict__ rowv, float level, int tiles_per_part, float* __restrict__ partial, size_t partial_per_batch) {
    __shared__ float4 tile[EMD_C];
    const size_t bi = blockIdx.z;
    const int part = blockIdx.y, parts = gridDim.y;
    const int row = blockIdx.x * EMD_R + threadIdx.x;
    const float* cx = cxyz + bi * cols * 3;
    const float* cv = colv + bi * cols;
    float x = 0.f, y = 0.f, z = 0.f, rl = 0.f;
    if (row < rows) {
        const float* r = rxyz + (bi * rows + row) * 3;
        x = r[0], y = r[1], z = r[2];
        if (MODE == 1) rl = rowv[bi * rows + row];
    }
    const int col_tiles = (cols + EMD_C - 1) / EMD_C;
    const int t0 = part * tiles_per_part, t1 = min(t0 + tiles_per_part, col_tiles);
    float acc = 0.f, accd = 0.f;
    for (int t = t0; t < t1; t++) {
        const int c = t * EMD_C + threadIdx.x;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);  // (a column past the end weighs 0: W is finite, so it adds exactly 0)
        if (c < cols) s = make_float4(cx[(size_t)c * 3], cx[(size_t)c * 3 + 1], cx[(size_t)c * 3 + 2], cv[c]);
        __syncthreads();  // the previous tile has been read by every wave
        tile[threadIdx.x] = s;
        __syncthreads();
        float a[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int i = 0; i < EMD_C; i += 4) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 p = tile[i + q];
                const float dx = p.x - x, dy = p.y - y, dz = p.z - z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                const float W = __expf(level * d2);
                if (MODE == 0) {
                    a[q] += W * p.w;
                } else {
                    const float w = (W * rl) * p.w;
                    a[q] += w;
                    d[q] += w * __builtin_amdgcn_sqrtf(d2);
                }
            }
        }
        acc += (a[0] + a[1]) + (a[2] + a[3]);
        if (MODE == 1) accd += (d[0] + d[1]) + (d[2] + d[3]);
    }
    if (row < rows) {
        float* o = partial + bi * partial_per_batch;
        o[(size_t)part * rows + row] = acc;
        if (MODE == 1) o[((size_t)parts + part) * rows + row] = accd;
    }
}

// One thread per row: the row's partials in part order (summed in fp64, rounded once), then the step's update.
//   step 1: ratio = remain / (1e-9 + s)                                                    (ratioL)
//   step 2: sumr = remain * s; ratio = min(remain / (sumr + 1e-9), 1) * remain; remain = max(0, remain - sumr)   (ratioR, remainR)
//   step 3: remain = max(0, remain - s); rowcost += the second sum                          (remainL)
__global__ void __launch_bounds__(256)
emd_finish_kernel(int step, int rows, int parts, const float* __restrict__ partial, size_t partial_per_batch, float* __restrict__ remain,
                  float* __restrict__ ratio, float* __restrict__ rowcost) {
    const size_t bi = blockIdx.z;
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const float* p = partial + bi * partial_per_batch;
    double s64 = 0.0, sd64 = 0.0;  // (up to 1024 parts: fp64 keeps their sum at one rounding)
    for (int q = 0; q < parts; q++) {
        s64 += (double)p[(size_t)q * rows + row];
        if (step == 3) sd64 += (double)p[((size_t)parts + q) * rows + row];
    }
    const float s = (float)s64, sd = (float)sd64;
    const size_t at = bi * rows + row;
    const float rem = remain[at];
    if (step == 1) {
        ratio[at] = rem / (1e-9f + s);
    } else if (step == 2) {
        const float sumr = rem * s;
        ratio[at] = fminf(rem / (sumr + 1e-9f), 1.0f) * rem;
        remain[at] = fmaxf(0.0f, rem - sumr);
    } else {
        remain[at] = fmaxf(0.0f, rem - s);
        rowcost[at] += sd;
    }
}

// One workgroup per batch element: cost = sum rowcost, residual = (sum remainL, sum remainR), fp64, in a fixed order.
__global__ void __launch_bounds__(256)
emd_reduce_kernel(int n, int m, const float* __restrict__ rowcost, const float* __restrict__ remainL, const float* __restrict__ remainR,
                  float* __restrict__ cost, float* __restrict__ residual) {
    __shared__ double red[4][3];
    const size_t bi = blockIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256) v[0] += (double)rowcost[bi * n + i], v[1] += (double)remainL[bi * n + i];
    for (int i = threadIdx.x; i < m; i += 256) v[2] += (double)remainR[bi * m + i];
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) v[q] += __shfl_xor(v[q], s, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < 3; q++) red[threadIdx.x >> 6][q] = v[q];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 3; q++) v[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
        cost[bi] = (float)v[0];
        if (residual) residual[bi * 2] = (float)v[1], residual[bi * 2 + 1] = (float)v[2];
    }
}


}  // namespace dgm

using namespace dgm;

extern "C" {

int dgm_emd_tile(int which) {
    return which == 0 ? EMD_R : which == 1 ? EMD_C : which == 2 ? EMD_TARGET_BLOCKS : which == 3 ? EMD_LEVELS : 0;
}

int dgm_emd_parts(int rows, int cols) {
    if (rows < 1 || cols < 1 || rows > EMD_MAX_POINTS || cols > EMD_MAX_POINTS) return 0;
    int parts, tpp;
    emd_split(rows, cols, &parts, &tpp);
    return parts;
}

size_t dgm_emd_scratch_floats(int b, int n, int m) {
    EmdPlan P;
    return emd_plan(b, n, m, &P) ? P.floats : 0;
}

int dgm_emd_approx(int b, int n, int m, const float* xyz1, const float* xyz2, float* scratch, float* cost, float* residual, void* stream) {
    EmdPlan P;
    if (!xyz1 || !xyz2 || !scratch || !cost || !emd_plan(b, n, m, &P)) {
        set_last_error("emd_approx: bad argument (1 <= b <= 65535, 1 <= n, m <= 2^28, no null pointer but residual)");
        return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    float *remainL = scratch + P.remainL, *ratioL = scratch + P.ratioL, *rowcost = scratch + P.rowcost;
    float *remainR = scratch + P.remainR, *ratioR = scratch + P.ratioR, *partial = scratch + P.partial;
    const float multiL = n >= m ? 1.f : (float)(m / n), multiR = n >= m ? (float)(n / m) : 1.f;
    const int big = n > m ? n : m;
    const dim3 rowsL((n + 255) / 256, 1, b), rowsR((m + 255) / 256, 1, b);
    const dim3 gridL((n + EMD_R - 1) / EMD_R, P.partsL, b), gridR((m + EMD_R - 1) / EMD_R, P.partsR, b);
    hipLaunchKernelGGL(emd_init_kernel, dim3((big + 255) / 256, 1, b), dim3(256), 0, st, n, m, multiL, multiR, remainL, remainR, rowcost);
    for (int j = 7; j > -2; j--) {
        const float level = -powf(4.0f, (float)j);
        hipLaunchKernelGGL(emd_sweep_kernel<0>, gridL, dim3(EMD_R), 0, st, n, m, xyz1, xyz2, (const float*)remainR, (const float*)nullptr,
                           level, P.tppL, partial, P.partial_per_batch);
        hipLaunchKernelGGL(emd_finish_kernel, rowsL, dim3(256), 0, st, 1, n, P.partsL, (const float*)partial, P.partial_per_batch, remainL,
                           ratioL, rowcost);
        hipLaunchKernelGGL(emd_sweep_kernel<0>, gridR, dim3(EMD_R), 0, st, m, n, xyz2, xyz1, (const float*)ratioL, (const float*)nullptr,
                           level, P.tppR, partial, P.partial_per_batch);
        hipLaunchKernelGGL(emd_finish_kernel, rowsR, dim3(256), 0, st, 2, m, P.partsR, (const float*)partial, P.partial_per_batch, remainR,
                           ratioR, rowcost);
        hipLaunchKernelGGL(emd_sweep_kernel<1>, gridL, dim3(EMD_R), 0, st, n, m, xyz1, xyz2, (const float*)ratioR, (const float*)ratioL,
                           level, P.tppL, partial, P.partial_per_batch);
        hipLaunchKernelGGL(emd_finish_kernel, rowsL, dim3(256), 0, st, 3, n, P.partsL, (const float*)partial, P.partial_per_batch, remainL,
                           ratioL, rowcost);
    }
    hipLaunchKernelGGL(emd_reduce_kernel, dim3(b), dim3(256), 0, st, n, m, (const float*)rowcost, (const float*)remainL,
                       (const float*)remainR, cost, residual);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_error(hipGetErrorString(e));
        return 1;
    }
    return 0;
}

}  // extern "C"
