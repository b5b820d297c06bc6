// Deformation / appearance MLP trunk for gfx950.
//
// Replaces the nn.Linear + F.relu chain of DeformNetwork* / AppearanceNetwork (R/utils/time_utils.py:104-129,
// 178-204, 252-266, 310-323): positional encoding of x, 8 x 256 ReLU layers with the skip re-injection of
// [PE(x), t_emb] before layer 5, linear heads -- forward and backward (dX, dW, db, dt_emb) -- plus the single-row
// time branch timenet(PE(t)).
//
// Arithmetics of the 256-wide GEMMs, selected by dgm_mlp_set_gemm() / DGM_MLP_GEMM (the list and the default are further down,
// at g_gemm_mode):
//  * f16x3p (mlp_planes.hpp, default): power-of-two scaled two-way binary16 split, three partial products per fp32 product on the
//    f16 matrix cores, activations and gradients kept in HBM as their two planes;
//  * f32 (this file): v_mfma_f32_32x32x2_f32; 64 x 128 output tile per 256-thread workgroup, K consumed in 16-deep
//    register-staged global -> LDS stages (A k-major with row pitch 66 = 2 mod 8: conflict-free transposing stores and
//    fragment reads), dW as row-chunk x 128-column-slab partial tiles.
// (Rounds 1-4 also shipped "bf16x6" and "f16x3" -- the same split arithmetic on fp32 rows, re-split by every consumer; round 5
// retired them: the plane path now takes per-row time inputs and batches of any size itself.)
// Common to both:
//  * the skip layer reads its input as TWO K-segments ([emb | h4]) -- the concatenation is never materialised;
//  * bias + ReLU are the forward epilogue, which also saves the ReLU mask as bits; the backward-data epilogue applies
//    the mask of the layer BELOW, so each backward GEMM directly emits the next layer's pre-masked gradient;
//  * weight gradients reduce over the rows in fixed order (partials + ordered reduction: deterministic, no atomics);
//    bias gradients ride along as column sums of the same G tiles;
//  * t is the same for every row in training, so dL/dt_emb = db . W[:, t-columns] (no per-row GEMM); the general
//    per-row case has its own small kernel.
#include <stdlib.h>
#include <string.h>

#include <utility>

#include "dgm_host.hpp"
#include "mlp_planes.hpp"
#include "mlp_planes5.hpp"

namespace dgm {

static constexpr int MLP_W = 256;     // trunk width (the reference hard-codes W=256)
static constexpr int MLP_EMB = 96;    // padded width of [PE(x) | t_emb]: 63 + 30 (blender) or 63 + 21, zero padded
static constexpr int MLP_XE = 63;     // PE(x) width: 3 + 3*2*10
static constexpr int GM = 64, GK = 16, GAP = 66;  // GEMM tile rows, K stage, padded LDS row stride of A (= 2 mod 8)
static constexpr int DW_ROWS = 512;   // rows per dW chunk
static constexpr int DW_SLAB = 128;   // K columns per dW workgroup
static constexpr int HD_ROWS = 256;   // rows per head-gradient chunk

// ---- weight preparation -----------------------------------------------------------------------------------------
// Wt (forward B operand): [Kp x 256] with Wt[k][j] = W[j][src(k)], zero rows for padding.
//   layer 0: Kp = 96,  src(k) = k for k < emb_dim
//   skip   : Kp = 352, src(k) = k for k < emb_dim ; src(k) = k - 96 + emb_dim for k >= 96
//   others : Kp = 256, src(k) = k
// Wd (backward-data B operand): [256 x 256] with Wd[k][j] = W[k][hoff + j]   (hoff = emb_dim for the skip layer)
__global__ void mlp_prep_kernel(int in_features, int Kp, int emb_dim, int is_skip, const float* __restrict__ W,
                                float* __restrict__ Wt, float* __restrict__ Wd) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < Kp * MLP_W) {
        const int k = idx / MLP_W, j = idx % MLP_W;
        int src = -1;
        if (Kp == MLP_W) src = k;
        else if (k < MLP_EMB) src = k < emb_dim ? k : -1;
        else src = k - MLP_EMB + emb_dim;
        Wt[idx] = src >= 0 ? W[(size_t)j * in_features + src] : 0.f;
    }
    if (Wd != nullptr && idx < MLP_W * MLP_W) {
        const int k = idx / MLP_W, j = idx % MLP_W;
        Wd[idx] = W[(size_t)k * in_features + (is_skip ? emb_dim : 0) + j];
    }
}

// ---- positional encoding -------------------------------------------------------------------------------------------
// emb[r] = [x, sin(x 2^0), cos(x 2^0), ..., sin(x 2^9), cos(x 2^9) | t_emb[r] | 0...]   (time_utils.py:24-55)
// One wave per TWO rows: lanes 0..59 evaluate sin AND cos of one (row, frequency, axis) triple with a single argument
// reduction (sincosf; the kernel is VALU-bound -- 60 transcendentals per row); then the 64 lanes copy x, the time embedding and
// the zero padding of both rows (36 columns each).
__global__ void __launch_bounds__(256)
mlp_embed_kernel(int N, const float* __restrict__ x, const float* __restrict__ temb, int temb_stride, int T,
                 float* __restrict__ emb) {
    const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2, lane = threadIdx.x & 63;
    if (r0 >= N) return;
    if (lane < 60) {
        const int sub = lane / 30, p = lane - 30 * sub, r = r0 + sub;
        if (r < N) {
            const int q = p / 3, a = p - 3 * q;
            float sn, cs;
            sincosf(x[3 * r + a] * (float)(1 << q), &sn, &cs);
            float* e = emb + (size_t)r * MLP_EMB + 3 + 6 * q + a;
            e[0] = sn;
            e[3] = cs;
        }
    }
    constexpr int REST = 3 + (MLP_EMB - MLP_XE);  // x and everything behind the positional encoding
    for (int i = lane; i < 2 * REST; i += 64) {
        const int sub = i / REST, j = i - REST * sub, r = r0 + sub;
        if (r >= N) continue;
        float* e = emb + (size_t)r * MLP_EMB;
        if (j < 3) e[j] = x[3 * r + j];
        else {
            const int t = j - 3;
            e[MLP_XE + t] = t < T ? temb[(size_t)r * temb_stride + t] : 0.f;
        }
    }
}

// ---- the 256-wide GEMM: C[M x 256] = [A1 | A2][M x (K1+K2)] * Bt[(K1+K2) x 256] ------------------------------------
// EPI 0: C = relu(acc + bias), and the ReLU mask is saved as bits: mask[row][col / 32] bit (col % 32)
// EPI 1: C = acc where the saved mask bit of the layer below is set, else 0  (backward data: the product is
//        directly the gradient w.r.t. the pre-activation of the layer below)
// 64 x 128 output tile per 256-thread workgroup (blockIdx.y = column half; 4 waves side by side, each 64 x 32 =
// two MFMA tiles, 32 accumulator VGPRs).  Small tiles keep the 100k-row problem balanced over 256 CUs (3126 tiles)
// and the low register count lets 5 workgroups share a CU, which is what hides the global->LDS staging latency.
static constexpr int GN = 128;
template <int EPI>
__global__ void __launch_bounds__(256)
mlp_gemm_kernel(int M, const float* __restrict__ A1, int lda1, int K1, const float* __restrict__ A2, int lda2, int K2,
                const float* __restrict__ Bt, const float* __restrict__ bias, unsigned* __restrict__ mask,
                float* __restrict__ C) {
    __shared__ float As[2][GK * GAP];
    __shared__ __attribute__((aligned(16))) float Bs[2][GK * GN];
    const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
    const int m0 = blockIdx.x * GM, n0 = blockIdx.y * GN;
    const int nk = (K1 + K2) / GK;
    const int a_row = tid >> 2, a_c4 = tid & 3;  // A tile: 64 rows x 4 float4
    const int b_k0 = tid >> 5, b_j4 = tid & 31;  // B tile: rows b_k0 and b_k0 + 8, 32 float4 per row
    const bool a_ok = (m0 + a_row) < M;
    // register staging of the next K stage (plain scalars + macros: an array or a by-reference lambda capture here
    // is demoted to scratch memory by the compiler)
    float4 ra, rb0, rb1;
#define MLP_LOAD_STAGE(kt_)                                                                                          \
    {                                                                                                                \
        const int k_ = (kt_) * GK;                                                                                   \
        const float* src_ = (k_ < K1) ? (A1 + (size_t)(m0 + a_row) * lda1 + k_)                                      \
                                      : (A2 + (size_t)(m0 + a_row) * lda2 + (k_ - K1));                              \
        ra = a_ok ? *reinterpret_cast<const float4*>(src_ + a_c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);             \
        const float* bsrc_ = Bt + (size_t)(k_ + b_k0) * MLP_W + n0 + b_j4 * 4;                                       \
        rb0 = *reinterpret_cast<const float4*>(bsrc_);                                                               \
        rb1 = *reinterpret_cast<const float4*>(bsrc_ + 8 * MLP_W);                                                   \
    }
#define MLP_STORE_STAGE(buf_)                                                                                        \
    {                                                                                                                \
        float* a_ = As[buf_] + (a_c4 * 4) * GAP + a_row;                                                             \
        a_[0] = ra.x;                                                                                                \
        a_[GAP] = ra.y;                                                                                              \
        a_[2 * GAP] = ra.z;                                                                                          \
        a_[3 * GAP] = ra.w;                                                                                          \
        float* b_ = Bs[buf_] + b_k0 * GN + b_j4 * 4;                                                                 \
        *reinterpret_cast<float4*>(b_) = rb0;                                                                        \
        *reinterpret_cast<float4*>(b_ + 8 * GN) = rb1;                                                               \
    }
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; r++) acc0[r] = 0.f, acc1[r] = 0.f;

    MLP_LOAD_STAGE(0)
    MLP_STORE_STAGE(0)
    __syncthreads();
    const int a_off = lane & 31, b_off = wn * 32 + (lane & 31), kh = lane >> 5;
    for (int kt = 0; kt < nk; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < nk) MLP_LOAD_STAGE(kt + 1)
        const float* as = As[buf];
        const float* bs = Bs[buf];
#pragma unroll
        for (int kk = 0; kk < GK / 2; kk++) {
            const int k = 2 * kk + kh;
            const float a0 = as[k * GAP + a_off], a1 = as[k * GAP + a_off + 32];
            const float b0 = bs[k * GN + b_off];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc1, 0, 0, 0);
        }
        if (kt + 1 < nk) MLP_STORE_STAGE(buf ^ 1)
        __syncthreads();
    }
    // epilogue: D[row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)][col = lane&31]
    const int col = n0 + wn * 32 + (lane & 31);
    const int mword = (n0 >> 5) + wn;  // 32-column group of this wave
    const float bv = (EPI == 0) ? bias[col] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; mt++) {
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = m0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            float v = mt == 0 ? acc0[r] : acc1[r];
            if (EPI == 0) {
                v = fmaxf(v + bv, 0.f);
                const unsigned long long bal = __ballot(v > 0.f);  // low half: row, high half: row + 4
                if ((lane & 31) == 0 && row < M) mask[(size_t)row * 8 + mword] = (unsigned)(bal >> (kh * 32));
            } else {
                const unsigned bits = row < M ? mask[(size_t)row * 8 + mword] : 0u;
                v = ((bits >> (lane & 31)) & 1u) ? v : 0.f;
            }
            if (row < M) C[(size_t)row * MLP_W + col] = v;
        }
    }
}

#undef MLP_LOAD_STAGE
#undef MLP_STORE_STAGE

// ---- weight gradient: partial[chunk][k][j] = sum_{rows of chunk} X[row][k] * G[row][j] --------------------------------
__global__ void __launch_bounds__(512)
mlp_dw_kernel(int M, const float* __restrict__ X1, int ldx1, int K1, const float* __restrict__ X2, int ldx2, int K2,
              const float* __restrict__ G, float* __restrict__ partial, float* __restrict__ partial_db) {
    __shared__ __attribute__((aligned(16))) float Xs[2][GK * DW_SLAB];
    __shared__ __attribute__((aligned(16))) float Gs[2][GK * MLP_W];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 2, wn = wv & 3;
    const int Kp = K1 + K2;
    const int slab = blockIdx.x, chunk = blockIdx.y;
    const int r0 = chunk * DW_ROWS;
    const int nst = DW_ROWS / GK;
    const int x_r = tid >> 5, x_c4 = tid & 31;      // X tile: 16 rows x 32 float4
    const int g_r0 = tid >> 6, g_j4 = tid & 63;     // G tile: rows g_r0, g_r0 + 8
    const int xk = slab * DW_SLAB + x_c4 * 4;       // concatenated K index of this thread's float4
    float4 rx, rg0, rg1;
    auto load_stage = [&](int st) {
        const int row = r0 + st * GK;
        const int rr = row + x_r;
        rx = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rr < M && xk < Kp)
            rx = (xk < K1) ? *reinterpret_cast<const float4*>(X1 + (size_t)rr * ldx1 + xk)
                           : *reinterpret_cast<const float4*>(X2 + (size_t)rr * ldx2 + (xk - K1));
        const int ga = row + g_r0, gb = row + g_r0 + 8;
        rg0 = ga < M ? *reinterpret_cast<const float4*>(G + (size_t)ga * MLP_W + g_j4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        rg1 = gb < M ? *reinterpret_cast<const float4*>(G + (size_t)gb * MLP_W + g_j4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto store_stage = [&](int buf) {
        *reinterpret_cast<float4*>(Xs[buf] + x_r * DW_SLAB + x_c4 * 4) = rx;
        *reinterpret_cast<float4*>(Gs[buf] + g_r0 * MLP_W + g_j4 * 4) = rg0;
        *reinterpret_cast<float4*>(Gs[buf] + (g_r0 + 8) * MLP_W + g_j4 * 4) = rg1;
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
    float colsum = 0.f;  // bias gradient of column `tid` (slab 0, threads 0..255)
    const bool do_db = (slab == 0) && (tid < MLP_W) && partial_db != nullptr;

    load_stage(0);
    store_stage(0);
    __syncthreads();
    const int a_off = wm * 64 + (lane & 31), b_off = wn * 64 + (lane & 31), kh = lane >> 5;
    for (int st = 0; st < nst; st++) {
        const int buf = st & 1;
        if (st + 1 < nst) load_stage(st + 1);
        const float* xs = Xs[buf];
        const float* gs = Gs[buf];
#pragma unroll
        for (int kk = 0; kk < GK / 2; kk++) {
            const int k = 2 * kk + kh;  // row inside the stage = reduction index
            const float a0 = xs[k * DW_SLAB + a_off], a1 = xs[k * DW_SLAB + a_off + 32];
            const float b0 = gs[k * MLP_W + b_off], b1 = gs[k * MLP_W + b_off + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (do_db) {
#pragma unroll
            for (int r = 0; r < GK; r++) colsum += gs[r * MLP_W + tid];
        }
        if (st + 1 < nst) store_stage(buf ^ 1);
        __syncthreads();
    }
    float* out = partial + (size_t)chunk * Kp * MLP_W;
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
            const int col = wn * 64 + nt * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int k = slab * DW_SLAB + wm * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (k < Kp) out[(size_t)k * MLP_W + col] = acc[mt][nt][r];
            }
        }
    if (do_db) partial_db[(size_t)chunk * MLP_W + tid] = colsum;
}

// dW[j][dst(k)] = sum_chunks partial[c][k][j] (PyTorch (out, in) layout, padding rows dropped); db[j] likewise
__global__ void mlp_reduce_dw_kernel(int chunks, int db_chunks, int Kp, int in_features, int emb_dim,
                                     const float* __restrict__ partial, const float* __restrict__ partial_db,
                                     float* __restrict__ dW, float* __restrict__ db) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < Kp * MLP_W) {
        const int k = idx / MLP_W, j = idx % MLP_W;
        int dst;
        if (Kp == MLP_W) dst = k;
        else if (k < MLP_EMB) dst = k < emb_dim ? k : -1;
        else dst = k - MLP_EMB + emb_dim;
        if (dst >= 0) {
            // sixteen independent partial sums keep sixteen loads in flight (a single dependent chain of
            // `chunks` loads is latency bound); the order is still fixed
            float sp[16];
#pragma unroll
            for (int u = 0; u < 16; u++) sp[u] = 0.f;
            const float* src = partial + (size_t)k * MLP_W + j;
            const size_t cs = (size_t)Kp * MLP_W;
            int c = 0;
            for (; c + 16 <= chunks; c += 16) {
#pragma unroll
                for (int u = 0; u < 16; u++) sp[u] += src[(size_t)(c + u) * cs];
            }
            for (; c < chunks; c++) sp[0] += src[(size_t)c * cs];
#pragma unroll
            for (int u = 8; u >= 1; u >>= 1)
#pragma unroll
                for (int v = 0; v < u; v++) sp[v] += sp[v + u];
            const float s = sp[0];
            dW[(size_t)j * in_features + dst] = s;
        }
    }
    if (idx < MLP_W && db != nullptr) {
        float sp[8];
#pragma unroll
        for (int u = 0; u < 8; u++) sp[u] = 0.f;
        int c = 0;
        for (; c + 8 <= db_chunks; c += 8) {
#pragma unroll
            for (int u = 0; u < 8; u++) sp[u] += partial_db[(size_t)(c + u) * MLP_W + idx];
        }
        for (; c < db_chunks; c++) sp[0] += partial_db[(size_t)c * MLP_W + idx];
        db[idx] = ((sp[0] + sp[1]) + (sp[2] + sp[3])) + ((sp[4] + sp[5]) + (sp[6] + sp[7]));
    }
}

// The same reduction in ONE pass for the matrix-core paths (256 partial tiles of 256 KB per layer: the read is the cost).
// (ReduceDwJob and the body of one piece, reduce_dw_piece, live in mlp_planes.hpp: the grouped paired launches run pieces too)
struct ReduceDwBatch {
    int n_jobs;
    ReduceDwJob job[18];  // (nine per network: a grouped backward pass reduces two networks in one launch)
    // blockIdx.y >= n_jobs: the heads' partial sums (mlp_heads_bwd_kernel) ride along, see reduce_heads_body; one set per network
    struct Heads {
        int chunks, bchunks, nout;  // (bchunks: rows of partial_b -- the plane path leaves one per 32-row tile)
        const float* partial_W;
        const float* partial_b;
        float* dW;
        float* db;
    } heads[2];
};
__device__ __forceinline__ void reduce_heads_body(int bx, int o, int chunks, int bchunks, const float* __restrict__ partial_W,
                                                  const float* __restrict__ partial_b, float* __restrict__ dWh,
                                                  float* __restrict__ dbh);
// All eight layers of a network in ONE launch at the end of its backward pass (blockIdx.y = layer; every layer keeps its own
// partial tiles until then).  Workgroup = one piece of a job (reduce_dw_piece, mlp_planes.hpp).  With eight layers in the grid there
// are enough workgroups (>= 2048) to read in segments of 256+ bytes and still fill the chip, which a single layer's launch could not.
// A grouped pass hands the first pieces of its hidden layers' jobs to the paired launches (ReduceDwJob::first_block); this launch
// does the rest, in the same job order.
// (round 4, measured at N = 100 k: 86-88 us whatever the piece shape -- RDW_KT = 1, 2, 4, 8, i.e. segments of 1 KB .. 128 B --
// and whatever the distance between consecutive chunks' tiles -- 256 KB, or padded by 256 B / 4 KB / 8.25 KB against channel
// aliasing: 323 MB of L2 misses at 3.7 TB/s is what a read of tiles the previous launches just wrote gets here)
static inline int reduce_dw_blocks(int Kp) { return (Kp / RDW_KT) * (MLP_W / RDW_JT); }
__global__ void __launch_bounds__(256)
mlp_reduce_dw_all_kernel(const ReduceDwBatch rb) {
    __shared__ __attribute__((aligned(16))) float red[RDW_LDS_FLOATS];
    if ((int)blockIdx.y >= rb.n_jobs) {  // (workgroup-uniform branch)
        const ReduceDwBatch::Heads& h = rb.heads[(int)blockIdx.y - rb.n_jobs];
        if ((int)blockIdx.x < 8 * h.nout)
            reduce_heads_body(blockIdx.x & 7, blockIdx.x >> 3, h.chunks, h.bchunks, h.partial_W, h.partial_b, h.dW, h.db);
        return;
    }
    const ReduceDwJob& jb = rb.job[blockIdx.y];
    if ((int)blockIdx.x < jb.first_block || (int)blockIdx.x >= jb.nblocks) return;
    reduce_dw_piece<16>(jb, (int)blockIdx.x, (int)threadIdx.x, red);
}

// ---- small dense ops around the trunk ----------------------------------------------------------------------------------
// out[r][c] (+)= sum_j A[r][j] * B(j, c) + bias[c],  j < 256, c < NC <= 16, B(j,c) = Bp[j*sj + c*sc].
// Four lanes share a row (each covers 64 of the 256 inputs in 16-byte pieces), so a wave load instruction touches
// 16 rows x 64 contiguous bytes.
__global__ void __launch_bounds__(256)
mlp_rows_small_kernel(int N, int NC, const float* __restrict__ A, const float* __restrict__ Bp, int sj, int sc,
                      const float* __restrict__ bias, float* __restrict__ out, int ldo, int accumulate) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int r = gid >> 2, q = gid & 3;
    float acc[16];
#pragma unroll
    for (int c = 0; c < 16; c++) acc[c] = 0.f;
    if (r < N) {
        const float* a = A + (size_t)r * MLP_W;
        for (int i = 0; i < 16; i++) {
            const int j = (i * 4 + q) * 4;
            const float4 v = *reinterpret_cast<const float4*>(a + j);
#pragma unroll
            for (int c = 0; c < 16; c++) {
                if (c < NC) {
                    const float* b = Bp + (size_t)j * sj + (size_t)c * sc;
                    acc[c] += v.x * b[0] + v.y * b[sj] + v.z * b[2 * sj] + v.w * b[3 * sj];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 16; c++) {
        acc[c] += __shfl_xor(acc[c], 1, 64);
        acc[c] += __shfl_xor(acc[c], 2, 64);
    }
    if (r < N && q == 0) {
#pragma unroll
        for (int c = 0; c < 16; c++) {
            if (c < NC) {
                float v = acc[c] + (bias ? bias[c] : 0.f);
                if (accumulate) v += out[(size_t)r * ldo + c];
                out[(size_t)r * ldo + c] = v;
            }
        }
    }
}

// Everything the heads' backward needs from one pass over Y7 (fp32 FMA on the vector units: K = n_out <= 16 is too thin for
// the matrix cores, and the pass is HBM-bound either way -- read Y7, write G7):
//   G7[r][c]                = (sum_o dOut[r][o] * Wh[o][c]) * (Y7[r][c] > 0)        (gradient entering layer 7)
//   partial_W[chunk][o][c]  = sum_rows dOut[r][o] * Y7[r][c],   partial_b[chunk][o] = sum_rows dOut[r][o]
// A wave owns whole rows (lane l: columns 4 l .. 4 l + 3, one 16-byte load / store per row; lane o also loads dOut[r][o], which
// v_readlane turns into the wave-uniform multiplier), keeps its four columns of Wh and its 16 x 4 weight-gradient sums in
// registers, eight rows in flight; the four waves of the workgroup meet in LDS in a fixed order.
typedef float hf2 __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(256)
mlp_heads_bwd_kernel(int N, int NC, const float* __restrict__ dOut, const float* __restrict__ Wh,
                     const float* __restrict__ Y7, float* __restrict__ G7, float* __restrict__ partial_W,
                     float* __restrict__ partial_b) {
    __shared__ __attribute__((aligned(16))) float sW[16][MLP_W];
    __shared__ float sB[4][16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, chunk = blockIdx.x;
    const int r0 = chunk * HD_ROWS, r1 = min(N, r0 + HD_ROWS);
    hf2 wa[16], wb[16], aa[16], ab[16];
#pragma unroll
    for (int o = 0; o < 16; o++) {
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (o < NC) w = *reinterpret_cast<const float4*>(Wh + (size_t)o * MLP_W + lane * 4);
        wa[o] = (hf2){w.x, w.y}, wb[o] = (hf2){w.z, w.w};
        aa[o] = (hf2){0.f, 0.f}, ab[o] = (hf2){0.f, 0.f};
    }
    float accb = 0.f;
    for (int rb = r0 + wv * 8; rb < r1; rb += 32) {
        float4 y[8];
        float dv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int r = rb + u;
            y[u] = make_float4(0.f, 0.f, 0.f, 0.f), dv[u] = 0.f;
            if (r < r1) {
                y[u] = *reinterpret_cast<const float4*>(Y7 + (size_t)r * MLP_W + lane * 4);
                if (lane < NC) dv[u] = dOut[(size_t)r * NC + lane];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (rb + u < r1) {  // wave-uniform
                const hf2 ya = {y[u].x, y[u].y}, yb = {y[u].z, y[u].w};
                hf2 sa = {0.f, 0.f}, sb = {0.f, 0.f};
#pragma unroll
                for (int o = 0; o < 16; o++) {  // (columns o >= NC: dv and Wh are zero)
                    const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dv[u]), o));
                    sa += d * wa[o], sb += d * wb[o];
                    aa[o] += d * ya, ab[o] += d * yb;
                }
                float4 g;
                g.x = y[u].x > 0.f ? sa.x : 0.f;
                g.y = y[u].y > 0.f ? sa.y : 0.f;
                g.z = y[u].z > 0.f ? sb.x : 0.f;
                g.w = y[u].w > 0.f ? sb.y : 0.f;
                *reinterpret_cast<float4*>(G7 + (size_t)(rb + u) * MLP_W + lane * 4) = g;
                accb += dv[u];
            }
        }
    }
    if (lane < 16) sB[wv][lane] = accb;
    for (int w = 0; w < 4; w++) {  // fixed order: wave 0, 1, 2, 3
        if (wv == w) {
#pragma unroll
            for (int o = 0; o < 16; o++) {
                float4* p = reinterpret_cast<float4*>(&sW[o][lane * 4]);
                float4 v = make_float4(aa[o].x, aa[o].y, ab[o].x, ab[o].y);
                if (w > 0) {
                    const float4 q = *p;
                    v.x += q.x, v.y += q.y, v.z += q.z, v.w += q.w;
                }
                *p = v;
            }
        }
        __syncthreads();
    }
    const int c = threadIdx.x;
#pragma unroll
    for (int o = 0; o < 16; o++)
        if (o < NC) partial_W[((size_t)chunk * 16 + o) * MLP_W + c] = sW[o][c];
    if (c < 16) partial_b[(size_t)chunk * 16 + c] = ((sB[0][c] + sB[1][c]) + sB[2][c]) + sB[3][c];
}

// dWh[o][c] = sum_chunks partial_W[chunk][o][c], dbh[o] = sum_chunks partial_b[chunk][o].  Grid (8 column blocks, n_out):
// a workgroup owns 32 columns of one output row as 8 float4 positions x 32 chunk groups (a wave instruction reads 128 contiguous
// bytes of eight chunks), group sums meet in LDS in a fixed order; the first column block of each row also reduces its bias.
__device__ __forceinline__ void reduce_heads_body(int bx, int o, int chunks, int bchunks, const float* __restrict__ partial_W,
                                                  const float* __restrict__ partial_b, float* __restrict__ dWh,
                                                  float* __restrict__ dbh) {
    __shared__ float4 red[32][8];
    __shared__ float redb[256];
    const int tid = threadIdx.x, pos = tid & 7, grp = tid >> 3;
    const int c0 = bx * 32 + pos * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* src = partial_W + (size_t)o * MLP_W + c0;
    int k = grp;
    for (; k + 96 < chunks; k += 128) {  // four loads in flight
        const float4 v0 = *reinterpret_cast<const float4*>(src + (size_t)k * 16 * MLP_W);
        const float4 v1 = *reinterpret_cast<const float4*>(src + (size_t)(k + 32) * 16 * MLP_W);
        const float4 v2 = *reinterpret_cast<const float4*>(src + (size_t)(k + 64) * 16 * MLP_W);
        const float4 v3 = *reinterpret_cast<const float4*>(src + (size_t)(k + 96) * 16 * MLP_W);
        s.x += (v0.x + v1.x) + (v2.x + v3.x), s.y += (v0.y + v1.y) + (v2.y + v3.y);
        s.z += (v0.z + v1.z) + (v2.z + v3.z), s.w += (v0.w + v1.w) + (v2.w + v3.w);
    }
    for (; k < chunks; k += 32) {
        const float4 v = *reinterpret_cast<const float4*>(src + (size_t)k * 16 * MLP_W);
        s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
    }
    red[grp][pos] = s;
    float sb = 0.f;
    if (bx == 0)
        for (int c = tid; c < bchunks; c += 256) sb += partial_b[(size_t)c * 16 + o];
    redb[tid] = sb;
    __syncthreads();
    if (tid < 8) {
        float4 t = red[0][tid];
        for (int g = 1; g < 32; g++) t.x += red[g][tid].x, t.y += red[g][tid].y, t.z += red[g][tid].z, t.w += red[g][tid].w;
        *reinterpret_cast<float4*>(dWh + (size_t)o * MLP_W + bx * 32 + tid * 4) = t;
    }
    if (bx == 0 && tid == 8) {
        float t = 0.f;
        for (int i = 0; i < 256; i++) t += redb[i];
        dbh[o] = t;
    }
}
__global__ void __launch_bounds__(256)
mlp_reduce_heads_kernel(int chunks, int NC, const float* __restrict__ partial_W, const float* __restrict__ partial_b,
                        float* __restrict__ dWh, float* __restrict__ dbh) {
    reduce_heads_body(blockIdx.x, blockIdx.y, chunks, chunks, partial_W, partial_b, dWh, dbh);
    (void)NC;
}

// broadcast t: dtemb[c] = sum_j db0[j] W0[j][63+c] + db5[j] W5[j][63+c]   (one 256-thread block per column c)
__global__ void __launch_bounds__(256)
mlp_dtemb_bcast_kernel(int T, const float* __restrict__ db0, const float* __restrict__ W0, int in0,
                       const float* __restrict__ db5, const float* __restrict__ W5, int in5, float* __restrict__ dtemb) {
    __shared__ float red[4];
    const int c = blockIdx.x, j = threadIdx.x;
    float v = db0[j] * W0[(size_t)j * in0 + MLP_XE + c] + db5[j] * W5[(size_t)j * in5 + MLP_XE + c];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((j & 63) == 0) red[j >> 6] = v;
    __syncthreads();
    if (j == 0) dtemb[c] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- time branch for ONE row: t_emb = timenet(PE(t)) (R/utils/time_utils.py:52-55, 178-204 with is_blender) ------------
// t is identical for every Gaussian of a training iteration (R/train.py:158), so the branch is a 13 -> 256 -> 30
// network on a single row: one workgroup, instead of ~45 one-element PyTorch kernels forward and ~50 backward.
// save = [pe (2 n_freq + 1) | h (hidden)]
__global__ void __launch_bounds__(256)
mlp_timenet_fwd_kernel(const float* __restrict__ t, int n_freq, const float* __restrict__ W1, const float* __restrict__ b1,
                       int hidden, const float* __restrict__ W2, const float* __restrict__ b2, int n_out,
                       float* __restrict__ save, float* __restrict__ out) {
    __shared__ float pe[64];
    __shared__ float h[1024];
    const int n_pe = 2 * n_freq + 1;
    const int tid = threadIdx.x;
    if (tid < n_pe) {
        const float tv = t[0];
        float v = tv;
        if (tid > 0) {
            const int q = (tid - 1) >> 1;
            const float arg = tv * (float)(1 << q);  // freq_bands = 2^linspace(0, n_freq - 1, n_freq)
            v = ((tid - 1) & 1) ? cosf(arg) : sinf(arg);
        }
        pe[tid] = v;
        save[tid] = v;
    }
    __syncthreads();
    for (int j = tid; j < hidden; j += 256) {
        float a = b1[j];
        for (int i = 0; i < n_pe; i++) a += W1[j * n_pe + i] * pe[i];
        a = fmaxf(a, 0.f);
        h[j] = a;
        save[n_pe + j] = a;
    }
    __syncthreads();
    // eight lanes per output, 32 outputs per round (one round for the reference's 30): every thread streams its slice of the
    // row with all loads in flight, three shuffles finish the sum -- the kernel is pure latency, so rounds are what costs
    for (int o0 = 0; o0 < n_out; o0 += 32) {
        const int o = o0 + (tid >> 3), l8 = tid & 7;
        float a = 0.f;
        if (o < n_out) {
#pragma unroll 8
            for (int j = l8; j < hidden; j += 8) a += W2[o * hidden + j] * h[j];
        }
        a += __shfl_xor(a, 1, 64);
        a += __shfl_xor(a, 2, 64);
        a += __shfl_xor(a, 4, 64);
        if (l8 == 0 && o < n_out) out[o] = a + b2[o];
    }
}

__global__ void __launch_bounds__(256)
mlp_timenet_bwd_kernel(const float* __restrict__ d_out, int n_freq, const float* __restrict__ W2, int hidden, int n_out,
                       const float* __restrict__ save, float* __restrict__ dW1, float* __restrict__ db1,
                       float* __restrict__ dW2, float* __restrict__ db2) {
    __shared__ float dO[64];
    const int n_pe = 2 * n_freq + 1;
    const int tid = threadIdx.x;
    if (tid < n_out) {
        dO[tid] = d_out[tid];
        db2[tid] = d_out[tid];
    }
    __syncthreads();
    const float* pe = save;
    const float* h = save + n_pe;
    for (int j = tid; j < hidden; j += 256) {
        const float hj = h[j];
        float dh = 0.f;
        for (int o = 0; o < n_out; o++) {
            dh += dO[o] * W2[o * hidden + j];
            dW2[o * hidden + j] = dO[o] * hj;
        }
        dh = hj > 0.f ? dh : 0.f;
        db1[j] = dh;
        for (int i = 0; i < n_pe; i++) dW1[j * n_pe + i] = dh * pe[i];
    }
}

}  // namespace dgm

// =================================================================================================================
// C ABI
// =================================================================================================================
using namespace dgm;

namespace dgm {
void prof_begin(int stage, hipStream_t st, int passes = 1);
void prof_end(int stage, hipStream_t st);
}
namespace {
struct Ws {
    float *emb, *Y[8], *Wt[8], *Wd[8], *Ga, *Gb, *partial, *partial_db, *partial_h, *partial_hb;
    float *partial_l[8], *partial_db_l[8];  // per layer: the weight-gradient partial tiles wait for the pass's one reduction
    unsigned* mask[8];
    // plane path (mlp_planes.hpp): weight planes and their inverse scales (wsc_e: the embedding half of the skip layer), tile
    // exponents of the embedding / Y_l / dOut / the two gradient buffers, the lane-native fp32 half of the skip layer, the dOut
    // planes, per-matrix maxima, the heads' planes and inverse scales
    uint4 *Wt3[8], *Wd3[8];
    float *wsc_f[8], *wsc_d[8], *wsc_e;
    int *Eexp, *Yexp[8], *Dexp, *Gexp[2];
    float4* Cin;
    unsigned char* Dp;
    unsigned* matmax;
    uint4 *Wh4f, *Wh4b;
    float *wsc_hf, *wsc_hb;
    float *bias_s[8];           // round 6: biases times their layer's column scales (prep4c_block)
    unsigned* tickets;          // eight counters: the reduce role of the grouped paired launches (pair_reduce_role), cleared by every grouped pass
    float *beff[2], *temb_row;  // round 6: the call's time row, kept for the backward pass (beff: the folded biases of the first version, unused -- they are formed where the biases are pre-scaled)
    size_t bytes;
};
int num_cus() {
    static int cache[DGM_MAX_DEVICES] = {0};  // per device: one process may drive several GPUs
    const int slot = current_device_slot();
    if (cache[slot] == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            n <= 0)
            n = 256;
        cache[slot] = n;
    }
    return cache[slot];
}
// ---- environment switches of the MLP: all of them, read once when the library is loaded -------------------------------------------
//   DGM_MLP_GEMM=f16x3p|f16x3p8|f16x3p5|f32  initial arithmetic mode (3 | 4 | 5 | 1, see g_gemm_mode; dgm_mlp_set_gemm changes it)
//   DGM_MLP_REDUCE_IN_PAIR=<n>                 initial g_reduce_in_pair (dgm_mlp_set_reduce_in_pair changes it); default P4_REDUCE_IN_PAIR = 0
//   DGM_MLP_PAIR=<n>                           weight-gradient workgroups of a paired backward launch (bwd_plan), 0 = two separate launches;
//                                              default: a fixed share of the CUs, chosen by measurement at N = 100 k
//   DGM_P4_EXPS_LIMIT=<n>                      tiles per workgroup whose exponents the layer GEMM keeps in its LDS table (1 .. 512 = default: N <= 4 M
//                                              rows on 256 CUs; the rest are read from HBM as they come): lets a test reach the second path at an ordinary batch size
//   DGM_MLP_HEADS_FUSED=0                      the heads in a launch of their own instead of inside layer 7's (forward_folded; A/B runs)
//   DGM_P4_XCD_OFF                             (-DP4_XCD_REDUCE variant builds only) dgm_p4_probe's paired launch without the per-XCD pre-reduction
// Three finished A/B switches went with the branches only they reached; their results stay where the kept code is: DGM_MLP_EMBED_MERGED
// (forward_folded), DGM_P4_G7_MULT (backward_planes), DGM_MLP_PAIR_CHUNKED (bwd_plan).
#ifndef P4_REDUCE_IN_PAIR
#define P4_REDUCE_IN_PAIR 0
#endif
struct MlpEnv {
    int gemm_mode, reduce_in_pair, pair, exps_limit;
    bool heads_fused;
#ifdef P4_XCD_REDUCE
    bool xcd_off;
#endif
};
const MlpEnv g_env = [] {
    auto num = [](const char* name, int dflt) {
        const char* e = getenv(name);
        return e ? atoi(e) : dflt;
    };
    MlpEnv v;
    v.gemm_mode = 3;
    if (const char* e = getenv("DGM_MLP_GEMM")) {
        if (strcmp(e, "f32") == 0) v.gemm_mode = 1;
        else if (strcmp(e, "f16x3p8") == 0) v.gemm_mode = 4;
        else if (strcmp(e, "f16x3p5") == 0) v.gemm_mode = 5;
        else if (strcmp(e, "f16x3p") != 0)
            fprintf(stderr, "libdgmesh_hip: unknown DGM_MLP_GEMM=\"%s\" (f16x3p | f16x3p8 | f16x3p5 | f32): using f16x3p\n", e);
    }
    v.reduce_in_pair = num("DGM_MLP_REDUCE_IN_PAIR", P4_REDUCE_IN_PAIR);
    if (v.reduce_in_pair < 0) v.reduce_in_pair = 0;
    v.pair = num("DGM_MLP_PAIR", -1);
    v.exps_limit = num("DGM_P4_EXPS_LIMIT", 512);
    v.exps_limit = v.exps_limit < 1 ? 1 : (v.exps_limit > 512 ? 512 : v.exps_limit);
    v.heads_fused = num("DGM_MLP_HEADS_FUSED", 1) != 0;
#ifdef P4_XCD_REDUCE
    v.xcd_off = getenv("DGM_P4_XCD_OFF") != nullptr;
#endif
    return v;
}();
// 3: f16x3p (default; mlp_planes.hpp): power-of-two scaled operands split into 2 binary16, 3 partial products on the f16 matrix
//    cores, on plane-format activations -- split once by the producer, one exponent per 32-row tile.
// 4: the same arithmetic on round 3-5's kernel forms ("f16x3p8": eight waves x 32 columns per layer GEMM, the skip layer's
//    embedding half as an fp32 `Cin` stream written by layer 0) -- what mode 3 still runs for a time input PER ROW; kept
//    selectable as the A/B partner of round 6's forms (one wave per SIMD, K = 320 skip layer, time row folded into the biases).
// 5: mode 3 with EVERY 256-wide layer GEMM in the one-wave-per-SIMD form ("f16x3p5": mlp_gemm5_kernel<0, 0> forward, <0, 1> in
//    unpaired backward passes).  Measured slower than the eight-wave form (50.5 vs 48.9 us under the power probe, 54.5
//    vs 48.4 inside a network pass), so mode 3 uses that form for the K = 320 skip layer only; kept selectable for the record.
// 1: native fp32 MFMA (v_mfma_f32_32x32x2_f32).
// (0 = "bf16x6 for every GEMM" was retired in round 4, 2 = "f16x3" on fp32 rows in round 5: both are ignored by dgm_mlp_set_gemm.)
int g_gemm_mode = g_env.gemm_mode;
// Pieces per K = 256 reduction job that a grouped backward pass reduces inside the NEXT layer's paired launch (pair_reduce_role,
// mlp_planes.hpp) instead of in the final mlp_reduce_dw_all_kernel launch: 0 = none (the launches of before), values above a job's
// piece count mean all of it.  The gradients do not depend on it.
// Off by default: at the full cap the kernels of a step take 59 us less, but the bench's gain of 1.2-1.8 % is smaller
// than its run-to-run spread on one box (profiles/reduce_in_pair_bench_ab.json), and a gain that cannot be told from noise is not one.
int g_reduce_in_pair = g_env.reduce_in_pair;
// arithmetic the last forward pass on a workspace ran in: the backward pass must match (its scales and masks were produced by
// that forward pass).  A small host-side table keyed by the workspace pointer; an unknown workspace is not checked.
struct WsMode {
    const void* ws;
    int mode;
};
WsMode g_ws_mode[64] = {};
unsigned g_ws_next = 0;
void remember_ws_mode(const void* ws, int mode) {
    for (auto& e : g_ws_mode)
        if (e.ws == ws) {
            e.mode = mode;
            return;
        }
    g_ws_mode[g_ws_next++ % 64] = WsMode{ws, mode};
}
int recall_ws_mode(const void* ws) {
    for (auto& e : g_ws_mode)
        if (e.ws == ws) return e.mode;
    return -1;
}
// plane path: a weight-gradient chunk is a run of whole 32-row tiles, one chunk per CU (or fewer)
struct P4Plan {
    int ntiles, tiles_per_chunk, chunks;
};
P4Plan p4_plan(int N) {
    P4Plan d;
    d.ntiles = (N + 31) / 32;
    d.tiles_per_chunk = (d.ntiles + num_cus() - 1) / num_cus();
    if (d.tiles_per_chunk < 1) d.tiles_per_chunk = 1;
    d.chunks = (d.ntiles + d.tiles_per_chunk - 1) / d.tiles_per_chunk;
    return d;
}
Ws carve(char* base, int N) {
    Ws w;
    char* p = align_ptr(base);
    auto take = [&](size_t b) {
        char* at = p;
        p = align_ptr(p + b);
        return (float*)at;
    };
    const size_t n = ((size_t)N + 31) / 32 * 32;  // every per-row tensor is padded to whole 32-row tiles (plane path)
    const size_t ntiles = n / 32;
    const size_t chunks = ((size_t)N + DW_ROWS - 1) / DW_ROWS;   // fp32-MFMA path: 512-row chunks
    const P4Plan pp = p4_plan(N > 0 ? N : 1);                     // plane path: chunks of whole tiles, at most one per CU
    w.emb = take(n * MLP_EMB * 4);
    for (int l = 0; l < 8; l++) w.Y[l] = take(n * MLP_W * 4);
    for (int l = 0; l < 8; l++) w.mask[l] = (unsigned*)take(n * 8 * 4);
    for (int l = 0; l < 8; l++) w.Wt[l] = take((size_t)(MLP_EMB + MLP_W) * MLP_W * 4);
    for (int l = 0; l < 8; l++) w.Wd[l] = take((size_t)MLP_W * MLP_W * 4);
    w.Ga = take(n * MLP_W * 4);
    w.Gb = take(n * MLP_W * 4);
    for (int l = 0; l < 8; l++) {  // (geometry is fixed: layer 0 consumes the embedding, layer 5 embedding | trunk)
        const int Kp = l == 0 ? MLP_EMB : (l == 5 ? MLP_EMB + MLP_W : MLP_W);
        size_t rows = (size_t)pp.chunks * Kp, dbr = (size_t)pp.chunks * 8;  // (plane path: 8 bias-gradient rows per chunk)
        if (l == 5) {  // the fp32-MFMA path reduces layer by layer through this one: room for its widest layer
            if (chunks * (MLP_EMB + MLP_W) > rows) rows = chunks * (MLP_EMB + MLP_W);
            if (chunks > dbr) dbr = chunks;
        }
        w.partial_l[l] = take(rows * MLP_W * 4);
        w.partial_db_l[l] = take(dbr * MLP_W * 4);
    }
    w.partial = w.partial_l[5];
    w.partial_db = w.partial_db_l[5];
    for (int l = 0; l < 8; l++) w.Wt3[l] = (uint4*)take((size_t)(MLP_EMB + MLP_W) * MLP_W * 4);
    for (int l = 0; l < 8; l++) w.Wd3[l] = (uint4*)take((size_t)MLP_W * MLP_W * 4);
    for (int l = 0; l < 8; l++) w.wsc_f[l] = take(1024);  // (one inverse scale per output column in round 6's kernel forms, [0] = the matrix's otherwise)
    for (int l = 0; l < 8; l++) w.wsc_d[l] = take(1024);
    w.wsc_e = take(256);
    size_t hchunks = ((size_t)N + HD_ROWS - 1) / HD_ROWS;
    if ((size_t)pp.chunks > hchunks) hchunks = pp.chunks;
    w.partial_h = take(hchunks * 16 * MLP_W * 4);
    w.partial_hb = take((hchunks > ntiles ? hchunks : ntiles) * 16 * 4);
    w.Eexp = (int*)take(ntiles * 4);
    for (int l = 0; l < 8; l++) w.Yexp[l] = (int*)take(ntiles * 4);
    w.Dexp = (int*)take(ntiles * 4);
    w.Gexp[0] = (int*)take(ntiles * 4);
    w.Gexp[1] = (int*)take(ntiles * 4);
    w.Cin = (float4*)take(n * MLP_W * 4);
    w.Dp = (unsigned char*)take(n * 128);
    w.matmax = (unsigned*)take(P4_MAX_MATS * 8 * 4);
    w.Wh4f = (uint4*)take((size_t)MLP_W * 32 * 4);
    w.Wh4b = (uint4*)take((size_t)16 * MLP_W * 4);
    w.wsc_hf = take(1024);
    w.wsc_hb = take(1024);
    w.beff[0] = take(MLP_W * 4);
    w.beff[1] = take(MLP_W * 4);
    for (int l = 0; l < 8; l++) w.bias_s[l] = take(MLP_W * 4);
    w.temb_row = take(64 * 4);
    w.tickets = (unsigned*)take(8 * 4);
    w.bytes = (size_t)(p - base) + 256;
    return w;
}
int layer_in(const dgm_mlp_params* p, int l) {
    if (l == 0) return p->emb_dim;
    if (l == p->skip_layer) return p->emb_dim + MLP_W;
    return MLP_W;
}
int layer_kp(const dgm_mlp_params* p, int l) {
    if (l == 0) return MLP_EMB;
    if (l == p->skip_layer) return MLP_EMB + MLP_W;
    return MLP_W;
}
int check_params(const dgm_mlp_params* p) {
    if (!p) return fail("mlp: params is NULL");
    if (p->n_layers != 8 || p->width != MLP_W) return fail("mlp: only D=8, W=256 is supported (the reference's only configuration)");
    if (p->emb_dim != MLP_XE + p->t_dim || p->emb_dim > MLP_EMB) return fail("mlp: emb_dim must be 63 + t_dim <= 96");
    if (p->skip_layer != 5) return fail("mlp: skip re-injection must feed layer 5 (skips=[4])");
    if (p->n_out < 1 || p->n_out > 16) return fail("mlp: 1..16 head outputs supported");
    for (int l = 0; l < 8; l++)
        if (!p->W[l] || !p->b[l]) return fail("mlp: NULL weight pointer");
    if (!p->Wh || !p->bh) return fail("mlp: NULL head pointer");
    return 0;
}

// ---- plane path (mlp_planes.hpp) -----------------------------------------------------------------------------------------
// Every launch with dynamic LDS: above 48 KB the kernel's limit has to be raised first, once per kernel (= per instantiation of
// this template) and device.  Returns 0, or 1 with the reason in dgm_last_error().
template <auto Kernel, typename... Args>
int launch_lds(dim3 grid, dim3 block, int lds, hipStream_t st, const Args&... args) {
    static int raised[DGM_MAX_DEVICES] = {0};  // bytes the kernel's limit stands at on each device
    int& have = raised[current_device_slot()];
    if (lds > have) {
        if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
            return fail("mlp: cannot raise the dynamic LDS limit of a plane-path kernel");
        have = lds;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return 0;
}
typedef Gemm4Cfg<16, 1024, 512, 0, false, 8> CfgFwd;
typedef Gemm4Cfg<16, 1024, 512, 2, false, 8> CfgSkip;
typedef Gemm4Cfg<16, 1024, 512, 1, false, 8> CfgBwd;
typedef Gemm4Cfg<6, 384, 192, 0, true, 8> CfgL0;
typedef Gemm4Cfg<4, 256, 128, 0, false, 8, true> CfgL0F;   // layer 0 on the 64-column embedding
typedef Gemm4Cfg<16, 1024, 512, 0, false, 8, true> CfgFwdC;   // round 6's forms: one weight scale per output column
typedef Gemm4Cfg<16, 1024, 512, 1, false, 8, true> CfgBwdC;
typedef Gemm5Cfg<0, 0> Cfg5Fwd;
typedef Gemm5Cfg<0, 1> Cfg5Bwd;
typedef Gemm5Cfg<4, 0> Cfg5Skip;
typedef Gemm5Cfg<0, 2> Cfg5FwdH;
typedef Dw4Cfg<2, 8, 256, 128, 1024, 512> CfgDwE64;
typedef Dw4Cfg<8, 8, 1024, 512, 1024, 512> CfgDw;
typedef Dw4Cfg<3, 8, 384, 192, 1024, 512> CfgDwE;
typedef Dw4Cfg<8, 1, 1024, 512, 128, 64> CfgDwH;
#ifndef P4_PAIR_SHARE_NUM
#define P4_PAIR_SHARE_NUM 128  // share of the CUs on the weight gradient in a paired backward launch: NUM / DEN (measured at N = 100 k: 96 -> 1.50, 112 -> 1.43, 128 -> 1.41, 144 -> 1.43, off -> 1.56 ms per network pass)
#define P4_PAIR_SHARE_DEN 256
#endif
// the paired launches' dynamic LDS: either role's (the larger form's, for both forms)
constexpr int LDS_PAIR = CfgBwdC::LDS > CfgDw::LDS ? CfgBwdC::LDS : CfgDw::LDS;

Gemm4Args gemm4_args(int N, int nt) {
    Gemm4Args a;
    memset(&a, 0, sizeof(a));
    a.ntiles = nt, a.M = N, a.exps_limit = g_env.exps_limit;
    return a;
}
Dw4Args dw4_args(int nt, int tiles_per_chunk, const void* X, const int* Xexp, const void* G, const int* Gexp, float* partial,
                 size_t chunk_stride, float* partial_db) {
    Dw4Args d;
    memset(&d, 0, sizeof(d));
    d.ntiles = nt, d.tiles_per_chunk = tiles_per_chunk, d.X = (const unsigned char*)X, d.Xexp = Xexp, d.G = (const unsigned char*)G, d.Gexp = Gexp;
    d.partial = partial, d.chunk_stride = chunk_stride, d.partial_db = partial_db;
    return d;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// The weight-plane jobs both forms have: the forward operand of layer l (or a K slice of it), its backward-data operand, the heads'.
Prep3Job layer_fwd_job(const dgm_mlp_params* p, int l, int Kp, int hoff, uint4* Bp, float* inv_scale) {
    return Prep3Job{0, Kp, MLP_W, layer_in(p, l), p->emb_dim, hoff, MLP_W, MLP_W, p->W[l], Bp, inv_scale};
}
Prep3Job layer_bwd_job(const dgm_mlp_params* p, int l, const Ws& w) {
    return Prep3Job{1, MLP_W, MLP_W, layer_in(p, l), p->emb_dim, l == p->skip_layer ? p->emb_dim : 0, MLP_W, MLP_W, p->W[l], w.Wd3[l], w.wsc_d[l]};
}
Prep3Job heads_fwd_job(const dgm_mlp_params* p, const Ws& w) {  // B[k][o] = Wh[o][k]
    return Prep3Job{0, MLP_W, 32, MLP_W, p->emb_dim, 0, MLP_W, p->n_out, p->Wh, w.Wh4f, w.wsc_hf};
}
Prep3Job heads_bwd_job(const dgm_mlp_params* p, const Ws& w) {  // B[o][c] = Wh[o][c]
    return Prep3Job{1, 16, MLP_W, MLP_W, p->emb_dim, 0, p->n_out, MLP_W, p->Wh, w.Wh4b, w.wsc_hb};
}
// heads in a launch of their own: out = Y7 Wh^T + bh (one computing wave per workgroup; HBM-bound: one pass over Y7)
template <bool COLSC>
int launch_heads(const dgm_mlp_params* p, int N, int nt, int gx, const Ws& w, float* out, hipStream_t st) {
    Gemm4Args a = gemm4_args(N, nt);
    a.A = (const unsigned char*)w.Y[7], a.Aexp = w.Yexp[7], a.Bp = w.Wh4f, a.b_inv = w.wsc_hf, a.bias = p->bh;
    a.out = out, a.ldo = p->n_out, a.n_valid = p->n_out;
    return launch_lds<mlp_gemm4_kernel<16, 1024, 512, 3, false, 1, COLSC>>(gx, 512, Gemm4Cfg<16, 1024, 512, 3, false, 1, COLSC>::LDS, st, a);
}

// One time value per call (temb_stride == 0) on round 6's kernel forms: the embedding is 64 columns wide, the time row sits in the
// biases of layer 0 and the skip layer, the skip layer is one K = 320 GEMM (no `Cin`), the 256-wide layers run one wave per SIMD
// where that buys something (all5: everywhere, mode 5).
int forward_folded(const dgm_mlp_params* p, int N, const float* x, const float* temb, const Ws& w, float* out, hipStream_t st,
                   const bool all5, const float* xadd, const int xadd_stride) {
    const int nt = p4_plan(N).ntiles, gx = nt < num_cus() ? nt : num_cus(), sk = p->skip_layer;
    // every weight matrix as two binary16 planes, one power-of-two scale per OUTPUT COLUMN, biases pre-scaled (prep4c_block) ...
    Prep4cBatch pc;
    int nc = 0;
    pc.temb = temb, pc.temb_row = w.temb_row, pc.T = p->t_dim;
    for (int l = 0; l < 8; l++) {
        const int Kp = l == 0 ? 64 : (l == sk ? 320 : MLP_W);
        pc.job[nc++] = Prep4cJob{layer_fwd_job(p, l, Kp, 0, w.Wt3[l], w.wsc_f[l]), p->b[l], w.bias_s[l], (l == 0 || l == sk) ? 1 : 0};
        if (l >= 1) pc.job[nc++] = Prep4cJob{layer_bwd_job(p, l, w), nullptr, nullptr, 0};
    }
    pc.job[nc++] = Prep4cJob{heads_fwd_job(p, w), nullptr, nullptr, 0};
    pc.job[nc++] = Prep4cJob{heads_bwd_job(p, w), nullptr, nullptr, 0};
    // ... in ONE launch with the embedding planes (two launches: 13.1 + 10.2 us)
    const int n_prep = (MLP_W / P4C_COLS) * nc;
    hipLaunchKernelGGL(mlp_embed4c_kernel, dim3(n_prep + nt), dim3(256), 0, st, N, x, (unsigned char*)w.emb, w.Eexp, 64, pc, n_prep, xadd, xadd_stride);
    // layer 0: K = 64, eight waves (HBM-bound: 26 MB in, 102 MB of planes out)
    Gemm4Args a = gemm4_args(N, nt);
    a.A = (const unsigned char*)w.emb, a.Aexp = w.Eexp, a.Bp = w.Wt3[0], a.b_inv = w.wsc_f[0], a.bias = w.bias_s[0];
    a.mask_out = w.mask[0], a.C = (unsigned char*)w.Y[0], a.Cexp = w.Yexp[0];
    if (launch_lds<mlp_gemm4_kernel<4, 256, 128, 0, false, 8, true>>(gx, 512, CfgL0F::LDS, st, a)) return 1;
    // the heads inside layer 7's launch (mlp_gemm5_kernel<0, 2>) instead of a launch of their own that reads Y_7 again: 64 us against
    // 50 + 26, +0.95 % on the bench (308.8 / 309.4 / 309.3 against 306.0 / 306.1 / 306.5 it/s, interleaved on one box)
    const bool heads_fused = g_env.heads_fused;
    Gemm5Args b;
    memset(&b, 0, sizeof(b));
    b.ntiles = nt, b.M = N, b.exps_limit = a.exps_limit;
    for (int l = 1; l < 8; l++) {
        b.A = (const unsigned char*)w.Y[l - 1], b.Aexp = w.Yexp[l - 1], b.Bp = w.Wt3[l], b.b_inv = w.wsc_f[l], b.bias = w.bias_s[l];
        b.mask_out = w.mask[l], b.C = (unsigned char*)w.Y[l], b.Cexp = w.Yexp[l];
        if (l == sk) {  // K = 320: the embedding's four K steps, then the trunk's sixteen
            b.A2 = (const unsigned char*)w.emb, b.A2exp = w.Eexp;
            if (launch_lds<mlp_gemm5_kernel<4, 0>>(gx, 256, Cfg5Skip::LDS, st, b)) return 1;
            b.A2 = nullptr, b.A2exp = nullptr;
        } else if (l == 7 && heads_fused) {  // the last trunk layer with the heads riding along (one wave per SIMD: the form with the registers for it)
            b.hBp = w.Wh4f, b.h_inv = w.wsc_hf, b.h_bias = p->bh, b.h_out = out, b.h_nout = p->n_out;
            if (launch_lds<mlp_gemm5_kernel<0, 2>>(gx, 256, Cfg5FwdH::LDS, st, b)) return 1;
        } else {
            dgm::prof_begin(DGM_STAGE_MLP_LAYER_FWD, st);
            if (all5) {
                if (launch_lds<mlp_gemm5_kernel<0, 0>>(gx, 256, Cfg5Fwd::LDS, st, b)) return 1;
            } else {  // the eight-wave form (measured faster for K = 256)
                a.A = b.A, a.Aexp = b.Aexp, a.Bp = b.Bp, a.b_inv = b.b_inv, a.bias = b.bias, a.mask_out = b.mask_out, a.C = b.C, a.Cexp = b.Cexp;
                if (launch_lds<mlp_gemm4_kernel<16, 1024, 512, 0, false, 8, true>>(gx, 512, CfgFwdC::LDS, st, a)) return 1;
            }
            dgm::prof_end(DGM_STAGE_MLP_LAYER_FWD, st);
        }
    }
    if (!heads_fused && launch_heads<true>(p, N, nt, gx, w, out, st)) return 1;
    return launch_status();
}

// Rounds 3-5's kernel forms: a time input per row, and all of mode 4 ("f16x3p8").  The embedding is 96 columns wide, one power-of-two
// scale per weight matrix, the skip layer's embedding half is an fp32 `Cin` stream that layer 0's launch writes.
int forward_per_row(const dgm_mlp_params* p, int N, const float* x, const float* temb, int temb_stride, const Ws& w, float* out,
                    hipStream_t st, const float* xadd, const int xadd_stride) {
    const int nt = p4_plan(N).ntiles, gx = nt < num_cus() ? nt : num_cus(), sk = p->skip_layer;
    // embedding planes + the maxima of the nine weight tensors (W_0 .. W_7, Wh)
    AbsMaxBatch am;
    am.n_jobs = 9;
    for (int l = 0; l < 8; l++) am.job[l].W = p->W[l], am.job[l].n = MLP_W * layer_in(p, l);
    am.job[8].W = p->Wh, am.job[8].n = p->n_out * MLP_W;
    hipLaunchKernelGGL(mlp_embed4_kernel, dim3(nt + 8 * am.n_jobs), dim3(256), 0, st, N, nt, x, temb, temb_stride, p->t_dim,
                       (unsigned char*)w.emb, w.Eexp, am, w.matmax, MLP_EMB, xadd, xadd_stride);
    // every weight matrix as two binary16 planes, one power-of-two scale per matrix (`mat`: its maximum's slot)
    Prep4Batch pb;
    int nj = 0;
    for (int l = 0; l < 8; l++) {
        if (l == sk) {  // K = 352 = embedding half (rides along with layer 0) | trunk half
            pb.job[nj++] = Prep4Job{layer_fwd_job(p, l, MLP_EMB, 0, w.Wt3[l], w.wsc_e), l};
            pb.job[nj++] = Prep4Job{layer_fwd_job(p, l, MLP_W, p->emb_dim, w.Wt3[l] + (size_t)MLP_EMB * MLP_W / 4, w.wsc_f[l]), l};
        } else
            pb.job[nj++] = Prep4Job{layer_fwd_job(p, l, layer_kp(p, l), 0, w.Wt3[l], w.wsc_f[l]), l};
        if (l >= 1) pb.job[nj++] = Prep4Job{layer_bwd_job(p, l, w), l};
    }
    pb.job[nj++] = Prep4Job{heads_fwd_job(p, w), 8};
    pb.job[nj++] = Prep4Job{heads_bwd_job(p, w), 8};
    hipLaunchKernelGGL(mlp_prep4_kernel, dim3(8, nj), dim3(256), 0, st, pb, w.matmax);
    // layer 0 (K = 96) with the embedding half of the skip layer as second output
    Gemm4Args a = gemm4_args(N, nt);
    a.A = (const unsigned char*)w.emb, a.Aexp = w.Eexp, a.Bp = w.Wt3[0], a.b_inv = w.wsc_f[0], a.bias = p->b[0];
    a.mask_out = w.mask[0], a.C = (unsigned char*)w.Y[0], a.Cexp = w.Yexp[0];
    a.Bp2 = w.Wt3[sk], a.b_inv2 = w.wsc_e, a.bias2 = p->b[sk], a.out2 = w.Cin;
    if (launch_lds<mlp_gemm4_kernel<6, 384, 192, 0, true, 8>>(gx, 512, CfgL0::LDS, st, a)) return 1;
    a.Bp2 = nullptr, a.b_inv2 = nullptr, a.bias2 = nullptr, a.out2 = nullptr;
    for (int l = 1; l < 8; l++) {
        a.A = (const unsigned char*)w.Y[l - 1], a.Aexp = w.Yexp[l - 1], a.b_inv = w.wsc_f[l], a.bias = p->b[l];
        a.mask_out = w.mask[l], a.C = (unsigned char*)w.Y[l], a.Cexp = w.Yexp[l];
        if (l == sk) {
            a.Bp = w.Wt3[l] + (size_t)MLP_EMB * MLP_W / 4, a.cin = w.Cin;
            if (launch_lds<mlp_gemm4_kernel<16, 1024, 512, 2, false, 8>>(gx, 512, CfgSkip::LDS, st, a)) return 1;
            a.cin = nullptr;
        } else {
            a.Bp = w.Wt3[l];
            dgm::prof_begin(DGM_STAGE_MLP_LAYER_FWD, st);
            if (launch_lds<mlp_gemm4_kernel<16, 1024, 512, 0, false, 8>>(gx, 512, CfgFwd::LDS, st, a)) return 1;
            dgm::prof_end(DGM_STAGE_MLP_LAYER_FWD, st);
        }
    }
    if (launch_heads<false>(p, N, nt, gx, w, out, st)) return 1;
    return launch_status();
}

// ---- backward: the plan ----------------------------------------------------------------------------------------------------------
// The geometry of a backward pass, computed once per call.  The single-network pass (backward_planes) and the grouped pass
// (backward_planes_group) both take their row chunks, their partial tiles and their reduction jobs from it through layer_dw():
// the grouped gradients have the bits of two single passes because there is one statement of all that, not two.
struct BwdPlan {
    bool fold;                     // round 6's forms (forward_folded); else rounds 3-5's (forward_per_row)
    int EW;                        // rows of the embedding's block of the K = EW / EW + 256 weight gradients: 64, or 96 with the time columns
    int nt, gx;                    // 32-row tiles; workgroups of a launch over all CUs
    int tiles_per_chunk, chunks;   // stand-alone weight-gradient launches: a chunk is a run of whole tiles, one chunk per CU (or fewer)
    int n_dw;                      // paired launches (layers 7 .. 1): workgroups on the weight gradient = its row chunks; 0 = two launches
    int tpc_pair, chunks_pair;     // ... tiles per chunk, ceil(nt / n_dw), and the chunks that have a tile: the last few workgroups may get
                                   // none and write no partial tile -- the reduction must only read the ones that exist
    int pair_grid, chunked;        // ... workgroups in all; chunked: the GEMM role walks the weight-gradient role's row chunks
};
BwdPlan bwd_plan(int N, bool fold) {
    const P4Plan pl = p4_plan(N);
    BwdPlan b;
    b.fold = fold, b.EW = fold ? 64 : MLP_EMB;
    b.nt = pl.ntiles, b.gx = b.nt < num_cus() ? b.nt : num_cus();
    b.tiles_per_chunk = pl.tiles_per_chunk, b.chunks = pl.chunks;
    // backward data (G_l -> G_{l-1}) and the weight gradient of layer l both consume G_l and nothing of each other: ONE launch, the
    // first n_dw workgroups on the weight gradient, the rest on the layer GEMM (mlp_bwd_pair_kernel).  Small problems have nothing to
    // balance; DGM_MLP_PAIR=<n> overrides the share (0: two launches over all CUs).
    b.n_dw = 0;
    if (b.gx >= 64 && b.nt >= 4 * b.gx) {
        b.n_dw = g_env.pair >= 0 ? g_env.pair : (b.gx * P4_PAIR_SHARE_NUM) / P4_PAIR_SHARE_DEN;
        if (b.n_dw >= b.gx) b.n_dw = b.gx - 1;
        if (b.n_dw > b.chunks) b.n_dw = b.chunks;  // (the skip layer's partial buffer is carved for pl.chunks tiles of 352 rows)
    }
    b.tpc_pair = b.n_dw > 0 ? (b.nt + b.n_dw - 1) / b.n_dw : 0;
    b.chunks_pair = b.n_dw > 0 ? (b.nt + b.tpc_pair - 1) / b.tpc_pair : 0;
    b.pair_grid = b.n_dw + (b.gx - b.n_dw > 0 ? b.gx - b.n_dw : 1);
    // chunked needs as many GEMM workgroups as chunks, and ids w, n_dw + w on the same XCD: G_l's second read then hits that XCD's
    // L2, -97 MB of fabric traffic per launch at the same kernel time (profiles/r04_pmc_bwd_pair.json)
    b.chunked = (b.pair_grid - b.n_dw == b.n_dw && (b.n_dw % 8) == 0) ? 1 : 0;
    return b;
}
// workgroups per role and network of a grouped paired launch: half of the chunks, a multiple of 8; 0 = no grouping
int group_split(const BwdPlan& bp) {
    const int n_wg = (bp.n_dw / 2) & ~7;
    return (n_wg < 8 || 4 * n_wg > bp.gx) ? 0 : n_wg;
}
// The weight gradient of layer l of one network: the arguments of its launches, and its reduction job(s) queued into
// rb.job[slot], rb.job[slot + step] (the caller counts them into rb.n_jobs: a grouped pass interleaves its two networks, step = 2).
struct LayerDw {
    Dw4Args emb;       // layers 0 and skip: the embedding's rows (rows 0 .. EW - 1 of the K = EW / EW + 256 gradient) with the layer's bias
                       // gradient: always a stand-alone launch of bp.chunks chunks (own partial tiles; paired skip layer: own reduction job)
    Dw4Args trunk;     // layers >= 1: the trunk's rows -- the weight-gradient role of the paired launch, or a stand-alone launch
    int trunk_chunks;  // ... its chunks
    int n_jobs;
};
LayerDw layer_dw(const BwdPlan& bp, const dgm_mlp_params* p, const Ws& w, int l, const unsigned char* G, const int* Ge, float* const* dW,
                 float* const* db, ReduceDwBatch& rb, int slot, int step) {
    const int sk = p->skip_layer, EW = bp.EW;
    const bool paired = bp.n_dw > 0 && l >= 1, split = paired && l == sk;
    const int Kp = l == 0 ? EW : (l == sk ? EW + MLP_W : MLP_W);
    LayerDw g;
    memset(&g, 0, sizeof(g));
    g.trunk_chunks = paired ? bp.chunks_pair : bp.chunks;
    g.n_jobs = split ? 2 : 1;
    // partial tiles of the layer: [chunk][Kp][256]; paired skip layer: trunk rows [n_dw][256][256], then embedding rows [chunks][EW][256]
    float* part_emb = w.partial_l[l];
    float* part_trunk = w.partial_l[l] + (l == sk ? (size_t)EW * MLP_W : 0);
    size_t stride_emb = (size_t)Kp * MLP_W, stride_trunk = (size_t)Kp * MLP_W;
    if (split) {
        part_trunk = w.partial_l[l], stride_trunk = (size_t)MLP_W * MLP_W;
        part_emb = w.partial_l[l] + (size_t)bp.n_dw * MLP_W * MLP_W, stride_emb = (size_t)EW * MLP_W;
    }
    if (l == 0 || l == sk) g.emb = dw4_args(bp.nt, bp.tiles_per_chunk, w.emb, w.Eexp, G, Ge, part_emb, stride_emb, w.partial_db_l[l]);
    if (l >= 1)  // (the skip layer's bias gradient came with its embedding half)
        g.trunk = dw4_args(bp.nt, paired ? bp.tpc_pair : bp.tiles_per_chunk, w.Y[l - 1], w.Yexp[l - 1], G, Ge, part_trunk, stride_trunk,
                           l == sk ? nullptr : w.partial_db_l[l]);
    auto job = [&](int at, int chunks, int db_rows, int jKp, int dst_off, const float* partial, const float* partial_db, float* dbp) {
        ReduceDwJob& jb = rb.job[at];
        jb.chunks = chunks, jb.db_rows = db_rows, jb.Kp = jKp, jb.in_features = layer_in(p, l), jb.nblocks = reduce_dw_blocks(jKp);
        jb.first_block = 0, jb.emb_rows = EW, jb.k_valid = bp.fold ? MLP_XE : p->emb_dim, jb.emb_dim = p->emb_dim;
        jb.dst_off = dst_off, jb.partial = partial, jb.partial_db = partial_db, jb.dW = dW[l], jb.db = dbp;
    };
    if (split) {  // two reduction jobs: embedding rows (with the bias gradient), trunk rows
        job(slot, bp.chunks, 8 * bp.chunks, EW, 0, part_emb, w.partial_db_l[l], db[l]);
        job(slot + step, g.trunk_chunks, 0, MLP_W, p->emb_dim, part_trunk, nullptr, nullptr);
    } else
        job(slot, g.trunk_chunks, 8 * g.trunk_chunks, Kp, 0, w.partial_l[l], w.partial_db_l[l], db[l]);
    return g;
}
// The pass's ONE reduction launch: all queued jobs (blockIdx.y = job; every layer keeps its partial tiles until then) and the heads'
// partial sums of n_nets networks.
void set_heads(ReduceDwBatch::Heads& h, const BwdPlan& bp, const dgm_mlp_params* p, const Ws& w, float* dWh, float* dbh) {
    h.chunks = bp.chunks, h.bchunks = bp.nt, h.nout = p->n_out;
    h.partial_W = w.partial_h, h.partial_b = w.partial_hb, h.dW = dWh, h.db = dbh;
}
void launch_reduce_all(const ReduceDwBatch& rb, int n_nets, hipStream_t st) {
    int gx = 0;
    for (int i = 0; i < rb.n_jobs; i++) gx = rb.job[i].nblocks > gx ? rb.job[i].nblocks : gx;
    hipLaunchKernelGGL(mlp_reduce_dw_all_kernel, dim3(gx, rb.n_jobs + n_nets), dim3(256), 0, st, rb);
}

// ---- backward: one network ---------------------------------------------------------------------------------------------------------
// COLSC: the pass's form, chosen once per call -- round 6's (one weight scale per output column, the time row folded: forward_folded)
// or rounds 3-5's.  all5 (mode 5, COLSC only): the unpaired backward-data GEMMs in the one-wave-per-SIMD form.
template <bool COLSC>
int backward_planes(const dgm_mlp_params* p, int N, const float* dOut, int temb_stride, const Ws& w, float* const* dW, float* const* db,
                    float* dWh, float* dbh, float* dtemb, hipStream_t st, const bool all5, const float* x_in, float* dX) {
    const BwdPlan bp = bwd_plan(N, COLSC);
    const int nt = bp.nt, gx = bp.gx, sk = p->skip_layer;
    const bool per_row_t = temb_stride != 0 && dtemb != nullptr;
    if (per_row_t && dX) return fail("mlp_backward: position gradients need a broadcast time row");
    // dOut -> planes (zero columns / rows beyond n_out / N) + the heads' bias-gradient partial sums
    hipLaunchKernelGGL(mlp_dout4_kernel, dim3((nt + 3) / 4), dim3(256), 0, st, N, nt, p->n_out, dOut, w.Dp, w.Dexp, w.partial_hb);
    unsigned char *G = (unsigned char*)w.Ga, *Gn = (unsigned char*)w.Gb;
    int *Ge = w.Gexp[0], *Gne = w.Gexp[1];
    // G_7 = (dOut Wh) masked by layer 7's ReLU.  One K step per tile: nothing to hide the epilogue's barriers under, so two workgroups
    // per CU (104 VGPRs, 54 KB of LDS; one per CU: 306.3 / 308.2 it/s against 308.8 / 309.0)
    // (tried, round 6: the heads' weight gradient on a side stream beside this launch -- a read stream over Y_7 beside a write stream,
    // joined again in front of the reduction: 308.8 / 309.0 it/s against 311.7 / 311.8 in order)
    Gemm4Args a = gemm4_args(N, nt);
    a.A = w.Dp, a.Aexp = w.Dexp, a.Bp = w.Wh4b, a.b_inv = w.wsc_hb, a.mask_in = w.mask[7], a.C = G, a.Cexp = Ge;
    const int g7 = nt < 2 * num_cus() ? nt : 2 * num_cus();
    if (launch_lds<mlp_gemm4_kernel<1, 128, 64, 1, false, 8, COLSC>>(g7, 512, Gemm4Cfg<1, 128, 64, 1, false, 8, COLSC>::LDS, st, a)) return 1;
    // heads' weight gradient: dWh[o][c] = sum_r dOut[r][o] Y7[r][c]
    const Dw4Args dh = dw4_args(nt, bp.tiles_per_chunk, w.Y[7], w.Yexp[7], w.Dp, w.Dexp, w.partial_h, 0, nullptr);
    if (launch_lds<mlp_dw4_kernel<8, 1, 1024, 512, 128, 64>>(bp.chunks, 512, CfgDwH::LDS, st, dh)) return 1;
    ReduceDwBatch rb;
    memset(&rb, 0, sizeof(rb));
    // Layers 7 .. 1: the paired launch, or (n_dw = 0) backward data and weight gradient as two launches over all CUs.  The embedding's
    // rows of the skip layer's gradient stay a launch of their own over all CUs.
    for (int l = 7; l >= 0; l--) {
        if (l >= 1)  // backward data: G_{l-1} = (G_l W_l) masked, into the other buffer
            a.A = G, a.Aexp = Ge, a.Bp = w.Wd3[l], a.b_inv = w.wsc_d[l], a.mask_in = w.mask[l - 1], a.C = Gn, a.Cexp = Gne;
        if (dX && (l == sk || l == 0))  // gradient w.r.t. the positions: G_5 W_5[:, :63] into scratch (the forward's Cin, idle now), then + G_0 W_0[:, :63] and PE'
            hipLaunchKernelGGL(mlp_dx4_kernel, dim3(nt), dim3(256), 0, st, N, (const unsigned char*)G, (const int*)Ge, p->W[l],
                               layer_in(p, l), 0, MLP_XE, reinterpret_cast<float*>(w.Cin), l == 0 ? 1 : 0, x_in, dX, 0);
        if (per_row_t && (l == sk || l == 0))  // a time input per row: dL/dt_emb[r] = G_5[r] W_5[:, 63:63+T] + G_0[r] W_0[:, 63:63+T]
            hipLaunchKernelGGL(mlp_dx4_kernel, dim3(nt), dim3(256), 0, st, N, (const unsigned char*)G, (const int*)Ge, p->W[l],
                               layer_in(p, l), MLP_XE, p->t_dim, reinterpret_cast<float*>(w.Cin), l == 0 ? 2 : 0, (const float*)nullptr,
                               dtemb, p->t_dim);
        const LayerDw g = layer_dw(bp, p, w, l, G, Ge, dW, db, rb, rb.n_jobs, 1);
        rb.n_jobs += g.n_jobs;
        if (l == 0 || l == sk) {
            if constexpr (COLSC) {
                if (launch_lds<mlp_dw4_kernel<2, 8, 256, 128, 1024, 512>>(bp.chunks, 512, CfgDwE64::LDS, st, g.emb)) return 1;
            } else {
                if (launch_lds<mlp_dw4_kernel<3, 8, 384, 192, 1024, 512>>(bp.chunks, 512, CfgDwE::LDS, st, g.emb)) return 1;
            }
        }
        if (l == 0) break;
        if (bp.n_dw > 0) {
            dgm::prof_begin(DGM_STAGE_MLP_BWD_PAIR, st);
            if (launch_lds<mlp_bwd_pair_kernel<COLSC>>(bp.pair_grid, 512, LDS_PAIR, st, a, g.trunk, bp.n_dw, bp.chunked)) return 1;
            dgm::prof_end(DGM_STAGE_MLP_BWD_PAIR, st);
        } else {
            dgm::prof_begin(DGM_STAGE_MLP_LAYER_BWD, st);
            if (all5) {
                Gemm5Args b;
                memset(&b, 0, sizeof(b));
                b.ntiles = nt, b.M = N, b.exps_limit = a.exps_limit;
                b.A = a.A, b.Aexp = a.Aexp, b.Bp = a.Bp, b.b_inv = a.b_inv, b.mask_in = a.mask_in, b.C = a.C, b.Cexp = a.Cexp;
                if (launch_lds<mlp_gemm5_kernel<0, 1>>(gx, 256, Cfg5Bwd::LDS, st, b)) return 1;
            } else if (launch_lds<mlp_gemm4_kernel<16, 1024, 512, 1, false, 8, COLSC>>(gx, 512, Gemm4Cfg<16, 1024, 512, 1, false, 8, COLSC>::LDS, st, a))
                return 1;
            dgm::prof_end(DGM_STAGE_MLP_LAYER_BWD, st);
            dgm::prof_begin(DGM_STAGE_MLP_LAYER_DW, st);
            if (launch_lds<mlp_dw4_kernel<8, 8, 1024, 512, 1024, 512>>(g.trunk_chunks, 512, CfgDw::LDS, st, g.trunk)) return 1;
            dgm::prof_end(DGM_STAGE_MLP_LAYER_DW, st);
        }
        std::swap(G, Gn), std::swap(Ge, Gne);
    }
    // (tried: the previous layer's partial tiles summed by the GEMM workgroups of the next paired launch, before their weight
    // prologue: the launch grows by 9 us (87 -> 96), six launches, while this reduction only shrinks 87 -> 52 us: a net loss)
    // (tried, round 5: each layer's tiles summed by a launch of its own right behind the layer's paired launch, while they are still
    // in the 256 MB MALL -- nine launches of 23 us against this one of 89: a single layer's 256 workgroups do not fill the chip)
    // (tried, round 6: TWO launches, layers 7 .. 4 reduced right behind layer 4's paired launch -- 130-160 MB of partial tiles each, a
    // thousand workgroups each, so that the reads could hit the MALL: 304.3 / 304.1 it/s against 309.1 / 308.3 with the single launch,
    // interleaved on one box, scripts/gpu_r6_rsplit.sh; the split at layer 3 or 5: 305.0 / 303.6)
    // (tried, round 6: this launch and what follows it on a side stream -- a second entry point running the pass in two pieces, the
    // trainer joining the streams before it looks at a gradient -- so that the first network's reduction runs beside the rasterizer's
    // VALU-bound backward: 305.5 / 305.6 / 305.4 it/s against 309.8 / 309.0 / 309.6 on one stream, and every consumer of a gradient
    // becomes a place to race; an unsafe timing run with NO join at all, the second network's reduction under Adam and the next
    // forward pass, showed +2 % -- that overlap is not available to a correct step)
    // (tried: each layer's reduction on a side stream under the next layer's launch -- its small workgroups do fit beside a
    // resident pair workgroup -- 265 vs 274 it/s: slower, the pair kernel's HBM-bound half gets the competition)
    set_heads(rb.heads[0], bp, p, w, dWh, dbh);
    launch_reduce_all(rb, 1, st);
    if constexpr (COLSC) {  // the time columns of dW_0 / dW_skip: db (x) t_emb; and dL/dt_emb (one launch)
        FoldGradArgs f;
        f.dW[0] = dW[0], f.db[0] = db[0], f.W[0] = p->W[0], f.in_features[0] = layer_in(p, 0);
        f.dW[1] = dW[sk], f.db[1] = db[sk], f.W[1] = p->W[sk], f.in_features[1] = layer_in(p, sk);
        f.temb = w.temb_row, f.T = p->t_dim, f.dtemb = (dtemb != nullptr && !per_row_t) ? dtemb : nullptr;
        hipLaunchKernelGGL(mlp_fold_grad_kernel, dim3(f.dtemb != nullptr ? 3 : 2, p->t_dim), dim3(256), 0, st, f);
    } else if (dtemb != nullptr && !per_row_t)
        hipLaunchKernelGGL(mlp_dtemb_bcast_kernel, dim3(p->t_dim), dim3(256), 0, st, p->t_dim, db[0], p->W[0], layer_in(p, 0),
                           db[sk], p->W[sk], layer_in(p, sk), dtemb);
    return launch_status();
}

// ---- backward: two networks in shared launches (dgm_mlp_backward_group) -------------------------------------------------------------
// The folded f16x3p forms with the paired launches only (the caller falls back to two ordinary passes otherwise).  Layers 7 .. 0
// are walked once; every launch of backward_planes<true>() appears once and serves both networks (the group kernels of
// mlp_planes.hpp).  The row chunks of every weight gradient, their partial tiles and the reduction's jobs come from the same
// bwd_plan() / layer_dw(): the gradients are bit-identical to two ordinary passes.  What the grouping saves is launches (eleven per
// step), the layer GEMM's weight prologue per tile, and the tail of a launch whose tiles do not divide by its workgroups.
struct GroupNet {
    const dgm_mlp_params* p;
    const float* dOut;
    Ws w;
    float* const* dW;
    float* const* db;
    float *dWh, *dbh, *dtemb;
};
int backward_planes_group(const GroupNet* nets, int N, const BwdPlan& bp, const int n_wg, hipStream_t st) {
    const int nt = bp.nt, sk = 5;
    const int cpw = (bp.n_dw + n_wg - 1) / n_wg;  // weight-gradient chunks of a network that one workgroup runs
    {
        Dout4GroupArgs da;
        for (int i = 0; i < 2; i++)
            da.NC[i] = nets[i].p->n_out, da.dOut[i] = nets[i].dOut, da.Dp[i] = nets[i].w.Dp, da.Dexp[i] = nets[i].w.Dexp, da.partial_b[i] = nets[i].w.partial_hb;
        da.tickets = nets[0].w.tickets;
        hipLaunchKernelGGL(mlp_dout4_group_kernel, dim3((nt + 3) / 4, 2), dim3(256), 0, st, N, nt, da);
    }
    unsigned char *G[2], *Gn[2];
    int *Ge[2], *Gne[2];
    PairGroupArgs pg;
    memset(&pg, 0, sizeof(pg));
    Gemm4GroupArgs g7a;  // G_7 = (dOut Wh) masked by layer 7's ReLU: two workgroups per CU in all, as in backward_planes()
    Dw4GroupArgs dg;     // heads' weight gradient: dWh[o][c] = sum_r dOut[r][o] Y7[r][c]
    memset(&dg, 0, sizeof(dg));
    for (int i = 0; i < 2; i++) {
        const Ws& w = nets[i].w;
        G[i] = (unsigned char*)w.Ga, Gn[i] = (unsigned char*)w.Gb, Ge[i] = w.Gexp[0], Gne[i] = w.Gexp[1];
        pg.ga[i] = gemm4_args(N, nt);
        Gemm4Args& a = g7a.a[i];
        a = pg.ga[i];
        a.A = w.Dp, a.Aexp = w.Dexp, a.Bp = w.Wh4b, a.b_inv = w.wsc_hb, a.mask_in = w.mask[7], a.C = G[i], a.Cexp = Ge[i];
        dg.a[i] = dw4_args(nt, bp.tiles_per_chunk, w.Y[7], w.Yexp[7], w.Dp, w.Dexp, w.partial_h, 0, nullptr);
    }
    if (launch_lds<mlp_gemm4_group_kernel<1, 128, 64, 1, false, 8, true>>(dim3(bp.gx, 2), 512, Gemm4Cfg<1, 128, 64, 1, false, 8, true>::LDS, st, g7a)) return 1;
    if (launch_lds<mlp_dw4_group_kernel<8, 1, 1024, 512, 128, 64>>(dim3(bp.chunks, 2), 512, CfgDwH::LDS, st, dg)) return 1;
    ReduceDwBatch rb;
    memset(&rb, 0, sizeof(rb));
    // Reduce role of the paired launches (pair_reduce_role, mlp_planes.hpp): the launch of layer l reduces the first n_hidden pieces
    // of layer l + 1's K = 256 jobs, whose tiles the launch before it wrote.  Layer 7's launch has nothing to reduce yet, layer 1's
    // jobs have no launch behind them: six of the seven layers can be hidden.
    const int n_hidden = g_reduce_in_pair < reduce_dw_blocks(MLP_W) ? g_reduce_in_pair : reduce_dw_blocks(MLP_W);
    PairReduceArgs pr;
    memset(&pr, 0, sizeof(pr));
    int hidden_slot[2] = {0, 0};  // rb.job slots of the K = 256 jobs the previous paired launch's tiles belong to
    for (int l = 7; l >= 0; l--) {
        LayerDw g[2];  // jobs per layer: the embedding rows' A, B (layers 5 and 0) first, then the trunk rows' A, B
        for (int i = 0; i < 2; i++) g[i] = layer_dw(bp, nets[i].p, nets[i].w, l, G[i], Ge[i], nets[i].dW, nets[i].db, rb, rb.n_jobs + i, 2);
        rb.n_jobs += 2 * g[0].n_jobs;
        if (l == 0 || l == sk) {  // the embedding's rows of the gradient, with the layer's bias gradient (blockIdx.y = network)
            for (int i = 0; i < 2; i++) dg.a[i] = g[i].emb;
            if (launch_lds<mlp_dw4_group_kernel<2, 8, 256, 128, 1024, 512>>(dim3(bp.chunks, 2), 512, CfgDwE64::LDS, st, dg)) return 1;
        }
        if (l == 0) break;
        for (int i = 0; i < 2; i++) {  // backward data G_{l-1} = (G_l W_l) masked, into the other buffer; the trunk rows of dW_l
            const Ws& w = nets[i].w;
            Gemm4Args& a = pg.ga[i];
            a.A = G[i], a.Aexp = Ge[i], a.Bp = w.Wd3[l], a.b_inv = w.wsc_d[l], a.mask_in = w.mask[l - 1], a.C = Gn[i], a.Cexp = Gne[i];
            pg.da[i] = g[i].trunk;
        }
        // this launch's reduce role: the jobs the previous iteration queued (their tiles are complete); the final launch skips those pieces
        pr.n_hidden = (l < 7 && n_hidden > 0) ? n_hidden : 0;
        pr.ticket = nets[0].w.tickets + l;
        if (pr.n_hidden > 0)
            for (int i = 0; i < 2; i++) {
                ReduceDwJob& jb = rb.job[hidden_slot[i]];
                jb.first_block = pr.n_hidden;
                pr.job[i] = jb;
            }
        for (int i = 0; i < 2; i++) hidden_slot[i] = rb.n_jobs - 2 + i;
        dgm::prof_begin(DGM_STAGE_MLP_BWD_PAIR, st, 2);  // (counts as the two layer passes it carries)
        static_assert(LDS_PAIR >= 2 * RDW_LDS_FLOATS * 4 + 16, "the reduce role's two pieces and its ticket slot live in the launch's LDS");
        if (launch_lds<mlp_bwd_pair_group_kernel<true>>(4 * n_wg, 512, LDS_PAIR, st, pg, n_wg, cpw, bp.n_dw, pr)) return 1;
        dgm::prof_end(DGM_STAGE_MLP_BWD_PAIR, st);
        for (int i = 0; i < 2; i++) std::swap(G[i], Gn[i]), std::swap(Ge[i], Gne[i]);
    }
    // rb.n_jobs = 18: what two backward_planes() passes queue, job for job
    for (int i = 0; i < 2; i++) set_heads(rb.heads[i], bp, nets[i].p, nets[i].w, nets[i].dWh, nets[i].dbh);
    launch_reduce_all(rb, 2, st);
    {   // the time columns of dW_0 / dW_skip: db (x) t_emb; and dL/dt_emb
        FoldGradGroupArgs fg;
        int tmax = 0;
        bool any_dt = false;
        for (int i = 0; i < 2; i++) {
            const dgm_mlp_params* p = nets[i].p;
            FoldGradArgs& f = fg.f[i];
            f.dW[0] = nets[i].dW[0], f.db[0] = nets[i].db[0], f.W[0] = p->W[0], f.in_features[0] = layer_in(p, 0);
            f.dW[1] = nets[i].dW[sk], f.db[1] = nets[i].db[sk], f.W[1] = p->W[sk], f.in_features[1] = layer_in(p, sk);
            f.temb = nets[i].w.temb_row, f.T = p->t_dim, f.dtemb = nets[i].dtemb;
            if (p->t_dim > tmax) tmax = p->t_dim;
            any_dt = any_dt || f.dtemb != nullptr;
        }
        hipLaunchKernelGGL(mlp_fold_grad_group_kernel, dim3(any_dt ? 3 : 2, tmax, 2), dim3(256), 0, st, fg);
    }
    return launch_status();
}
}  // namespace

extern "C" {

int dgm_mlp_set_gemm(int mode) {
    const int prev = g_gemm_mode;
    if (mode == 1 || mode == 3 || mode == 4 || mode == 5) g_gemm_mode = mode;  // (0, "bf16x6 for every GEMM", and 2, "f16x3" on fp32 rows, are retired: ignored)
    return prev;
}

int dgm_mlp_set_reduce_in_pair(int pieces) {
    const int prev = g_reduce_in_pair;
    if (pieces >= 0) g_reduce_in_pair = pieces;
    return prev;
}

size_t dgm_mlp_workspace_bytes(int N) {
    Ws w = carve(nullptr, N > 0 ? N : 0);
    return w.bytes;
}

#ifdef P4_TIMING
int dgm_p4_timing(unsigned long long* out) {  // (variant builds only: phase timers of the layer GEMM, see mlp_planes.hpp)
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(dgm::g_p4_timing), sizeof(unsigned long long) * 256 * 8 * 16);
}
#endif

#ifdef P4_PROBE
// (variant builds only, tools/power_probe.py: ONE plane-path kernel in a loop on synthetic operands, for clock / power telemetry)
//   kind 0: forward layer GEMM (mlp_gemm4_kernel<16,1024,512,0>)   1: weight gradient alone (mlp_dw4_kernel<8,8>)
//   kind 2: the paired backward launch (mlp_bwd_pair_kernel, the production split)        3: backward-data GEMM alone
// zero != 0: all operands zero (same instruction stream, no data toggling).  The buffers are this probe's own.
namespace {
__global__ void p4_probe_fill_kernel(unsigned* __restrict__ p, size_t n, unsigned seed, int zero) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned x = (unsigned)i * 2654435761u + seed;
        x ^= x >> 15, x *= 0x2c1b3c6du, x ^= x >> 12;
        // two binary16 values of magnitude < 2: sign | exponent <= 15 | mantissa
        p[i] = zero ? 0u : (x & 0xbfffbfffu);
    }
}
}  // namespace
int dgm_p4_probe(int N, int kind, int iters, int zero, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const BwdPlan bp = bwd_plan(N, false);
    const int nt = bp.nt, gx = bp.gx;
    static unsigned char *A = nullptr, *C = nullptr, *G = nullptr;
    static int* ex = nullptr;
    static uint4* Bp = nullptr;
    static float *binv = nullptr, *bias = nullptr, *partial = nullptr, *pdb = nullptr;
    static unsigned* mask = nullptr;
    static int cap = 0;
    const size_t rows = (size_t)nt * 32;
    if (cap < nt) {
        if (hipMalloc((void**)&A, rows * 1024) != hipSuccess || hipMalloc((void**)&C, rows * 1024) != hipSuccess ||
            hipMalloc((void**)&G, rows * 1024) != hipSuccess || hipMalloc((void**)&ex, (size_t)nt * 4 * 4) != hipSuccess ||
            hipMalloc((void**)&Bp, 16 * 4 * 256 * 16) != hipSuccess || hipMalloc((void**)&binv, 1024) != hipSuccess ||
            hipMalloc((void**)&bias, 1024) != hipSuccess || hipMalloc((void**)&mask, (size_t)nt * 1024) != hipSuccess ||
            hipMalloc((void**)&partial, (size_t)256 * 256 * 256 * 4) != hipSuccess || hipMalloc((void**)&pdb, (size_t)256 * 8 * 256 * 4) != hipSuccess)
            return fail("p4_probe: hipMalloc failed");
        cap = nt;
    }
    hipLaunchKernelGGL(p4_probe_fill_kernel, dim3(1024), dim3(256), 0, st, (unsigned*)A, rows * 256, 1u, zero);
    hipLaunchKernelGGL(p4_probe_fill_kernel, dim3(1024), dim3(256), 0, st, (unsigned*)G, rows * 256, 2u, zero);
    hipLaunchKernelGGL(p4_probe_fill_kernel, dim3(64), dim3(256), 0, st, (unsigned*)Bp, (size_t)16 * 4 * 256 * 4, 3u, zero);
    hipLaunchKernelGGL(p4_probe_fill_kernel, dim3(256), dim3(256), 0, st, mask, (size_t)nt * 256, 4u, 0);
    (void)hipMemsetAsync(ex, 0, (size_t)nt * 4 * 4, st);
    (void)hipMemsetAsync(bias, 0, 1024, st);
    const float one = 1.0f / 65536.0f;
    {
        float ones[256];
        for (int i = 0; i < 256; i++) ones[i] = one;
        (void)hipMemcpyAsync(binv, ones, sizeof(ones), hipMemcpyHostToDevice, st);
        (void)hipStreamSynchronize(st);
    }
    Gemm4Args a;
    memset(&a, 0, sizeof(a));
    a.exps_limit = 512;
    a.ntiles = nt, a.M = N, a.A = kind == 0 ? A : G, a.Aexp = ex, a.Bp = Bp, a.b_inv = binv, a.bias = bias, a.mask_in = mask,
    a.mask_out = mask + (size_t)0, a.C = C, a.Cexp = ex + nt;
    const Dw4Args d = dw4_args(nt, bp.tiles_per_chunk, A, ex + 2 * nt, G, ex + 3 * nt, partial, (size_t)256 * 256, pdb);
    Gemm5Args a5;
    memset(&a5, 0, sizeof(a5));
    a5.exps_limit = 512, a5.ntiles = nt, a5.M = N, a5.A = (kind == 4) ? A : G, a5.Aexp = ex, a5.Bp = Bp, a5.b_inv = binv, a5.bias = bias;
    a5.mask_in = mask, a5.mask_out = mask, a5.C = C, a5.Cexp = ex + nt;
    for (int it = 0; it < iters; it++) {
        if (kind == 4) {  // round 6: the one-wave-per-SIMD forms
            if (launch_lds<mlp_gemm5_kernel<0, 0>>(gx, 256, Cfg5Fwd::LDS, st, a5)) return 1;
        } else if (kind == 5) {
            if (launch_lds<mlp_gemm5_kernel<0, 1>>(gx, 256, Cfg5Bwd::LDS, st, a5)) return 1;
        } else if (kind == 0) {
            if (launch_lds<mlp_gemm4_kernel<16, 1024, 512, 0, false, 8>>(gx, 512, CfgFwd::LDS, st, a)) return 1;
        } else if (kind == 3) {
            if (launch_lds<mlp_gemm4_kernel<16, 1024, 512, 1, false, 8>>(gx, 512, CfgBwd::LDS, st, a)) return 1;
        } else if (kind == 1) {
            if (launch_lds<mlp_dw4_kernel<8, 8, 1024, 512, 1024, 512>>(bp.chunks, 512, CfgDw::LDS, st, d)) return 1;
        } else {
            if (bp.n_dw <= 0) return fail("p4_probe: no pair split at this size");
            constexpr int LDS_PROBE = CfgBwd::LDS > CfgDw::LDS ? CfgBwd::LDS : CfgDw::LDS;
            Dw4Args dp = d;
            dp.tiles_per_chunk = bp.tpc_pair;
#ifdef P4_XCD_REDUCE
            {
                static unsigned* xs = nullptr;
                static float* xp = nullptr;
                static int gen = 0;
                if (!xs) {
                    if (hipMalloc((void**)&xs, 8 * 128) != hipSuccess || hipMalloc((void**)&xp, (size_t)8 * 65536 * 4) != hipSuccess) return fail("p4_probe: hipMalloc");
                    (void)hipMemsetAsync(xs, 0, 8 * 128, st);
                }
                dp.xsync = g_env.xcd_off ? nullptr : xs, dp.xpartial = xp, dp.xgen = gen++, dp.xchunks = bp.chunks_pair;
            }
#endif
            if (launch_lds<mlp_bwd_pair_kernel<false>>(bp.pair_grid, 512, LDS_PROBE, st, a, dp, bp.n_dw, bp.chunked)) return 1;
        }
    }
    return launch_status();
}
#endif

int dgm_mlp_describe_workspace(int N, size_t* offs, int capacity) {
    Ws w = carve(nullptr, N > 0 ? N : 0);
    const char* base = nullptr;
    const void* f[DGM_MLP_WS_FIELDS];
    int n = 0;
    f[n++] = w.emb;
    for (int l = 0; l < 8; l++) f[n++] = w.Y[l];
    for (int l = 0; l < 8; l++) f[n++] = w.mask[l];
    f[n++] = w.Ga, f[n++] = w.Gb;
    f[n++] = w.Eexp;
    for (int l = 0; l < 8; l++) f[n++] = w.Yexp[l];
    f[n++] = w.Dexp, f[n++] = w.Gexp[0], f[n++] = w.Gexp[1];
    f[n++] = w.Cin, f[n++] = w.Dp;
    for (int l = 0; l < 8; l++) f[n++] = w.partial_l[l];
    for (int l = 0; l < 8; l++) f[n++] = w.partial_db_l[l];
    for (int i = 0; i < n && i < capacity; i++) offs[i] = (size_t)((const char*)f[i] - base);
    return n;
}

int dgm_mlp_forward(const dgm_mlp_params* p, int N, const float* x, const float* temb, int temb_stride, char* workspace,
                    float* out, void* stream) {
    return dgm_mlp_forward_add(p, N, x, nullptr, 0, temb, temb_stride, workspace, out, stream);
}

int dgm_mlp_forward_add(const dgm_mlp_params* p, int N, const float* x, const float* x_add, int x_add_stride, const float* temb,
                        int temb_stride, char* workspace, float* out, void* stream) {
    if (check_params(p)) return 1;
    if (N <= 0) return 0;
    if (!x || !temb || !workspace || !out) return fail("mlp_forward: NULL pointer");
    if (x_add && (g_gemm_mode < 3 || x_add_stride < 3))
        return fail("mlp_forward_add: the addend exists in the plane arithmetic only (f16x3p), rows of at least 3 floats");
    hipStream_t st = (hipStream_t)stream;
    Ws w = carve(workspace, N);
    const int mode = g_gemm_mode;
    const bool fold = (mode == 3 || mode == 5) && temb_stride == 0;
    remember_ws_mode(workspace, mode + (fold ? 16 : 0));
    if (mode >= 3)
        return fold ? forward_folded(p, N, x, temb, w, out, st, mode == 5, x_add, x_add_stride)
                    : forward_per_row(p, N, x, temb, temb_stride, w, out, st, x_add, x_add_stride);
    // ---- native fp32 MFMA
    for (int l = 0; l < 8; l++) {
        const int Kp = layer_kp(p, l);
        const int n = (Kp > MLP_W ? Kp : MLP_W) * MLP_W;
        hipLaunchKernelGGL(mlp_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, st, layer_in(p, l), Kp, p->emb_dim,
                           l == p->skip_layer ? 1 : 0, p->W[l], w.Wt[l], l >= 1 ? w.Wd[l] : nullptr);
    }
    hipLaunchKernelGGL(mlp_embed_kernel, dim3((N + 7) / 8), dim3(256), 0, st, N, x, temb, temb_stride, p->t_dim, w.emb);
    const int grid = (N + GM - 1) / GM;
    for (int l = 0; l < 8; l++) {
        const float *A1, *A2 = nullptr;
        int lda1, K1, lda2 = 0, K2 = 0;
        if (l == 0) {
            A1 = w.emb, lda1 = MLP_EMB, K1 = MLP_EMB;
        } else if (l == p->skip_layer) {
            A1 = w.emb, lda1 = MLP_EMB, K1 = MLP_EMB, A2 = w.Y[l - 1], lda2 = MLP_W, K2 = MLP_W;
        } else {
            A1 = w.Y[l - 1], lda1 = MLP_W, K1 = MLP_W;
        }
        hipLaunchKernelGGL(mlp_gemm_kernel<0>, dim3(grid, MLP_W / GN), dim3(256), 0, st, N, A1, lda1, K1, A2, lda2, K2, w.Wt[l],
                           p->b[l], w.mask[l], w.Y[l]);
    }
    hipLaunchKernelGGL(mlp_rows_small_kernel, dim3((N * 4 + 255) / 256), dim3(256), 0, st, N, p->n_out, w.Y[7], p->Wh, 1,
                       MLP_W, p->bh, out, p->n_out, 0);
    return launch_status();
}

int dgm_mlp_backward(const dgm_mlp_params* p, int N, const float* dOut, int temb_stride, char* workspace, float* const* dW,
                     float* const* db, float* dWh, float* dbh, float* dtemb, void* stream) {
    return dgm_mlp_backward_dx(p, N, dOut, temb_stride, workspace, dW, db, dWh, dbh, dtemb, nullptr, nullptr, stream);
}

int dgm_mlp_backward_dx(const dgm_mlp_params* p, int N, const float* dOut, int temb_stride, char* workspace, float* const* dW,
                        float* const* db, float* dWh, float* dbh, float* dtemb, const float* x, float* dX, void* stream) {
    if (check_params(p)) return 1;
    if (N <= 0) return 0;
    if (!dOut || !workspace || !dW || !db || !dWh || !dbh) return fail("mlp_backward: NULL pointer");
    if ((x == nullptr) != (dX == nullptr)) return fail("mlp_backward: x and dX come together");
    const int mode = g_gemm_mode;
    if (dX && (mode < 3 || temb_stride != 0))
        return fail("mlp_backward: the gradient w.r.t. the positions exists in the plane arithmetic only (f16x3p, broadcast time row)");
    {
        const int fm = recall_ws_mode(workspace);
        if (fm >= 0 && (fm & 15) != mode)
            return fail("mlp_backward: the arithmetic mode changed since the forward pass on this workspace (dgm_mlp_set_gemm)");
        if (fm >= 0 && ((fm & 16) != 0) != ((mode == 3 || mode == 5) && temb_stride == 0))
            return fail("mlp_backward: temb_stride differs from the forward pass on this workspace");
    }
    hipStream_t st = (hipStream_t)stream;
    Ws w = carve(workspace, N);
    if (mode >= 3) {
        const bool fold = (mode == 3 || mode == 5) && temb_stride == 0;
        return fold ? backward_planes<true>(p, N, dOut, temb_stride, w, dW, db, dWh, dbh, dtemb, st, mode == 5, x, dX)
                    : backward_planes<false>(p, N, dOut, temb_stride, w, dW, db, dWh, dbh, dtemb, st, false, x, dX);
    }
    // ---- native fp32 MFMA
    const int chunks = (N + DW_ROWS - 1) / DW_ROWS;
    const int grid = (N + GM - 1) / GM;
    // heads: G7 (masked by layer 7's ReLU, read off Y7 itself) and the partial sums of dWh / dbh in one pass over Y7
    const int hchunks = (N + HD_ROWS - 1) / HD_ROWS;
    hipLaunchKernelGGL(mlp_heads_bwd_kernel, dim3(hchunks), dim3(256), 0, st, N, p->n_out, dOut, p->Wh, w.Y[7], w.Ga,
                       w.partial_h, w.partial_hb);
    hipLaunchKernelGGL(mlp_reduce_heads_kernel, dim3(8, p->n_out), dim3(256), 0, st, hchunks, p->n_out, w.partial_h,
                       w.partial_hb, dWh, dbh);
    float* G = w.Ga;
    float* Gn = w.Gb;
    const bool per_row_t = temb_stride != 0 && dtemb != nullptr;
    for (int l = 7; l >= 0; l--) {
        const float *X1, *X2 = nullptr;
        int ldx1, K1, ldx2 = 0, K2 = 0;
        if (l == 0) {
            X1 = w.emb, ldx1 = MLP_EMB, K1 = MLP_EMB;
        } else if (l == p->skip_layer) {
            X1 = w.emb, ldx1 = MLP_EMB, K1 = MLP_EMB, X2 = w.Y[l - 1], ldx2 = MLP_W, K2 = MLP_W;
        } else {
            X1 = w.Y[l - 1], ldx1 = MLP_W, K1 = MLP_W;
        }
        // backward data first: G_{l-1} = (G_l W_l) masked, into the other buffer
        if (l >= 1)
            hipLaunchKernelGGL(mlp_gemm_kernel<1>, dim3(grid, MLP_W / GN), dim3(256), 0, st, N, G, MLP_W, MLP_W,
                               (const float*)nullptr, 0, 0, w.Wd[l], (const float*)nullptr, w.mask[l - 1], Gn);
        const int Kp = K1 + K2;
        const int slabs = (Kp + DW_SLAB - 1) / DW_SLAB;
        hipLaunchKernelGGL(mlp_dw_kernel, dim3(slabs, chunks), dim3(512), 0, st, N, X1, ldx1, K1, X2, ldx2, K2, G, w.partial,
                           w.partial_db);
        hipLaunchKernelGGL(mlp_reduce_dw_kernel, dim3((Kp * MLP_W + 255) / 256), dim3(256), 0, st, chunks, chunks, Kp,
                           layer_in(p, l), p->emb_dim, w.partial, w.partial_db, dW[l], db[l]);
        if (per_row_t && (l == p->skip_layer || l == 0))  // dL/dt_emb[r] += G_l[r] . W_l[:, 63:63+T]
            for (int c0 = 0; c0 < p->t_dim; c0 += 16)     // the small kernel handles 16 output columns per pass
                hipLaunchKernelGGL(mlp_rows_small_kernel, dim3((N * 4 + 255) / 256), dim3(256), 0, st, N,
                                   p->t_dim - c0 < 16 ? p->t_dim - c0 : 16, G, p->W[l] + MLP_XE + c0, layer_in(p, l), 1,
                                   (const float*)nullptr, dtemb + c0, p->t_dim, l == 0 ? 1 : 0);
        if (l >= 1) {  // (the backward-data GEMM of this layer was launched above: G_l stays intact in its buffer)
            float* t = G;
            G = Gn;
            Gn = t;
        }
    }
    if (!per_row_t && dtemb != nullptr)
        hipLaunchKernelGGL(mlp_dtemb_bcast_kernel, dim3(p->t_dim), dim3(256), 0, st, p->t_dim, db[0], p->W[0], layer_in(p, 0),
                           db[p->skip_layer], p->W[p->skip_layer], layer_in(p, p->skip_layer), dtemb);
    return launch_status();
}

int dgm_mlp_backward_group(const dgm_mlp_backward_job* a, const dgm_mlp_backward_job* b, int N, int temb_stride, void* stream) {
    if (!a || !b) return fail("mlp_backward_group: NULL job");
    const dgm_mlp_backward_job* jobs[2] = {a, b};
    if (check_params(a->params) || check_params(b->params)) return 1;
    if (N <= 0) return 0;
    for (const dgm_mlp_backward_job* j : jobs)
        if (!j->dOut || !j->workspace || !j->dWh || !j->dbh) return fail("mlp_backward_group: NULL pointer");
    if (a->workspace == b->workspace) return fail("mlp_backward_group: the two networks need workspaces of their own");
    const int mode = g_gemm_mode;
    const int fa = recall_ws_mode(a->workspace), fb = recall_ws_mode(b->workspace);
    const BwdPlan bp = bwd_plan(N, true);
    const int n_wg = group_split(bp);
    const bool grouped = n_wg > 0 && mode == 3 && temb_stride == 0 && fa == (3 | 16) && fb == (3 | 16) &&
                         a->params->emb_dim == b->params->emb_dim;
    if (!grouped) {  // two ordinary passes back to back: what the caller would have run (and every check of theirs)
        for (const dgm_mlp_backward_job* j : jobs)
            if (dgm_mlp_backward(j->params, N, j->dOut, temb_stride, j->workspace, j->dW, j->db, j->dWh, j->dbh, j->dtemb, stream)) return 1;
        return 0;
    }
    GroupNet nets[2];
    for (int i = 0; i < 2; i++) {
        const dgm_mlp_backward_job* j = jobs[i];
        for (int l = 0; l < 8; l++)
            if (!j->dW[l] || !j->db[l]) return fail("mlp_backward_group: NULL gradient pointer");
        nets[i].p = j->params, nets[i].dOut = j->dOut, nets[i].w = carve(j->workspace, N);
        nets[i].dW = j->dW, nets[i].db = j->db, nets[i].dWh = j->dWh, nets[i].dbh = j->dbh, nets[i].dtemb = j->dtemb;
    }
    return backward_planes_group(nets, N, bp, n_wg, (hipStream_t)stream);
}

int dgm_timenet_forward(const float* t, int n_freq, const float* W1, const float* b1, int hidden, const float* W2,
                        const float* b2, int n_out, float* save, float* out, void* stream) {
    if (!t || !W1 || !b1 || !W2 || !b2 || !save || !out) return fail("timenet_forward: NULL pointer");
    if (n_freq < 0 || 2 * n_freq + 1 > 64 || hidden < 1 || hidden > 1024 || n_out < 1 || n_out > 64)
        return fail("timenet_forward: unsupported size (2 n_freq + 1 <= 64, hidden <= 1024, n_out <= 64)");
    hipLaunchKernelGGL(mlp_timenet_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, t, n_freq, W1, b1, hidden, W2, b2,
                       n_out, save, out);
    return launch_status();
}

int dgm_timenet_backward(const float* d_out, int n_freq, const float* W2, int hidden, int n_out, const float* save,
                         float* dW1, float* db1, float* dW2, float* db2, void* stream) {
    if (!d_out || !W2 || !save || !dW1 || !db1 || !dW2 || !db2) return fail("timenet_backward: NULL pointer");
    if (n_freq < 0 || 2 * n_freq + 1 > 64 || hidden < 1 || hidden > 1024 || n_out < 1 || n_out > 64)
        return fail("timenet_backward: unsupported size");
    hipLaunchKernelGGL(mlp_timenet_bwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, d_out, n_freq, W2, hidden, n_out,
                       save, dW1, db1, dW2, db2);
    return launch_status();
}

}  // extern "C"
