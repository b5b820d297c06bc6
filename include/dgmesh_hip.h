/*
 * dgmesh_hip.h -- C ABI of libdgmesh_hip.so, the MI355X (gfx950) implementation of the
 * DG-Mesh training hot path: differentiable 3D-Gaussian rasterizer, simple-knn, fused
 * deformation MLP.
 *
 * This header is the drop-in boundary.  Every entry point replaces one interface of the
 * reference (paths relative to /root/reference/dgmesh/submodules/):
 *
 *   dgm_rasterize_forward   <- CudaRasterizer::Rasterizer::forward
 *                              diff-gaussian-rasterization/cuda_rasterizer/rasterizer.h:35-59
 *                              (impl rasterizer_impl.cu:198-336), reached from Python through
 *                              RasterizeGaussiansCUDA, rasterize_points.cu:35-114
 *   dgm_rasterize_backward  <- CudaRasterizer::Rasterizer::backward, rasterizer.h:61-85
 *                              (impl rasterizer_impl.cu:340-434); RasterizeGaussiansBackwardCUDA,
 *                              rasterize_points.cu:117-196
 *   dgm_mark_visible        <- CudaRasterizer::Rasterizer::markVisible, rasterizer.h:28-33
 *                              (impl rasterizer_impl.cu:141-153); markVisible, rasterize_points.cu:198-217
 *   dgm_knn_mean_dist2      <- SimpleKNN::knn, simple-knn/simple_knn.h:16-19 (impl simple_knn.cu:185-221);
 *                              distCUDA2, simple-knn/spatial.cu:15-26
 *   dgm_mlp_*               <- DeformNetwork* / AppearanceNetwork forward+backward,
 *                              dgmesh/utils/time_utils.py:58-323 (plain nn.Linear there)
 *
 * Conventions (same as the reference unless stated):
 *   - all `const float*` / `float*` / `int*` arguments are DEVICE pointers; optional inputs are
 *     passed as NULL exactly where the reference receives data_ptr()==nullptr from a 0-element
 *     tensor (colors_precomp, cov3D_precomp, shs, scales, rotations);
 *   - matrices are the reference's transposed (row-vector) 4x4 fp32, i.e. column-major for the
 *     kernels (dgmesh/scene/cameras.py:60-71);
 *   - scratch memory is caller-owned: forward obtains three opaque byte buffers through
 *     allocator callbacks (the reference's std::function<char*(size_t)>), backward receives the
 *     same three pointers back.  Their layout is private to this library (dgm_describe_state
 *     exposes it for the parity tests only);
 *   - every function returns 0 on success, non-zero on error (message via dgm_last_error());
 *     the reference throws std::runtime_error / AT_ERROR at the same points;
 *   - `stream` is a hipStream_t (NULL = default stream).  Unlike the reference (legacy default
 *     stream everywhere) all work is enqueued on the caller's stream;
 *   - outputs are fully OVERWRITTEN (the reference accumulates into pre-zeroed tensors); callers
 *     need not zero-fill out_color, radii or any dL_d* array;
 *   - memory contracts (tabulated in DESIGN.md "Memory contracts"; tests/test_redzone.py enforces the sizes, the bounds, the initial
 *     state and 16-byte alignment of byte scratch -- alignment figures below 16 are read from the launchers): a call reads its inputs and
 *     writes its outputs within exactly the shapes stated here, and touches exactly dgm_*_bytes(...) / dgm_*_floats(...) of a scratch
 *     buffer from the pointer it is handed -- a size already contains whatever the library needs to align that pointer itself.
 *     Unless an entry says otherwise a scratch buffer has NO INITIAL STATE (its bytes on entry do not matter, whatever an earlier
 *     call left there included) and may start at any 16-byte aligned address; tensors of floats / ints need their natural 4-byte
 *     alignment only (a 16-byte aligned start merely selects a vector code path where one exists, with identical results).  The
 *     exceptions: dgm_knn_mean_dist2 (256-byte aligned scratch, checked), dgm_ninit_bbox (scratch zero before its first call),
 *     the (P, 4) float4 arrays of the rasterizer -- rotations, dL_dconic, dL_drot: 16-byte aligned, checked -- and the tables of
 *     dgm_resample (stated there).
 */
#ifndef DGMESH_HIP_H
#define DGMESH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (a binding must check dgm_abi_version() against the header it was generated from):
 *   3: dgm_knn_mean_dist2 takes a caller-owned scratch buffer (dgm_knn_scratch_bytes); two replay-unit lists in dgm_state_layout.
 *   4: dgm_state_layout lost `upos` and `block_offs`, `inst` became uint2[R] (8-byte instance records; the backward forms the
 *      gradient row of an instance itself); dgm_laplace_* added.  Entry points' signatures are unchanged from 3.
 *   5: dgm_rasterize_forward_capacity added (a forward that never waits for the device); dgm_se3_* added (6-DoF heads);
 *      dgm_mlp_set_gemm knows modes 4 and 5.
 *      Every entry point of 4 is unchanged.
 *      Later additions that leave every existing entry point and layout unchanged keep the number: dgm_mc_* (marching cubes),
 *      dgm_tri_* (mesh rasterizer), dgm_anchor_* (Gaussian-mesh anchoring), dgm_ninit_* (entering the mesh phase),
 *      dgm_image_metrics* (test-view metrics), dgm_vertex_normals / dgm_mesh_shade / dgm_point_splat* / dgm_compose_frame
 *      (rendering a checkpoint), dgm_emd_* (mesh evaluation), dgm_png_unfilter / dgm_image_ingest (reading a dataset),
 *      dgm_image_composite_bytes / dgm_resample (resizing a dataset's images), dgm_lpips* (LPIPS of the test views),
 *      dgm_png_expand / dgm_image_ingest_masked / dgm_resample_nearest (real captures: mask PNGs and masked frames); dgm_png_unfilter
 *      also takes channels = 1; dgm_mesh_* (cleaning an extracted mesh); dgm_surf_* / dgm_corr_palette (mesh correspondence);
 *      dgm_ray_* (ray casting against a mesh); dgm_mlp_set_reduce_in_pair. */
#define DGM_ABI_VERSION 5

/* Allocator callback: must return a device pointer to at least `bytes` bytes (128-byte aligned),
 * valid until the matching backward has run.  Mirrors resizeFunctional, rasterize_points.cu:27-33.
 * `bytes` is exactly dgm_geometry_bytes / dgm_binning_bytes / dgm_image_bytes of the frame; each contains the 256 bytes by which
 * the library aligns the pointer up, so the caller adds nothing.  The chunks have no initial state. */
typedef char* (*dgm_alloc_fn)(void* ctx, size_t bytes);

int dgm_abi_version(void);
const char* dgm_last_error(void);

/* ---- rasterizer ------------------------------------------------------------------------- */

/* P Gaussians, D = active SH degree, M = SH coefficients per Gaussian (0 if shs == NULL).
 * out_color: (3,H,W) fp32.  radii: (P) int32 or NULL.  *num_rendered receives R (host int),
 * which costs one 4-byte device->host read-back exactly like rasterizer_impl.cu:281. */
int dgm_rasterize_forward(dgm_alloc_fn geom_alloc, void* geom_ctx, dgm_alloc_fn binning_alloc, void* binning_ctx,
                          dgm_alloc_fn image_alloc, void* image_ctx, int P, int D, int M, const float* background,
                          int width, int height, const float* means3D, const float* shs, const float* colors_precomp,
                          const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                          const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                          const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color,
                          int* radii, int debug, void* stream, int* num_rendered);

/* Gradient outputs (all fully written): dL_dmean2D (P,3), dL_dconic (P,4: slots x,y,w used),
 * dL_dopacity (P), dL_dcolor (P,3), dL_dmean3D (P,3), dL_dcov3D (P,6), dL_dsh (P,M,3) or NULL when
 * M == 0, dL_dscale (P,3), dL_drot (P,4). */
int dgm_rasterize_backward(int P, int D, int M, int R, const float* background, int width, int height,
                           const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                           float scale_modifier, const float* rotations, const float* cov3D_precomp,
                           const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                           float tan_fovy, const int* radii, char* geom_buffer, char* binning_buffer,
                           char* image_buffer, const float* dL_dpix, float* dL_dmean2D, float* dL_dconic,
                           float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                           float* dL_dscale, float* dL_drot, int debug, void* stream);

/* The same two calls for SH coefficients stored in two tensors, as the reference's model keeps them (_features_dc (P,1,3)
 * and _features_rest (P,M-1,3), gaussian_model_dpsr_dynamic_anchor.py:135-138): shs = the DC rows, shs_rest = the others;
 * the backward writes dL_dsh (P,1,3) and dL_dsh_rest (P,M-1,3).  Spares the caller torch.cat (get_features) and the
 * strided split of its gradient.  shs_rest == NULL (and dL_dsh_rest == NULL): exactly the calls above. */
int dgm_rasterize_forward_split_sh(dgm_alloc_fn geom_alloc, void* geom_ctx, dgm_alloc_fn binning_alloc, void* binning_ctx,
                                   dgm_alloc_fn image_alloc, void* image_ctx, int P, int D, int M, const float* background,
                                   int width, int height, const float* means3D, const float* shs, const float* shs_rest,
                                   const float* colors_precomp, const float* opacities, const float* scales,
                                   float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                   const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                                   float tan_fovy, int prefiltered, float* out_color, int* radii, int debug, void* stream,
                                   int* num_rendered);
/* The forward WITHOUT the host round trip (round 6).  Replaces -- and improves on -- the one blocking step of
 * CudaRasterizer::Rasterizer::forward, DGR/cuda_rasterizer/rasterizer_impl.cu:281 (`cudaMemcpy(&num_rendered, ...)` between the
 * scan and the allocation of the binning state): the caller sizes the binning buffer for `capacity` tile instances UP FRONT (e.g.
 * 1.25 x the previous frame's R), every array offset follows dgm_describe_state(P, width, height, capacity), and the call only
 * enqueues.  {R, flags, two worklist lengths} are copied to host_result[0..3] (caller-owned, page-locked host memory) behind the
 * scan; they are valid once an event the caller records after this call has completed.  flags bit 0: "point is filtered although
 * prefiltered is set" (auxiliary.h:156-160; the synchronous calls fail on it); bit 1: R > capacity -- the frame was neutralised on
 * the device (no tile has a range, no Gaussian a tile: image = background, the backward writes zero gradients, nothing is written
 * or read beyond `capacity` rows) and must be rendered again with capacity >= host_result[0].  The matching backward call takes
 * R = capacity.  Otherwise exactly dgm_rasterize_forward_split_sh (shs_rest may be NULL). */
int dgm_rasterize_forward_capacity(dgm_alloc_fn geom_alloc, void* geom_ctx, dgm_alloc_fn binning_alloc, void* binning_ctx,
                                   dgm_alloc_fn image_alloc, void* image_ctx, int P, int D, int M, const float* background,
                                   int width, int height, const float* means3D, const float* shs, const float* shs_rest,
                                   const float* colors_precomp, const float* opacities, const float* scales,
                                   float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                   const float* viewmatrix, const float* projmatrix, const float* cam_pos, float tan_fovx,
                                   float tan_fovy, int prefiltered, float* out_color, int* radii, int debug, void* stream,
                                   int capacity, unsigned* host_result);
int dgm_rasterize_backward_split_sh(int P, int D, int M, int R, const float* background, int width, int height,
                                    const float* means3D, const float* shs, const float* shs_rest,
                                    const float* colors_precomp, const float* scales, float scale_modifier,
                                    const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                                    const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy,
                                    const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                                    const float* dL_dpix, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity,
                                    float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest,
                                    float* dL_dscale, float* dL_drot, int debug, void* stream);

/* present: (P) bytes, 1 = view-space z > 0.2 */
int dgm_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     void* stream);

/* Sizes of the three scratch buffers (exactly what the allocator callbacks will be asked for, alignment slack included;
 * dgm_binning_bytes(R) with the R that *num_rendered receives -- or the capacity, in capacity mode). */
size_t dgm_geometry_bytes(int P, int width, int height);
size_t dgm_binning_bytes(int R);
size_t dgm_image_bytes(int width, int height);

/* Byte offsets of the arrays inside the scratch buffers -- TEST/INTROSPECTION ONLY. */
typedef struct {
    /* geometry buffer */
    size_t rec;           /* float[P][12]: x, y, conic a, b, c, opacity, r, g, b, rect(u32), offs(u32), 0 */
    size_t depth;         /* float[P]   view-space z */
    size_t radii;         /* int[P]     */
    size_t tiles_touched; /* u32[P]     */
    size_t offs;          /* u32[P]     EXCLUSIVE scan of tiles_touched (reference stores the inclusive scan) */
    size_t cov3D;         /* float[P][6] */
    size_t clamped;       /* u8[P]      bit ch set = colour channel ch clamped at 0 */
    size_t block_sums;    /* u32[ceil(P/256)] tiles touched per 256 Gaussians (preprocess -> the count kernel's offs) */
    size_t hist;          /* u32[n_chunks][tiles] */
    size_t tile_count;    /* u32[tiles]: per-tile list lengths during binning; after the forward call, the tiles in descending order of
                             their list length class (the order in which the forward blend takes them) */
    size_t tile_offset;   /* u32[tiles+1] */
    size_t big_list;      /* u32[tiles] worklists: tiles with more than 4096 instances from the front, tiles with 2049 ..
                             4096 from the end */
    size_t counters;      /* u32[8 + 64]: [0] = num_rendered, [1] = error flags, [2] = big worklist length, [3] = mid worklist length,
                             [4] = arrival counter of the tile scan; [8] = full replay units listed, [8 + 32] = last replay units
                             listed (the backward's work list, written by the forward; one 128-byte line each) */
    size_t geometry_bytes;
    /* binning buffer */
    size_t inst;       /* uint2[R] instance records (gaussian, depth bits), grouped by tile, in arrival order within a tile
                          (the tile sort's input) */
    size_t point_list; /* u32[R]  gaussian ids, by tile then depth then id: identical to the reference's */
    size_t slab;       /* float[R][9] per-instance gradient rows written by backward AT ROW offs[g] + k for Gaussian g's k-th tile
                          instance (k counts the tiles of g's rectangle row by row; rec[g][9] = packed rectangle, rec[g][10] =
                          offs[g]: the backward forms the row from the record it loads anyway -- ABI <= 3 carried it in a
                          u32[R] array `upos`).  Rows are therefore grouped by Gaussian and the per-Gaussian sum reads them
                          contiguously: colour r,g,b | moments of
                          g = G dL/dalpha about the splat centre: dx, dy, dx^2, dx dy, dy^2, 1.  Only rows with live[row] != 0
                          are written */
    size_t live;       /* u8[R] live[row] = 1 iff some pixel blended the instance, i.e. slab[row] was written by this backward */
    size_t ckpt;       /* float4[R/256 + 1][256]: (T, C.rgb) of a tile's pixels after each 256 list entries (forward ->
                          segment-parallel backward) */
    size_t ckpt64;     /* float4[R/u + 1][256], u = 64 (32 when R < 2^20: sparse frames): tiles with <= 4096 list entries leave
                          (T, C.rgb) after each u entries instead (slot (first + u i) / u), so that the backward replays them in
                          u-entry units on more waves */
    size_t ulist_full; /* uint4[R/u + 1]: the backward's work list, full u-entry units (256-entry ones for lists beyond 4096) in the
                          order the forward's tiles finished, a tile's run contiguous: (tile | short-list flag << 31, unit index,
                          first list slot, replay bound) */
    size_t binning_bytes;
    /* image buffer */
    size_t final_T;   /* float[H*W] */
    size_t n_contrib; /* u32[H*W] */
    size_t ranges;    /* uint2[tiles] */
    size_t nproc;     /* u32[tiles] list entries the backward has to replay (deepest contributor of the tile) */
    size_t cfin;      /* float4[tiles][256]: final (T, C.rgb without background) per pixel, backward lane order */
    size_t ulist_last; /* uint4[tiles + 1]: the tiles' last (partial) replay units, same record */
    size_t image_bytes;
    int tiles_x, tiles_y, n_chunks, chunk_size;
} dgm_state_layout;

int dgm_describe_state(int P, int width, int height, int R, dgm_state_layout* out);

/* Per-stage device timings, measured with hipEvents recorded on the caller's stream around each stage.
 * dgm_set_profiling(1): immediate -- every forward/backward call synchronises the stream and
 *     dgm_get_stage_ms() returns the durations of the most recent call;
 * dgm_set_profiling(2): deferred -- calls only record events (no synchronisation inside a timed region);
 *     after the caller has synchronised, dgm_collect_stage_ms() returns the average duration and the
 *     number of launches of every stage since the mode was set (and resets them);
 * dgm_set_profiling(0): off.  State is process-wide (PyTorch runs backward on its own thread).
 * dgm_set_profiling_sampling(n): in deferred mode bracket only every n-th launch of a stage (default 1); the averages are
 *     over the sampled launches, the counts are all launches. */
enum {
    DGM_STAGE_PREPROCESS = 0,
    DGM_STAGE_BIN_COUNT,
    DGM_STAGE_BIN_SCAN,
    DGM_STAGE_BIN_SCATTER,
    DGM_STAGE_TILE_SORT,
    DGM_STAGE_RENDER_FWD,
    DGM_STAGE_RENDER_BWD,
    DGM_STAGE_PREPROCESS_BWD,
    DGM_STAGE_MLP_LAYER_FWD, /* one 256 -> 256 trunk layer, forward GEMM launch (deferred mode only) */
    DGM_STAGE_MLP_LAYER_BWD, /* one 256 -> 256 backward-data GEMM launch */
    DGM_STAGE_MLP_LAYER_DW,  /* one 256 x 256 weight-gradient GEMM launch (without its reductions) */
    DGM_STAGE_MLP_BWD_PAIR,  /* backward data + weight gradient of one 256-wide layer in one launch (plane arithmetic) */
    DGM_STAGE_COUNT
};
void dgm_set_profiling(int mode);
void dgm_set_profiling_sampling(int every);
int dgm_get_stage_ms(float* ms, int capacity);
int dgm_collect_stage_ms(float* avg_ms, int* counts, int capacity);
const char* dgm_stage_name(int stage);

/* ---- simple-knn --------------------------------------------------------------------------- */

/* points: (P,3) fp32 device; mean_dists: (P) fp32 device = mean of the 3 smallest squared distances.
 * scratch: dgm_knn_scratch_bytes(P) bytes of caller-owned device memory, 256-byte aligned (Morton codes, the sort's
 * ping-pong buffers, the sorted points and the box table; contents are meaningless between calls).  Like every other entry
 * point the library neither allocates nor synchronises here (the reference's SimpleKNN::knn allocates five thrust vectors per
 * call, simple_knn.cu:187-210). */
size_t dgm_knn_scratch_bytes(int P);
int dgm_knn_mean_dist2(int P, const float* points, float* mean_dists, char* scratch, void* stream);

/* ---- deformation / appearance MLP trunk ---------------------------------------------------------- */

/* Weights in PyTorch nn.Linear layout (out_features, in_features), fp32, device pointers.
 * Geometry is the reference's only one: D = 8 layers, W = 256, skips = [4] (layer 5 consumes
 * [PE(x) | t_emb | h]), PE(x) = 63 columns, t_emb = t_dim columns (30 = timenet output for
 * is_blender, 21 = PE(t) otherwise).  Heads are passed concatenated: Wh (n_out, 256), bh (n_out). */
typedef struct {
    int n_layers;   /* 8 */
    int width;      /* 256 */
    int emb_dim;    /* 63 + t_dim */
    int t_dim;      /* 30 or 21 */
    int skip_layer; /* 5 */
    int n_out;      /* total head outputs, <= 16 */
    const float* W[8];
    const float* b[8];
    const float* Wh;
    const float* bh;
} dgm_mlp_params;

/* Arithmetic of the trunk GEMMs.  3 (default): "f16x3p" -- every fp32 operand scaled by a power of two and split into two binary16
 * numbers, three partial products accumulated in fp32 on the f16 matrix cores, on plane-format activations: every activation /
 * gradient tensor lives in HBM as its two binary16 planes with one power-of-two exponent per 32-row tile, split once by the kernel
 * that produces it.  1: native fp32 MFMA.  Both are fp32 GEMMs to rounding.  4 ("f16x3p8") and 5 ("f16x3p5") are mode 3's
 * arithmetic on other kernel forms, kept selectable as its A/B partners: 4 runs the forms of a time input per row for every call,
 * 5 every 256-wide layer GEMM with one wave per SIMD.  (0, "bf16x6", and 2, "f16x3" on fp32 rows, were retired in rounds 4 / 5 and
 * are ignored.)  Returns the previous mode; any other value only queries.  Process-wide; the initial value comes from the
 * environment variable DGM_MLP_GEMM=f16x3p|f16x3p8|f16x3p5|f32.  A forward and its backward must run in the same mode. */
int dgm_mlp_set_gemm(int mode);

/* Where a grouped backward pass (dgm_mlp_backward_group) sums the weight-gradient partial tiles of its hidden layers: `pieces` of
 * every such layer's reduction (of 256) run inside the next layer's paired launch, on workgroups that have finished their own
 * share, the rest in the pass's final reduction launch.  0: none (the final launch does all of it); values above 256 mean all.
 * The sums and their order are the same wherever a piece runs: the gradients do not depend on this value.  Returns the previous
 * value; a negative argument only queries.  Process-wide; the initial value is 0 or DGM_MLP_REDUCE_IN_PAIR=<n>. */
int dgm_mlp_set_reduce_in_pair(int pieces);

/* Bytes of the workspace that forward fills (embedding, the 8 post-ReLU activations, re-laid-out
 * weights, scratch) and backward consumes; caller-owned, must stay alive between the two calls.  The same size in every
 * arithmetic; any alignment (the library aligns to 256 itself, the size contains that); no initial state for forward, and backward
 * reads only what its forward wrote. */
size_t dgm_mlp_workspace_bytes(int N);

/* Introspection for tests and tools: byte offsets of the workspace's per-row tensors for N rows, in this order:
 * emb, Y[0..7], mask[0..7], Ga, Gb, Eexp, Yexp[0..7], Dexp, Gexp[0..1], Cin, Dp, partial[0..7], partial_db[0..7]
 * (DGM_MLP_WS_FIELDS entries).  In the plane arithmetic (mode 3) emb / Y / G rows are [h : K halves | l : K halves] with one
 * int exponent per 32-row tile in the matching *exp array: value = (h + l) * 2^-e.  Returns the number of fields. */
#define DGM_MLP_WS_FIELDS 49
int dgm_mlp_describe_workspace(int N, size_t* offs, int capacity);

/* out (N, n_out) = heads(trunk(x (N,3), temb)).  temb: (N, t_dim) with row stride temb_stride floats,
 * or ONE row broadcast to all N when temb_stride == 0 (t is identical for all rows in training). */
int dgm_mlp_forward(const dgm_mlp_params* p, int N, const float* x, const float* temb, int temb_stride,
                    char* workspace, float* out, void* stream);

/* The same with the positions formed on the fly: row r of the input is x[r] + x_add[r][0..2] (one fp32 sum; x_add has rows of
 * x_add_stride >= 3 floats) -- the inverse deformation network on the deformed means x + d_xyz, read straight from the deformation
 * network's output rows.  x_add may be NULL (= dgm_mlp_forward); plane arithmetic only, otherwise an error is returned. */
int dgm_mlp_forward_add(const dgm_mlp_params* p, int N, const float* x, const float* x_add, int x_add_stride, const float* temb,
                        int temb_stride, char* workspace, float* out, void* stream);

/* Given dOut (N, n_out): dW[l] / db[l] in the layout of W[l] / b[l], dWh, dbh, and dtemb
 * ((t_dim) summed over rows when temb_stride == 0, else (N, t_dim)); dtemb may be NULL. */
int dgm_mlp_backward(const dgm_mlp_params* p, int N, const float* dOut, int temb_stride, char* workspace,
                     float* const* dW, float* const* db, float* dWh, float* dbh, float* dtemb, void* stream);
/* The same, plus dX (N, 3) = dL/dx through both uses of PE(x) (layer 0 and the skip layer) and the derivative of the positional
 * encoding; x is the forward pass's input.  For networks whose input carries a gradient -- the appearance network on mesh
 * vertices moved by deform_back (dgmesh/utils/renderer.py:179-181, dgmesh/utils/time_utils.py:269-323).  x and dX may both be
 * NULL (= dgm_mlp_backward).  Plane arithmetic (the default) with a broadcast time row only: otherwise an error is returned rather
 * than the gradient dropped. */
int dgm_mlp_backward_dx(const dgm_mlp_params* p, int N, const float* dOut, int temb_stride, char* workspace,
                        float* const* dW, float* const* db, float* dWh, float* dbh, float* dtemb, const float* x, float* dX,
                        void* stream);

/* The backward passes of TWO networks over the same N rows in shared launches: the deformation network and its inverse
 * (dgmesh/train.py:156-216: deform and deform_back), whose backward passes need nothing of each other once both dOut exist.
 * One job per network: what dgm_mlp_backward takes (dtemb may be NULL).  Every launch of the pass then serves both networks
 * (eleven launches fewer), a layer-GEMM workgroup keeps one network's weights for twice the tiles, and ONE reduction launch sums
 * both networks' partial tiles.  The weight gradients keep the row chunks and the summation order of dgm_mlp_backward: the
 * gradients are bit-identical to two dgm_mlp_backward calls.  Grouping needs the default arithmetic (f16x3p) with a broadcast time row
 * (temb_stride == 0) on both workspaces, the same emb_dim, and a batch large enough for the paired launches (N >= 32 768 on
 * 256 CUs; DGM_MLP_PAIR=0 turns them off); otherwise the call runs two ordinary passes back to back, a then b, and is
 * bit-identical to them. */
typedef struct {
    const dgm_mlp_params* params;
    const float* dOut; /* (N, n_out) */
    char* workspace;   /* of this network's forward pass */
    float* dW[8];
    float* db[8];
    float* dWh;
    float* dbh;
    float* dtemb;
} dgm_mlp_backward_job;
int dgm_mlp_backward_group(const dgm_mlp_backward_job* a, const dgm_mlp_backward_job* b, int N, int temb_stride, void* stream);

/* The time branch of the is_blender networks for ONE row (t is identical for every Gaussian of an iteration,
 * dgmesh/train.py:158): out (n_out) = W2 relu(W1 PE(t) + b1) + b2 with PE(t) = [t, sin(2^k t), cos(2^k t), k < n_freq]
 * (dgmesh/utils/time_utils.py:24-55, 150-153: timenet = Linear(13, 256), ReLU, Linear(256, 30), n_freq = 6).
 * t: one device float; W1 (hidden, 2 n_freq + 1), W2 (n_out, hidden) row-major as nn.Linear stores them;
 * save: 2 n_freq + 1 + hidden floats kept for backward.  backward writes dW1, db1, dW2, db2 (t gets no gradient). */
int dgm_timenet_forward(const float* t, int n_freq, const float* W1, const float* b1, int hidden, const float* W2,
                        const float* b2, int n_out, float* save, float* out, void* stream);
int dgm_timenet_backward(const float* d_out, int n_freq, const float* W2, int hidden, int n_out, const float* save,
                         float* dW1, float* db1, float* dW2, float* db2, void* stream);

/* ---- fused image loss -------------------------------------------------------------------------------- */

/* loss = (1 - lambda) * mean|image - gt| + lambda * (1 - mean SSIM(image, gt)), the Gaussian-branch image loss of
 * dgmesh/train.py:307-311 (l1_loss + ssim of dgmesh/utils/loss_utils.py:18-19, 32-76; 11x11 window, sigma 1.5,
 * zero padding).  image, gt: (channels, H, W) fp32 device; out: 3 floats {loss, L1 term, mean SSIM};
 * the workspace filled by forward is consumed by backward (any alignment: aligned to 256 by the library, the size contains
 * that; no initial state for forward).  gt receives no gradient.  H, W >= 1: no minimum size. */
size_t dgm_image_loss_workspace_bytes(int channels, int H, int W);
int dgm_image_loss_forward(const float* image, const float* gt, int channels, int H, int W, float lambda_dssim,
                           char* workspace, float* out, void* stream);
/* grad_out: device scalar dL/dloss; d_image (channels, H, W) is fully written. */
int dgm_image_loss_backward(const float* image, const float* gt, int channels, int H, int W, float lambda_dssim,
                            const char* workspace, const float* grad_out, float* d_image, void* stream);

/* ---- test-view image metrics (csrc/metrics.hip) ------------------------------------------------------- */

/* MSE, PSNR, SSIM and MS-SSIM of B images against ONE target, as testing() (dgmesh/train.py:559-761) reports them; nothing is read
 * back.  images: (B, C, H, W) fp32 device; gt: (C, H, W) fp32 device; data_range L > 0; levels is 1 or 5.
 * out: (B, 4) DOUBLES on the device = {mse, psnr, ssim, ms_ssim}:
 *   mse     mean squared error over all channels and pixels;  psnr = -10 log10(mse)  (get_psnr, dgmesh/utils/image_utils.py:24-28);
 *   ssim    rgb_ssim of dgmesh/utils/metric_utils.py:26-79: 11-tap window exp(-(i-5)^2 / (2 1.5^2)) normalised to sum 1, separable,
 *           "valid" (the map of an H x W plane is (H-10) x (W-10)), C1 = (0.01 L)^2, C2 = (0.03 L)^2, variances clipped at 0,
 *           |sigma01| bounded by sqrt(sigma00 sigma11), mean over pixels and channels;
 *   ms_ssim (levels == 5; NaN otherwise) the defaults of the pytorch_msssim package in this project's own words: weights
 *           (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); per level and channel, no clipping, cs = mean((2 sigma01 + C2) /
 *           (sigma00 + sigma11 + C2)) and ssim_l = mean(((2 mu0 mu1 + C1) / (mu0^2 + mu1^2 + C1)) cs_map); between levels both images
 *           are 2x2 average-pooled with stride 2, an odd side zero-padded by one on BOTH ends, divisor 4; per channel
 *           prod_{l<4} relu(cs_l)^w_l * relu(ssim_4)^w_4; mean over channels.
 * levels == 5 needs min(H, W) > 160, levels == 1 min(H, W) >= 11: otherwise the call fails and workspace_bytes returns 0.
 * Inputs are fp32, all arithmetic is fp64; sums run over a fixed partition in a fixed order (no atomics), so the results are
 * bit-reproducible and row b does not depend on B.  workspace: dgm_image_metrics_workspace_bytes(...) bytes, caller-owned, no
 * initial state. */
size_t dgm_image_metrics_workspace_bytes(int B, int C, int H, int W, int levels);
int dgm_image_metrics(const float* images, const float* gt, int B, int C, int H, int W, float data_range, int levels, char* workspace,
                      double* out, void* stream);

/* LPIPS 0.1 of B images against ONE target (csrc/lpips.hip): images (B, 3, H, W) and gt (3, H, W), fp32 in [0, 1], row-major.
 * net: 0 = alex, 1 = vgg.  Both inputs become ((2x - 1) - shift_c) / scale_c, shift = (-0.030, -0.088, -0.188), scale = (0.458,
 * 0.448, 0.450), and run through the feature stack, every convolution followed by bias and ReLU:
 *   alex: conv 3->64 k11 s4 p2 (tap), maxpool 3/2, conv 64->192 k5 p2 (tap), maxpool 3/2, conv 192->384 k3 p1 (tap),
 *         conv 384->256 k3 p1 (tap), conv 256->256 k3 p1 (tap); min(H, W) >= 31.
 *   vgg : all k3 p1: 64, 64 (tap), maxpool 2/2, 128, 128 (tap), maxpool, 256, 256, 256 (tap), maxpool, 512, 512, 512 (tap),
 *         maxpool, 512, 512, 512 (tap); min(H, W) >= 16.
 * Max-pools have stride 2, no padding and floor output size.  Tap k of an image (features a) and of the target (features b), both
 * (h, w, C), gives mean over the h w pixels of sum_c lin_k[c] (a_c / (|a|_2 + 1e-10) - b_c / (|b|_2 + 1e-10))^2, norms over channels.
 * out: (B, 6) float64 = the five tap terms and their sum.  The target's features are computed once per call.
 * conv_w[i]: the i-th convolution's weight, packed (Kp, C_out) with row (ky kw + kx) C_in + c = weight[:, c, ky, kx] and
 * Kp = kh kw C_in rounded up to a multiple of 16, the rows past kh kw C_in zero; conv_b[i]: (C_out); lin[k]: (C_k).  conv_w, conv_b
 * and lin are HOST arrays (5 / 13 convolutions, 5 taps) of DEVICE pointers to fp32.
 * Convolutions are fp32 (a k-ordered fma chain per output element), the tap terms fp64 over a fixed partition in a fixed order
 * (no atomics): the results are bit-reproducible and row b does not depend on B.
 * workspace: dgm_lpips_workspace_bytes(...) bytes, caller-owned, no initial state; 0 for unsupported arguments, which dgm_lpips
 * refuses before any device work. */
size_t dgm_lpips_workspace_bytes(int net, int B, int H, int W);
int dgm_lpips(int net, const float* const* conv_w, const float* const* conv_b, const float* const* lin, const float* images,
              const float* gt, int B, int H, int W, char* workspace, double* out, void* stream);

/* ---- per-Gaussian glue of the train step ------------------------------------------------------------------ */

/* Activations + deformation in front of the rasterizer (dgmesh/gaussian_renderer/__init__.py:77-95 with the accessors
 * of dgmesh/scene/gaussian_model_dpsr_dynamic_anchor.py:92-128):  means3D = xyz + d_xyz, scales = exp(scaling) +
 * d_scaling, rotations = normalize(rotation) + d_rotation, opacities = sigmoid(opacity).  delta: raw (P, ld) head
 * output of the deformation network, columns [d_xyz 0:3 | d_rotation 3:7 | d_scaling 7:10 | ...], ld >= 10.
 * backward: given the rasterizer's gradients writes the parameter gradients and d_delta (P, ld; columns >= 10 zero). */
int dgm_gaussian_apply_forward(int P, const float* xyz, const float* scaling, const float* rotation, const float* opacity,
                               const float* delta, int ld, float* means3D, float* scales, float* rotations,
                               float* opacities, void* stream);
int dgm_gaussian_apply_backward(int P, const float* scaling, const float* rotation, const float* opacity,
                                const float* g_means3D, const float* g_scales, const float* g_rotations,
                                const float* g_opacities, float* d_xyz, float* d_scaling, float* d_rotation,
                                float* d_opacity, float* d_delta, int ld, void* stream);

/* 6-DoF deformation heads (is_6dof=True; round 6).  dgm_se3_exp_*: rows wv[i * ld + 0..5] = the raw outputs (w, v) of branch_w /
 * branch_v -> T (N, 4, 4) row-major, exactly dgmesh/utils/time_utils.py:116-123 (theta = |w|, w / theta + 1e-5, v / theta + 1e-5)
 * followed by exp_se3 of dgmesh/utils/rigid_utils.py:60-83 (Rodrigues' formula :40-57, rp_to_se3 :23-37); backward: dT (N, 16) ->
 * d_wv[i * ldd + 0..5].  dgm_se3_transform_*: the 6-DoF branch of render() (dgmesh/gaussian_renderer/__init__.py:68-75):
 * out = (T [xyz, 1])[:3] / (T [xyz, 1])[3]; backward writes dT (N, 16) and d_xyz (N, 3) in full. */
int dgm_se3_exp_forward(int N, const float* wv, int ld, float* T, void* stream);
int dgm_se3_exp_backward(int N, const float* wv, int ld, const float* dT, float* d_wv, int ldd, void* stream);
int dgm_se3_transform_forward(int N, const float* T, const float* xyz, float* out, void* stream);
int dgm_se3_transform_backward(int N, const float* T, const float* xyz, const float* g_out, float* dT, float* d_xyz, void* stream);

/* Cycle-consistency loss of dgmesh/train.py:221-238 on the raw (N, ld) outputs a (deform) and b (deform_back):
 * out[0] = (mean|b_xyz + a_xyz| + mean|b_rot + a_rot| + mean|b_scale + a_scale|) / 3, out[1..3] the three terms.
 * Fixed-order two-level reduction.  backward: grad_out = device scalar; d_a, d_b (N, ld) fully written.
 * workspace: dgm_cycle_loss_workspace_bytes(N) bytes of floats (4-byte aligned), used by the forward only, no initial state. */
size_t dgm_cycle_loss_workspace_bytes(int N);
int dgm_cycle_loss_forward(int N, const float* a, const float* b, int ld, char* workspace, float* out, void* stream);
int dgm_cycle_loss_backward(int N, const float* a, const float* b, int ld, const float* grad_out, float* d_a, float* d_b,
                            void* stream);

/* ---- optimizer ---------------------------------------------------------------------------------------- */

/* torch.optim.Adam (amsgrad=False, weight_decay=0) over n_tensors tensors in ONE kernel launch: the Adam steps that
 * close a train iteration (dgmesh/train.py:518-524; groups of gaussian_model_dpsr_dynamic_anchor.py:186-212 and
 * deform_model.py:33-44).  All arrays are HOST arrays of length n_tensors; params / grads / exp_avg / exp_avg_sq hold
 * fp32 device pointers, lr[i] the tensor's learning rate, step[i] >= 1 its step count AFTER this update (bias
 * correction 1 - beta^step).  Tensors with numel 0 are skipped. */
int dgm_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const long long* numel, const float* lr, const int* step, float beta1,
                  float beta2, float eps, void* stream);

/* ---- densification / pruning on the device (csrc/densify.hip) ----------------------------------------------------------
 * Replaces GaussianModelDPSRDynamicAnchor.densify_and_prune / prune_points
 * (dgmesh/scene/gaussian_model_dpsr_dynamic_anchor.py:383-551): decide keep / clone / split / prune per Gaussian, scan,
 * then gather every parameter and Adam moment into the final set with one multi-tensor launch.
 *   dgm_densify_decide: grad = grad_accum / denom (NaN -> 0); clone if grad >= thr and max(exp(scaling)) <= dense_extent,
 *     split if grad >= thr and larger; pruned if sigmoid(opacity) < min_opacity or max(exp(scaling)) > big_extent
 *     (pass +inf to switch the size limit off).  With keep_mask != NULL (bytes 0/1, device) the decision is the mask
 *     (prune_points).  After the stream reaches this point the three u32 at scratch + dgm_densify_totals_offset(P) hold
 *     the numbers of kept originals K, kept clones C and kept split parents S; new size = K + C + 2 S, ordered
 *     [originals | clones | first children | second children] like the reference's cat / prune sequence.
 *   dgm_densify_apply: out[t][j] = in[t][source(j)] for all n_tensors (<= 24) tensors of row width width[t] floats; rows of
 *     new points are zero where is_moment[t] != 0; the xyz / scaling rows of split children are rewritten from the
 *     caller's standard-normal samples z[2][P][3] (device).  src_scratch: (K + C + 2 S) * 4 bytes.
 *   scratch: dgm_densify_scratch_bytes(P) bytes, 4-byte aligned, no initial state; _decide writes it (flags, three scans, the totals
 *     at dgm_densify_totals_offset(P), which is a multiple of 256 and leaves 256 bytes behind it) and _apply of the same P reads it. */
/* Per-iteration statistics (dgmesh/train.py:489-496, gaussian_model_dpsr_dynamic_anchor.py:679-682), in place, for the
 * Gaussians with radii > 0: max_radii2D = max(max_radii2D, radii); with grad2d != NULL (dL/dmeans2D, (P,3)) also
 * grad_accum += |grad2d[:, :2]| and denom += 1.  All (P) fp32 on the device. */
int dgm_densify_stats(int P, const float* grad2d, const int* radii, float* max_radii2D, float* grad_accum, float* denom,
                      void* stream);
size_t dgm_densify_scratch_bytes(int P);
size_t dgm_densify_totals_offset(int P);
int dgm_densify_decide(int P, const float* grad_accum, const float* denom, const float* scaling, const float* opacity,
                       float grad_threshold, float dense_extent, float min_opacity, float big_extent,
                       const uint8_t* keep_mask, char* scratch, void* stream);
int dgm_densify_apply(int P, unsigned K, unsigned C, unsigned S, const char* scratch, unsigned* src_scratch, int n_tensors,
                      const float* const* in, float* const* out, const int* width, const int* is_moment, int xyz_index,
                      int scaling_index, int rotation_index, const float* z, void* stream);

/* ---- DPSR pieces (csrc/dpsr.hip) --------------------------------------------------------------------------------------
 * Replace point_rasterize / grid_interp (dgmesh/nvdiffrast_utils/dpsr_utils.py:69-198) and the spectral solve between the
 * two FFTs of DPSR.forward (dgmesh/nvdiffrast_utils/dpsr.py:28-69).  V: points in (0,1)^3 [n][3]; N: normals [n][3];
 * grids are res^3 (periodic), row-major [x][y][z]; spectra are the rfftn layout [res][res][res/2+1] of float2.
 *   splat_forward : grid[3][res^3] = sum_p w_c(p) N[p]  (the callee zeroes grid);  splat_backward: dV, dN from dgrid
 *   interp_forward: fv[p] = trilinear phi(V[p]);  interp_backward: dphi (zeroed by the callee, then accumulated), dV
 *   spectral      : adjoint == 0: out[k] = sum_d (-i c_d) in[d][k];  adjoint != 0: out[d][k] = (+i c_d) in[k];
 *                   c_d = omega_d G / (Lap + 1e-6), G = exp(-0.5 (2 sig |f| / res)^2), out(0) = 0. */
int dgm_dpsr_splat_forward(int n, int res, const float* V, const float* N, float* grid, void* stream);
int dgm_dpsr_splat_backward(int n, int res, const float* V, const float* N, const float* dgrid, float* dV, float* dN,
                            void* stream);
int dgm_dpsr_interp_forward(int n, int res, const float* phi, const float* V, float* fv, void* stream);
int dgm_dpsr_interp_backward(int n, int res, const float* phi, const float* V, const float* dfv, float* dphi, float* dV,
                             void* stream);
int dgm_dpsr_spectral(int res, float sig, const float* in, float* out, int adjoint, void* stream);

/* Umbrella-operator Laplacian regulariser of a triangle mesh, laplace_regularizer_const (dgmesh/nvdiffrast_utils/regularizer.py:40-60):
 * loss[0] = mean over the 3 V components of (term / max(norm, 1))^2, term[v] = sum over the faces at v of (a - v) + (b - v),
 * norm[v] = 2 x faces at v.  v_pos (V, 3) fp32, faces (F, 3) int32, scratch: dgm_laplace_scratch_floats(V) floats of caller-owned
 * device memory (no initial state: the forward zeroes what it accumulates into) that the backward reads again (normalised term,
 * norm).  dv (V, 3) = dloss[0] x d loss / d v_pos (overwritten).  Face indices must lie in [0, V): they are not range-checked.
 * Sums use fp32 atomics like the reference's scatter_add_: results agree to rounding, not bit for bit, run to run. */
size_t dgm_laplace_scratch_floats(int V);
int dgm_laplace_forward(int V, int F, const float* v_pos, const int* faces, float* scratch, float* loss, void* stream);
int dgm_laplace_backward(int V, int F, const int* faces, const float* scratch, const float* dloss, float* dv, void* stream);

/* ---- opacity field on a regular grid (csrc/opacity_field.hip) ------------------------------------------------------------
 * Replaces get_opacity_field_from_gaussians (dgmesh/utils/mesh_utils.py:7-76): occ[res^3] = sum over the Gaussians of the
 * cell's block (centre strictly inside the block's box grown by `margin`, opacity > opacity_threshold) of
 * opacity * exp(-0.5 d^T Sigma^-1 d), Sigma from (scalings, rotations) as build_covariance_from_scaling_rotation,
 * inverse by cofactors + 1e-24 (gaussian_3d_coeff).  coords[res]: the grid coordinates along an axis.
 * scratch: dgm_opacity_field_scratch_bytes(P) bytes = 12 floats per Gaussian (4-byte aligned) and 256 spare; no initial state;
 * not read for P == 0.  res need not be a multiple of num_blocks: the last block of an axis is shorter, as torch's split. */
size_t dgm_opacity_field_scratch_bytes(int P);
int dgm_opacity_field(int P, const float* xyz, const float* rotations, const float* scalings, const float* opacities,
                      float opacity_threshold, int res, int num_blocks, float margin, const float* coords, char* scratch,
                      float* occ, void* stream);

/* ---- marching cubes (csrc/marching_cubes.hip) -------------------------------------------------------------------------------
 * Replaces diso.DiffMC (the reference's mesh extraction, dgmesh/utils/renderer.py:171).  grid (X, Y, Z) fp32 row-major [x][y][z],
 * every dimension >= 2 and 5 X Y Z < 2^31; point (i, j, k) sits at (i, j, k) (+ deform[i][j][k][0..2] when deform != NULL).
 * A point is inside iff f < iso (NaN: outside); edge a->b is crossed iff inside(a) != inside(b); its vertex is
 * p_a + t (p_b - p_a), t = (iso - fa) / (fb - fa), divided by (dim - 1) per axis when normalize != 0.
 * Vertices: one per crossed edge, ordered by the owning point's linear index (i Y + j) Z + k (a point owns its +x, +y, +z edges),
 * then by axis.  Faces: int32 vertex triples ordered by cell linear index (i (Y-1) + j) (Z-1) + k, then by the case table
 * (csrc/mc_tables.hpp, generated by tools/gen_mc_tables.py), wound so that (v1 - v0) x (v2 - v0) points towards f >= iso.
 * All orders come from prefix sums: output is identical run to run.
 *   dgm_mc_scratch_bytes: caller-owned device scratch for one extraction (0 for invalid dimensions); count, emit and backward of
 *                         one extraction use the same scratch, and the grid must not change between them.  16-byte aligned (the
 *                         arrays inside sit at multiples of 256 from the pointer as given); no initial state for count.
 *   dgm_mc_count   : classifies the cells and writes counts[0] = V, counts[1] = F (device ints).  The caller reads them back
 *                    (the extraction's one host synchronisation) and sizes the outputs.
 *   dgm_mc_emit    : writes verts (V, 3) fp32 and faces (F, 3) int32 (V, F: the counts; NULL allowed where a count is 0).
 *   dgm_mc_backward: dgrid (X, Y, Z) and, when deform != NULL, ddeform (X, Y, Z, 3) = the gradients of sum(dverts * verts),
 *                    both overwritten; a gather without atomics (bit-reproducible). */
size_t dgm_mc_scratch_bytes(int X, int Y, int Z);
int dgm_mc_count(int X, int Y, int Z, const float* grid, float iso, char* scratch, int* counts, void* stream);
int dgm_mc_emit(int X, int Y, int Z, const float* grid, const float* deform, float iso, int normalize, char* scratch, int V, int F,
                float* verts, int* faces, void* stream);
int dgm_mc_backward(int X, int Y, int Z, const float* grid, const float* deform, float iso, int normalize, const char* scratch, int V,
                    const float* dverts, float* dgrid, float* ddeform, void* stream);

/* ---- mesh rasterizer (csrc/mesh_raster.hip) ---------------------------------------------------------------------------------
 * Replaces nvdiffrast's rasterize / interpolate / antialias (dgmesh/utils/renderer.py:33-121), batch size 1.  pos (V, 4) fp32
 * clip-space positions, tri (F, 3) int32, F < 2^24, 0 < H, W <= 16384.  Screen s = ((x/w + 1) W/2, (y/w + 1) H/2); pixel (px, py)
 * is centred at (px + .5, py + .5), row 0 at NDC y = -1.  A face with a vertex at w <= 0 (or an index outside [0, V), or zero
 * screen area) is dropped.  A centre is covered when the three oriented edge functions, each evaluated with its endpoints in
 * ascending vertex-id order, are >= 0.  Depth z/w, linear in screen space; the smaller wins, ties to the lower face id.
 *   dgm_tri_raster_scratch_bytes: device scratch of one rasterize forward (0 for invalid sizes): 64-bit keys first, so 8-byte
 *                               aligned at least; no initial state (the forward clears it); not needed by the backward.
 *   dgm_tri_rasterize_forward : rast (H, W, 4) = (u, v, z/w, id + 1), zeros on background; (u, v) perspective-correct
 *                               barycentrics of vertices 0 and 1.  Bit-reproducible.
 *   dgm_tri_rasterize_backward: dpos (V, 4) (overwritten) = the gradient of sum(drast[..., 0:2] * rast[..., 0:2]) w.r.t. x, y, w;
 *                               the z column is zero.
 *   dgm_tri_interpolate_*     : out (H, W, C) = u a0 + v a1 + (1 - u - v) a2 (zeros on background); backward writes dattr (V, C)
 *                               and drast (H, W, 4) (channels 2, 3 zero), both overwritten.
 *   dgm_tri_aa_scratch_bytes: device scratch of one antialias forward (the edge topology); its backward reads it again.  8-byte
 *                               aligned at least; no initial state for the forward.
 *   dgm_tri_antialias_forward : out (H, W, C) = color + the analytic blend across silhouette edges (csrc/mesh_raster.hip).
 *                               Bit-reproducible.
 *   dgm_tri_antialias_backward: dcolor (H, W, C) (a gather, bit-reproducible) and dpos (V, 4) (overwritten).
 * dpos and dattr are summed with fp32 atomics: they agree to rounding, not bit for bit, run to run. */
size_t dgm_tri_raster_scratch_bytes(int F, int H, int W);
int dgm_tri_rasterize_forward(int V, int F, int H, int W, const float* pos, const int* tri, char* scratch, float* rast, void* stream);
int dgm_tri_rasterize_backward(int V, int F, int H, int W, const float* pos, const int* tri, const float* rast, const float* drast,
                               float* dpos, void* stream);
int dgm_tri_interpolate_forward(int V, int F, int H, int W, int C, const float* attr, const float* rast, const int* tri, float* out,
                                void* stream);
int dgm_tri_interpolate_backward(int V, int F, int H, int W, int C, const float* attr, const float* rast, const int* tri,
                                 const float* dout, float* dattr, float* drast, void* stream);
size_t dgm_tri_aa_scratch_bytes(int F);
int dgm_tri_antialias_forward(int V, int F, int H, int W, int C, const float* color, const float* rast, const float* pos, const int* tri,
                              char* scratch, float* out, void* stream);
int dgm_tri_antialias_backward(int V, int F, int H, int W, int C, const float* color, const float* rast, const float* pos, const int* tri,
                               const char* scratch, const float* dout, float* dcolor, float* dpos, void* stream);

/* ---- texture sampling and the texture atlas (csrc/mesh_texture.hip) -------------------------------------------------------------------
 * nvdiffrast.torch.texture without mip-maps (the reference samples with it in dgmesh/nvdiffrast_utils/regularizer.py:24), and the
 * atlas that mesh_texture.py bakes appearance into.  Every buffer is device memory; nothing is allocated and nothing is read back.
 * fp32, no FMA; csrc/mesh_texture.hip states every formula and the operation order.
 *   dgm_tri_texture_forward: tex (Ht, Wt, C), uv (n, 2) -> out (n, C).  Texel (i, j) is centred at u = (i + .5) / Wt, v = (j + .5) / Ht;
 *       row 0 of memory is at v = 0.  filter DGM_TEX_LINEAR: bilinear over the four texels around (u Wt - .5, v Ht - .5);
 *       DGM_TEX_NEAREST: texel (floor(u Wt), floor(v Ht)).  boundary DGM_TEX_WRAP: indices modulo the size; DGM_TEX_CLAMP: indices
 *       clamped; DGM_TEX_ZERO: texels outside count as 0.  A sample with a non-finite u or v gives 0 in every channel; a finite uv
 *       of any magnitude is reduced in float before it is converted, so nothing is read outside tex.  1 <= Ht, Wt <= 16384.
 *       With C == 4 and 16-byte aligned tex and out a texel is one 16-byte access; 4-byte alignment otherwise.  Bit-reproducible.
 *   dgm_tri_texture_backward: dtex (Ht, Wt, C) (zeroed by the call, summed with fp32 atomics: agrees to rounding, not bit for bit, run
 *       to run) and duv (n, 2) (plain stores, from the bilinear weights' derivatives; zero for DGM_TEX_NEAREST and for a non-finite
 *       sample, which adds nothing to dtex either).
 *   dgm_atlas_uv: the atlas gives each pair of faces (2c, 2c + 1) the square cell c of `cell` = s >= 4 texels a side, size / s cells
 *       a row (size <= 16384), L = s - 3; in texel-centre index coordinates local to the cell face 2c has its corners at (0, 0),
 *       (L, 0), (0, L) and face 2c + 1 at (s - 1, s - 1), (2, s - 1), (s - 1, 2).  uv_out (F, 3, 2): a corner at local (i, j) of cell
 *       (cx, cy) has u = ((float)(cx s + i) + .5f) / (float)size, v alike.  More face pairs than cells is an error.
 *   dgm_atlas_interpolate: one value per texel: out (size, size, C) and face_id (size, size), every texel written.  Local texel (i, j)
 *       belongs to face 2c when i + j <= s - 2 (b1 = i / L, b2 = j / L), to face 2c + 1 when i + j >= s (b1 = (s - 1 - i) / L,
 *       b2 = (s - 1 - j) / L), to nobody when i + j = s - 1; b0 = (1 - b1) - b2, NOT clamped: texels of a chart's bilinear footprint
 *       outside the triangle hold the affine extrapolation.  Owned: out = (b0 a0 + b1 a1) + b2 a2 of attr (V, C) at the face's
 *       corners, face_id = the face.  Unowned -- the diagonal, the margin right of or below the last whole cell, a face >= F, a face
 *       with an index outside [0, V) (checked before any use) -- : zeros and -1.  Bit-reproducible. */
#define DGM_TEX_NEAREST 0
#define DGM_TEX_LINEAR 1
#define DGM_TEX_WRAP 0
#define DGM_TEX_CLAMP 1
#define DGM_TEX_ZERO 2
int dgm_tri_texture_forward(int n, int Ht, int Wt, int C, int filter, int boundary, const float* tex, const float* uv, float* out,
                            void* stream);
int dgm_tri_texture_backward(int n, int Ht, int Wt, int C, int filter, int boundary, const float* tex, const float* uv, const float* dout,
                             float* dtex, float* duv, void* stream);
int dgm_atlas_uv(int F, int size, int cell, float* uv_out, void* stream);
int dgm_atlas_interpolate(int V, int F, int C, int size, int cell, const float* attr, const int* faces, float* out, int* face_id,
                          void* stream);

/* ---- Gaussian-mesh anchoring (csrc/anchor.hip) --------------------------------------------------------------------------------
 * Replace the trimesh / pytorch3d.knn_points / torch.unique work of GaussianModelDPSRDynamicAnchor.anchor_mesh
 * (dgmesh/scene/gaussian_model_dpsr_dynamic_anchor.py:745-829).  Every buffer is device memory; nothing is read back.
 *   dgm_anchor_face_geometry: centroids (F, 3) = ((v0 + v1) + v2) / 3 and unit normals (F, 3) of cross(v1 - v0, v2 - v0), zero where
 *       the cross product has zero length (trimesh's face_normals).  A face with an index outside [0, V) gets a NaN centroid (no
 *       query can choose it) and a zero normal.  fp32, no FMA.
 *   dgm_anchor_nn: for each of Nq query points (Nq, 3), idx[q] = the target (Nt, 3) with the least d2 = (dx*dx + dy*dy) + dz*dz (fp32,
 *       no FMA), ties to the smallest target index, reported only if d2 < max_d2 (strict); otherwise idx = -1, d2 = +inf.  max_d2 may
 *       be +inf (the unbounded search).  Bit-reproducible; independent of the targets' order up to the index mapping.
 *       scratch: dgm_anchor_nn_scratch_bytes(Nq, Nt) bytes (unused for max_d2 = +inf, may then be NULL).
 *   dgm_anchor_classify: face_of (P) int32 (the Gaussian's face, -1 or out of [0, F): invalid) ->
 *       counts (F) = valid Gaussians per face; offsets (F) = exclusive prefix sum of counts;
 *       lists (F) = [faces with count 1 | count > 1 | count 0], each part ascending;
 *       members (P) = the valid Gaussians grouped by face, ascending face, ascending index within a face (members[offsets[f] + r]
 *       is the r-th Gaussian of face f), then -1;  rank (P) = r for a valid Gaussian, -1 otherwise;
 *       totals (4) = (n_1_1, n_n_1, n_0_1, valid Gaussians) -- the caller's one read-back.
 *       scratch: dgm_anchor_classify_scratch_bytes(P, F) bytes. */
int dgm_anchor_face_geometry(int V, int F, const float* verts, const int* faces, float* centroids, float* normals, void* stream);
size_t dgm_anchor_nn_scratch_bytes(int Nq, int Nt);
int dgm_anchor_nn(int Nq, int Nt, const float* queries, const float* targets, float max_d2, char* scratch, int* idx, float* d2,
                  void* stream);
size_t dgm_anchor_classify_scratch_bytes(int P, int F);
int dgm_anchor_classify(int P, int F, const int* face_of, char* scratch, int* counts, int* offsets, int* lists, int* members, int* rank,
                        int* totals, void* stream);

/* ---- entering the mesh phase (csrc/normal_init.hip) ------------------------------------------------------------------------------
 * The device side of update_scale_center and normal_initialization (dgmesh/scene/gaussian_model_dpsr_dynamic_anchor.py:93-120,
 * 684-734).  Every buffer is device memory; nothing is read back.
 *   dgm_ninit_bbox: out6 = (min x, min y, min z, max x, max y, max z) of the P rows xyz + d_xyz (one fp32 addition; d_xyz may be
 *       NULL = zero), in one launch.  Exact, with -0 ordered below +0, hence independent of the reduction order (the sign of a
 *       zero extremum may differ from torch.aminmax's); a NaN coordinate makes both extrema of its axis NaN.  P >= 1.  scratch: dgm_ninit_bbox_scratch_bytes() bytes that are ZERO before the first call; every call leaves
 *       them ready for the next one on the same stream.
 *   dgm_ninit_face_areas: area[f] = 0.5 |cross(v1 - v0, v2 - v0)| (fp32, no FMA); 0 for a face with an index outside [0, V) and
 *       for a non-finite result.
 *   dgm_ninit_area_scan: cum[i] = area[0] + ... + area[i] in fp64 over a fixed partition (tiles of 4096 faces, 16 per thread;
 *       thread totals in thread order, tile totals in tile order): non-decreasing exactly, bit-reproducible.
 *       scratch: dgm_ninit_scan_scratch_bytes(F) bytes.
 *   dgm_ninit_sample: for each of `count` draws u (count, 3) in [0, 1): pick = (double)u0 * cum[F - 1]; face_index = the smallest
 *       i with cum[i] >= pick and cum[i] > 0 (numpy searchsorted side="left"; a face of area 0 is never chosen); if u1 + u2 > 1
 *       both become 1 - u; points = v0 + (u1 (v1 - v0) + u2 (v2 - v0)) (fp32, no FMA).  cum[F - 1] == 0: face_index = -1 and NaN
 *       points.  F >= 1. */
size_t dgm_ninit_bbox_scratch_bytes(void);
int dgm_ninit_bbox(int P, const float* xyz, const float* d_xyz, char* scratch, float* out6, void* stream);
int dgm_ninit_face_areas(int V, int F, const float* verts, const int* faces, float* area, void* stream);
size_t dgm_ninit_scan_scratch_bytes(int F);
int dgm_ninit_area_scan(int F, const float* area, char* scratch, double* cum, void* stream);
int dgm_ninit_sample(int V, int F, int count, const float* verts, const int* faces, const double* cum, const float* u, float* points,
                     int* face_index, void* stream);

/* ---- rendering a checkpoint (csrc/visualize.hip) --------------------------------------------------------------------------------
 * The device side of mesh_shape_renderer / pointcloud_renderer (dgmesh/utils/renderer.py:236-374) and of the frame composition of
 * render_test.py / render_trajectory.py.  Every pointer is device memory unless it says host; nothing is read back.  fp32, no FMA.
 *   dgm_vertex_normals: normals (V, 3) (zeroed by the call) = the area-weighted vertex normals: cross(v1 - v0, v2 - v0) of every face
 *       added to its three vertices, each vertex then divided by its length; a length below 1e-6 gives (0, 0, 0).  A face with an index
 *       outside [0, V) is skipped.  The sums are fp32 atomics: the result agrees to rounding, not bit for bit, run to run.
 *   dgm_mesh_shade: a deferred hard-Phong pass over the mesh rasterizer's rast (H, W, 4) = (u, v, z/w, id + 1).  Per covered pixel:
 *       p and n interpolated with (u, v, 1 - u - v) from verts and normals, n scaled by normal_sign and renormalised (length < 1e-6:
 *       zero); one directional light l (unit vector towards the light): diffuse = max(n.l, 0), r = 2 (n.l) n - l,
 *       view = normalize(camera_center - p), spec = n.l > 0 ? max(view.r, 0)^shininess : 0;
 *       image (H, W, 3) = clamp((ambient + diffuse_k * diffuse) * base_color + specular_k * spec, 0, 1); background where id is 0 (or
 *       names no valid face).  params: ONE dgm_shade_params in device memory (the light may have been computed on the device).
 *   dgm_point_splat: every point of pos_clip (N, 4) with w > 0 and finite coordinates lands on pixel floor(s), s = ((x/w + 1) W/2,
 *       (y/w + 1) H/2) (the mesh rasterizer's mapping), and covers the size x size square of pixels centred there, clipped to the image
 *       (size odd, 1..15).  Per pixel the smallest z/w wins, ties to the lower point id: one 64-bit atomicMin of
 *       (ordered z/w bits) << 32 | id.  image (H, W, 3) = the winner's colour -- colors (N, 3), or, when colors is NULL,
 *       bg_color6[3..5] -- and bg_color6[0..2] elsewhere; bg_color6 is a HOST array of six floats.  Bit-reproducible.
 *       scratch: dgm_point_splat_scratch_bytes(H, W) bytes (0 for invalid sizes) = H W uint64 rounded up to 256, used from the
 *       pointer as given: it must be 8-byte aligned (64-bit atomics; the size holds no alignment slack), no initial state (the call
 *       sets it to all ones); after the call its first H W uint64 hold the winning keys (all ones: empty; low 32 bits: the point id).
 *   dgm_compose_frame: n_panels (1..4) fp32 panels of H x W pixels, panels[k] (a HOST array of device pointers) laid out (3, H, W)
 *       when layouts[k] (HOST) is 0 and (H, W, 3) when it is 1, side by side into out_u8 (H/d, n_panels W/d, 3) uint8.  d = downsample
 *       is 1 or 2 (then H and W are even): each 2x2 block averages as ((a + b) + (c + d)) * 0.25, top row first.  Then
 *       clamp to [0, 1], times 255, truncated toward zero; NaN writes 0. */
typedef struct dgm_shade_params {
    float light_dir[3];      /* unit vector from the surface towards the light */
    float ambient;
    float camera_center[3];
    float diffuse;           /* light diffuse x material diffuse */
    float background[3];
    float specular;          /* light specular x material specular */
    float base_color[3];
    float shininess;
    float normal_sign;       /* +1, or -1 for a mesh wound inwards */
    float pad[3];
} dgm_shade_params;
int dgm_vertex_normals(int V, int F, const float* verts, const int* faces, float* normals, void* stream);
int dgm_mesh_shade(int V, int F, int H, int W, const float* verts, const float* normals, const int* faces, const float* rast,
                   const dgm_shade_params* params, float* image, void* stream);
size_t dgm_point_splat_scratch_bytes(int H, int W);
int dgm_point_splat(int N, int H, int W, const float* pos_clip, const float* colors, int size, const float* bg_color6, char* scratch,
                    float* image, void* stream);
int dgm_compose_frame(int n_panels, const float* const* panels, const int* layouts, int H, int W, int downsample, unsigned char* out_u8,
                      void* stream);

/* ---- mesh evaluation: approximate earth mover's distance (csrc/emd.hip) -------------------------------------------------------------
 * Replaces approxmatchkernel + matchcostkernel (dgmesh/metrics/pytorch_structural_losses/src/approxmatch.cu:3-224), the match cost
 * behind the EMD column of dgmesh/mesh_evaluation.py.  xyz1 (b, n, 3), xyz2 (b, m, 3) fp32; every buffer is device memory, nothing
 * is allocated and nothing is read back.  No n x m array is formed: sum(match * dist) is accumulated while the match is computed.
 * The iteration, with its integer-division mass rule (multiL, multiR) = (1, n / m) or (m / n, 1) and its nine levels -4^7 .. -4^-1,
 * is stated at the top of csrc/emd.hip.  No atomics: two calls on the same input return the same bits, and a batch returns the bits
 * its elements return alone.
 *   dgm_emd_tile: constants of the launch structure: which = 0 the rows per workgroup, 1 the columns per LDS tile, 2 the number of
 *       workgroups a sweep aims for per batch element, 3 the number of levels; 0 for any other `which`.
 *   dgm_emd_parts: the number of column parts of a sweep over `rows` rows and `cols` columns: with rt = ceil(rows / tile 0) and
 *       ct = ceil(cols / tile 1), want = min(ct, ceil(tile 2 / rt)), each part takes ceil(ct / want) column tiles.  0 for sizes
 *       outside [1, 2^28].
 *   dgm_emd_scratch_floats: the caller-owned scratch of one call, in floats: five vectors of b n or b m floats and the partial
 *       sums, b max(2 n parts(n, m), m parts(m, n)) floats, each rounded up to 64 floats; 0 for invalid sizes.  Its contents on entry
 *       do not matter; 4-byte aligned.
 *   dgm_emd_approx: cost (b) = sum over the nine levels of sum w[k,l] sqrt(d2[k,l]) (not divided by n); residual (b, 2), unless
 *       NULL, = (sum remainL, sum remainR) after the last level, the mass that was not transported.  1 <= b <= 65535,
 *       1 <= n, m <= 2^28: row, column and tile indices are int, which that cap keeps far from overflow; every buffer offset
 *       (b n 3, b parts n) is 64-bit. */
int dgm_emd_tile(int which);
int dgm_emd_parts(int rows, int cols);
size_t dgm_emd_scratch_floats(int b, int n, int m);
int dgm_emd_approx(int b, int n, int m, const float* xyz1, const float* xyz2, float* scratch, float* cost, float* residual,
                   void* stream);

/* ---- cleaning an extracted mesh: components, floaters, compaction (csrc/mesh_clean.hip) ---------------------------------------------
 * Replaces verts_on_largest_mesh (dgmesh/nvdiffrast_utils/dpsr_utils.py:345-368, igl on the host) and pymeshlab's
 * meshing_remove_connected_component_by_* calls (dgmesh/scene/gaussian_model.py:633-650).  verts (V, 3) fp32, faces (F, 3) int32;
 * every buffer is device memory, nothing is allocated and nothing is read back; integers, comparisons and copies only, so every
 * output is bit-reproducible.  A face is VALID iff its three indices are in [0, V) and pairwise different; two vertices are
 * connected when a valid face uses both (through shared vertices, as igl's adjacency_matrix + connected_components).
 *   dgm_mesh_clean_tile: the integers per workgroup of the scans (their fixed partition).
 *   dgm_mesh_cc_label: labels[v] = the smallest vertex index of v's component (a vertex no valid face uses: v itself).  info[0] =
 *       the faces with an index outside [0, V), info[1] = the faces with indices in range of which two are equal; neither kind
 *       connects anything, and no index is used before it is range-checked.  scratch: dgm_mesh_cc_scratch_bytes(V, F) bytes (0
 *       for a negative size), contents irrelevant.  Lock-free union-find by minimum: one hooking launch, one labelling launch.
 *   dgm_mesh_cc_stats: indexed by root (= label): comp_faces (V) valid faces, comp_verts (V) vertices, comp_bbox (V, 6) = (min xyz,
 *       max xyz); an index that is no root gets 0, 0 and (+inf, -inf).  Floats are ordered by their bits (-0 < +0; a NaN beyond
 *       the infinity of its sign).  A label outside [0, V) is skipped.
 *   dgm_mesh_cc_select: keep[f] (F bytes, 0 / 1) = f is valid, and, where largest != 0, its component is the one with the most valid
 *       faces (ties: the smaller label); and, where min_faces > 0, comp_faces >= min_faces; and, where min_diameter_frac > 0,
 *       d2(component) >= (frac * frac) * d2(mesh) with d2(box) = (dx dx + dy dy) + dz dz, d = max - min, all in fp32 without
 *       contraction, the mesh's box being the min / max over the roots' boxes.  scratch: dgm_mesh_cc_select_scratch_bytes() bytes.
 *   dgm_mesh_compact_count: counts[0] = V', the vertices used by a kept face; counts[1] = F', the kept faces (a kept face with an
 *       index outside [0, V) counts as dropped).  The caller reads the two ints back to size the outputs.  scratch:
 *       dgm_mesh_compact_scratch_bytes(V, F) bytes (0 for a negative size), handed on to the emit call unchanged.
 *   dgm_mesh_compact_emit: the survivors in their old order: verts_out (V', 3), faces_out (F', 3) re-indexed, vert_index (V') and
 *       face_index (F') = the old index of each.  Vn, Fn: the counts; nothing is written at or behind them.  NULL outputs are
 *       allowed where a count is 0. */
int dgm_mesh_clean_tile(void);
size_t dgm_mesh_cc_scratch_bytes(int V, int F);
int dgm_mesh_cc_label(int V, int F, const int* faces, char* scratch, int* labels, int* info, void* stream);
int dgm_mesh_cc_stats(int V, int F, const float* verts, const int* faces, const int* labels, int* comp_faces, int* comp_verts,
                      float* comp_bbox, void* stream);
size_t dgm_mesh_cc_select_scratch_bytes(void);
int dgm_mesh_cc_select(int V, int F, const int* faces, const int* labels, const int* comp_faces, const int* comp_verts,
                       const float* comp_bbox, int largest, int min_faces, float min_diameter_frac, char* scratch, unsigned char* keep,
                       void* stream);
size_t dgm_mesh_compact_scratch_bytes(int V, int F);
int dgm_mesh_compact_count(int V, int F, const int* faces, const unsigned char* keep, char* scratch, int* counts, void* stream);
int dgm_mesh_compact_emit(int V, int F, const float* verts, const int* faces, char* scratch, int Vn, int Fn, float* verts_out,
                          int* faces_out, int* vert_index, int* face_index, void* stream);

/* ---- simplifying an extracted mesh: quadric vertex clustering (csrc/mesh_simplify.hip) ------------------------------------------------
 * Uniform-grid vertex clustering with quadric-error placement (Lindstrom 2000); with a tiny cell it is pymeshlab's
 * meshing_merge_close_vertices + meshing_remove_duplicate_faces + meshing_remove_null_faces (dgmesh/scene/gaussian_model.py:603-697).
 * verts (V, 3) fp32, faces (F, 3) int32, cell size h > 0 fp32; every buffer is device memory, nothing is allocated and nothing is
 * read back.  Definitions:
 *   VALID face: indices in [0, V) (range-checked before any use) and pairwise different, all nine coordinates finite; every other
 *       face is dropped.  A vertex is USED when a valid face uses it.
 *   BOX: per axis the min o and the max hi over the used vertices, floats ordered by their bits (-0 < +0), no float arithmetic.
 *   CELLS: n_k = max(1, ceil((hi_k - o_k) / h)), idx_k = min(n_k - 1, floor((x_k - o_k) / h)), fp32 with correctly rounded subtract
 *       and divide, no contraction; n_k <= 2^20; key = (idx_z n_y + idx_y) n_x + idx_x, 64-bit.  The caller computes n from the box
 *       it read back and passes o, n, h to the later calls.
 *   CLUSTERS: the used vertices of one occupied cell; representative = the smallest old vertex index; new vertices are ordered by
 *       representative.  vert_map (V) old -> new, -1 for a vertex no surviving face uses; vert_index new -> representative.
 *   FACES: every valid face remapped; NULL when two new indices coincide, DUPLICATE when a face with a smaller old index has the
 *       same unordered triple; both are dropped, survivors keep their order, face_index new -> old; a cluster left without a face is
 *       dropped.  Winding is kept as remapped (clustering can flip a triangle; not repaired).  The triple is not packed into one
 *       word: there is no limit on the number of clusters.
 *   PLACEMENT (fp64 from the fp32 inputs, no contraction): per cluster with cell centre c = o + (idx + 0.5) h, over the valid faces S
 *       with at least one corner in it, each once, in ascending old face index: n = (p1 - p0) x (p2 - p0), d = -n . (p0 - c),
 *       g = (p0 + p1 + p2) / 3 - c; A = sum n n^T, b = sum n d, xh = (sum g) / |S|; mu = regularization tr(A); mu == 0: x = xh,
 *       otherwise (A + mu I) x = mu xh - b (Cholesky); x clamped per component to [-h, h]; new vertex = fp32(c + x).
 * Every output is bit-reproducible: the per-cluster sums run over an inverted index in ascending face order, no float is added by
 * an atomic.  F <= 2^29.
 *   dgm_mesh_simplify_box: marks valid faces and used vertices in scratch; box (6 floats, device) = (o, hi), (+inf, -inf) without a
 *       valid face.  scratch: dgm_mesh_simplify_scratch_bytes(V, F) bytes (0 for a negative or unsupported size), handed on to the
 *       later calls unchanged.
 *   dgm_mesh_simplify_count (no placement): after _box; the cluster map, rep_faces (F, 3) = every face's corners replaced by their
 *       representatives' OLD indices (-1 for an invalid face), keep (F bytes) = valid, not null, not duplicate, and through
 *       dgm_mesh_compact_count on (rep_faces, keep) counts[0] = V', counts[1] = F'.  compact_scratch:
 *       dgm_mesh_compact_scratch_bytes(V, F) bytes.  May be called again with another h on the same scratch.
 *   dgm_mesh_simplify_place: after _count with the same grid; placed (V, 3) = the new position at every representative's row (other
 *       rows: the old position).  dgm_mesh_compact_emit on (placed, rep_faces, compact_scratch) then gives verts', faces',
 *       vert_index and face_index.
 *   dgm_mesh_simplify_vert_map: after the emit; vert_map (V) from vert_index (Vn). */
size_t dgm_mesh_simplify_scratch_bytes(int V, int F);
int dgm_mesh_simplify_box(int V, int F, const float* verts, const int* faces, char* scratch, float* box, void* stream);
int dgm_mesh_simplify_count(int V, int F, const float* verts, const int* faces, float ox, float oy, float oz, int nx, int ny, int nz,
                            float h, char* scratch, char* compact_scratch, int* rep_faces, unsigned char* keep, int* counts,
                            void* stream);
int dgm_mesh_simplify_place(int V, int F, const float* verts, const int* faces, const int* rep_faces, float ox, float oy, float oz, int nx,
                            int ny, int nz, float h, double regularization, char* scratch, float* placed, void* stream);
int dgm_mesh_simplify_vert_map(int V, int F, int Vn, const int* vert_index, char* scratch, int* vert_map, void* stream);

/* ---- the edge table of a mesh, its topology classes, Taubin / Laplacian smoothing (csrc/mesh_edges.hip) -------------------------------
 * Replaces compute_edges and compute_edge_to_face_mapping (dgmesh/nvdiffrast_utils/mesh.py:97-149, torch.unique) and gives what a
 * host mesh library is otherwise asked for: is the mesh closed, where is its rim, lambda | mu smoothing (Taubin 1995).  faces (F, 3)
 * int32, verts (V, 3) fp32; every buffer is device memory, nothing is allocated and nothing is read back.  Definitions:
 *   VALID face: indices in [0, V) (range-checked before any use) and pairwise different (mesh_clean's definition; coordinates play
 *       no part in topology).  A valid face (a, b, c) TRAVERSES the directed half-edges a->b, b->c and c->a.  A vertex is USED when a
 *       valid face uses it.
 *   ADJACENCY: adj_offset (V + 1) and adj (2 E) int32: adj[adj_offset[v] .. adj_offset[v + 1]) = the distinct vertices that share
 *       a valid face's side with v, ascending; empty for an unused vertex; adj_offset[V] = 2 E.
 *   EDGES: edges (E, 2) int32 = the distinct unordered sides {u, v} of the valid faces as u < v, in lexicographic order: on a mesh
 *       of valid faces what compute_edges returns (torch.unique(dim=0) order).  edge_count (E, 2) int32 = the valid faces that traverse
 *       u->v (column 0) and v->u (column 1); edge_faces (E, 2) int32 = the smallest index among those faces per column, -1 for none
 *       (the reference's table writes 0 there and keeps an arbitrary face where several compete).
 *   CLASSES of an edge from its counts: BOUNDARY, they sum to 1; MISORIENTED, (2, 0) or (0, 2); NON-MANIFOLD, the sum is >= 3;
 *       REGULAR, (1, 1).  adj_kind (2 E) bytes = the class of the edge to each adjacency entry: 0 regular, 1 boundary,
 *       2 non-manifold, 3 misoriented.  vert_flag (V) bytes: bit 0 used, bit 1 on a boundary edge, bit 2 on a non-manifold or
 *       misoriented edge.
 *   SMOOTHING STEP with factor f on vertex i with neighbour set N: m = (the sum of in[n], n in N, in fp64, starting from 0, in
 *       ascending n) / (double)|N|, out[i] = (float)(x + f (m - x)) with x = (double)in[i], per coordinate, no contraction: one
 *       rounding to fp32.  Copied unchanged: a vertex with a non-finite coordinate, one with an empty N, and with boundary = 0 (FIXED)
 *       a vertex with flag bit 1.  boundary = 1 (CURVE): for a vertex with flag bit 1, N is restricted to the neighbours it is joined
 *       to by a boundary edge; boundary = 2 (FREE): no distinction.  A non-finite NEIGHBOUR is not left out: its vertex's sum, and
 *       with it that output row, becomes non-finite by the rules of IEEE arithmetic.
 * Every output is bit-reproducible: integer atomics hand out counts and places only, every list is then ordered by ranking, no
 * float is added by an atomic.  F <= 2^28.
 *   dgm_mesh_edges_count: builds the sorted lists in scratch; adj_offset (V + 1), vert_flag (V) and info (8 ints) = E, boundary edges,
 *       non-manifold edges, misoriented edges, regular edges, used vertices, valid faces, 2 E.  The caller reads info back to size
 *       the outputs of the emit call.  scratch: dgm_mesh_edges_scratch_bytes(V, F) bytes (0 for a negative or unsupported size),
 *       handed on to the emit call unchanged.
 *   dgm_mesh_edges_emit: after _count on the same scratch and adj_offset, E = info[0]; writes adj (2 E), adj_kind (2 E), edges,
 *       edge_faces and edge_count ((E, 2) each); any of them may be NULL and is then left out; nothing is written at or behind E
 *       rows or 2 E entries.
 *   dgm_mesh_smooth_step: one step verts_in -> verts_out (different buffers), A = the entries of adj; adj_kind is read with
 *       boundary = 1 only.  An adjacency offset outside [0, A] or a neighbour outside [0, V) copies its vertex unchanged.  A Taubin
 *       iteration is two calls, f = lambda and then f = mu. */
size_t dgm_mesh_edges_scratch_bytes(int V, int F);
int dgm_mesh_edges_count(int V, int F, const int* faces, char* scratch, int* adj_offset, unsigned char* vert_flag, int* info, void* stream);
int dgm_mesh_edges_emit(int V, int F, char* scratch, int E, const int* adj_offset, int* adj, unsigned char* adj_kind, int* edges,
                        int* edge_faces, int* edge_count, void* stream);
int dgm_mesh_smooth_step(int V, int A, const float* verts_in, const int* adj_offset, const int* adj, const unsigned char* adj_kind,
                         const unsigned char* vert_flag, double factor, int boundary, float* verts_out, void* stream);

/* ---- mesh repair: a consistent, outward orientation per body and hole filling (csrc/mesh_repair.hip) ------------------------------------
 * The last stage of the reference's mesh clean-up (pymeshlab meshing_close_holes, trimesh fill_holes, fix_inversion, fix_normals;
 * dgmesh/scene/gaussian_model.py:652-691).  verts (V, 3) fp32, faces (F, 3) int32; every buffer is device memory, nothing is allocated
 * and nothing is read back.  Both parts read the sorted lists that dgm_mesh_edges_count(V, F, faces, edges_scratch, ...) left in
 * edges_scratch, for the SAME V, F and faces.  VALID faces, half-edges and edge classes are those of the edge table above; an
 * invalid face is passed through and never flipped.  Everything is decided by integers: bit-reproducible.  F <= 2^28.
 *   ADJACENT: two valid faces that share an edge which exactly two valid faces traverse; with counts (1, 1) they AGREE, with (2, 0)
 *       or (0, 2) they DISAGREE.  Boundary and non-manifold edges connect nothing.  COMPONENTS are those of this adjacency; the
 *       label of a component is its smallest face.  A component is ORIENTABLE when flips can make every connecting edge agree, CLOSED
 *       when every half-edge of its faces lies on a connecting edge.
 *   ORIENTATION: a non-orientable component is left as it is.  An orientable one has two consistent orientations, K (keeps its
 *       smallest face) and the opposite.  The OPEN RULE takes the one that flips fewer faces, K on a tie.  With `outward`, a closed
 *       component whose signed volume sum in orientation K is not 0 takes K when the sum is positive and the opposite when negative
 *       (counted in "components inverted"); every other component takes the open rule.  Nested inner shells are turned outward too.
 *       A flipped face (a, b, c) becomes (a, c, b).
 *   SIGNED VOLUME: lo, hi = the fp32 box of the used vertices, e = the smallest integer with 2^e >= the longest side (fp64 hi - lo);
 *       per face in orientation K, p, q, r = the fp64 corners minus fp64 lo,
 *       det = px (qy rz - qz ry) - py (qx rz - qz rx) + pz (qx ry - qy rx) in that order without contraction, term = llrint(det
 *       2^(30 - 3 e)) (round half even; |term| <= 6 2^30), 0 for a non-finite det; the component's sum is int64 (< 2^61).  A box that
 *       is not finite or has no extent (or no used vertex) skips the volume rule for the whole mesh: "outward skipped" = 1.
 *   dgm_mesh_orient: faces_out (F, 3) (not `faces` itself), flipped (F) bytes, info (8 ints) = components, closed components,
 *       unorientable components, faces flipped, components inverted, outward skipped, 0, 0.  scratch:
 *       dgm_mesh_orient_scratch_bytes(V, F) bytes (0 for a negative or unsupported size).
 *   BOUNDARY HALF-EDGE: the directed side a->b that the single valid face of a boundary edge traverses -- reversed where `flipped`
 *       (NULL: nothing is) marks that face, so the table of the unflipped faces serves the oriented mesh.  Its index is the rank of
 *       its edge among the boundary edges in the edge table's order; B = info[1] of dgm_mesh_edges_count.  A vertex is SIMPLE when
 *       exactly one boundary half-edge leaves it and exactly one arrives; next(a->b) = the boundary half-edge leaving b when b is
 *       simple.  A HOLE is a closed cycle of next of n <= max_hole_edges half-edges (always n >= 3); its LEADER is its smallest
 *       half-edge.  Longer cycles are counted ("holes too long"), as are the half-edges of chains that end at a vertex that is not
 *       simple ("edges on open chains"); both are left open.
 *   FILL: n == 3: one face (b, a, c') from the leader a->b and c' the head of its next.  n >= 4: one new vertex, (float)((the sum of
 *       the rim vertices in fp64 from 0, in loop order from the leader's tail) / (double)n), and one face (b, a, new vertex) per
 *       half-edge a->b.  New vertices follow the V given ones in leader order, new faces follow the F given ones in half-edge order.
 *   dgm_mesh_fill_count: info (8 ints) = boundary edges, holes filled, holes too long, edges on open chains, vertices added, faces
 *       added, 0, 0; the caller reads it back to size the outputs.  scratch: dgm_mesh_fill_scratch_bytes(V, B) bytes, handed on to
 *       the emit call unchanged.
 *   dgm_mesh_fill_emit: verts_out (V + nv, 3) and faces_out (F + nf, 3) = the given rows (`faces` may be the oriented faces), then
 *       the new ones; nothing is written at or behind V + nv and F + nf rows. */
size_t dgm_mesh_orient_scratch_bytes(int V, int F);
int dgm_mesh_orient(int V, int F, const float* verts, const int* faces, char* edges_scratch, char* scratch, int outward, int* faces_out,
                    unsigned char* flipped, int* info, void* stream);
size_t dgm_mesh_fill_scratch_bytes(int V, int B);
int dgm_mesh_fill_count(int V, int F, int B, const float* verts, char* edges_scratch, const unsigned char* flipped, int max_hole_edges,
                        char* scratch, int* info, void* stream);
int dgm_mesh_fill_emit(int V, int F, int B, const float* verts, const int* faces, char* scratch, int nv, int nf, float* verts_out,
                       int* faces_out, void* stream);

/* ---- inside / outside: the generalised winding number of query points (csrc/mesh_inside.hip) ------------------------------------------
 * What answers whether a point is inside a mesh (mesh_inside.py: contains, signed_distance, occupancy_grid, volume_iou).  points
 * (N, 3), verts (V, 3) fp32, faces (F, 3) int32; every buffer is device memory, nothing is allocated and nothing is read back.
 * WINDING NUMBER.  For query p and a face with corners v0, v1, v2, all in fp32 without contraction, a = v0 - p, b = v1 - p, c = v2 - p:
 *       det = a . (b x c),  den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|,  omega = 2 atan2(det, den)  (van Oosterom and Strackee),
 *       w(p) = (1 / 4 pi) sum over the faces of omega -- the order of every operation is written out at the head of
 *       csrc/mesh_inside.hip; the lengths come from the hardware's square root (within 1 ulp), atan2 is the device library's atan2f.  1 inside a closed mesh wound outwards, 0 outside, -1 inside one wound inwards; the sum over nested or
 *       overlapping shells; a fraction near an open rim.  A face adds exactly 0 when one of its indices lies outside [0, V) (checked
 *       before any use), when a corner coordinate is not finite, or when det is exactly 0 or not finite: a face with b = c or three
 *       equal corners, and the arbitrary +-2 pi of atan2(+-0, negative) for a query in a face's plane (another face without area has
 *       a det of rounding noise and adds about as little).  A query with a non-finite coordinate gets NaN.  On
 *       the surface itself the value is unspecified but finite.  V = 0 or F = 0: w = 0.  N = 0: nothing is done.
 * SUMMATION ORDER.  Faces in index order; omega is added in fp32, from 0, within a chunk of 256 faces; the chunk sums are added in
 *       fp64, in order, within a slice of 64 chunks (16384 faces); the slice sums are added in fp64, in order; w = (float)(sum / (4 pi)),
 *       one rounding.  The structure is a function of F alone: a query's w is the same bit pattern whether it is asked alone or
 *       among others, and from run to run; a caller may split N into batches freely.  No atomics.
 *   dgm_wind_scratch_bytes: N * ceil(F / 16384) * 8, the fp64 slice sums (0 for a negative size).
 *   dgm_wind_number: w (N) fp32.  scratch: dgm_wind_scratch_bytes(N, F) bytes, 8-byte aligned, contents irrelevant; not touched (and
 *       may be NULL) when F <= 16384.  N x slices beyond 2^31 - 1 workgroups of 256 queries is refused: split N. */
size_t dgm_wind_scratch_bytes(int N, int F);
int dgm_wind_number(int N, int V, int F, const float* points, const float* verts, const int* faces, char* scratch, float* w, void* stream);

/* ---- ray casting against a triangle mesh: nearest hit, any hit (csrc/mesh_ray.hip) ---------------------------------------------------
 * What answers what a ray hits first (mesh_ray.py: ray_cast, occluded, visible, depth_map, ambient_occlusion).  origins, dirs (N, 3),
 * verts (V, 3) fp32, faces (F, 3) int32; every buffer is device memory, nothing is allocated and nothing is read back.
 * PAIR TEST.  The watertight test of Woop, Benthin and Wald (JCGT 2013) in fp32 without contraction, / correctly rounded: with kz the
 *       axis of largest |d| (ties: the lowest index), kx = kz + 1, ky = kx + 1 (mod 3), swapped when d[kz] < 0, Sx = d[kx] / d[kz],
 *       Sy = d[ky] / d[kz], Sz = 1 / d[kz], and per corner a = v - o, Ax = a[kx] - Sx a[kz], Ay = a[ky] - Sy a[kz], Az = Sz a[kz]:
 *       U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax; when one of them is exactly 0 all three are taken again in fp64 from
 *       the fp32 sheared coordinates (exact products, exact signs; the sign test reads the fp64 values, then they are rounded to
 *       fp32); a miss when one is < 0 and one > 0; det = (U + V) + W, a miss when det == 0; t = ((U Az + V Bz) + W Cz) / det,
 *       accepted when t_min <= t < t_max and t is finite; bary = (U, V, W) / det.  The order of every operation is written out at the
 *       head of csrc/mesh_ray.hip.  Seen from the two faces of a shared edge the edge's value is one number and its exact negation,
 *       and a zero counts for both: no ray slips between faces that share an edge or a vertex.  d is not normalised: t is in units
 *       of |d|.
 * ANSWER.  The lexicographic minimum of (t, face index) over the accepted faces: independent of the visiting order, of the batch and
 *       of the run.  None: face = -1, t = +inf, bary = 0.  Never accepted: a face with an index outside [0, V) (checked before any
 *       use) or a non-finite corner coordinate.  A ray with a non-finite component or d = 0 gets the miss answer.  F = 0 or V = 0:
 *       misses everywhere.  N = 0: nothing is done.  t_max <= t_min or a NaN bound: misses everywhere.
 * TWO PATHS.  accel = NULL: a tiled brute force, N x F pairs.  accel = the structure dgm_ray_build made of the same verts and faces: the
 *       faces sorted by the Morton code of their centroid, one box per chunk of 256; a workgroup of 256 rays tests only the chunks
 *       whose box one of its rays may hit.  The box test rejects only what the pair test cannot accept (the argument is at the head
 *       of csrc/mesh_ray.hip), and the candidates carry their original index: face, t and bary are the brute force's bit for bit.
 *   dgm_ray_accel_bytes: ceil(F / 256) * (256 * 48 + 32), a function of F alone (0 for a negative or unsupported size).
 *   dgm_ray_build_scratch_bytes: the build's scratch (0 for a negative or unsupported size); contents irrelevant, any alignment.
 *   dgm_ray_build: writes every byte of accel (16-byte aligned).  F = 0 does nothing.  Deterministic.
 *   dgm_ray_cast: face (N) int32, t (N) fp32, bary (N, 3) fp32.  accel NULL or 16-byte aligned.  ceil(N / 256) workgroups, which an
 *       int N keeps inside the grid limit.  F up to 2^31 - 257.
 *   dgm_ray_occluded: hit (N) bytes, 1 where at least one face is accepted (= face >= 0 of dgm_ray_cast), else 0. */
size_t dgm_ray_accel_bytes(int F);
size_t dgm_ray_build_scratch_bytes(int F);
int dgm_ray_build(int V, int F, const float* verts, const int* faces, char* scratch, char* accel, void* stream);
int dgm_ray_cast(int N, int V, int F, const float* origins, const float* dirs, float t_min, float t_max, const float* verts, const int* faces,
                 const char* accel, int* face, float* t, float* bary, void* stream);
int dgm_ray_occluded(int N, int V, int F, const float* origins, const float* dirs, float t_min, float t_max, const float* verts,
                     const int* faces, const char* accel, unsigned char* hit, void* stream);

/* ---- closest point on a triangle mesh, interpolation, correspondence colours (csrc/surface.hip) -------------------------------------
 * What carries a surface point from one frame's mesh onto another's (correspondence.py).  verts (V, 3) fp32, faces (F, 3) int32;
 * every buffer is device memory, nothing is allocated and nothing is read back.
 *   dgm_surf_closest: per query point (N, 3) the closest point of the mesh as face (N) int32, d2 (N) fp32 = its squared distance and
 *       bary (N, 3) fp32 = ((1 - v) - w, v, w).  Per (point, face) pair Ericson's region test in fp32 without contraction, in the
 *       order written out at the head of csrc/surface.hip; the answer is the lexicographic minimum of (d2, face index) over the
 *       faces with d2 < max_d2 (strict), none: face = -1, d2 = +inf, bary = 0.  Never chosen: a face with an index outside [0, V),
 *       one whose fp32 normal length is not positive and finite, a NaN d2.  Bit-reproducible.  Finite max_d2: a hashed grid over
 *       the faces in scratch, dgm_surf_closest_scratch_bytes(N, F) bytes (0 for a negative size; unused for max_d2 = +inf, may
 *       then be NULL); max_d2 = +inf: a tiled brute force.
 *   dgm_surf_interp: out (N, C) = (attr[i0] b0 + attr[i1] b1) + attr[i2] b2 per channel, attr (V, C) fp32, (i0, i1, i2) the
 *       corners of face[n], b = bary[n]; a row whose face is outside [0, F) or has an index outside [0, V) is `fill`.
 *   dgm_corr_palette: out (N, 3) = the colour of position xyz (N, 3): u = clamp(((x - center) / scale) 0.5 + 0.5, 0, 1) per axis,
 *       center (3) and scale (1) fp32 in DEVICE memory; mode 0: u; mode 1: u times 0.55 where
 *       floor(u_x cells) + floor(u_y cells) + floor(u_z cells) is odd (1 <= cells <= 4096); a row with a NaN: (1, 0, 1). */
size_t dgm_surf_closest_scratch_bytes(int N, int F);
int dgm_surf_closest(int N, int V, int F, const float* points, const float* verts, const int* faces, float max_d2, char* scratch,
                     int* face, float* d2, float* bary, void* stream);
int dgm_surf_interp(int N, int V, int F, int C, const float* attr, const int* faces, const int* face, const float* bary, float fill,
                    float* out, void* stream);
int dgm_corr_palette(int N, const float* xyz, const float* center, const float* scale, int mode, int cells, float* out, void* stream);

/* ---- dataset ingest: PNG unfiltering and compositing over the background (csrc/ingest.hip) -------------------------------------------
 * Replaces PIL's decoder and the numpy compositing of readCamerasFromTransforms + PILtoTorch (dgmesh/scene/dataset_readers.py:288-302,
 * dgmesh/utils/general_utils.py:23-29).  Every buffer but bg3 is device memory; nothing is allocated and nothing is read back.
 *   dgm_png_unfilter: `filtered` holds B inflated IDAT streams of 8-bit, non-interlaced images of one W, H and channels (3: colour type
 *       2, 4: colour type 6, 1: 8-bit grey or palette, or the packed rows of a 1-, 2- or 4-bit image with W = the row's bytes, whose
 *       filters work on bytes), back to back: each H rows of 1 + W channels bytes, the first byte of a row its filter type 0..4 (None,
 *       Sub, Up, Average with floor((a + b) / 2), Paeth with the specification's tie order; arithmetic mod 256 per byte, neighbours
 *       `channels` bytes apart).  out (B, H, W, channels) uint8, 4-byte aligned unless channels is 1.  A filter type above 4 is read as 0: the caller checks
 *       the type bytes before the upload.  One workgroup per image, one lane per row, rows skewed by one pixel; the trip counts are
 *       uniform and no thread waits on memory.  1 <= W, H <= 2^24; offsets are 64-bit.
 *   dgm_image_ingest: in (B, H, W, C) uint8, C 3 or 4 (C = 3: alpha 255); bg3 a HOST array of three floats.  In fp64 and in this
 *       order, without contraction: n = byte / 255.0, v = (n_c n_a + bg (1 - n_a)) 255.0, q = v truncated to a byte; then
 *       image (B, 3, H, W) = (float)q / 255.0f correctly rounded, and mask (B, H, W, 1) = (float)n_a.  1 <= B <= 65535.  image and
 *       mask are 4-byte aligned; `in` is 4-byte aligned for C = 4 and may start at any byte for C = 3.
 *   dgm_png_expand: packed (B, H, ceil(W depth / 8)) bytes, the unfiltered rows of a grey or palette image of bit depth 1, 2, 4 or 8
 *       -> out (B, H, W) bytes, one per pixel: the sample (most significant bits first; a row's padding bits are not read) times
 *       `scale`.  Pillow scales grey samples by 255, 85, 17, 1 for depths 1, 2, 4, 8 and leaves palette indices alone (scale 1);
 *       scale (2^depth - 1) <= 255.  1 <= B <= 65535.
 *   dgm_image_ingest_masked: the real captures' compositing (readNerfiesCameras / readiPhoneCameras / readNeuralActorCameras,
 *       dgmesh/scene/dataset_readers.py:545-865).  in (B, H, W, C) uint8, C 3 or 4 (a fourth channel is dropped); mask (B, H, W, Cm)
 *       uint8, Cm 1, 3 or 4, of which channel 0 counts: m = mask[..., 0] > 0.  q_c = m ? in_c : the background byte, which is
 *       dgm_image_ingest's q for alpha 0 (255 bg truncated).  flags 0: image (B, 3, H, W) = (float)q / 255.0f correctly rounded,
 *       alpha (B, H, W, 1) = m as 0 / 1; bytes_out unused.  DGM_INGEST_BYTES: bytes_out (B, H, W, 4) = (q_R, q_G, q_B, 255 m), the
 *       input of a `resolution` resize (dgm_resample with DGM_RESAMPLE_PLANES); image and alpha unused.  The unused outputs may be NULL.
 *       Outputs 4-byte aligned; `in` 4-byte aligned for C = 4; mask at any byte. */
#define DGM_INGEST_BYTES 1
int dgm_png_unfilter(int B, int W, int H, int channels, const unsigned char* filtered, unsigned char* out, void* stream);
int dgm_image_ingest(int B, int H, int W, int C, const unsigned char* in, const float* bg3, float* image, float* mask, void* stream);
int dgm_png_expand(int B, int W, int H, int depth, int scale, const unsigned char* packed, unsigned char* out, void* stream);
int dgm_image_ingest_masked(int B, int H, int W, int C, const unsigned char* in, int Cm, const unsigned char* mask, const float* bg3, int flags,
                            float* image, float* alpha, unsigned char* bytes_out, void* stream);

/* ---- image resampling: Pillow's 8-bit Image.resize on the device (csrc/resample.hip, csrc/ingest.hip) -----------------------------
 * Replaces image.resize(..., LANCZOS) of readCamerasFromTransforms (dgmesh/scene/dataset_readers.py:289) and the bicubic
 * image.resize of PILtoTorch (dgmesh/utils/general_utils.py:23-29).  The arithmetic is Pillow's, in integers: every output byte is
 * clamp((2^21 + sum_k pixel[min + k] coeff[k]) >> 22, 0, 255) with an int32 accumulator and an arithmetic shift; a horizontal
 * pass, a byte intermediate, a vertical pass.  The host computes the fixed-point coefficients (resample.coefficients).
 *   dgm_image_composite_bytes: dgm_image_ingest's q (above) as bytes: out (B, H, W, 4) = (q_R, q_G, q_B, a), a = 255 for C = 3.
 *       Same limits as dgm_image_ingest; out is 4-byte aligned.
 *   dgm_resample: in (B, H, W, C) uint8, C 1, 3 or 4 -> (B, oh, ow, C).  All sizes within [1, 2^20], 1 <= B <= 65535.
 *       Horizontal pass (run when kx != NULL; then ow may differ from W, otherwise ow == W): kx (ksize_x, owp) int32 with
 *       owp = ow rounded up to a multiple of 4 -- tap-major, so that neighbouring lanes read neighbouring words -- and
 *       bounds_x (2, owp) int32: row 0 the first input column of every output column, row 1 its tap count.  Taps past the count and
 *       the padding columns are zero.  kx and bounds_x are 16-byte aligned.
 *       Vertical pass (run when ky != NULL; otherwise oh == H): ky (oh, ksize_y) int32, bounds_y (oh, 2) int32 = (first input row,
 *       tap count) of every output row.  At least one pass must run.  Input indices read from the tables are clamped into the
 *       image and counts to ksize, so no table content can make the kernels read outside `in`.
 *       tmp: (B, H, ow, C) bytes, used (and required) only when both passes run.
 *       flags: DGM_RESAMPLE_PREMULTIPLIED (C = 4 only): colour bytes are premultiplied by alpha as the first pass loads them,
 *       c' = ((t >> 8) + t) >> 8 with t = c a + 128, and divided out as the last pass stores them: unchanged for a = 0 or 255,
 *       otherwise min(255, 255 c' / a) in integers.  DGM_RESAMPLE_PLANES (C = 3 or 4): the last pass writes image (B, 3, oh, ow) =
 *       (float) byte / 255.0f, correctly rounded, and mask (B, oh, ow, 1) = (float) ((double) a / 255.0) (1 for C = 3) instead of
 *       out_bytes (B, oh, ow, C).  The unused one of out_bytes and (image, mask) may be NULL.  in, tmp and out_bytes are 4-byte
 *       aligned for C = 4 and may start at any byte otherwise; image and mask are 4-byte aligned.
 *   dgm_resample_nearest: Pillow's NEAREST, which Image.resize substitutes for any filter on modes P and 1: out (B, oh, ow, C) =
 *       in[b][ys[y]][xs[x]], xs (ow) and ys (oh) int32 device tables of source indices, computed on the host as Pillow's affine
 *       scaler walks an axis (resample.nearest_indices): in float64 the coordinate starts at 0.5 in / out, in / out is added per output
 *       pixel, and each index is the running sum truncated; indices are clamped into the image.  C 1, 3 or 4; sizes as dgm_resample. */
#define DGM_RESAMPLE_PREMULTIPLIED 1
#define DGM_RESAMPLE_PLANES 2
int dgm_image_composite_bytes(int B, int H, int W, int C, const unsigned char* in, const float* bg3, unsigned char* out, void* stream);
int dgm_resample(int B, int H, int W, int C, const unsigned char* in, int oh, int ow, const int* kx, const int* bounds_x, int ksize_x,
                 const int* ky, const int* bounds_y, int ksize_y, int flags, unsigned char* tmp, unsigned char* out_bytes, float* image,
                 float* mask, void* stream);
int dgm_resample_nearest(int B, int H, int W, int C, const unsigned char* in, int oh, int ow, const int* xs, const int* ys,
                         unsigned char* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DGMESH_HIP_H */
