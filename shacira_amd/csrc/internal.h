// internal.h -- declarations shared between the translation units of libshacira_hip.so (not part of the ABI).
#pragma once

#include <atomic>
#include <mutex>

#include "hashgrid_device.h"

namespace shacira {

// hipFuncSetAttribute (the opt-in for > 64 KiB of dynamic LDS) is a per-DEVICE setting: the opt-ins run once for every
// device this process launches on (the current device must be the one the caller's stream belongs to; the PyTorch
// wrappers enter `torch.cuda.device(tensor.device)` around every call).
constexpr int kMaxDevices = 64;
struct PerDeviceOnce {
    std::once_flag flag[kMaxDevices];
    hipError_t err[kMaxDevices] = {};
    template <typename Fn> hipError_t run(Fn &&fn) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
        std::call_once(flag[dev], [&] { err[dev] = fn(); });
        return err[dev];
    }
};

// hashgrid_fwd.hip
// `caller_plan`: the call brings a plan buffer of its own, so the workspace holds none
size_t hashgrid_forward_workspace(int dim, int dtype, const LevelTable &lt, int64_t n, bool caller_plan = false);
hipError_t hashgrid_forward_dispatch(int dim, int dtype, const LevelTable &lt, const int32_t *first_idx,
                                     const float *coords, const void *table, void *feats, void *workspace, int64_t n,
                                     hipStream_t s, void *plan = nullptr, bool plan_ready = false);
// levels [lt.level_begin, lt.level_end) of the level-per-XCD pair kernel into a level-major staging buffer [L][N][F]
hipError_t hashgrid_forward_levels_staged(int dim, int dtype, const LevelTable &lt, const int32_t *first_idx,
                                          const float *coords, const void *table, void *staged, int64_t n,
                                          hipStream_t s);
// coarse levels [0, lc) over cell-sorted coordinates + assembly of whole feature rows through perm
hipError_t hashgrid_forward_rows(int dim, int dtype, const LevelTable &lt, const int32_t *first_idx, const float *sorted4,
                                 const void *table, const void *staged, void *feats, int64_t n, int lc, hipStream_t s);
// hashgrid_tiled.hip: cell-sorted ("tiled") forward for large batches
bool tiled_supported(int dim, int dtype, const LevelTable &lt, int64_t n);
size_t tiled_forward_workspace(int dim, int dtype, const LevelTable &lt, int64_t n, bool caller_plan = false);
// `plan`: caller-owned plan buffer (sample_plan_bytes) the sort writes into, NULL = inside the workspace; `plan_ready`: it
// already holds this batch's plan (the sort is skipped)
hipError_t tiled_forward(int dim, int dtype, const LevelTable &lt, const int32_t *first_idx, const float *coords,
                         const void *table, void *feats, void *workspace, int64_t n, hipStream_t s, void *plan = nullptr,
                         bool plan_ready = false);
// The PLAN of a coordinate batch: its samples counting-sorted by spatial block (16-byte records {x, y, z, sample index}) and
// the blocks' offsets -- what the cell-sorted forward computes first and the backward's brick pass walks again. A function
// of (dim, n, coords) only; (dim, n) fix its layout and block grid.
struct SortedBatch {
    const float4 *sorted4;        // [n]
    const uint32_t *block_start;  // [num_blocks + 1]
    uint32_t num_blocks;
    int32_t nb[3];                // blocks per axis; block id = qx + nb[0] * (qy + nb[1] * qz)
};
size_t sample_plan_bytes(int dim, int64_t n);
size_t sample_plan_scratch_bytes(int dim, int64_t n);
hipError_t sample_plan_build(int dim, const float *coords, int64_t n, void *plan, void *scratch, hipStream_t s);
void sample_plan_view(int dim, int64_t n, const void *plan, SortedBatch &out);
void sample_plan_grid(int dim, int64_t n, SortedBatch &out);   // block grid only (no buffer)
hipError_t hashgrid_debug_corners(int dim, const LevelTable &lt, const float *coords, int64_t n, int32_t *idx, float *w,
                                  hipStream_t s);
// hashgrid_coord_grad.hip: grad_coords [n, dim] fp32 (overwritten); `plan`: the batch's plan or NULL
hipError_t hashgrid_coord_grad_dispatch(int dim, int dtype, const LevelTable &lt, const int32_t *first_idx,
                                        const float *coords, const void *table, const void *grad_out,
                                        float *grad_coords, int64_t n, hipStream_t s, const void *plan);
// hashgrid_coord_grad2.hip: the backward of the call above for `vv` = dL/dgrad_coords [n, dim]; NULL outputs are not computed
// (ggo [n, L * F] of the table's dtype, grad_table [table_rows, F] overwritten -- fp16: accumulated in `workspace` --,
// grad_coords [n, dim] fp32)
hipError_t hashgrid_coord_grad2_dispatch(int dim, int dtype, const LevelTable &lt, const int32_t *first_idx,
                                         const float *coords, const void *table, const void *grad_out, const float *vv,
                                         void *ggo, void *grad_table, float *grad_coords, void *workspace, int64_t n,
                                         hipStream_t s, const void *plan);
// hashgrid_bwd.hip
hipError_t zero_fill_async(float *p, int64_t n, hipStream_t s);   // zero fill as a kernel (graph-capture safe)
size_t hashgrid_backward_workspace(int dim, int dtype, const LevelTable &lt, int64_t n);
// ... of a call that brings the batch's plan (whole level range; 16-byte aligned grad_output or not)
size_t hashgrid_backward_workspace_planned(int dim, int dtype, const LevelTable &lt, int64_t n, bool grad_aligned);
hipError_t hashgrid_backward_dispatch(int dim, int dtype, const LevelTable &lt, const int32_t *first_idx,
                                      const float *coords, const void *grad_out, void *grad_table, void *workspace,
                                      size_t workspace_bytes, int64_t n, hipStream_t s, const void *plan, bool *too_small);

// triplane.hip: the planes of one call, by value in the kernel arguments ([3 * l + p], p = 0 fmx, 1 fmy, 2 fmz)
struct TriplaneArgs {
    const float *plane[3 * SHACIRA_TRIPLANE_MAX_LODS];   // NCHW [fdim, side, side] each
    float *grad[3 * SHACIRA_TRIPLANE_MAX_LODS];          // backward: the same shapes (overwritten)
    int64_t hwc_off[3 * SHACIRA_TRIPLANE_MAX_LODS];      // forward, HWC layout: plane offsets in the workspace (floats)
    int32_t side[SHACIRA_TRIPLANE_MAX_LODS];             // 2^lod + 1 texels
    int32_t num_lods;
    int32_t fdim;
};
// the plane backward's sort and windows (a function of the shape, built on the host)
struct TriBwdPlan {
    int32_t nb, nbins;        // blocks per cube axis, nb^3
    int32_t sort_side;        // texels a side of the finest LOD (the sort's coordinate frame)
    int32_t cells;            // its cells per block edge
    int32_t sum;              // grad_output is [N, 3F] ('sum') or [N, L * 3F]
    int32_t win[SHACIRA_TRIPLANE_MAX_LODS];   // window side per LOD in texels, 0 = no LDS window (global adds)
};
constexpr int kTriDefaultHwc = 1;   // forward layout rule (option triplane_layout = -1), profiles/triplane.md
size_t triplane_forward_workspace(const TriplaneArgs &a, int64_t n);
hipError_t triplane_forward_dispatch(TriplaneArgs a, const float *coords, int sum, float *feats, void *workspace,
                                     int64_t n, hipStream_t s);
void triplane_backward_plan(const TriplaneArgs &a, int sum, TriBwdPlan &bp);
size_t triplane_backward_workspace(const TriplaneArgs &a, int sum, int64_t n);
// planes: write the plane gradients; grad_coords != NULL: the coordinate gradient (reads a.plane)
hipError_t triplane_backward_dispatch(const TriplaneArgs &a, const float *coords, const float *grad_out, int sum,
                                      bool planes, float *grad_coords, void *workspace, int64_t n, hipStream_t s);

// octree.hip: the levels of one call, by value in the kernel arguments
struct OctreeArgs {
    const float *table[SHACIRA_OCTREE_MAX_LEVELS];      // [rows + 1, fdim]
    float *grad[SHACIRA_OCTREE_MAX_LEVELS];             // backward: the same shapes (overwritten)
    const uint2 *corner[SHACIRA_OCTREE_MAX_LEVELS];     // per 32 lattice keys {bits, rows before}
    const uint32_t *occ[SHACIRA_OCTREE_MAX_LEVELS];     // cell bits
    int64_t rows[SHACIRA_OCTREE_MAX_LEVELS];            // corner rows C (the padding row not counted)
    int32_t level[SHACIRA_OCTREE_MAX_LEVELS];
    int32_t num_levels;
    int32_t fdim;
};
// the feature backward's sort and LDS windows (a function of the shape, built on the host)
struct OctBwdPlan {
    int32_t fine;             // the finest level of the call (the sort's cell frame)
    int32_t cells_log2;       // log2 of a block's edge in cells of that level
    int32_t nb, nbins;        // blocks per axis, nb^3
    int32_t sum;              // grad_output is [N, F] ('sum') or [N, L * F]
    int32_t wside[SHACIRA_OCTREE_MAX_LEVELS];   // window side per level in lattice points, 0 = no window (global adds)
    int32_t woff[SHACIRA_OCTREE_MAX_LEVELS];    // its offset in LDS (floats)
    int32_t wtotal;           // floats of LDS
};
void octree_backward_plan(const OctreeArgs &a, int sum, OctBwdPlan &bp);
size_t octree_backward_workspace(const OctreeArgs &a, int sum, int64_t n);
hipError_t octree_forward_dispatch(const OctreeArgs &a, const float *coords, int sum, float *feats, int64_t n,
                                   hipStream_t s);
// features: write the table gradients; grad_coords != NULL: the coordinate gradient (reads a.table)
hipError_t octree_backward_dispatch(const OctreeArgs &a, const float *coords, const float *grad_out, int sum,
                                    bool features, float *grad_coords, void *workspace, int64_t n, hipStream_t s);

// mesh_sdf.hip: signed distance of n points to t triangles (0 <= n, t < 2^31, checked by the entry point)
size_t mesh_sdf_workspace(int64_t n, int64_t t);
hipError_t mesh_sdf_dispatch(int64_t n, int64_t t, const float *points, const float *tris, float *sdf, void *workspace,
                             hipStream_t s);
// the same with the winner: distance, closest point and triangle index (flags validated by the entry point)
size_t mesh_closest_workspace(int64_t n, int64_t t);
hipError_t mesh_closest_dispatch(int64_t n, int64_t t, const float *points, const float *tris, bool is_signed, float *dist,
                                 float *hit, int32_t *tidx, void *workspace, hipStream_t s);

// mesh_voxelize.hip: t triangles into the occupancy words of `level` (and the byte grid when grid != NULL); arguments checked by
// the entry point. Synchronises the stream once per pass of triangles (the host reads the pass's unit count)
size_t mesh_voxelize_workspace(int64_t t);
hipError_t mesh_voxelize_dispatch(int64_t t, const float *tris, int level, float margin, uint32_t *words, uint8_t *grid,
                                  void *workspace, hipStream_t s);

// mesh_sample.hip: n samples on, near or around a mesh, each a function of (seed, index), optionally only those inside the
// occupied cells of one octree level (arguments checked by the entry points; by value in the kernel arguments)
struct MeshSampleArgs {
    int32_t mode;                 // SHACIRA_MESH_SAMPLE_*
    uint32_t key0, key1;          // the seed's low and high word
    uint32_t segment;
    int64_t n, index_base;
    const uint32_t *words;        // [n, 8] or NULL
    int64_t num_triangles;
    const float *triangles;       // [T, 3, 3]
    const uint32_t *cdf;          // [T]
    float sigma;
    int32_t samples_per_cell, cell_level;
    const int16_t *corners;       // [C, 3]
    const uint32_t *occupancy;    // packed words of occupancy_level or NULL (no filter)
    int32_t occupancy_level;
};
hipError_t mesh_sample_count_dispatch(const MeshSampleArgs &a, int32_t *block_counts, hipStream_t s);
// block_offsets == NULL: sample i to row i; else the kept samples to block_offsets[i / 256] + rank within the block
hipError_t mesh_sample_write_dispatch(const MeshSampleArgs &a, const int64_t *block_offsets, float *points, float *normals,
                                      int32_t *face_idx, int64_t *source_idx, hipStream_t s);

// ssim.hip: structural similarity of two [H, W, cin] fp32 images over their first C channels (arguments checked by the entry
// points). Forward: value[0] fp64, map [H, W, C] or NULL; backward: grad_x [H, W, cin] for the device scalar grad[0]
int64_t ssim_tiles(int64_t H, int64_t W);
size_t ssim_workspace(int64_t H, int64_t W, int C, bool backward);
hipError_t ssim_forward_dispatch(int64_t H, int64_t W, int cin, int C, const float *x, const float *y, float data_range,
                                 double *value, float *map, void *workspace, hipStream_t s);
hipError_t ssim_backward_dispatch(int64_t H, int64_t W, int cin, int C, const float *x, const float *y, float data_range,
                                  const float *grad, float *grad_x, void *workspace, hipStream_t s);

// posenc.hip: the decoder's input row [prefix | coords | sin | cos] and its two backward passes (arguments checked by the entry
// points; I = d when the coordinates are part of the row, else 0; strides in floats)
hipError_t posenc_forward_dispatch(int64_t n, int d, int F, int I, int P, const float *coords, int64_t cstride,
                                   const float *prefix, int64_t pstride, const float *bands, float *out, int64_t ostride,
                                   hipStream_t s);
hipError_t posenc_backward_dispatch(int64_t n, int d, int F, int I, int P, const float *row, int64_t rstride,
                                    const float *grad_out, int64_t gstride, const float *bands, float *grad_coords,
                                    hipStream_t s);
hipError_t posenc_backward2_dispatch(int64_t n, int d, int F, int I, int P, const float *gg, const float *row, int64_t rstride,
                                     const float *grad_out, int64_t gstride, const float *bands, float *grad_row,
                                     float *grad_grad, hipStream_t s);

// raygen.hip: rays and composited target colours of (view, pixel) pairs (arguments checked by the entry point; view_idx == NULL is
// the whole-view form; images == NULL: no rgb, no mask)
hipError_t raygen_dispatch(const float *cams, int num_views, int width, int height, const int32_t *view_idx,
                           const int32_t *pixel_idx, const float *jitter, int64_t n, const uint8_t *images, int channels,
                           bool bg_black, float *origins, float *dirs, float *rgb, uint8_t *mask, hipStream_t s);
// the same with the colours of a mip level: sums uint16 [V, H, W, channels], each the sum of 4^mip bytes
hipError_t raygen_sums_dispatch(const float *cams, int num_views, int width, int height, const int32_t *view_idx,
                                const int32_t *pixel_idx, const float *jitter, int64_t n, const uint16_t *sums, int channels,
                                int mip, bool bg_black, float *origins, float *dirs, float *rgb, uint8_t *mask, hipStream_t s);

// image_mip.hip: the uint16 block sums of one mip level of uint8 images (arguments checked by the entry point)
hipError_t image_mip_dispatch(const uint8_t *images, int64_t num_views, int64_t height, int64_t width, int channels, int mip,
                              uint16_t *sums, hipStream_t s);

// spc.hip: structured point clouds from depth images or point clouds, and their first-hit tracer (arguments checked by the entry
// points). DepthArgs names the [V, H, W] pixels of a depth data set: by value in the kernel arguments
struct DepthArgs {
    const float *cams;            // [V, SHACIRA_RAYGEN_RECORD_FLOATS]
    int32_t num_views, width, height;
    const float *depth;           // [V, H, W], not finite = no point
    const void *images;           // uint8 [V, H, W, channels] (mip 0) or uint16 sums (mip > 0), or NULL where no colour is made
    int32_t channels, mip, bg_black;
};
hipError_t depth_bounds_dispatch(const DepthArgs &a, float *bounds, int64_t *count, hipStream_t s);
hipError_t depth_points_dispatch(bool count, const DepthArgs &a, int32_t *block_counts, const int64_t *block_offsets,
                                 float *points, uint8_t *rgb, hipStream_t s);
hipError_t spc_mark_points_dispatch(int64_t n, const float *points, int level, uint32_t *words, hipStream_t s);
hipError_t spc_mark_depth_dispatch(const DepthArgs &a, int level, uint32_t *words, hipStream_t s);
hipError_t spc_popcount_dispatch(int64_t num_words, const uint32_t *words, int32_t *counts, hipStream_t s);
hipError_t spc_accumulate_points_dispatch(int64_t n, const float *points, const uint8_t *rgb, int level, const uint32_t *words,
                                          const int32_t *rank, int64_t cells, uint64_t *sums, hipStream_t s);
hipError_t spc_accumulate_depth_dispatch(const DepthArgs &a, int level, const uint32_t *words, const int32_t *rank, int64_t cells,
                                         uint64_t *sums, hipStream_t s);
hipError_t spc_resolve_dispatch(int64_t cells, const uint64_t *sums, uint8_t *colors, hipStream_t s);
hipError_t spc_first_hit_dispatch(int64_t num_rays, const float *origins, const float *dirs, int level, const uint32_t *words,
                                  const int32_t *rank, const uint8_t *colors, float *depth, uint8_t *hit, int32_t *pidx,
                                  float *rgb, hipStream_t s);

// shade.hip: the offline renderer's per-pixel passes (arguments checked by the entry points; mm_host may be NULL, light_host not)
hipError_t shade_view_dispatch(int64_t n, int mode, float *normal, const float *dirs, const uint8_t *hit, const float *mm_host,
                               const uint8_t *tex, int mh, int mw, int mc, float *rgb, float *uv_out, uint8_t *rgb8_out,
                               hipStream_t s);
hipError_t shadow_rays_dispatch(int64_t n, const float *origins, const float *dirs, const float *light_host, float min_y,
                                uint64_t seed, float *depth, float *xyz, float *normal, uint8_t *hit, float *so, float *sd,
                                uint8_t *light_hit, uint8_t *plane_hit, hipStream_t s);
hipError_t shadow_apply_dispatch(int64_t H, int64_t W, int C, const uint8_t *occluded, const uint8_t *light_hit,
                                 uint8_t *shadow_out, float *rgb, void *workspace, hipStream_t s);
hipError_t sdf_slice_colors_dispatch(int64_t n, const float *d, float *vis, hipStream_t s);

// pixels.hip: coordinates and colours of pixels of one uint8 [H, W, 3] image, and the squared-error loss of predictions against
// them (arguments checked by the entry points; pixel_idx == NULL is the range form, pixel i = start + i)
size_t pixel_loss_workspace(int64_t n);
hipError_t pixel_batch_dispatch(const uint8_t *image, int64_t height, int64_t width, const void *pixel_idx, int idx_bits,
                                int64_t start, int64_t n, float *coords, float *rgb, hipStream_t s);
hipError_t pixel_loss_forward_dispatch(const float *pred, int64_t pred_stride, const uint8_t *image, int64_t height,
                                       int64_t width, const void *pixel_idx, int idx_bits, int64_t start, int64_t n,
                                       uint8_t *out_image, double *stats, void *workspace, hipStream_t s);
hipError_t pixel_loss_backward_dispatch(const float *pred, int64_t pred_stride, const uint8_t *image, int64_t height,
                                        int64_t width, const void *pixel_idx, int idx_bits, int64_t start, int64_t n,
                                        const float *grad, float *grad_pred, hipStream_t s);

// sphere_trace.hip: find_depth_bound and the fused sphere-trace step (0 < P <= K < 2^31, checked by the entry points)
hipError_t find_depth_bound_launch(int64_t P, int64_t K, const float *query, const int32_t *curr, const int32_t *pack_end,
                                   const float *depth, int32_t *out, hipStream_t s);
hipError_t sphere_trace_step_launch(int64_t P, int64_t K, int64_t num_active, bool first, const int32_t *active_in,
                                    const float *sdf, const float *origins, const float *dirs, const float *depth,
                                    const int32_t *pack_end, const int32_t *pidx, float step_size, float min_dis,
                                    float dist_max, float *t, float *dist, float *dist_prev, int32_t *curr, float *x,
                                    uint8_t *active, uint8_t *hit, int32_t *active_out, float *coords_out,
                                    int32_t *pidx_out, int32_t *count_out, int32_t *count_next, hipStream_t s);

// latent.hip
struct DecodeArgs {
    const float *latent, *div, *matrix, *colscale, *shift;
    float clampw;
    float *decoded;
    const float *grad_decoded;
    float *grad_latent, *grad_matrix, *grad_colscale, *grad_shift;
    double *partials;
    int64_t rows;
    const float *uniforms;   // non-NULL: stochastic Gumbel annealing instead of rounding ([rows, ld, 2] uniforms)
    float temperature;
    int diff_sampling;
    const float *temperature_dev;   // non-NULL: SGA temperature read on the device (single / per-level decoders)
};
struct MultiArgs {   // passed to multi_decode_kernel by value
    const float *latent, *alpha, *div, *scale, *dft, *shift, *uniforms, *grad_decoded;
    float *decoded, *grad_latent, *grad_alpha, *grad_scale, *grad_shift;
    double *partials;
    int64_t rows;
    int K, straight_through, diff_sampling;
    float temperature, clampw;
};
struct EntropyArgs {
    const float *latent, *noise, *params, *grad_total;
    int num_layers;
    float *total_bits, *grad_latent, *grad_params;
    double *partials;
    int64_t rows;
};
// latent_mlp.hip
struct LatentMlpArgs {
    int num_layers;
    const int32_t *widths;   // host
    const float *latent, *uniforms, *div, *params;
    float temperature;
    int diff_sampling, act, final_act;
    float clampw;
    float *decoded;
    const float *grad_decoded;
    float *grad_latent, *grad_params;
    double *partials;
    int64_t rows;
};
bool latent_mlp_supported(int num_layers, const int32_t *widths);
size_t latent_mlp_workspace_bytes(int num_layers, const int32_t *widths);
hipError_t latent_mlp_dispatch(bool bwd, const LatentMlpArgs &a, hipStream_t s);

size_t latent_workspace_bytes();
bool latent_decode_supported(int ld, int f);
// level l owns rows [offsets[l], offsets[l + 1]) (host array of levels + 1); offsets == NULL: the plain decoder, which is the
// one level {0, a.rows}
hipError_t latent_decode_dispatch(bool bwd, int ld, int f, int levels, const int64_t *offsets, const DecodeArgs &a,
                                  hipStream_t s);
bool latent_multi_supported(int ld, int f, int K);
hipError_t latent_multi_dispatch(bool bwd, int ld, int f, bool dft, const MultiArgs &a, hipStream_t s);
bool entropy_supported(int ld);
hipError_t entropy_dispatch(bool bwd, int ld, const EntropyArgs &a, hipStream_t s);

// symbols.hip
bool symbols_supported(int ld);
hipError_t symbol_range_launch(const float *latent, int64_t rows, int ld, int32_t *minmax, hipStream_t s);
hipError_t symbol_histogram_launch(const float *latent, int64_t rows, int ld, const int32_t *minmax, int nbins,
                                   uint64_t *counts, hipStream_t s);
size_t rc_encode_bound(int64_t n);
int rc_encode(const int32_t *sym, int64_t n, const uint32_t *freq, int nsym, uint8_t *out, size_t cap, size_t *len);
int rc_decode(const uint8_t *in, size_t len, const uint32_t *freq, int nsym, int64_t n, int32_t *sym);
// interleaved rANS ("rans64"): host coder, and one wavefront per (block, channel) on the device
bool rans_steps_ok(int steps);
size_t rans_encode_bound(int64_t n, int steps);
int rans_encode(const int32_t *sym, int64_t n, const uint32_t *freq, int nsym, int steps, uint8_t *out, size_t cap,
                size_t *len);
int rans_decode(const uint8_t *in, size_t len, const uint32_t *freq, int nsym, int64_t n, int steps, int32_t *sym);
int rans_device_args_ok(int64_t rows, int ld, const int32_t *nbins, int cdf_stride, int steps, const int64_t *payload,
                        const int64_t *words, size_t bytes);
hipError_t rans_encode_launch(const float *latent, int64_t rows, int ld, const int32_t *lo, const int32_t *nbins,
                              const uint32_t *cdf, int cdf_stride, int steps, uint32_t *counts, uint32_t *states,
                              uint16_t *slots, hipStream_t s);
hipError_t rans_pack_launch(int64_t rows, int ld, const int32_t *nbins, int steps, const uint32_t *counts,
                            const uint32_t *states, const uint16_t *slots, const int64_t *block_start,
                            const int64_t *payload, const int64_t *words, uint8_t *out, hipStream_t s);
hipError_t rans_decode_launch(const uint8_t *data, int64_t rows, int ld, const int32_t *lo, const int32_t *nbins,
                              const int64_t *payload, const int64_t *words, const uint32_t *cdf, int cdf_stride,
                              const int64_t *block_start, int steps, float *out, int32_t *error, hipStream_t s);

// render.hip
hipError_t pack_integrate_launch(bool bwd, int64_t R, int C, const float *feats, const float *tau,
                                 const int64_t *pack_start, float *ray_feats, float *weights, const float *g_ray,
                                 const float *g_w, float *g_feats, float *g_tau, hipStream_t s);
hipError_t pack_sum_launch(bool broadcast, int64_t R, int C, const float *in, const int64_t *pack_start, float *out,
                           hipStream_t s);
hipError_t raymarch_ray_launch(bool emit, int64_t num_rays, int ns, const float *origins, const float *dirs,
                               float dist_min, float dist_max, const float *lin, const float *jitter,
                               const uint8_t *occ, int level, int32_t *counts, const int64_t *offsets, int64_t *ridx,
                               float *samples, float *depth, float *deltas, uint8_t *boundary, int64_t capacity,
                               hipStream_t s);
hipError_t raytrace_dense_launch(bool emit, int64_t num_rays, const float *origins, const float *dirs,
                                 const uint8_t *occ, int level, int32_t *counts, const int64_t *offsets, int32_t *ridx,
                                 int32_t *pidx, float *depth, hipStream_t s);
hipError_t raymarch_voxel_launch(int64_t num_rays, int ns, const float *origins, const float *dirs, const uint8_t *occ,
                                 int level, const int64_t *offsets, uint64_t seed, int64_t step, const int64_t *step_dev,
                                 int64_t capacity, void *workspace, int64_t *ridx, float *samples, float *depth,
                                 float *deltas, uint8_t *boundary, hipStream_t s);

// probe.hip
hipError_t stream_probe_launch(int kind, const void *a, void *b, size_t bytes, uint32_t *sink, hipStream_t s);

// adam.hip
hipError_t adam_step_launch(float *p, float *g, float *m, float *v, int64_t n, float lr, float b1, float b2, float eps,
                            float wd, int step, const int32_t *step_dev, int zero_grad, hipStream_t s);

hipError_t adam_multi_launch(int count, float *const *p, float *const *g, float *const *m, float *const *v,
                             const int64_t *n, const float *lr, const float *wd, float b1, float b2, float eps,
                             int step, const int32_t *step_dev, const float *grad_scale, const float *found_inf,
                             int zero_grad, hipStream_t s);

hipError_t rmsprop_multi_launch(int count, float *const *p, float *const *g, float *const *sq, float *const *buf,
                                const int64_t *n, const float *lr, const float *wd, float alpha, float eps,
                                float momentum, const float *grad_scale, const float *found_inf, int zero_grad,
                                hipStream_t s);

// mlp.hip / mlp_mfma.hip
constexpr int kMlpMaxBlocks = 512;        // backward grid (= rows of the fp64 partial-gradient workspace), VALU and wide MFMA
constexpr int kMlpNarrowMaxBlocks = 512; // same for the narrow (16x16x4) MFMA decoders (measured: 256 / 1024 / 2048 slower)
bool mlp_supported(int in, int h, int nh, int out);
int mlp_num_params(int in, int h, int nh, int out);
size_t mlp_workspace_bytes(int in, int h, int nh, int out);
hipError_t mlp_dispatch(bool bwd, int in, int h, int nh, int out, int64_t N, const float *x, const float *params,
                        float *y, const float *gy, float *gx, float *gparams, double *partials, hipStream_t s);

// api.hip: tunables. shacira_set_option() stores process-wide atomics; every API entry point takes ONE snapshot of them
// into a thread-local Options and everything below reads that snapshot (opt()), so a call -- its workspace-size check
// included -- sees one consistent set of values even while another thread changes an option.
struct Options {
    int fwd_variant = -1;         // -1 measured rule, 0 reference-shaped kernel, 3 lane pairs, 6 level-per-XCD staged, 8 cell-sorted
    int bwd_variant = -1;         // -1 by batch size, 0 scattered atomics (the reference's design), 1 binned
    int mlp_variant = -1;         // -1 MFMA decoders wherever instantiated, 0 VALU kernels
    int bwd_compact = 1;          // dense 3-D levels: one two-slot item per sample, z-slab buckets with a halo plane
    int bwd_selective_zero = 1;   // zero only the rows the consume pass does not overwrite (0: the whole table)
    int bwd_persistent = 1;       // consume pass: persistent workgroups fetching units from a counter
    int bwd_fork = 1;             // table zeroing + direct levels on a side stream when the batch is large
    int bwd_item12 = -1;          // 12-byte item units for fp32 tables (3-D, F = 2, batches >= 2^17): 1 always, 0 never (the 16-byte
                                  // stream), -1 = with the brick pass (planned calls in sorted order: the one place they pay)
    int bwd_run_pad = 1;          // scatter pass: (tile, bucket) runs reserved in whole 64-byte pieces (SHACIRA_RUN_ALIGN; large batches:
                                  // 4 units of 16 bytes, 16 units of 12 bytes = 192 bytes; the 8-byte half-precision units are not padded)
    int bin_acc_kib = 0;          // LDS accumulator image per consumer workgroup: 64, 128, 0 = by batch size
    int bin_batch_mib = 1536;     // cap of the backward's item array per sub-batch
    int tiled = -1;               // cell-sorted forward: -1 by batch size, 0 never, 1 whenever the shape allows
    int tiled_lc_fwd = -1;        // its number of coarse levels (rows kernel), -1 = planner
    int bwd_brick = -1;           // brick pass of the backward (needs the batch's plan): -1 / 1 whenever the shape allows, 0 never
    int bwd_brick_lo = -1;        // explicit brick level range [lo, hi) instead of the planner's rule (-1 = planner)
    int bwd_brick_hi = -1;
    int bwd_brick_fork = 2;       // where the brick pass runs: 0 last on the caller's stream, 1 / 2 side stream from behind the front / scatter pass
    int bwd_brick_span = 0;       // blocks per brick unit along x (0 = planner)
    int bwd_ext_fork = 1;         // planned calls: the brick pass's fork event rides on the scatter launch (hipExtLaunchKernelGGL)
    int coord_variant = -1;       // coordinate backward: -1 rule (8 with a plan in 3-D, else 0), 0 lane per sample, 3 lane pairs, 8 sorted pairs
    int fwd_direct = -1;          // level-per-XCD forward writes the output rows itself (no staging): -1 = small batches, 0 / 1
    int triplane_layout = -1;     // triplane forward reads: -1 rule (kTriDefaultHwc), 0 the NCHW parameters, 1 an HWC copy
};
const Options &opt();             // the calling thread's snapshot
void options_snapshot();          // taken at every extern "C" entry point that reads options

// The decoder MLP's ReLU (mlp.hip, mlp_mfma.hip) as torch.relu has it: a NaN stays a NaN (fmaxf returns the other operand).
// llvm.maximum is IEEE 754-2019 maximum, one v_maximum3_f32 on gfx950; the select "z < 0 ? 0 : z" means the same but made the
// VALU forward kernels spill 400-850 bytes per lane.
__device__ __forceinline__ float relu_keep_nan(float z) { return __builtin_elementwise_maximum(z, 0.0f); }

}  // namespace shacira
